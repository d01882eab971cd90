"""End to end on a real MI355X: operator binary + local cluster + the HIP MNIST worker.

A PyTorchJob asking for ``amd.com/gpu: 1`` is scheduled by the kubelet emulator onto the
box's GPU (HIP_VISIBLE_DEVICES), the worker trains on the fused gfx950 kernels with
``--backend rccl`` and the job must reach Succeeded with a learned model.
"""
import json
import time

import pytest

from pytorch_operator_amd.cluster.local import LocalCluster
from kubeflow.pytorchjob.rest import PODS, PYTORCHJOBS

pytestmark = pytest.mark.gpu


def _wait(c, name, timeout=300):
    t0 = time.time()
    while time.time() - t0 < timeout:
        j = c.rest.get(PYTORCHJOBS, name, "default")
        types = [x["type"] for x in (j.get("status") or {}).get("conditions") or []]
        if "Succeeded" in types or "Failed" in types:
            return j, types
        time.sleep(0.2)
    raise TimeoutError(name)


def test_gpu_mnist_job_hip_kernels(tmp_path):
    job = {"apiVersion": "kubeflow.org/v1", "kind": "PyTorchJob", "metadata": {"name": "mnist-gpu"},
           "spec": {"cleanPodPolicy": "None", "pytorchReplicaSpecs": {"Master": {
               "replicas": 1, "restartPolicy": "OnFailure",
               "template": {"spec": {"containers": [{
                   "name": "pytorch", "image": "pytorch-operator-amd/worker:latest",
                   "args": ["--backend", "rccl", "--dataset-size", "20000", "--test-size", "2000",
                            "--log-interval", "10"],
                   "resources": {"limits": {"amd.com/gpu": 1}}}]}}}}}}
    with LocalCluster(workdir=str(tmp_path / "c"), gpus=[0]) as c:
        c.wait_operator_ready()
        t0 = time.time()
        c.rest.create(PYTORCHJOBS, job, "default")
        j, types = _wait(c, "mnist-gpu")
        elapsed = time.time() - t0
        log = c.rest.pod_log("mnist-gpu-master-0", "default")
        assert types[-1] == "Succeeded", log[-3000:]
        events = [json.loads(x) for x in log.splitlines() if x.startswith('{"event"')]
        start = next(e for e in events if e["event"] == "start")
        done = next(e for e in events if e["event"] == "train_done")
        assert start["kernels"] == "hip"
        assert done["accuracy"] > 0.9, log[-2000:]
        print(f"job wall {elapsed:.2f}s, train {done['samples_per_sec']} samples/s, acc {done['accuracy']}")


@pytest.mark.parametrize("topology", [False, True])
def test_two_pod_xgmi_job_needs_the_pod_topology(tmp_path, topology):
    """Two one-GPU pods of one job exchanging gradients over peer memory (the xGMI kernel;
    gloo carries only the rendezvous because both pods share this box's single GPU).
    With the kubelet giving pods their own PID/IPC namespaces, the peer-memory IPC exchange
    must FAIL unless the operator's --xgmi-pod-topology put the pods in the node's
    namespaces (docs/xgmi_pods.md) -- then the job succeeds on the xGMI path.
    The isolated job fails in one of the two IPC calls: the import (hipIpcOpenMemHandle) cannot
    reach an exporter in another PID namespace; and where the pods' workers are each PID 1 of
    their own PID namespace but share the emulator's network namespace, the dmabuf export
    (hipIpcGetMemHandle) of the second pod to ask already fails (seen on ROCm 7.2)."""
    from pytorch_operator_amd.cluster.kubelet import namespaces_available
    ok, why = namespaces_available()
    if not ok and not topology:
        # (the MI355X pool's boxes refuse user namespaces: "unshare failed: No space left on
        # device"; the isolated case then cannot be built there -- the CPU suite covers the
        # kubelet's isolation, tests/test_e2e_local.py::test_pod_namespaces_follow_host_pid_ipc)
        pytest.skip(f"no user namespaces on this host: {why}")
    name = f"xgmi-pods-{'topo' if topology else 'plain'}"
    rs = {"replicas": 1, "restartPolicy": "Never",
          "template": {"spec": {"containers": [{
              "name": "pytorch", "image": "pytorch-operator-amd/worker:latest",
              "args": ["--backend", "gloo", "--allreduce", "xgmi", "--dataset-size", "2560",
                       "--test-size", "500", "--log-interval", "10"],
              "resources": {"limits": {"amd.com/gpu": 1}}}]}}}
    job = {"apiVersion": "kubeflow.org/v1", "kind": "PyTorchJob", "metadata": {"name": name},
           "spec": {"cleanPodPolicy": "None", "pytorchReplicaSpecs": {"Master": rs, "Worker": rs}}}
    op_args = ["--inject-rccl-env"] + (["--xgmi-pod-topology"] if topology else [])
    with LocalCluster(workdir=str(tmp_path / "c"), gpus=[0, 0], operator_args=op_args,
                      isolation="namespaces") as c:
        c.wait_operator_ready()
        c.rest.create(PYTORCHJOBS, job, "default")
        j, types = _wait(c, name, timeout=240)
        logs = {p: c.rest.pod_log(p, "default") for p in (f"{name}-master-0", f"{name}-worker-0")}
        pod = c.rest.get(PODS, f"{name}-worker-0", "default")
        blob = "\n".join(v[-3000:] for v in logs.values())
        if topology:
            assert pod["spec"].get("hostPID") is True and pod["spec"].get("hostIPC") is True
            assert types[-1] == "Succeeded", blob
            for v in logs.values():
                assert '"path": "xgmi"' in v
        else:
            assert not pod["spec"].get("hostPID")
            assert types[-1] == "Failed", blob
            assert "hipIpcOpenMemHandle failed" in blob or "hipIpcGetMemHandle failed" in blob, blob
            for v in logs.values():
                assert '"path": "xgmi"' not in v
