"""Pre-tokenised training data for the Llama worker (``--data``): a read-only, memory-mapped stream
of token ids cut into fixed windows.

``TokenStream(path, vocab_size, dtype="auto")``: ``path`` is one file, or a directory whose ``*.npy``
/ ``*.bin`` files are concatenated in sorted name order.  ``.npy`` holds a 1-D uint16 / uint32 /
int32 array (dtype from its header); ``.bin`` holds raw little-endian ids whose width is ``dtype``
(``auto``: uint16 when ``vocab_size <= 65536``, else uint32).

Window ``k`` of length ``S`` is tokens ``[k*S, k*S + S + 1)`` -- inputs plus the last target -- and
there are ``n_windows = (n_tokens - 1) // S`` of them.  The batch of optimizer step ``t`` (1-based),
micro-batch ``m`` of ``N``, rank ``r`` of ``W``, row ``b`` of ``B`` is window
``(((t-1)*N + m)*W + r)*B + b`` modulo ``n_windows``: a pure function of the step, so a resumed run
continues the stream from its checkpoint's step with nothing else saved, and ranks never share a
window within a step.

There is no shuffling: pre-training shards are shuffled when they are written, and a reader that
walks them in order keeps every read sequential.
"""
from __future__ import annotations

import os
from typing import List, Tuple

import numpy as np

_NPY_DTYPES = (np.dtype("uint16"), np.dtype("uint32"), np.dtype("int32"))
_BIN_DTYPES = {"uint16": np.dtype("<u2"), "uint32": np.dtype("<u4")}


def _bin_dtype(dtype: str, vocab_size: int) -> np.dtype:
    if dtype == "auto":
        dtype = "uint16" if vocab_size <= 65536 else "uint32"
    if dtype not in _BIN_DTYPES:
        raise ValueError(f"token dtype: auto, uint16 or uint32; got {dtype!r}")
    return _BIN_DTYPES[dtype]


def _open(path: str, bin_dtype: np.dtype) -> np.ndarray:
    if path.endswith(".npy"):
        a = np.load(path, mmap_mode="r", allow_pickle=False)
        if a.ndim != 1:
            raise ValueError(f"{path}: a 1-D array of token ids; got shape {a.shape}")
        if a.dtype not in _NPY_DTYPES:
            raise ValueError(f"{path}: uint16, uint32 or int32 token ids; got {a.dtype}")
        return a
    if path.endswith(".bin"):
        size = os.path.getsize(path)
        if size % bin_dtype.itemsize:
            raise ValueError(f"{path}: {size} bytes is no whole number of {bin_dtype.name} ids")
        if size == 0:
            return np.empty(0, dtype=bin_dtype)
        return np.memmap(path, dtype=bin_dtype, mode="r")
    raise ValueError(f"{path}: token files are .npy or .bin")


class TokenStream:
    """The files of ``path`` as one logical 1-D stream of token ids (see the module docstring).
    ``bind`` fixes the batch geometry; ``span`` then returns one micro-batch's narrow tokens."""

    def __init__(self, path: str, vocab_size: int, dtype: str = "auto"):
        self.path = path
        self.vocab_size = int(vocab_size)
        bin_dtype = _bin_dtype(dtype, self.vocab_size)
        if os.path.isdir(path):
            names = sorted(n for n in os.listdir(path) if n.endswith((".npy", ".bin")))
            if not names:
                raise ValueError(f"{path}: no .npy or .bin token files")
            files = [os.path.join(path, n) for n in names]
        elif os.path.isfile(path):
            files = [path]
        else:
            raise ValueError(f"{path}: no such token file or directory")
        self.files: List[str] = files
        self._arrays = [a for a in (_open(f, bin_dtype) for f in files) if a.shape[0] > 0]
        # offsets[i] = logical index of the first token of array i; offsets[-1] = n_tokens
        self._offsets = np.concatenate([[0], np.cumsum([a.shape[0] for a in self._arrays])]).astype(np.int64)
        self.n_tokens = int(self._offsets[-1])
        if self.n_tokens == 0:
            raise ValueError(f"{path}: an empty token stream")
        # the narrow dtype spans are returned in (int32 ids are reinterpreted: a negative id becomes
        # an id >= vocab, which the batch kernel clamps and counts)
        self.dtype = (np.dtype("uint16") if all(a.dtype == np.dtype("uint16") for a in self._arrays)
                      else np.dtype("uint32"))
        self.seq_len = self.batch_size = self.grad_accum = self.world = None
        self.n_windows = 0

    def bind(self, seq_len: int, batch_size: int, grad_accum: int = 1, world: int = 1) -> "TokenStream":
        if min(seq_len, batch_size, grad_accum, world) < 1:
            raise ValueError("seq_len, batch_size, grad_accum and world are positive")
        if self.n_tokens < seq_len + 1:
            raise ValueError(f"{self.path}: {self.n_tokens} tokens are fewer than one window of "
                             f"{seq_len} + 1")
        self.seq_len, self.batch_size, self.grad_accum, self.world = seq_len, batch_size, grad_accum, world
        self.n_windows = (self.n_tokens - 1) // seq_len
        return self

    def window_index(self, t: int, m: int, r: int, b: int) -> int:
        """The window of step ``t`` (1-based), micro-batch ``m``, rank ``r``, row ``b``."""
        return ((((t - 1) * self.grad_accum + m) * self.world + r) * self.batch_size + b) % self.n_windows

    def _narrow(self, a: np.ndarray) -> np.ndarray:
        if a.dtype == self.dtype:
            return a
        if a.dtype == np.dtype("int32"):
            return a.view(np.uint32)
        return a.astype(self.dtype)  # uint16 file in a mixed stream

    def read(self, start: int, stop: int) -> np.ndarray:
        """Tokens ``[start, stop)`` of the logical stream, stitched across file boundaries."""
        if not 0 <= start <= stop <= self.n_tokens:
            raise IndexError(f"tokens [{start}, {stop}) of a stream of {self.n_tokens}")
        i = int(np.searchsorted(self._offsets, start, side="right")) - 1
        if stop <= self._offsets[i + 1]:
            o = int(self._offsets[i])
            return self._narrow(self._arrays[i][start - o:stop - o])
        out = np.empty(stop - start, dtype=self.dtype)
        pos = start
        while pos < stop:
            o, e = int(self._offsets[i]), int(self._offsets[i + 1])
            n = min(stop, e) - pos
            out[pos - start:pos - start + n] = self._narrow(self._arrays[i][pos - o:pos - o + n])
            pos += n
            i += 1
        return out

    def window(self, k: int) -> np.ndarray:
        """The ``S + 1`` tokens of window ``k``."""
        S = self.seq_len
        return self.read(k * S, k * S + S + 1)

    def span(self, t: int, m: int, r: int) -> Tuple[np.ndarray, int]:
        """``(tokens, row_stride)`` of one micro-batch: row ``b`` is ``tokens[b*row_stride : b*row_stride
        + S + 1]``.  Where the B windows lie back to back inside one file, one slice of ``B*S + 1``
        tokens (a view of the mapping) with ``row_stride = S``; at the wrap and across file boundaries,
        B gathered rows of ``S + 1`` tokens with ``row_stride = S + 1``."""
        S, B = self.seq_len, self.batch_size
        k0 = self.window_index(t, m, r, 0)
        if k0 + B <= self.n_windows:
            start, stop = k0 * S, (k0 + B) * S + 1
            i = int(np.searchsorted(self._offsets, start, side="right")) - 1
            if stop <= self._offsets[i + 1]:
                return self.read(start, stop), S
        rows = np.empty((B, S + 1), dtype=self.dtype)
        for b in range(B):
            rows[b] = self.window((k0 + b) % self.n_windows)
        return rows.reshape(-1), S + 1
