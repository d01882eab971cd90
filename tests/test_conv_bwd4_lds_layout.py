"""conv_bwd4's LDS operand layout (round 9): 2a fetches a lane's four A values of a k row with one
16-byte read, and one 2b wave feeds the three co tiles of a (j tile, K half) from one im2col read.

CPU part: a numpy model of the W2-slice index map and of both 2a forms (the parent's: row stride
144, element (co, j) at column j + cig, four 4-byte reads 16 columns apart, dcolT stored by j; this
one: row stride G_WS, one float4 at column 64 h + 4 sig(i), dcolT stored by window column j + cig).
Every LDS word holds its own (co, window column) id, so "the same operand value" is checked as "the
same id": for every wave, lane, k-step and tile, the value that reaches the accumulator of dcolT
element (j, pos) in k slot g is W2[4 s + g][j] in both forms -- with the products and their order
unchanged, bit-identity follows.  Also the map's bijection into its region, the 16-byte alignment
of every wide access, the neighbouring regions, and 2b's wave -> (tile, K half) cover.

GPU part: conv_bwd4 + the slab reduction at B = 1, 4, 5 (tools/conv_bwd4_numerics.py's cases; B = 5
has a partial last chunk and blocks b >= B): two runs bit-equal, and the dcol-dependent gradients
(dW_conv1, db_conv1: col2im -> dz1 -> phase 4) against the tool's fp64 reference.  Tolerance: the
parent kernel's own error on the same case, as recorded by that tool
(profiles/r8_bwd4_2b/numerics.json; the parent's 2a, col2im and phase 4 are round 7's) -- this
kernel runs the same operations in the same order, so it may not exceed it.
"""
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
SRC = ROOT / "csrc" / "kernels" / "mnist_kernels.hip"
RECORD = ROOT / "profiles" / "r8_bwd4_2b" / "numerics.json"


def _const(name):
    m = re.search(rf"constexpr int {name} = (\d+);", SRC.read_text())
    assert m, name
    return int(m.group(1))


G_WS, G_DZS, G_DZR = _const("G_WS"), _const("G_DZS"), _const("G_DZR")
F_DC, F_Z1, F_RED1 = _const("F_DC"), _const("F_Z1"), _const("F_RED1")
G_OFF_W = 4 * G_DZR * G_DZS           # behind the 4 samples' dz images
G_OFF_DCOL = G_OFF_W + 52 * G_WS
STATIC_LDS = 16                       # bytes in front of the dynamic array (test_conv_bwd4_lds_align.py)
P_WS = 144                            # the parent's row stride


def sig(i):
    return 4 * (i & 3) + (i >> 2)


def stage_image():
    """The staging stores: thread tid writes float4 [tid & 31] of rows tid >> 5 and (tid + 1024) >> 5.
    Returns offset (floats, relative to the region) -> (co, window column m), and the store offsets."""
    img, stores = {}, []
    for tid in range(1024):
        rows = [tid >> 5] + ([(tid + 1024) >> 5] if tid < 640 else [])
        for co in rows:
            off = co * G_WS + 4 * (tid & 31)
            stores.append(off)
            for k in range(4):
                assert off + k not in img
                img[off + k] = (co, 4 * (tid & 31) + k)
    return img, stores


def test_w2_slice_map_is_a_bijection_into_its_region():
    img, _ = stage_image()
    assert sorted(img) == list(range(52 * G_WS))            # every word of the region, once
    assert len(set(img.values())) == 52 * 128                 # every (co, m), once
    for off, (co, m) in img.items():
        assert off == co * G_WS + m
    assert G_OFF_W + max(img) < G_OFF_DCOL                    # ends where dcolT starts
    assert G_OFF_W >= 4 * G_DZR * G_DZS                       # starts behind the dz images
    assert 5 * F_Z1 + 16 * F_RED1 <= 52 * G_WS                # the aliases (pooled dz1, phase-4 partials) fit
    assert (5 * F_Z1) % 4 == 0


def test_wide_accesses_are_16_byte_aligned():
    _, stores = stage_image()
    for off in stores:
        assert (STATIC_LDS + 4 * (G_OFF_W + off)) % 16 == 0
    for w in range(8):
        for lane in range(64):
            i, g = lane & 15, lane >> 4
            for s in range(13):
                off = (4 * s + g) * G_WS + 64 * (w >> 2) + 4 * sig(i)
                assert (STATIC_LDS + 4 * (G_OFF_W + off)) % 16 == 0
                assert 0 <= off and off + 3 < 52 * G_WS


def _dcol_feed_parent(cig):
    """(j, pos, s, g) -> (co, m) delivered, the parent's 2a; and dcolT offset of (j, pos)."""
    feed, where = {}, {}
    for w in range(8):
        pt, jt0 = w & 3, (w >> 2) * 4
        for s in range(13):
            for t in range(4):
                # A operand: lane (i, g) supplies row i, k slot g
                a = {(i, g): ((4 * s + g), cig + (jt0 + t) * 16 + i) for i in range(16) for g in range(4)}
                for row in range(16):
                    j = (jt0 + t) * 16 + row
                    for col in range(16):
                        for g in range(4):
                            co, off_m = a[(row, g)]
                            assert off_m < P_WS
                            feed[(j, pt * 16 + col, s, g)] = (co, off_m)
        for t in range(4):
            for g in range(4):
                for rr in range(4):
                    for i in range(16):
                        j = (jt0 + t) * 16 + 4 * g + rr          # accumulator row 4 g + rr of tile t
                        where[(j, pt * 16 + i)] = j * F_DC + pt * 16 + i
    return feed, where


def _dcol_feed_new(cig, img):
    feed, where = {}, {}
    for w in range(8):
        pt, h = w & 3, w >> 2
        for s in range(13):
            a = {}
            for i in range(16):
                for g in range(4):
                    off = (4 * s + g) * G_WS + 64 * h + 4 * sig(i)
                    a[(i, g)] = [img[off + t] for t in range(4)]
            for t in range(4):
                for row in range(16):
                    m = 64 * h + 4 * sig(row) + t               # the window column MFMA row `row` holds
                    for g in range(4):
                        co, mm = a[(row, g)][t]
                        assert mm == m
                        for col in range(16):
                            feed[(m - cig, pt * 16 + col, s, g)] = (co, mm)
        for t in range(4):
            for g in range(4):
                for rr in range(4):
                    m_store = 64 * h + 16 * rr + 4 * g + t      # the kernel's store row
                    assert m_store == 64 * h + 4 * sig(4 * g + rr) + t
                    assert 0 <= m_store < 128
                    for i in range(16):
                        where[(m_store - cig, pt * 16 + i)] = m_store * F_DC + pt * 16 + i
    return feed, where


@pytest.mark.parametrize("cig", [0, 1, 2, 3])
def test_2a_feeds_every_dcol_element_the_parents_operands(cig):
    img, _ = stage_image()
    fp, wp = _dcol_feed_parent(cig)
    fn, wn = _dcol_feed_new(cig, img)
    for j in range(125):                                       # the columns col2im reads
        for pos in range(64):
            for s in range(13):
                for g in range(4):
                    assert fn[(j, pos, s, g)] == fp[(j, pos, s, g)] == (4 * s + g, j + cig)
            # col2im reads row j + cig where the parent read row j: the same logical element
            assert wn[(j, pos)] == wp[(j, pos)] + cig * F_DC
    offs = [v for v in wn.values()]
    assert len(set(offs)) == len(offs) and max(offs) < 128 * F_DC and min(offs) >= 0


def test_2b_waves_cover_every_tile_and_k_half_once():
    seen, slots = set(), {}
    for w8 in range(4):
        jt, kh = w8 & 1, (w8 >> 1) & 1
        for ct in range(3):
            assert (ct, jt, kh) not in seen
            seen.add((ct, jt, kh))
        handed = [0, 1] if kh else [2]                          # through pk_s, slot 2 ct + jt
        for ct in handed:
            slot = 2 * ct + jt
            assert slot not in slots and slot < 6
            slots[slot] = (ct, jt, kh)
    assert len(seen) == 12 and len(slots) == 6
    for slot, (ct, jt, kh) in slots.items():                    # the other half's wave writes the tile
        assert (ct, jt, 1 - kh) in seen


@pytest.fixture(scope="module")
def num():
    import conv_bwd4_numerics
    return conv_bwd4_numerics


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 4, 5])
def test_dcol_dependent_gradients_and_determinism(num, B):
    import torch
    from pytorch_operator_amd.ops import _native
    _native.load()
    parent = json.loads(RECORD.read_text())["batches"][str(B)]["max_rel_err"]
    case = num.make_case(B)
    grads, inputs = num.run_case(case)
    again, _ = num.run_case(case)
    for n in num.NAMES:
        assert torch.equal(grads[n], again[n]), (B, n)
    ref = num.reference(*inputs)
    for n in ("conv1.weight", "conv1.bias"):
        err = num.rel_err(grads[n], ref[n])
        print(f"B={B} {n}: max rel err {err:.3e} (parent: {parent[n]:.3e})")
        assert err <= parent[n], (B, n, err, parent[n])
