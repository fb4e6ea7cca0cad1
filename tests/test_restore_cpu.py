"""Whole-image restoration, host side (no GPU): the window plan of include/vit_unet_amd.h (vu_tile_plan_count / _axis,
`restore.tile_plan`) against its stated properties, and the numpy restatement of the plan, the reflection, the weights
and the float64 blend that tests/test_gpu_restore.py holds the HIP kernels against."""
import ctypes as C

import numpy as np
import pytest
import torch

from vit_unet.torch import _lib
from vit_unet.torch.restore import TiledRestorer, tile_plan


# ---------------------------------------------------------------- numpy restatement (independent of the C code)
def ref_axis(L, T, overlap):
    """Origins of one axis: one window at 0 when L <= T, else ceil((L - T) / S) + 1 windows at min(i S, L - T)."""
    if L <= T:
        return [0]
    S = T - overlap
    n = -(-(L - T) // S) + 1
    return [min(i * S, L - T) for i in range(n)]


def ref_src(L, T, origin):
    """Source indices of the T positions of a window: the pixels themselves, or (L < T) reflected without the edge."""
    k = origin + np.arange(T)
    if L >= T:
        return k
    if L == 1:
        return np.zeros(T, dtype=np.int64)
    m = 2 * (L - 1)
    k = k % m
    return np.where(k < L, k, m - k)


def ref_windows_hwc(img, T, overlap):
    """(H,W,C) image -> (nt,T,T,C) windows of the plan, row-major (ty outer, tx inner)."""
    H, W = img.shape[:2]
    return np.stack([img[ref_src(H, T, oy)][:, ref_src(W, T, ox)] for oy in ref_axis(H, T, overlap) for ox in ref_axis(W, T, overlap)])


def ref_weight(T, overlap, dtype=np.float64):
    i = np.arange(T)
    return (np.minimum(np.minimum(i + 1, T - i), overlap + 1).astype(dtype) / dtype(overlap + 1)).astype(dtype)


def ref_blend(tiles, H, W, T, overlap, dtype=np.float64):
    """tiles (nt,C,T,T) -> (C,H,W): acc += w v, ws += w over the windows in ascending plan order, out = acc / ws."""
    oys, oxs = ref_axis(H, T, overlap), ref_axis(W, T, overlap)
    Cn = tiles.shape[1]
    w1 = ref_weight(T, overlap, dtype)
    acc, ws = np.zeros((Cn, H, W), dtype), np.zeros((H, W), dtype)
    for ty, oy in enumerate(oys):
        for tx, ox in enumerate(oxs):
            h, w = min(T, H - oy), min(T, W - ox)          # L <= T: only the first L rows / columns are used
            w2 = (w1[:h, None] * w1[None, :w]).astype(dtype)
            acc[:, oy:oy + h, ox:ox + w] += w2 * tiles[ty * len(oxs) + tx, :, :h, :w].astype(dtype)
            ws[oy:oy + h, ox:ox + w] += w2
    assert (ws > 0).all()
    return acc / ws


def overlaps(T):
    return sorted({0, 1, T // 8, T // 4, T // 2 - 1, T // 2})


def lengths(T):
    return list(range(1, 3 * T + 7)) + [1000, 3000, 4032]


# ---------------------------------------------------------------- 1. plan properties through the C entry points
@pytest.mark.parametrize("T", [32, 64, 224])
def test_plan_axis_properties(T):
    L_ = _lib.lib()
    cap = 4032 // (T // 2) + 4
    arr = (C.c_int * cap)()
    for ov in range(T // 2 + 1):
        S = T - ov
        for L in lengths(T):
            n = L_.vu_tile_plan_axis(L, T, ov, arr, cap)
            assert n >= 1, (L, T, ov, L_.vu_last_error())
            o = list(arr[:n])
            assert o == ref_axis(L, T, ov), (L, T, ov)
            assert o[0] == 0 and all(b > a for a, b in zip(o, o[1:])), (L, T, ov, o)      # strictly increasing
            if L <= T:
                assert o == [0]
                continue
            assert o[-1] + T == L                                                          # the last window ends at L
            assert all(b - a <= S for a, b in zip(o, o[1:]))                               # no gap: every pixel covered
            cover = np.zeros(L, dtype=np.int64)
            for a in o:
                cover[a:a + T] += 1
            assert cover.min() >= 1 and cover.max() <= 3, (L, T, ov, cover.max())


def test_tile_plan_wrapper_and_count():
    oy, ox = tile_plan(3024, 4032, 224, 32)
    assert oy == ref_axis(3024, 224, 32) and ox == ref_axis(4032, 224, 32)
    assert (len(oy), len(ox)) == (16, 21) and oy[-1] == 3024 - 224 and ox[-1] == 4032 - 224
    assert tile_plan(10, 500, 32, 8) == ([0], ref_axis(500, 32, 8))
    assert tile_plan(1, 1, 32, 16) == ([0], [0])
    L_ = _lib.lib()
    ny, nx = C.c_int(-1), C.c_int(-1)
    for H, W, T, ov in ((83, 121, 32, 8), (224, 224, 224, 112), (225, 223, 224, 0), (4032, 3024, 224, 32)):
        assert L_.vu_tile_plan_count(H, W, T, ov, C.byref(ny), C.byref(nx)) == 0
        assert (ny.value, nx.value) == (len(ref_axis(H, T, ov)), len(ref_axis(W, T, ov)))


def test_plan_argument_errors():
    L_ = _lib.lib()
    arr = (C.c_int * 8)()
    ny, nx = C.c_int(0), C.c_int(0)
    for call, word in ((lambda: L_.vu_tile_plan_axis(100, 32, 17, arr, 8), "overlap"),          # overlap > T / 2
                       (lambda: L_.vu_tile_plan_axis(100, 32, -1, arr, 8), "overlap"),
                       (lambda: L_.vu_tile_plan_axis(100, 0, 0, arr, 8), "window"),             # T <= 0
                       (lambda: L_.vu_tile_plan_axis(100, -4, 0, arr, 8), "window"),
                       (lambda: L_.vu_tile_plan_axis(0, 32, 8, arr, 8), "empty"),
                       (lambda: L_.vu_tile_plan_axis(1000, 32, 8, arr, 8), "capacity"),         # 42 windows in 8 slots
                       (lambda: L_.vu_tile_plan_axis(100, 32, 8, None, 8), "capacity"),
                       (lambda: L_.vu_tile_plan_count(100, 100, 32, 17, C.byref(ny), C.byref(nx)), "overlap"),
                       (lambda: L_.vu_tile_plan_count(100, 100, 0, 0, C.byref(ny), C.byref(nx)), "window"),
                       (lambda: L_.vu_tile_plan_count(100, 0, 32, 8, C.byref(ny), C.byref(nx)), "empty"),
                       (lambda: L_.vu_tile_plan_count(100, 100, 32, 8, None, None), "null")):
        assert call() < 0
        assert word in L_.vu_last_error().decode(), L_.vu_last_error()
    with pytest.raises(_lib.VuError, match="overlap"):
        tile_plan(100, 100, 32, 17)


def test_restorer_argument_errors():
    from vit_unet.torch import model as M
    m = M.HViT_UNet(1, 1, 1, "conv", 32, 8, 3, 16, 2, 0., 0., 0.)
    for kw in (dict(overlap=17), dict(overlap=-1), dict(batch=0), dict(std=0.0)):
        with pytest.raises(_lib.VuError):
            TiledRestorer(m, **kw)
    r = TiledRestorer(m, overlap=16, batch=4)
    assert (r.T, r.overlap, r.batch) == (32, 16, 4)
    with pytest.raises(_lib.VuError):                 # a CPU model: refused, no fallback
        r(np.zeros((40, 40, 3), np.uint8))
    with pytest.raises(_lib.VuError):
        m.restore(torch.zeros(3, 40, 40))


# ---------------------------------------------------------------- 2. the restatement itself
def test_reflection_indices():
    assert ref_src(5, 8, 0).tolist() == [0, 1, 2, 3, 4, 3, 2, 1]               # no repeated edge
    assert ref_src(3, 8, 0).tolist() == [0, 1, 2, 1, 0, 1, 2, 1]               # wraps with period 2 (L - 1)
    assert ref_src(1, 4, 0).tolist() == [0, 0, 0, 0]                           # L == 1 replicates
    assert ref_src(2, 5, 0).tolist() == [0, 1, 0, 1, 0]
    assert ref_src(40, 8, 32).tolist() == list(range(32, 40))                  # L >= T: a plain crop
    x = np.arange(5)
    assert np.array_equal(x[ref_src(5, 8, 0)], np.pad(x, (0, 3), mode="reflect"))
    assert np.array_equal(np.arange(3)[ref_src(3, 5, 0)], np.pad(np.arange(3), (0, 2), mode="reflect"))


def test_weights():
    assert np.array_equal(ref_weight(8, 0), np.ones(8))
    assert np.allclose(ref_weight(8, 3), np.array([1, 2, 3, 4, 4, 3, 2, 1]) / 4)
    assert np.allclose(ref_weight(8, 1), np.array([1, 2, 2, 2, 2, 2, 2, 1]) / 2)
    for T in (32, 224):
        for ov in overlaps(T):
            w = ref_weight(T, ov)
            assert w.min() == 1 / (ov + 1) and w.max() == min(T // 2, ov + 1) / (ov + 1) and np.array_equal(w, w[::-1])


@pytest.mark.parametrize("H,W,T,ov", [(83, 121, 32, 8), (32, 32, 32, 16), (20, 70, 32, 5), (7, 9, 32, 16), (1, 33, 32, 0),
                                      (100, 64, 32, 16), (450, 230, 224, 32)])
def test_blend_of_constant_windows_is_the_constant(H, W, T, ov):
    nt = len(ref_axis(H, T, ov)) * len(ref_axis(W, T, ov))
    tiles = np.full((nt, 2, T, T), 0.37)
    tiles[:, 1] = -5.25
    out = ref_blend(tiles, H, W, T, ov)
    assert out.shape == (2, H, W)
    assert np.abs(out[0] - 0.37).max() < 1e-15 and np.abs(out[1] + 5.25).max() < 1e-14


@pytest.mark.parametrize("H,W,T", [(64, 96, 32), (32, 32, 32), (448, 224, 224)])
def test_blend_without_overlap_is_plain_reassembly(H, W, T):
    rng = np.random.default_rng(H + W)
    img = rng.standard_normal((3, H, W))
    hwc = np.ascontiguousarray(img.transpose(1, 2, 0))
    tiles = ref_windows_hwc(hwc, T, 0).transpose(0, 3, 1, 2)                   # (nt,C,T,T): disjoint T x T blocks
    assert tiles.shape[0] == (H // T) * (W // T)
    blocks = img.reshape(3, H // T, T, W // T, T).transpose(1, 3, 0, 2, 4).reshape(-1, 3, T, T)
    assert np.array_equal(tiles, blocks)
    assert np.array_equal(ref_blend(tiles, H, W, T, 0), img)
    # gather then blend is the identity for any overlap too (every window holds the image's own values)
    for ov in (8, T // 2):
        t2 = ref_windows_hwc(hwc, T, ov).transpose(0, 3, 1, 2)
        assert np.abs(ref_blend(t2, H, W, T, ov) - img).max() < 1e-14


def test_float32_blend_stays_inside_the_stated_bound():
    """The bound tests/test_gpu_restore.py holds the kernel to, |out - ref| <= 2e-6 max|v|: at most 9 terms; each weight
    carries 2 roundings and each product 1, the two running sums at most 8 each, one division: about 22 units of 2^-24 =
    1.3e-6 relative to sum(w |v|) / sum(w) <= max|v|.  A float32 numpy blend must sit inside it."""
    H, W, T, ov = 83, 121, 32, 8
    rng = np.random.default_rng(0)
    nt = len(ref_axis(H, T, ov)) * len(ref_axis(W, T, ov))
    tiles = rng.uniform(-1, 1, (nt, 3, T, T)).astype(np.float32)
    err = np.abs(ref_blend(tiles, H, W, T, ov, np.float32).astype(np.float64) - ref_blend(tiles, H, W, T, ov)).max()
    assert err <= 2e-6 * np.abs(tiles).max(), err
