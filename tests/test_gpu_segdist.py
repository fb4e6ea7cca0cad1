"""Surface-distance metrics on the GPU (csrc/vu_segdist.hip, segment.SurfaceDistance, TiledSegmenter(surface=)).

Through the C ABI with sentinel-filled outputs; every integer is compared EXACTLY against the restatements of
tests/test_segdist_cpu.py, on masks built around the kernels' own geometry (vu_segdist_geometry: L = the piece of a y / z line
a workgroup holds in LDS, C = the lines a workgroup owns, X = the pixels of a row a wave scans per trip):
  vu_edt_sq        == ref_edt_sq, dims 2 x fg 0 / 1 x spacing (1,1,1) / (3,1,2) and dims 3
  vu_mask_surface  == ref_surface
  vu_surface_dist  stats and order == ref_surface_dist; sums within a relative 1e-9 of the float64 numpy sum (for <= 2^20 positive
                   terms the error of any summation order is below n 2^-53 plus one rounding per sqrt, < 2^-32)
  two runs of every entry are bit-equal, sums included
End to end: TiledSegmenter(surface=None) is today's segmenter key for key and bit for bit; with a SurfaceDistance the "surface"
values are surface_metrics of the restatement on the returned mask (also after clean=); hd95_tiled agrees and a two-fold
run_segmentation(surface=) reports the three metrics."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_gpu_segment import small_model, volume_i16
from test_segdist_cpu import ref_edt_sq, ref_surface, ref_surface_dist
from vit_unet.torch import _lib, functions as F
from vit_unet.torch._lib import check, lib, ptr
from vit_unet.torch.segment import NO_SITE, MaskCleaner, SurfaceDistance, TiledSegmenter, surface_metrics

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPACINGS = [(1, 1, 1), (3, 1, 2)]


@functools.lru_cache(maxsize=None)
def geometry():
    g = [C.c_int(0) for _ in range(3)]
    check(lib().vu_segdist_geometry(*(C.byref(v) for v in g)))
    return tuple(v.value for v in g)                                    # L, C, X


def st():
    return _lib.stream_ptr()


def ends(n, k=3):
    """Sites only in the first and last k positions of a line of n."""
    v = np.zeros(n, dtype=np.uint8)
    v[:k] = 1
    v[-k:] = 1
    return v


# ---------------------------------------------------------------- masks, by name (built once, never changed)
@functools.lru_cache(maxsize=None)
def case(name):
    L, Cc, X = geometry()
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "zeros":
        return np.zeros((2, 9, 13), dtype=np.uint8)
    if name == "ones":
        return np.full((2, 9, 13), 255, dtype=np.uint8)
    if name == "last_corner":
        m = np.zeros((2, 11, 70), dtype=np.uint8)
        m[-1, -1, -1] = 1
        return m
    if name == "opposite_corners":                            # a unit must not see its neighbour's site
        m = np.zeros((2, 10, 15), dtype=np.uint8)
        m[0, 0, 0] = 1
        m[1, -1, -1] = 1
        return m
    if name == "checkerboard":
        yy, xx = np.mgrid[0:9, 0:14]
        return ((yy + xx) % 2).astype(np.uint8)[None]
    if name == "odd_w":
        return (rng.random((3, 37, 45)) < 0.1).astype(np.uint8)
    if name == "w_mod_4":                                     # wider than one trip of the row scan
        return (rng.random((2, 7, X + 8)) < 0.02).astype(np.uint8)
    if name == "small_slice":
        return (rng.random((1, 5, 3)) < 0.4).astype(np.uint8)
    if name == "tall_ends":                                   # the envelope spans the piece boundary
        return np.ascontiguousarray(np.broadcast_to(ends(L + 5)[None, :, None], (1, L + 5, 9)))
    if name == "wide_ends":
        return np.ascontiguousarray(np.broadcast_to(ends(L + 5)[None, None, :], (1, 9, L + 5)))
    if name == "row_ends":                                    # sites on either side of the row scan's trip boundary only
        return np.ascontiguousarray(np.broadcast_to(ends(X + 9)[None, None, :], (1, 3, X + 9)))
    if name == "tall_sparse":                                 # three pieces, more than one group of lines, every piece needed
        return (rng.random((1, 2 * L + 7, Cc + 6)) < 0.004).astype(np.uint8)
    if name == "tall_blob":                                   # three pieces, most of them voted away
        m = np.zeros((1, 2 * L + 7, Cc + 6), dtype=np.uint8)
        yy, xx = np.mgrid[0:2 * L + 7, 0:Cc + 6]
        m[0] = ((yy - L) ** 2 + (xx - 30) ** 2 < 40 ** 2) | ((yy - 5) ** 2 + (xx - 60) ** 2 < 9)
        return m
    if name == "random2":
        return (rng.random((2, 70, 150)) < 0.02).astype(np.uint8)
    if name == "random60":
        return (rng.random((2, 70, 150)) < 0.6).astype(np.uint8) * 3
    # ---- volumes
    if name == "vol_small":
        return (rng.random((2, 9, 11)) < 0.05).astype(np.uint8)
    if name == "vol_odd":
        return (rng.random((5, 37, 45)) < 0.01).astype(np.uint8)
    if name == "vol_deep":                                    # the z line spans the piece boundary
        return np.ascontiguousarray(np.broadcast_to(ends(L + 5)[:, None, None], (L + 5, 3, 5)))
    if name == "vol_deep_one":                                # one site at the far end of a long z line
        m = np.zeros((L + 5, 3, 5), dtype=np.uint8)
        m[-1, 2, 4] = 1
        return m
    if name == "through_z":                                   # slice 0 has a site only in its far corner: most of it is nearer through z
        m = np.zeros((3, 12, 70), dtype=np.uint8)
        m[0, 11, 69] = 1
        m[2, 3, 4] = 1
        return m
    if name == "empty_slice":                                 # slice 1 holds nothing and takes its distances from its neighbours
        m = (rng.random((3, 20, 33)) < 0.05).astype(np.uint8)
        m[1] = 0
        return m
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def edt_ref(name, dims, fg, spacing):
    return ref_edt_sq(case(name), dims, fg, spacing)


def run_edt(mask, dims, fg, spacing):
    """One vu_edt_sq into a sentinel-filled output -> dist2 as int64 (uint32 values), on the host."""
    L = lib()
    D, H, W = mask.shape
    d = torch.from_numpy(mask).to(DEV)
    out = torch.full((D, H, W), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    nbytes = int(L.vu_edt_scratch_bytes(D, H, W, dims))
    scratch = torch.full(((nbytes + 15) // 16 * 4,), -1, dtype=torch.int32, device=DEV)
    check(L.vu_edt_sq(ptr(d), ptr(out), ptr(scratch), nbytes, D, H, W, dims, fg, *spacing, st()), "vu_edt_sq")
    torch.cuda.synchronize()
    assert torch.equal(d.cpu(), torch.from_numpy(mask))                       # the input is left alone
    return out.cpu().numpy().view(np.uint32).astype(np.int64)


SLICE_CASES = ["zeros", "ones", "last_corner", "opposite_corners", "checkerboard", "odd_w", "w_mod_4", "small_slice", "tall_ends",
               "wide_ends", "row_ends", "tall_sparse", "tall_blob", "random2", "random60"]
VOLUME_CASES = ["vol_small", "vol_odd", "vol_deep", "vol_deep_one", "through_z", "empty_slice"]


# ---------------------------------------------------------------- 1. the transform
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("fg", [1, 0])
@pytest.mark.parametrize("name", SLICE_CASES)
def test_edt_slices(name, fg, spacing):
    want = edt_ref(name, 2, fg, spacing)
    got = run_edt(case(name), 2, fg, spacing)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])


def test_edt_known_answers():
    assert (edt_ref("zeros", 2, 1, (1, 1, 1)) == NO_SITE).all() and (edt_ref("zeros", 2, 0, (1, 1, 1)) == 0).all()
    assert (edt_ref("ones", 2, 1, (1, 1, 1)) == 0).all() and (edt_ref("ones", 2, 0, (3, 1, 2)) == NO_SITE).all()
    d = edt_ref("last_corner", 2, 1, (3, 1, 2))
    assert (d[0] == NO_SITE).all() and d[1, 0, 0] == 10 ** 2 + (2 * 69) ** 2 and d[1, -1, -1] == 0
    d = edt_ref("opposite_corners", 2, 1, (1, 1, 1))
    assert d[0, -1, -1] == 9 ** 2 + 14 ** 2 and d[1, 0, 0] == 9 ** 2 + 14 ** 2
    L, _, X = geometry()
    d = edt_ref("tall_ends", 2, 1, (1, 1, 1))
    assert d[0, (L + 5) // 2, 4] == ((L + 5) // 2 - 2) ** 2 and int(d.max()) == ((L + 5) // 2 - 2) ** 2
    d = edt_ref("row_ends", 2, 1, (3, 1, 2))
    assert int(d.max()) == (2 * ((X + 9) // 2 - 2)) ** 2


@pytest.mark.parametrize("name", VOLUME_CASES)
def test_edt_volumes(name):
    for fg, spacing in ((1, (1, 1, 1)), (1, (3, 1, 2)), (0, (1, 1, 1))):
        want = edt_ref(name, 3, fg, spacing)
        got = run_edt(case(name), 3, fg, spacing)
        assert np.array_equal(got, want), (fg, spacing, np.argwhere(got != want)[:5])
    if name == "through_z":
        d = edt_ref(name, 3, 1, (1, 1, 1))
        assert d[0, 3, 4] == 4 and d[0, 3, 4] < edt_ref(name, 2, 1, (1, 1, 1))[0, 3, 4]      # visible only through z
    if name == "empty_slice":
        d3, d2 = edt_ref(name, 3, 1, (1, 1, 1)), edt_ref(name, 2, 1, (1, 1, 1))
        assert (d2[1] == NO_SITE).all() and (d3[1] >= 1).all() and (d3[1] < NO_SITE).all()
        assert np.array_equal(d3[1], np.minimum(d2[0], d2[2]) + 1)


def test_edt_coarse_sz_prefers_the_in_slice_site():
    m = np.zeros((2, 1, 8), dtype=np.uint8)
    m[0, 0, 4] = 1
    m[1, 0, 0] = 1
    assert run_edt(m, 3, 1, (1, 1, 1))[1, 0, 4] == 1
    got = run_edt(m, 3, 1, (5, 1, 1))
    assert got[1, 0, 4] == 16 and np.array_equal(got, ref_edt_sq(m, 3, 1, (5, 1, 1)))


def test_edt_unaligned_buffers():
    """A W % 4 == 0 mask one byte, and a destination one word, off their allocations: the scalar paths of the row pass."""
    m = case("w_mod_4")
    D, H, W = m.shape
    want = edt_ref("w_mod_4", 2, 1, (3, 1, 2))
    nbytes = int(lib().vu_edt_scratch_bytes(D, H, W, 2))
    for moff, doff in ((1, 0), (0, 1), (4, 1), (1, 4)):
        buf = torch.zeros(m.size + moff, dtype=torch.uint8, device=DEV)
        buf[moff:].copy_(torch.from_numpy(m).reshape(-1))
        out = torch.full((m.size + doff + 1,), -7, dtype=torch.int32, device=DEV)
        scratch = torch.full((nbytes // 4 + 1,), -1, dtype=torch.int32, device=DEV)
        check(lib().vu_edt_sq(ptr(buf[moff:]), ptr(out[doff:]), ptr(scratch[1:]), nbytes, D, H, W, 2, 1, 3, 1, 2, st()))
        o = out.cpu().numpy()
        assert (o[:doff] == -7).all() and o[-1] == -7 and int(scratch[0]) == -1
        assert np.array_equal(o[doff:-1].view(np.uint32).astype(np.int64).reshape(m.shape), want), (moff, doff)


# ---------------------------------------------------------------- 2. the surface
def run_surface(mask, dims, label):
    D, H, W = mask.shape
    d = torch.from_numpy(mask).to(DEV)
    out = torch.full((D, H, W), 0xAA, dtype=torch.uint8, device=DEV)
    check(lib().vu_mask_surface(ptr(d), ptr(out), D, H, W, dims, label, st()), "vu_mask_surface")
    return out.cpu().numpy()


def test_mask_surface():
    full = np.ones((2, 5, 6), dtype=np.uint8)
    s = run_surface(full, 2, -1)
    assert np.array_equal(s, ref_surface(full, 2, -1)) and s[:, 1:-1, 1:-1].sum() == 0 and s.sum() == 2 * (30 - 12)
    line = np.zeros((1, 5, 6), dtype=np.uint8)
    line[0, 2, 1:5] = 9
    assert np.array_equal(run_surface(line, 2, -1), (line != 0).astype(np.uint8))
    box = np.zeros((1, 9, 9), dtype=np.uint8)
    box[0, 1:8, 1:8] = 1
    box[0, 3:6, 3:6] = 0
    assert np.array_equal(run_surface(box, 2, -1), ref_surface(box, 2, -1)) and run_surface(box, 2, -1).sum() == 36
    lab = case("random60")                                                   # values 0 and 3
    lab2 = np.where(np.random.default_rng(5).random(lab.shape) < 0.5, lab, 2).astype(np.uint8)
    for label in (-1, 2, 3, 0):
        assert np.array_equal(run_surface(lab2, 2, label), ref_surface(lab2, 2, label)), label
    cube = np.zeros((5, 5, 5), dtype=np.uint8)
    cube[1:4, 1:4, 1:4] = 1
    s3 = run_surface(cube, 3, -1)
    assert np.array_equal(s3, ref_surface(cube, 3, -1)) and s3[2, 2, 2] == 0 and s3.sum() == 26
    slab = np.zeros((4, 5, 5), dtype=np.uint8)
    slab[1:3, 1:4, 1:4] = 1
    assert np.array_equal(run_surface(slab, 3, -1), slab)
    v = case("vol_odd")
    dense = (np.random.default_rng(6).random(v.shape) < 0.8).astype(np.uint8)
    for dims in (2, 3):
        assert np.array_equal(run_surface(dense, dims, -1), ref_surface(dense, dims, -1)), dims


# ---------------------------------------------------------------- 3. the surface distances
def square(shape, z, y0, x0, k):
    m = np.zeros(shape, dtype=np.uint8)
    m[z, y0:y0 + k, x0:x0 + k] = 1
    return m


@functools.lru_cache(maxsize=None)
def pair(name):
    """(pred, truth, dims)"""
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    shape = (1, 40, 70)
    if name == "identical":
        a = (rng.random((2, 30, 41)) < 0.5).astype(np.uint8)
        return a, a.copy(), 2
    if name == "shifted":                                     # 6 x 6 squares: 20 + 20 surface pixels
        return square(shape, 0, 5, 5, 6), square(shape, 0, 8, 9, 6), 2
    if name == "stray":                                       # one stray pixel far from the organ: 21 + 20 surface pixels
        p = square(shape, 0, 5, 5, 6)
        p[0, 38, 68] = 1
        return p, square(shape, 0, 6, 6, 6), 2
    if name == "empties":                                     # prediction empty, truth empty, both empty, both present
        p, t = np.zeros((4, 12, 14), dtype=np.uint8), np.zeros((4, 12, 14), dtype=np.uint8)
        t[0, 2:6, 2:7] = 1
        p[1, 3:9, 3:5] = 1
        p[3, 1:5, 1:5] = 1
        t[3, 3:8, 2:9] = 1
        return p, t, 2
    if name == "empty_pred_volume":
        t = np.zeros((2, 6, 6), dtype=np.uint8)
        t[1, 2:4, 2:4] = 1
        return np.zeros((2, 6, 6), dtype=np.uint8), t, 3
    if name == "random2d":
        yy, xx = np.mgrid[0:70, 0:150]
        blob = ((yy - 35) ** 2 + (xx - 70) ** 2 < 28 ** 2)
        p = np.stack([blob ^ (rng.random((70, 150)) < 0.03), rng.random((70, 150)) < 0.3]).astype(np.uint8)
        t = np.stack([blob, rng.random((70, 150)) < 0.3]).astype(np.uint8) * 2
        t[0][rng.random((70, 150)) < 0.02] = 1                  # a second label inside and around the organ
        return p, t, 2
    if name == "random3d":
        zz, yy, xx = np.mgrid[0:6, 0:37, 0:45]
        blob = ((3 * (zz - 3)) ** 2 + (yy - 18) ** 2 + (xx - 22) ** 2 < 14 ** 2)
        p = (blob ^ (rng.random(blob.shape) < 0.02)).astype(np.uint8)
        t = np.roll(blob, (1, 2, -3), (0, 1, 2)).astype(np.uint8) * 2
        return p, t, 3
    raise KeyError(name)


def run_dist(pred, truth, dims, spacing=(1, 1, 1), label=-1, tol2=1, qnum=19, qden=20, maps=True):
    """One vu_surface_dist into sentinel-filled outputs -> (stats int64, sums, order int64, dist_pt, dist_tp or None)."""
    L = lib()
    D, H, W = pred.shape
    U = 1 if dims == 3 else D
    p, t = torch.from_numpy(pred).to(DEV), torch.from_numpy(truth).to(DEV)
    stats = torch.full((U, 6), -1, dtype=torch.int64, device=DEV)
    sums = torch.full((U, 2), float("nan"), dtype=torch.float64, device=DEV)
    order = torch.full((U, 3, 2), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    dpt = torch.full((D, H, W), 0x5a5a5a5a, dtype=torch.int32, device=DEV) if maps else None
    dtp = torch.full((D, H, W), 0x5a5a5a5a, dtype=torch.int32, device=DEV) if maps else None
    nbytes = int(L.vu_surface_dist_scratch_bytes(D, H, W, dims))
    scratch = torch.full(((nbytes + 15) // 16 * 4,), -1, dtype=torch.int32, device=DEV)
    check(L.vu_surface_dist(ptr(p), ptr(t), ptr(stats), ptr(sums), ptr(order), ptr(dpt), ptr(dtp), ptr(scratch), nbytes, D, H, W, dims,
                            *spacing, label, tol2, qnum, qden, st()), "vu_surface_dist")
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), torch.from_numpy(pred)) and torch.equal(t.cpu(), torch.from_numpy(truth))
    u32 = lambda x: x.cpu().numpy().view(np.uint32).astype(np.int64)
    return (stats.cpu().numpy(), sums.cpu().numpy(), u32(order), u32(dpt) if maps else None, u32(dtp) if maps else None)


def check_dist(got, want):
    stats, sums, order, dpt, dtp = got
    assert np.array_equal(stats, want[0]), (stats, want[0])
    assert np.array_equal(order, want[2]), (order, want[2])
    print("sums", sums.tolist(), want[1].tolist())
    assert np.all(np.abs(sums - want[1]) <= 1e-9 * np.abs(want[1])), (sums, want[1])
    if dpt is not None:
        assert np.array_equal(dpt, want[3]) and np.array_equal(dtp, want[4])


QUANTILES = [(0, 1), (1, 2), (95, 100), (1, 1)]


@pytest.mark.parametrize("name", ["identical", "shifted", "stray", "empties", "empty_pred_volume", "random2d", "random3d"])
def test_surface_dist(name):
    pred, truth, dims = pair(name)
    k = 0
    for (qnum, qden), tol2 in zip(QUANTILES, (0, 4, 4, 0)):
        for spacing in SPACINGS:
            label = 2 if name.startswith("random") and k % 2 else -1        # both truth rules
            want = ref_surface_dist(pred, truth, dims, spacing, label, tol2, qnum, qden)
            got = run_dist(pred, truth, dims, spacing, label, tol2, qnum, qden, maps=k % 3 != 1)
            check_dist(got, want)
            k += 1


def test_surface_dist_known_answers():
    pred, truth, _ = pair("identical")
    stats, sums, order, _, _ = ref_surface_dist(pred, truth, 2, tol2=0)
    assert (stats[:, 2:4] == 0).all() and (sums == 0).all() and (order == 0).all() and np.array_equal(stats[:, 4:6], stats[:, 0:2])
    # frac = (qnum (n - 1) mod qden) / qden: non-zero for the 40 pooled distances of "shifted", zero for the 41 of "stray"
    s40 = ref_surface_dist(*pair("shifted")[:2], 2, qnum=95, qden=100)
    s41 = ref_surface_dist(*pair("stray")[:2], 2, qnum=95, qden=100)
    assert s40[0][0, :2].tolist() == [20, 20] and s41[0][0, :2].tolist() == [21, 20]
    assert (95 * 39) % 100 != 0 and (95 * 40) % 100 == 0 and (1 * 39) % 2 != 0 and (1 * 40) % 2 == 0
    r40, r41 = surface_metrics(*s40[:3], 95, 100), surface_metrics(*s41[:3], 95, 100)
    assert r40["hd"] == 5.0 and r41["hd"] > 40.0 and r41["hd95"] < 3.0        # one stray pixel ruins hd, not hd95
    e = ref_surface_dist(*pair("empties")[:2], 2)
    assert e[0][:, :2].tolist() == [[0, 14], [12, 0], [0, 0], [12, 20]]
    assert e[0][0, 2:].tolist() == [0, NO_SITE, 0, 0] and e[0][1, 2:].tolist() == [NO_SITE, 0, 0, 0] and (e[2][:3] == NO_SITE).all()
    v = ref_surface_dist(*pair("empty_pred_volume")[:2], 3)
    assert v[0].tolist() == [[0, 4, 0, NO_SITE, 0, 0]]


def test_pred_may_be_the_truth_buffer():
    a = pair("identical")[0]
    D, H, W = a.shape
    d = torch.from_numpy(a).to(DEV)
    stats = torch.full((D, 6), -1, dtype=torch.int64, device=DEV)
    sums = torch.full((D, 2), float("nan"), dtype=torch.float64, device=DEV)
    order = torch.full((D, 3, 2), -1, dtype=torch.int32, device=DEV)
    nbytes = int(lib().vu_surface_dist_scratch_bytes(D, H, W, 2))
    scratch = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.int32, device=DEV)
    check(lib().vu_surface_dist(ptr(d), ptr(d), ptr(stats), ptr(sums), ptr(order), None, None, ptr(scratch), nbytes, D, H, W, 2, 1, 1, 1,
                                -1, 0, 19, 20, st()))
    want = ref_surface_dist(a, a, 2, tol2=0)
    assert np.array_equal(stats.cpu().numpy(), want[0]) and (sums.cpu().numpy() == 0).all() and (order.cpu().numpy() == 0).all()


def test_two_runs_are_bit_equal():
    for name, dims in (("random2", 2), ("tall_sparse", 2), ("vol_odd", 3)):
        assert np.array_equal(run_edt(case(name), dims, 1, (3, 1, 2)), run_edt(case(name), dims, 1, (3, 1, 2)))
        assert np.array_equal(run_surface(case(name), dims, -1), run_surface(case(name), dims, -1))
    for name in ("random2d", "random3d", "empties"):
        pred, truth, dims = pair(name)
        a, b = run_dist(pred, truth, dims, (3, 1, 2), -1, 4, 95, 100), run_dist(pred, truth, dims, (3, 1, 2), -1, 4, 95, 100)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))           # sums bit for bit


# ---------------------------------------------------------------- 4. SurfaceDistance
def test_surface_distance_class():
    pred, truth, _ = pair("random2d")
    sd = SurfaceDistance(2, (3, 1, 2), tolerance=2.5, percentile=95)
    want = ref_surface_dist(pred, truth, 2, (3, 1, 2), 2, 6, 19, 20)
    res = sd.score(pred, truth, label=2)
    assert np.array_equal(res["stats"].numpy(), want[0]) and np.array_equal(res["order"].numpy(), want[2])
    ref = surface_metrics(want[0], res["sums"].numpy(), want[2], 19, 20)
    for k in ("hd", "hd95", "hd95_directed", "assd", "nsd", "units"):
        assert res[k] == ref[k], k
    assert res["assd"] == pytest.approx(surface_metrics(*want[:3], 19, 20)["assd"], rel=1e-9)
    d, e = sd.edt(pred), ref_edt_sq(pred, 2, 1, (3, 1, 2))
    assert d.is_cuda and d.dtype == torch.int64 and np.array_equal(d.cpu().numpy(), np.where(e == NO_SITE, -1, e))
    assert np.array_equal(sd.edt(torch.from_numpy(pred[0]).to(DEV), fg=False).cpu().numpy(), ref_edt_sq(pred[:1], 2, 0, (3, 1, 2))[0])
    assert (sd.edt(np.zeros((3, 4), np.uint8)) == -1).all()
    s = sd.surface(truth, label=2)
    assert s.dtype == torch.uint8 and np.array_equal(s.cpu().numpy(), ref_surface(truth, 2, 2))
    assert [np.array_equal(x.cpu().numpy(), ref_surface(pred, 2, -1)) for x in sd.surface([pred, pred])] == [True, True]
    p3, t3, _ = pair("random3d")
    r3 = SurfaceDistance(3, (3, 1, 1)).score(p3, t3)
    w3 = ref_surface_dist(p3, t3, 3, (3, 1, 1), -1, 1, 19, 20)
    assert np.array_equal(r3["stats"].numpy(), w3[0]) and np.array_equal(r3["order"].numpy(), w3[2]) and r3["units"] == 1


# ---------------------------------------------------------------- 5. end to end
def test_segmenter_with_and_without_surface():
    m, _, _ = small_model(torch.float32)
    vol = volume_i16(3, 70, 90, seed=4)
    vol = (vol // 24).astype(np.int16)                                        # inside the window: a mask with structure
    truth = np.zeros(vol.shape, dtype=np.uint8)
    truth[:, 10:50, 20:70] = 1
    kw = dict(overlap=8, batch=8)
    base = TiledSegmenter(m, **kw).score(vol, truth)
    none = TiledSegmenter(m, surface=None, **kw).score(vol, truth)
    assert list(none) == list(base)                                            # key for key ...
    for k in base:                                                             # ... and bit for bit
        assert torch.equal(none[k], base[k]) if torch.is_tensor(base[k]) else none[k] == base[k], k
    raw = base["mask"].cpu().numpy()
    assert 0 < raw.sum() < raw.size
    for sd, cleaner in ((SurfaceDistance(2, (1, 1, 1), tolerance=2.0), None), (SurfaceDistance(3, (4, 1, 1)), None),
                        (SurfaceDistance(2, (1, 2, 2), percentile=50), MaskCleaner(8, min_size=4, keep_largest=True, fill_holes=True))):
        s = TiledSegmenter(m, surface=sd, clean=cleaner, **kw)
        res = s.score(vol, truth)
        mask = res["mask"].cpu().numpy()
        if cleaner is None:
            assert np.array_equal(mask, raw) and set(res) == set(base) | {"surface"} and res["dice"] == base["dice"]
        else:
            assert set(res) == set(base) | {"surface", "stats", "raw_counts"} and torch.equal(res["raw_counts"], base["counts"])
        want = ref_surface_dist(mask, truth, sd.dims, sd.spacing, -1, sd.tol2, sd.qnum, sd.qden)
        got = res["surface"]
        assert np.array_equal(got["stats"].numpy(), want[0]) and np.array_equal(got["order"].numpy(), want[2])
        assert np.all(np.abs(got["sums"].numpy() - want[1]) <= 1e-9 * np.abs(want[1]))
        ref = surface_metrics(want[0], got["sums"].numpy(), want[2], sd.qnum, sd.qden)
        for k in ("hd", "hd95", "hd95_directed", "assd", "nsd", "units"):
            assert got[k] == ref[k], k
        assert F.hd95_tiled(m, [(vol, truth)], surface=sd, clean=cleaner, **kw).tolist() == [got["hd95"]]
        assert F.assd_tiled(m, [(vol, truth)], surface=sd, clean=cleaner, **kw).tolist() == [got["assd"]]
        assert F.nsd_tiled(m, [(vol, truth)], surface=sd, clean=cleaner, **kw).tolist() == [got["nsd"]]
        assert np.array_equal(m.segment(vol, surface=sd, clean=cleaner, **kw).cpu().numpy(), mask)
    assert F.dice_tiled(m, [(vol, truth)], **kw).tolist() == [base["dice"]]


def test_run_segmentation_with_surface(tmp_path):
    from vit_unet.torch.run import run_segmentation
    rng = np.random.default_rng(21)
    vols = [rng.integers(-1500, 1500, (2, 40, 48)).astype(np.int16) for _ in range(4)]
    truths = []
    for k in range(4):
        tr = np.zeros((2, 40, 48), np.uint8)
        tr[:, 5 + k:25 + k, 8:30] = 1
        truths.append(tr)
    res = run_segmentation(vols, truths, n_epochs=1, folds=2, model_string="lite", batch_size=4, im_size=32, crops_per_volume=2,
                           fg=0.5, dtype=torch.float32, folder=str(tmp_path / "models"), seed=1,
                           surface=SurfaceDistance(2, (1, 1, 1), tolerance=2.0))
    assert [len(d) for d in res["dice"]] == [2, 2] and 0.0 <= res["dice_mean"] <= 1.0
    for k in ("hd95", "assd", "nsd"):
        assert [len(d) for d in res[k]] == [2, 2] and k + "_mean" in res and k + "_std" in res
        assert all((d >= 0.0).all() for d in res[k])                           # inf where a slice's mask is empty
    assert all((d <= 1.0).all() for d in res["nsd"])
