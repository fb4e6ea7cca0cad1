"""Surface-distance metrics, host side (no GPU): restatements of csrc/vu_segdist.hip written from the text of
include/vit_unet_amd.h, that tests/test_gpu_segdist.py holds the HIP kernels against; their answers on hand-made masks; the
float64 formulas of segment.surface_metrics against numpy; every VuError of segment.SurfaceDistance and every refusal of the C
entries (fake pointers: the checks run before any launch).

  ref_edt_sq        a separable integer lower envelope (x, then y, then z), itself checked against an all-pairs brute force
  ref_surface       foreground with an axis neighbour in the background or outside the unit
  ref_surface_dist  stats, sums, order and the two maps of vu_surface_dist"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from vit_unet.torch import _lib, functions as F
from vit_unet.torch.segment import NO_SITE, SurfaceDistance, TiledSegmenter, surface_metrics

INF = 1 << 62


def _envelope(g, s, axis):
    """out[i] = min_j g[j] + (s (i - j))^2 along `axis`, int64; INF stays INF."""
    g = np.moveaxis(g, axis, -1)
    L = g.shape[-1]
    i = np.arange(L, dtype=np.int64)
    out = np.full(g.shape, INF, dtype=np.int64)
    for j in range(L):
        out = np.minimum(out, np.minimum(g[..., j:j + 1] + (s * (i - j)) ** 2, INF))
    return np.moveaxis(out, -1, axis)


def ref_edt_sq(mask, dims=2, fg=1, spacing=(1, 1, 1)):
    """(D,H,W) uint8 -> (D,H,W) int64: squared distance to the nearest site of the same unit, NO_SITE in a unit without one."""
    sz, sy, sx = spacing
    site = (mask != 0) if fg else (mask == 0)
    g = np.where(site, 0, INF).astype(np.int64)
    g = _envelope(g, sx, 2)
    g = _envelope(g, sy, 1)
    if dims == 3:
        g = _envelope(g, sz, 0)
    return np.where(g >= INF, NO_SITE, g)


def brute_edt_sq(mask, dims, fg, spacing):
    sz, sy, sx = spacing
    site = (mask != 0) if fg else (mask == 0)
    out = np.full(mask.shape, NO_SITE, dtype=np.int64)
    pts = np.argwhere(site)
    for z, y, x in itertools.product(*(range(n) for n in mask.shape)):
        p = pts if dims == 3 else pts[pts[:, 0] == z]
        if len(p):
            out[z, y, x] = (((p[:, 0] - z) * sz) ** 2 + ((p[:, 1] - y) * sy) ** 2 + ((p[:, 2] - x) * sx) ** 2).min()
    return out


def ref_fg(mask, label):
    return (mask != 0) if label < 0 else (mask == label)


def ref_surface(mask, dims=2, label=-1):
    f = ref_fg(mask, label)
    p = np.pad(f, 1)                                                   # outside the unit counts as background
    inner = p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1]
    if dims == 3:
        inner = inner & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1]
    return (f & ~inner).astype(np.uint8)


def ref_order(values, qnum, qden):
    n = len(values)
    v = np.sort(np.asarray(values, dtype=np.int64))
    lo = (qnum * (n - 1)) // qden
    return [int(v[lo]), int(v[min(lo + 1, n - 1)])]


def ref_surface_dist(pred, truth, dims=2, spacing=(1, 1, 1), label=-1, tol2=1, qnum=19, qden=20):
    """-> stats (U,6) int64, sums (U,2) float64, order (U,3,2) int64, dist_pt, dist_tp (D,H,W) int64."""
    sp, st = ref_surface(pred, dims, -1), ref_surface(truth, dims, label)
    to_t, to_p = ref_edt_sq(st, dims, 1, spacing), ref_edt_sq(sp, dims, 1, spacing)
    units = [slice(None)] if dims == 3 else [slice(z, z + 1) for z in range(pred.shape[0])]
    stats, sums, order = [], [], []
    for u in units:
        dpt, dtp = to_t[u][sp[u] != 0], to_p[u][st[u] != 0]
        n_p, n_t = len(dpt), len(dtp)
        if n_p == 0 or n_t == 0:
            stats.append([n_p, n_t, NO_SITE if n_p else 0, NO_SITE if n_t else 0, 0, 0])
            sums.append([0.0, 0.0])
            order.append([[NO_SITE] * 2] * 3)
            continue
        stats.append([n_p, n_t, int(dpt.max()), int(dtp.max()), int((dpt <= tol2).sum()), int((dtp <= tol2).sum())])
        sums.append([float(np.sqrt(dpt.astype(np.float64)).sum()), float(np.sqrt(dtp.astype(np.float64)).sum())])
        order.append([ref_order(dpt, qnum, qden), ref_order(dtp, qnum, qden), ref_order(np.concatenate([dpt, dtp]), qnum, qden)])
    return (np.array(stats, dtype=np.int64), np.array(sums, dtype=np.float64), np.array(order, dtype=np.int64).reshape(-1, 3, 2),
            to_t, to_p)


# ---------------------------------------------------------------- the restatements themselves
@pytest.mark.parametrize("spacing", [(1, 1, 1), (3, 1, 2)])
@pytest.mark.parametrize("fg", [1, 0])
@pytest.mark.parametrize("dims", [2, 3])
def test_ref_edt_equals_all_pairs_brute_force(dims, fg, spacing):
    rng = np.random.default_rng(dims * 10 + fg)
    for shape, p in (((4, 12, 12), 0.05), ((3, 7, 11), 0.5), ((2, 5, 3), 0.9), ((4, 6, 6), 0.0)):
        m = (rng.random(shape) < p).astype(np.uint8) * 7
        if p == 0.05:
            m[1] = 0                                                   # a slice without a foreground pixel inside a volume that has some
        assert np.array_equal(ref_edt_sq(m, dims, fg, spacing), brute_edt_sq(m, dims, fg, spacing))


def test_edt_single_site_and_units():
    m = np.zeros((2, 5, 6), dtype=np.uint8)
    m[0, 1, 2] = 1
    d = ref_edt_sq(m, 2, 1)
    yy, xx = np.mgrid[0:5, 0:6]
    assert np.array_equal(d[0], (yy - 1) ** 2 + (xx - 2) ** 2)
    assert (d[1] == NO_SITE).all()                                     # a unit does not see its neighbour's site
    d3 = ref_edt_sq(m, 3, 1)
    assert np.array_equal(d3[1], d[0] + 1)
    # anisotropic (sz, sy, sx) = (3, 1, 2)
    a = ref_edt_sq(m, 3, 1, (3, 1, 2))
    assert np.array_equal(a[0], (yy - 1) ** 2 + (2 * (xx - 2)) ** 2) and np.array_equal(a[1], a[0] + 9)
    assert a[1, 1, 2] == 9 and a[0, 4, 5] == 9 + 36
    # fg = 0: the sites are the background
    b = ref_edt_sq(m, 2, 0)
    assert b[0, 1, 2] == 1 and b[0].sum() == 1 and (b[1] == 0).all()
    assert (ref_edt_sq(np.ones((1, 3, 3), np.uint8), 2, 0) == NO_SITE).all()


def test_in_slice_site_wins_over_the_nearer_slice_at_a_coarse_sz():
    m = np.zeros((2, 1, 8), dtype=np.uint8)
    m[0, 0, 4] = 1                                                     # directly below (1, 0, 4): one slice away
    m[1, 0, 0] = 1                                                     # four pixels away in the slice
    assert ref_edt_sq(m, 3, 1, (1, 1, 1))[1, 0, 4] == 1
    assert ref_edt_sq(m, 3, 1, (5, 1, 1))[1, 0, 4] == 16               # sz = 5: 25 > 16, the in-slice site wins


def test_surface_rule():
    full = np.ones((1, 5, 6), dtype=np.uint8)
    s = ref_surface(full)
    assert s[0, 1:-1, 1:-1].sum() == 0 and s.sum() == 5 * 6 - 3 * 4    # only the frame
    line = np.zeros((1, 5, 6), dtype=np.uint8)
    line[0, 2, 1:5] = 1
    assert np.array_equal(ref_surface(line), line)
    box = np.zeros((1, 9, 9), dtype=np.uint8)
    box[0, 1:8, 1:8] = 1
    box[0, 3:6, 3:6] = 0
    s = ref_surface(box)[0]
    assert s[1, 1:8].all() and s[2, 3:6].all() and s[2, 1] == 1 and s[2, 2] == 0 and s[4, 4] == 0 and s.sum() == 24 + 16 - 4
    lab = np.array([[[1, 2, 2, 2, 1], [1, 2, 2, 2, 1], [1, 2, 2, 2, 1]]], dtype=np.uint8)
    assert ref_surface(lab, 2, -1).sum() == 12 and ref_surface(lab, 2, 2)[0, 1].tolist() == [0, 1, 0, 1, 0]
    cube = np.zeros((5, 5, 5), dtype=np.uint8)
    cube[1:4, 1:4, 1:4] = 1
    assert ref_surface(cube, 3).sum() == 26 and ref_surface(cube, 3)[2, 2, 2] == 0 and ref_surface(cube, 2)[2].sum() == 8
    slab = np.zeros((4, 5, 5), dtype=np.uint8)
    slab[1:3, 1:4, 1:4] = 1
    assert np.array_equal(ref_surface(slab, 3), slab)                  # 3 x 3 x 2: all surface


def test_two_squares_and_a_shifted_square():
    a = np.zeros((1, 20, 30), dtype=np.uint8)
    b = np.zeros((1, 20, 30), dtype=np.uint8)
    a[0, 5:10, 3:8] = 1
    b[0, 5:10, 17:22] = 1                                              # the same square 14 to the right
    stats, sums, order, _, _ = ref_surface_dist(a, b, tol2=0, qnum=1, qden=1)
    assert stats[0, :2].tolist() == [16, 16]
    assert stats[0, 2] == stats[0, 3] == 14 ** 2                       # the far edge of one to the near edge of the other
    assert stats[0, 4] == stats[0, 5] == 0 and order[0, 2].tolist() == [196, 196]
    res = surface_metrics(stats, sums, order, 1, 1)
    assert res["hd"] == 14.0 and res["hd95"] == 14.0 and res["nsd"] == 0.0 and res["units"] == 1
    c = np.zeros((1, 20, 30), dtype=np.uint8)
    c[0, 5 + 3:10 + 3, 3 + 4:8 + 4] = 1                                # shifted by (3, 4)
    stats, sums, order, _, _ = ref_surface_dist(a, c, tol2=4)
    res = surface_metrics(stats, sums, order, 19, 20)
    assert res["hd"] == 5.0 and res["hd95_directed"] <= 5.0 and 0.0 < res["assd"] < 5.0 and 0.0 < res["nsd"] < 1.0
    # anisotropic: the same pair at (sz, sy, sx) = (3, 1, 2): the corner moves by (3, 2 * 4)
    stats, sums, order, _, _ = ref_surface_dist(a, c, spacing=(3, 1, 2))
    assert surface_metrics(stats, sums, order, 19, 20)["hd"] == math.sqrt(9 + 64)
    # identical masks: all zeros, nsd 1
    stats, sums, order, _, _ = ref_surface_dist(a, a, tol2=0)
    res = surface_metrics(stats, sums, order, 19, 20)
    assert (res["hd"], res["hd95"], res["assd"], res["nsd"]) == (0.0, 0.0, 0.0, 1.0) and sums.sum() == 0.0


def test_empty_units():
    a = np.zeros((4, 6, 6), dtype=np.uint8)
    t = np.zeros((4, 6, 6), dtype=np.uint8)
    a[0, 2:4, 2:4] = 1                                                  # prediction only
    t[1, 2:4, 2:4] = 1                                                  # truth only
    a[3, 1:3, 1:3] = 1                                                  # unit 2: both empty; unit 3: both
    t[3, 2:4, 2:4] = 1
    stats, sums, order, _, _ = ref_surface_dist(a, t)
    assert stats[0].tolist() == [4, 0, NO_SITE, 0, 0, 0] and stats[1].tolist() == [0, 4, 0, NO_SITE, 0, 0]
    assert stats[2].tolist() == [0] * 6 and (order[:3] == NO_SITE).all() and (sums[:3] == 0).all()
    res = surface_metrics(stats, sums, order, 19, 20)
    assert res["units"] == 3 and res["hd"] == math.inf and res["assd"] == math.inf and res["nsd"] == pytest.approx(res["nsd_units"][3] / 3)
    assert res["hd_units"][:3].tolist() == [math.inf, math.inf, 0.0] and res["nsd_units"][:3].tolist() == [0.0, 0.0, 1.0]
    assert res["hd_units"][3] == math.sqrt(2)
    only = surface_metrics(stats[2:3], sums[2:3], order[2:3], 19, 20)
    assert (only["hd"], only["hd95"], only["assd"], only["nsd"], only["units"]) == (0.0, 0.0, 0.0, 1.0, 0)


# ---------------------------------------------------------------- the float64 formulas against numpy
@pytest.mark.parametrize("q", [(0, 1), (1, 2), (19, 20), (1, 1), (999, 1000)])
def test_surface_metrics_against_numpy(q):
    qnum, qden = q
    rng = np.random.default_rng(qnum + qden)
    stats, sums, order, sets = [], [], [], []
    for n_p, n_t in ((21, 20), (41, 40), (7, 1), (300, 513)):          # 19 (n - 1) mod 20 is zero for n = 41 and for n = 81 pooled
        dpt, dtp = rng.integers(0, 5000, n_p), rng.integers(0, 5000, n_t)
        sets.append((dpt, dtp))
        stats.append([n_p, n_t, dpt.max(), dtp.max(), (dpt <= 100).sum(), (dtp <= 100).sum()])
        sums.append([np.sqrt(dpt.astype(np.float64)).sum(), np.sqrt(dtp.astype(np.float64)).sum()])
        order.append([ref_order(dpt, qnum, qden), ref_order(dtp, qnum, qden), ref_order(np.concatenate([dpt, dtp]), qnum, qden)])
    res = surface_metrics(np.array(stats), np.array(sums), np.array(order), qnum, qden)
    pct = 100.0 * qnum / qden
    for u, (dpt, dtp) in enumerate(sets):
        both = np.sqrt(np.concatenate([dpt, dtp]).astype(np.float64))
        assert res["hd_units"][u] == pytest.approx(both.max(), rel=1e-12)
        assert res["hd95_units"][u] == pytest.approx(np.percentile(both, pct, method="linear"), rel=1e-12)
        directed = max(np.percentile(np.sqrt(dpt.astype(np.float64)), pct, method="linear"),
                       np.percentile(np.sqrt(dtp.astype(np.float64)), pct, method="linear"))
        assert res["hd95_directed_units"][u] == pytest.approx(directed, rel=1e-12)
        assert res["assd_units"][u] == pytest.approx(both.mean(), rel=1e-12)
        assert res["nsd_units"][u] == pytest.approx((both <= 10.0).mean(), rel=1e-12)
    assert res["units"] == 4 and res["hd95"] == pytest.approx(res["hd95_units"].mean(), rel=1e-12)
    with pytest.raises(_lib.VuError, match="quantile"):
        surface_metrics(np.array(stats), np.array(sums), np.array(order), 3, 2)
    with pytest.raises(_lib.VuError, match="units"):
        surface_metrics(np.array(stats), np.array(sums)[:2], np.array(order), 1, 2)


# ---------------------------------------------------------------- argument errors, before any GPU call
def test_surface_distance_constructor():
    for bad in (1, 4, "2", None, True):
        with pytest.raises(_lib.VuError, match="dims"):
            SurfaceDistance(dims=bad)
    for bad in ((1, 1), (1, 1, 0), (1.5, 1, 1), (1, -2, 1), 3, (True, 1, 1), "abc"):
        with pytest.raises(_lib.VuError, match="spacing"):
            SurfaceDistance(spacing=bad)
    for bad in (-0.5, math.inf, math.nan, "1", None):
        with pytest.raises(_lib.VuError, match="tolerance"):
            SurfaceDistance(tolerance=bad)
    for bad in (-1, 100.5, math.nan, "95", None):
        with pytest.raises(_lib.VuError, match="percentile"):
            SurfaceDistance(percentile=bad)
    sd = SurfaceDistance(3, (np.int64(3), 1, 2), tolerance=2.5, percentile=99.9)
    assert (sd.dims, sd.spacing, sd.tol2, sd.qnum, sd.qden) == (3, (3, 1, 2), 6, 999, 1000)
    d = SurfaceDistance()
    assert (d.dims, d.spacing, d.tol2, d.qnum, d.qden) == (2, (1, 1, 1), 1, 19, 20)
    assert (SurfaceDistance(percentile=100).qnum, SurfaceDistance(percentile=100).qden) == (1, 1)
    assert (SurfaceDistance(percentile=0).qnum, SurfaceDistance(percentile=50).qden) == (0, 2)


def test_surface_distance_call_errors():
    sd = SurfaceDistance()
    u8 = np.zeros((4, 4), dtype=np.uint8)
    for call in (sd.edt, sd.surface, lambda m: sd.score(m, u8)):
        with pytest.raises(_lib.VuError, match="uint8"):
            call(np.zeros((4, 4), dtype=np.int16))
        with pytest.raises(_lib.VuError, match="uint8"):
            call(np.zeros((1, 2, 4, 4), dtype=np.uint8))
        with pytest.raises(_lib.VuError, match="empty"):
            call(np.zeros((0, 4), dtype=np.uint8))
    for vol in (u8, u8[None]):
        for call in (SurfaceDistance(3).edt, SurfaceDistance(3).surface, lambda m: SurfaceDistance(3).score(m, m)):
            with pytest.raises(_lib.VuError, match="needs a"):
                call(vol)
    with pytest.raises(_lib.VuError, match="shape"):
        sd.score(u8, np.zeros((4, 5), dtype=np.uint8))
    with pytest.raises(_lib.VuError, match="uint8"):
        sd.score(u8, np.zeros((4, 4), dtype=np.int32))
    with pytest.raises(_lib.VuError, match="label"):
        sd.score(u8, u8, label=256)
    with pytest.raises(_lib.VuError, match="label"):
        sd.surface(u8, label=300)
    with pytest.raises(_lib.VuError, match="largest squared distance"):
        SurfaceDistance(spacing=(1, 40000, 1)).edt(np.zeros((3, 3), dtype=np.uint8))
    with pytest.raises(_lib.VuError, match="largest squared distance"):
        SurfaceDistance(3, spacing=(30000, 1, 1)).score(np.zeros((3, 3, 3), np.uint8), np.zeros((3, 3, 3), np.uint8))


class _Model:
    im_size, num_channels = 32, 1


def test_pass_through_argument_errors():
    with pytest.raises(_lib.VuError, match="SurfaceDistance"):
        TiledSegmenter(_Model(), overlap=8, surface="hd95")
    s = TiledSegmenter(_Model(), overlap=8, surface=SurfaceDistance(3))
    assert TiledSegmenter(_Model(), overlap=8).surface is None and s.surface.dims == 3
    with pytest.raises(_lib.VuError, match="needs a"):
        s.score(np.zeros((1, 40, 40), dtype=np.int16), np.zeros((1, 40, 40), dtype=np.uint8))
    for fn in (F.hd95_tiled, F.assd_tiled, F.nsd_tiled):
        with pytest.raises(_lib.VuError, match="SurfaceDistance"):
            fn(_Model(), [], overlap=8)


def _rc(fn, *a):
    rc = fn(*a)
    return rc, _lib.lib().vu_last_error().decode()


def test_c_entry_argument_errors():
    """Every refusal of the header, with fake (never dereferenced) pointers: the checks run before any launch."""
    L = _lib.lib()
    g = [C.c_int(0) for _ in range(3)]
    assert L.vu_segdist_geometry(*(C.byref(v) for v in g)) == 0 and all(v.value > 0 for v in g) and g[2].value % 4 == 0
    assert L.vu_segdist_geometry(None, C.byref(g[1]), C.byref(g[2])) == -1
    D, H, W = 2, 8, 12
    N = D * H * W
    P = 1 << 20                                   # distinct, aligned, non-overlapping fake addresses
    mask, dist2, scratch, surf, truth, stats, sums, order, dpt, dtp = (C.c_void_p(P * (i + 1)) for i in range(10))
    need = L.vu_edt_scratch_bytes(D, H, W, 2)
    assert need >= 4 * N and L.vu_edt_scratch_bytes(0, H, W, 2) == 0 and L.vu_edt_scratch_bytes(D, H, W, 4) == 0
    assert L.vu_edt_scratch_bytes(2048, 1024, 1024, 2) == 0

    def edt(mask=mask, dist2=dist2, scratch=scratch, nbytes=need, D=D, H=H, W=W, dims=2, fg=1, sp=(1, 1, 1)):
        return _rc(L.vu_edt_sq, mask, dist2, scratch, nbytes, D, H, W, dims, fg, *sp, None)

    shape_errors = [(dict(dims=1), "dims"), (dict(dims=4), "dims"), (dict(dims=3, D=1), "single slice"),
                    (dict(D=0), "empty"), (dict(H=-1), "empty"), (dict(W=0), "empty"), (dict(D=2048, H=1024, W=1024), "2^31")]
    spacing_errors = [(dict(sp=(0, 1, 1)), "spacing"), (dict(sp=(1, -1, 1)), "spacing"), (dict(sp=(1, 1, 0)), "spacing"),
                      (dict(sp=(1, 1, 4213)), "squared distance"),          # (4213 * 11)^2 > 2^31 - 1
                      (dict(sp=(1, 6620, 27)), "squared distance"),         # (6620 * 7)^2 = 46340^2 fits, with (27 * 11)^2 it does not ...
                      (dict(sp=(46341, 1, 1), dims=3), "squared distance"),
                      (dict(H=40000, W=40000, D=1), "squared distance")]
    for kw, text in shape_errors + spacing_errors + [
            (dict(fg=2), "fg"), (dict(fg=-1), "fg"),
            (dict(mask=None), "null"), (dict(dist2=None), "null"), (dict(scratch=None), "null"),
            (dict(nbytes=need - 1), "scratch"), (dict(scratch=C.c_void_p(P * 3 + 2)), "scratch"),
            (dict(dist2=C.c_void_p(P * 2 + 2)), "aligned"),
            (dict(dist2=C.c_void_p(P + 4)), "overlap"), (dict(scratch=C.c_void_p(P * 2 + 8)), "overlap"),
            (dict(scratch=C.c_void_p(P - 8)), "overlap")]:
        rc, msg = edt(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    # ... and the sz term is left out for dims 2: the same spacing passes the checks up to the null scratch
    rc, msg = edt(sp=(46341, 1, 1), scratch=None)
    assert rc == -1 and "null" in msg
    rc, msg = edt(sp=(1, 6620, 26), scratch=None)               # ... and with (26 * 11)^2 it still does
    assert rc == -1 and "null" in msg

    def surface(mask=mask, surf=surf, D=D, H=H, W=W, dims=2, label=-1):
        return _rc(L.vu_mask_surface, mask, surf, D, H, W, dims, label, None)

    for kw, text in shape_errors + [(dict(label=256), "label"), (dict(mask=None), "null"), (dict(surf=None), "null"),
                                    (dict(surf=C.c_void_p(P + 5)), "overlap")]:
        rc, msg = surface(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)

    need = L.vu_surface_dist_scratch_bytes(D, H, W, 2)
    assert need >= 14 * N and L.vu_surface_dist_scratch_bytes(D, 0, W, 2) == 0 and L.vu_surface_dist_scratch_bytes(D, H, W, 0) == 0
    scr = C.c_void_p(P * 16)

    def dist(pred=mask, truth=truth, stats=stats, sums=sums, order=order, dpt=dpt, dtp=dtp, scratch=scr, nbytes=need, D=D, H=H, W=W,
             dims=2, sp=(1, 1, 1), label=-1, tol2=1, qnum=19, qden=20):
        return _rc(L.vu_surface_dist, pred, truth, stats, sums, order, dpt, dtp, scratch, nbytes, D, H, W, dims, *sp, label, tol2,
                   qnum, qden, None)

    for kw, text in shape_errors + spacing_errors + [
            (dict(label=256), "label"), (dict(qden=0), "quantile"), (dict(qnum=21), "quantile"), (dict(qnum=1, qden=1000001), "quantile"),
            (dict(pred=None), "null"), (dict(truth=None), "null"), (dict(stats=None), "null"), (dict(sums=None), "null"),
            (dict(order=None), "null"), (dict(scratch=None), "null"),
            (dict(nbytes=need - 1), "scratch"), (dict(scratch=C.c_void_p(P * 16 + 8)), "scratch"),
            (dict(stats=C.c_void_p(P * 6 + 4)), "aligned"), (dict(sums=C.c_void_p(P * 7 + 4)), "aligned"),
            (dict(order=C.c_void_p(P * 8 + 2)), "aligned"), (dict(dpt=C.c_void_p(P * 9 + 1)), "aligned"),
            (dict(truth=C.c_void_p(P + 1)), "overlap"), (dict(stats=C.c_void_p(P + 8)), "overlap"),
            (dict(order=C.c_void_p(P * 7 + 8)), "overlap"), (dict(dtp=C.c_void_p(P * 9 + 16)), "overlap"),
            (dict(dpt=C.c_void_p(P * 5 + 4)), "overlap"), (dict(scratch=C.c_void_p(P * 10 + 16)), "overlap"),
            (dict(sums=C.c_void_p(P * 16 + 64)), "overlap")]:
        rc, msg = dist(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
