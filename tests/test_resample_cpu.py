"""Host side of volume resampling (csrc/vu_resample.hip, segment.VolumeResampler): the numpy restatements the GPU tests compare
against, checked on their own, plus everything that needs no GPU.

  ref_axis_linear / ref_axis_nearest   the tables of include/vit_unet_amd.h written with fractions.Fraction, against the host
                                       entries vu_resample_axis_linear / _nearest
  ref_resample_i16 / _u8 / _f32        staged restatements (x, then y, then z), int64 and float32 operations one at a time
The int16 restatement is held against scipy.ndimage.zoom(order=1, mode="nearest", grid_mode=True) in float64 within 4.5: three
stages of at most half a unit of rounding each, and a weight that is off by at most 2^-16 on a difference of at most 65535 in each
of the three stages (1.5 + 3 * 65535 / 65536 < 4.5).  The float32 restatement within 3 * 2^-16 * (max - min) (the same weight
quantisation) plus 1e-6 of the largest magnitude (a handful of float32 roundings).  The nearest restatement equals zoom(order=0,
grid_mode=True) wherever a coordinate is no tie - at a tie this definition takes the upper sample - and two cases are written
out by hand.  Then VolumeResampler.out_shape, every VuError and every refusal of the C entries (fake pointers: the checks run
before any launch)."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from vit_unet.torch import _lib
from vit_unet.torch._lib import VuError
from vit_unet.torch.segment import TiledSegmenter, VolumeResampler

Q = 1 << 15
AXIS_PAIRS = [(a, b) for a in range(1, 41) for b in range(1, 41)] + [(512, 307), (307, 512), (3, 1000)]
SHAPES = [((5, 7, 9), (7, 5, 13)), ((3, 64, 64), (3, 3, 100)), ((4, 33, 17), (9, 33, 40)), ((1, 6, 6), (1, 9, 4)), ((2, 1, 5), (3, 4, 1))]


# ---------------------------------------------------------------- restatements
def ref_axis_linear(n_in, n_out):
    """(i0, w) int64 arrays: position ((2 i + 1) n_in - n_out) / (2 n_out), edges replicated, w = round-half-up(Q frac)."""
    i0, w = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64)
    for i in range(n_out):
        pos = Fraction((2 * i + 1) * n_in - n_out, 2 * n_out)
        if pos <= 0:
            continue
        k = math.floor(pos)
        if k >= n_in - 1:
            i0[i] = n_in - 1
            continue
        i0[i], w[i] = k, math.floor(Q * (pos - k) + Fraction(1, 2))
    return i0, w


def ref_axis_nearest(n_in, n_out):
    return np.array([math.floor(Fraction((2 * i + 1) * n_in, 2 * n_out)) for i in range(n_out)], dtype=np.int64)


def _taps(v, axis, n_out):
    n_in = v.shape[axis]
    i0, w = ref_axis_linear(n_in, n_out)
    i1 = np.minimum(i0 + 1, n_in - 1)
    shape = [1, 1, 1]
    shape[axis] = n_out
    return np.take(v, i0, axis=axis), np.take(v, i1, axis=axis), w.reshape(shape)


def ref_resample_i16(vol, oshape):
    """Staged x, y, z in int64; a stage is (a (Q - w) + b w + Q / 2) >> 15 and its result an int16 value."""
    v = np.asarray(vol).astype(np.int64)
    for axis in (2, 1, 0):
        a, b, w = _taps(v, axis, oshape[axis])
        v = (a * (Q - w) + b * w + Q // 2) >> 15
        assert v.min() >= -32768 and v.max() <= 32767
    return v.astype(np.int16)


def ref_resample_f32(z, oshape):
    """Staged x, y, z in float32; a stage is a + (b - a) * wf, each operation rounded to float32 on its own, wf = w / Q exactly."""
    v = np.asarray(z, dtype=np.float32)
    for axis in (2, 1, 0):
        a, b, w = _taps(v, axis, oshape[axis])
        wf = w.astype(np.float32) / np.float32(Q)
        assert np.array_equal(wf.astype(np.float64) * Q, w)
        d = (b - a).astype(np.float32)
        t = (d * wf).astype(np.float32)
        v = (a + t).astype(np.float32)
    return v


def ref_resample_u8(mask, oshape):
    m = np.asarray(mask)
    sz, sy, sx = (ref_axis_nearest(n, o) for n, o in zip(m.shape, oshape))
    return np.ascontiguousarray(m[np.ix_(sz, sy, sx)])


def ref_mask_counts(z, truth, zthr, label):
    """mask = z >= zthr; counts (D,3) int64: mask pixels, truth pixels, both, per slice."""
    m = (z >= np.float32(zthr)).astype(np.uint8)
    t = (truth != 0) if label < 0 else (truth == label)
    counts = np.stack([m.sum((1, 2)), t.sum((1, 2)), (m.astype(bool) & t).sum((1, 2))], axis=1).astype(np.int64)
    return m, counts


# ---------------------------------------------------------------- tables
def c_axis_linear(n_in, n_out, capacity=None):
    cap = n_out if capacity is None else capacity
    i0, w = (C.c_int * max(cap, 1))(), (C.c_int * max(cap, 1))()
    rc = _lib.lib().vu_resample_axis_linear(n_in, n_out, i0, w, cap)
    return rc, np.array(i0[:max(rc, 0)], dtype=np.int64), np.array(w[:max(rc, 0)], dtype=np.int64)


def c_axis_nearest(n_in, n_out, capacity=None):
    cap = n_out if capacity is None else capacity
    src = (C.c_int * max(cap, 1))()
    rc = _lib.lib().vu_resample_axis_nearest(n_in, n_out, src, cap)
    return rc, np.array(src[:max(rc, 0)], dtype=np.int64)


def test_axis_tables_match_the_host_entries():
    for n_in, n_out in AXIS_PAIRS:
        i0, w = ref_axis_linear(n_in, n_out)
        rc, ci0, cw = c_axis_linear(n_in, n_out)
        assert rc == n_out and np.array_equal(ci0, i0) and np.array_equal(cw, w), (n_in, n_out)
        assert w.min() >= 0 and w.max() <= Q and i0.min() >= 0 and i0.max() <= n_in - 1
        assert (w[i0 == n_in - 1] == 0).all()
        if n_in == n_out:
            assert np.array_equal(i0, np.arange(n_in)) and not w.any()
        src = ref_axis_nearest(n_in, n_out)
        rc, csrc = c_axis_nearest(n_in, n_out)
        assert rc == n_out and np.array_equal(csrc, src), (n_in, n_out)
        assert src.min() >= 0 and src.max() <= n_in - 1 and (np.diff(src) >= 0).all()
        if n_in == n_out:
            assert np.array_equal(src, np.arange(n_in))


def test_axis_tables_by_hand():
    assert ref_axis_nearest(2, 5).tolist() == [0, 0, 1, 1, 1] and ref_axis_nearest(5, 2).tolist() == [1, 3]
    i0, w = ref_axis_linear(2, 4)                       # positions -0.25, 0.25, 0.75, 1.25
    assert i0.tolist() == [0, 0, 0, 1] and w.tolist() == [0, Q // 4, 3 * Q // 4, 0]
    i0, w = ref_axis_linear(4, 2)                       # positions 0.5, 2.5
    assert i0.tolist() == [0, 2] and w.tolist() == [Q // 2, Q // 2]
    i0, w = ref_axis_linear(1, 3)
    assert i0.tolist() == [0, 0, 0] and w.tolist() == [0, 0, 0]


def test_axis_entries_refuse():
    L = _lib.lib()
    buf = (C.c_int * 8)()
    for rc in (L.vu_resample_axis_linear(0, 4, buf, buf, 8), L.vu_resample_axis_linear(4, 0, buf, buf, 8),
               L.vu_resample_axis_linear(4, 8, None, buf, 8), L.vu_resample_axis_linear(4, 8, buf, None, 8),
               L.vu_resample_axis_linear(4, 8, buf, buf, 7), L.vu_resample_axis_nearest(-1, 4, buf, 8),
               L.vu_resample_axis_nearest(4, 0, buf, 8), L.vu_resample_axis_nearest(4, 8, None, 8),
               L.vu_resample_axis_nearest(4, 8, buf, 7)):
        assert rc == -1 and L.vu_last_error().decode()


# ---------------------------------------------------------------- restatements against scipy
def zoom(v, oshape, order):
    from scipy import ndimage
    out = ndimage.zoom(v, [o / n for o, n in zip(oshape, v.shape)], order=order, mode="nearest", grid_mode=True)
    assert out.shape == tuple(oshape)
    return out


@pytest.mark.parametrize("ishape,oshape", SHAPES)
def test_i16_restatement_against_zoom(ishape, oshape):
    vol = np.random.default_rng(sum(ishape) + 7 * sum(oshape)).integers(-32768, 32768, ishape).astype(np.int16)
    vol.reshape(-1)[:2] = (-32768, 32767)
    got = ref_resample_i16(vol, oshape)
    assert got.dtype == np.int16 and got.shape == tuple(oshape)
    err = np.abs(got.astype(np.float64) - zoom(vol.astype(np.float64), oshape, 1)).max()
    print(f"int16 {ishape} -> {oshape}: max |restatement - zoom| = {err:.3f}")
    assert err <= 4.5
    assert np.array_equal(ref_resample_i16(vol, ishape), vol)                      # the identity is exact
    c = np.full(ishape, -32768, np.int16)
    assert (ref_resample_i16(c, oshape) == -32768).all() and (ref_resample_i16(-(c + 1), oshape) == 32767).all()


@pytest.mark.parametrize("ishape,oshape", SHAPES)
def test_f32_restatement_against_zoom(ishape, oshape):
    z = (np.random.default_rng(sum(ishape) + 3 * sum(oshape)).standard_normal(ishape) * 4).astype(np.float32)
    got = ref_resample_f32(z, oshape)
    assert got.dtype == np.float32 and got.shape == tuple(oshape)
    tol = 3 * 2.0 ** -16 * float(z.max() - z.min()) + 1e-6 * float(np.abs(z).max())
    err = np.abs(got.astype(np.float64) - zoom(z.astype(np.float64), oshape, 1)).max()
    print(f"float32 {ishape} -> {oshape}: max |restatement - zoom| = {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    assert np.array_equal(ref_resample_f32(z, ishape), z)


@pytest.mark.parametrize("ishape,oshape", SHAPES)
def test_u8_restatement_against_zoom(ishape, oshape):
    m = np.random.default_rng(sum(ishape) + sum(oshape)).integers(0, 256, ishape).astype(np.uint8)
    got = ref_resample_u8(m, oshape)
    assert got.dtype == np.uint8 and got.shape == tuple(oshape) and set(np.unique(got)) <= set(np.unique(m))
    want = zoom(m, oshape, 0)
    # the two conventions agree wherever the source coordinate is no tie between two samples
    keep = [np.array([((2 * i + 1) * n) % (2 * o) != 0 for i in range(o)]) for n, o in zip(ishape, oshape)]
    sel = np.ix_(*keep)
    assert sum(k.sum() for k in keep) > 0 and np.array_equal(got[sel], want[sel])
    assert np.array_equal(ref_resample_u8(m, ishape), m)


def test_u8_by_hand():
    row = np.array([[[10, 20]]], dtype=np.uint8)
    assert ref_resample_u8(row, (1, 1, 5)).reshape(-1).tolist() == [10, 10, 20, 20, 20]
    row = np.array([[[1, 2, 3, 4, 5]]], dtype=np.uint8)
    assert ref_resample_u8(row, (1, 1, 2)).reshape(-1).tolist() == [2, 4]


def test_mask_counts_restatement():
    z = np.array([[[-1.0, 0.0, 0.5], [2.0, -0.0, -3.0]]], dtype=np.float32)
    truth = np.array([[[0, 2, 1], [2, 0, 0]]], dtype=np.uint8)
    m, c = ref_mask_counts(z, truth, 0.0, -1)
    assert m.reshape(-1).tolist() == [0, 1, 1, 1, 1, 0] and c.tolist() == [[4, 3, 3]]
    m, c = ref_mask_counts(z, truth, 0.5, 2)
    assert m.reshape(-1).tolist() == [0, 0, 1, 1, 0, 0] and c.tolist() == [[2, 2, 1]]


# ---------------------------------------------------------------- VolumeResampler without a GPU
def test_out_shape():
    r = VolumeResampler((None, 1, 1))
    assert r.out_shape((10, 512, 512), (5, 0.7, 0.7)) == (10, 358, 358)           # 358.4 -> 358
    assert r.out_shape((3, 40, 52), (2, 1.5, 0.75)) == (3, 60, 39)
    assert r.out_shape((40, 52), (1.5, 0.75)) == (60, 39) and r.out_shape((40, 52), (9, 1.5, 0.75)) == (60, 39)
    assert VolumeResampler((2.5, 1, 1)).out_shape((10, 4, 4), (5, 1, 1)) == (20, 4, 4)
    assert VolumeResampler((1, 1, 1)).out_shape((3, 5, 5), (0.5, 0.5, 0.1)) == (2, 3, 1)     # 1.5 -> 2 (half up), 2.5 -> 3, 0.5 -> 1
    assert VolumeResampler((1, 1, 1000)).out_shape((3, 5, 5), (1, 1, 1)) == (3, 5, 1)        # never below one sample
    assert VolumeResampler((None, None, None)).out_shape((3, 5, 7), (9, 9, 9)) == (3, 5, 7)
    # the round trip: where the ratio is exact the inverse resampler finds the original shape ...
    for shape, sp in (((10, 512, 512), (5, 0.5, 0.5)), ((7, 300, 250), (3, 2, 2)), ((4, 124, 456), (1, 0.25, 0.75))):
        work = r.out_shape(shape, sp)
        assert VolumeResampler((None,) + sp[1:]).out_shape(work, (sp[0], 1, 1)) == shape
    # ... and where it is not it may miss it (358 / 0.7 = 511.4): the way back, logits_to, takes the native shape itself
    assert VolumeResampler((None, 0.7, 0.7)).out_shape((10, 358, 358), (5, 1, 1)) == (10, 511, 511)
    # exact rational arithmetic: 0.1 * 3 is not 0.30000000000000004 here
    assert VolumeResampler((1, 1, 0.2)).out_shape((1, 1, 5), (1, 1, 0.1)) == (1, 1, 3)       # 2.5 -> 3


def test_volume_resampler_argument_errors():
    for bad in (None, (1, 1), (1, 1, 1, 1), (0, 1, 1), (1, -1, 1), (1, 1, float("nan")), (1, 1, float("inf")), ("a", 1, 1), (True, 1, 1),
                (1, 1, 1e-9), 3):
        with pytest.raises(VuError):
            VolumeResampler(bad)
    r = VolumeResampler((None, 1, 1))
    for shape, sp in (((3, 4, 5), (1, 1)), ((3, 4, 5), (1, 1, 0)), ((3, 4, 5), None), ((4,), (1, 1, 1)), ((3, 0, 5), (1, 1, 1)),
                      ((3, 4, 5), (1, 1, -2)), ((4, 5), (1, 1, 1, 1)), ((2, 40000, 40000), (1, 1, 1))):
        with pytest.raises(VuError):
            r.out_shape(shape, sp)
    vol = np.zeros((2, 4, 5), np.int16)
    with pytest.raises(VuError):
        r.image(vol.astype(np.float32), (1, 1, 1))                                 # wrong dtype
    with pytest.raises(VuError):
        r.labels(vol, (1, 1, 1))
    with pytest.raises(VuError):
        r.image(vol[0, 0], (1, 1, 1))                                              # one dimension
    with pytest.raises(VuError):
        r.image(vol, (1, 1))
    with pytest.raises(VuError):
        r.image([vol, vol], [(1, 1, 1)])                                           # two volumes, one spacing in a list
    with pytest.raises(VuError):
        r.image(np.zeros((0, 4, 5), np.int16), (1, 1, 1))
    z = np.zeros((2, 4, 5), np.float32)
    with pytest.raises(VuError):
        r.logits_to(z, (4, 5))                                                     # rank
    with pytest.raises(VuError):
        r.logits_to(z, (2, 0, 5))
    with pytest.raises(VuError):
        r.logits_to(vol, (2, 4, 5))                                                # dtype
    with pytest.raises(VuError):
        r.logits_to(z, (2, 8, 9), truth=np.zeros((2, 8, 8), np.uint8))
    with pytest.raises(VuError):
        r.logits_to(z, (2, 8, 9), truth=np.zeros((2, 8, 9), np.int16))
    with pytest.raises(VuError):
        r.logits_to(z, (2, 8, 9), label=256)
    with pytest.raises(VuError):
        r.logits_to(z, (2, 8, 9), zthr=float("nan"))
    if not torch.cuda.is_available():                                              # valid arguments: no CPU fallback
        with pytest.raises(VuError):
            r.image(vol, (1, 1, 1))
        with pytest.raises(VuError):
            r.logits_to(z, (2, 8, 9))


class _Model:
    im_size, num_channels = 32, 1


def test_segmenter_spacing_and_resampler_go_together():
    vol = np.zeros((2, 40, 40), np.int16)
    plain, res = TiledSegmenter(_Model(), overlap=8), TiledSegmenter(_Model(), overlap=8, resample=(None, 1, 1))
    assert plain.resample is None and isinstance(res.resample, VolumeResampler)
    assert isinstance(TiledSegmenter(_Model(), overlap=8, resample=VolumeResampler((1, 1, 1))).resample, VolumeResampler)
    with pytest.raises(VuError):
        TiledSegmenter(_Model(), overlap=8, resample=(1, 1))
    with pytest.raises(VuError, match="resampler"):
        plain(vol, spacing=(1, 1, 1))
    with pytest.raises(VuError, match="resampler"):
        plain.score(vol, vol.astype(np.uint8), spacing=(1, 1, 1))
    with pytest.raises(VuError, match="spacing"):
        res(vol)
    with pytest.raises(VuError, match="spacing"):
        res.score(vol, vol.astype(np.uint8))
    with pytest.raises(VuError):
        res(vol, spacing=(1, 0, 1))


# ---------------------------------------------------------------- C entries: every refusal, before any launch
def _rc(fn, *a):
    rc = fn(*a)
    return rc, _lib.lib().vu_last_error().decode()


def test_c_entry_argument_errors():
    L = _lib.lib()
    g = [C.c_int(0) for _ in range(3)]
    assert L.vu_resample_geometry(*(C.byref(v) for v in g)) == 0 and all(v.value >= 1 for v in g) and g[0].value % 4 == 0
    assert L.vu_resample_geometry(None, C.byref(g[1]), C.byref(g[2])) == -1
    P = 1 << 24                                   # distinct, aligned, non-overlapping fake addresses
    src, dst, truth, mask, counts, scratch = (C.c_void_p(P * (i + 1)) for i in range(6))
    shp = dict(Di=2, Hi=8, Wi=12, Do=3, Ho=5, Wo=9)

    def call(fn, src=src, dst=dst, **kw):
        s = {**shp, **kw}
        return _rc(fn, src, dst, s["Di"], s["Hi"], s["Wi"], s["Do"], s["Ho"], s["Wo"], None)

    shape_errors = [(dict(Di=0), "at least 1"), (dict(Hi=-1), "at least 1"), (dict(Wi=0), "at least 1"), (dict(Do=0), "at least 1"),
                    (dict(Ho=0), "at least 1"), (dict(Wo=-3), "at least 1"), (dict(Di=2048, Hi=1024, Wi=1024), "2^31"),
                    (dict(Do=2048, Ho=1024, Wo=1024), "2^31")]
    for fn, width in ((L.vu_resample_i16, 2), (L.vu_resample_u8_nearest, 1)):
        for kw, word in shape_errors:
            rc, msg = call(fn, **kw)
            assert rc == -1 and word in msg, (kw, msg)
        assert call(fn, src=None)[0] == -1 and call(fn, dst=None)[0] == -1
        for alias in (src, C.c_void_p(P + width * 2 * 8 * 12 - 1), C.c_void_p(P - width * 3 * 5 * 9 + 1)):
            rc, msg = call(fn, dst=alias)
            assert rc == -1 and "alias" in msg, msg
    need = L.vu_resample_f32_scratch_bytes(3, 5, 9)
    assert need == 3 * 12 and L.vu_resample_f32_scratch_bytes(0, 5, 9) == 0 and L.vu_resample_f32_scratch_bytes(3, 5, -1) == 0
    assert L.vu_resample_f32_scratch_bytes(2, g[1].value + 1, g[0].value + 1) == 2 * 4 * 12

    def f32(src=src, truth=truth, out=dst, mask=mask, counts=counts, scratch=scratch, nbytes=need, zthr=0.0, label=-1, **kw):
        s = {**shp, **kw}
        return _rc(L.vu_resample_f32, src, truth, out, mask, counts, scratch, nbytes, s["Di"], s["Hi"], s["Wi"], s["Do"], s["Ho"], s["Wo"],
                   zthr, label, None)

    for kw, word in shape_errors:
        rc, msg = f32(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    for kw, word in ((dict(src=None), "null"), (dict(out=None, mask=None, counts=None), "null"), (dict(truth=None), "truth"),
                     (dict(label=256), "label"), (dict(zthr=float("nan")), "not a number"), (dict(scratch=None), "scratch"),
                     (dict(nbytes=need - 1), "scratch"), (dict(scratch=C.c_void_p(6 * P + 2)), "scratch"),
                     (dict(counts=C.c_void_p(5 * P + 4)), "8-byte"), (dict(out=src), "alias"), (dict(mask=src), "alias"),
                     (dict(counts=src), "alias"), (dict(out=C.c_void_p(P + 4 * 2 * 8 * 12 - 4)), "alias"),
                     (dict(mask=dst), "overlap"), (dict(mask=truth), "overlap"), (dict(out=truth), "overlap"),
                     (dict(scratch=src), "alias"), (dict(scratch=truth), "alias"), (dict(scratch=dst), "alias"),
                     (dict(scratch=mask), "alias"), (dict(scratch=counts), "alias")):
        rc, msg = f32(**kw)
        assert rc == -1 and word in msg, (kw, msg)
