"""Host side of per-volume intensity normalisation (csrc/vu_intensity.hip, segment.IntensityNormalizer): the numpy restatements the
GPU tests compare against, checked on their own, plus everything that needs no GPU.

  ref_hist     np.bincount of the selected values under the three selection rules of include/vit_unet_amd.h
  ref_bbox     the inclusive extent of the selected voxels, (D, -1, H, -1, W, -1) when there is none
  ref_stats    the (8 + 4 nq) integers of vu_intensity_stats from a histogram, by cumulative sums in Python integers
  ref_window   the (lo, hi) of IntensityNormalizer.window from the sorted selected values, in fractions.Fraction
ref_stats is held against a brute-force sort, order statistic by order statistic.  The percentile window is held against
np.percentile(method="linear") within 1e-9 absolute: values are bounded by 2^15 and both sides are a few float64 roundings
(2^15 * 2^-52 is about 7e-12 each), so 1e-9 leaves more than two orders of magnitude; the float32 rounding of the window is applied
to both sides.  The z-score window is held against float64 mean / std within 1e-6 relative on 10^5 voxels (numpy's pairwise sums
are good to about 1e-13 there).  Then vu_intensity_rank against Python integers, every refusal of the C entries (fake pointers: the
checks run before any launch), every constructor refusal, and that a (lo, hi) window builds the objects it always built."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from vit_unet.torch import _lib
from vit_unet.torch._lib import VuError
from vit_unet.torch.dataset import SegmentationPatchTransform
from vit_unet.torch.segment import IntensityNormalizer, TiledSegmenter

PD = 10 ** 6
SELECT = {"all": 0, "above": 1, "mask": 2}


# ---------------------------------------------------------------- restatements
def ref_selected(vol, select="all", floor=0, label=-1, mask=None):
    """The boolean selection of include/vit_unet_amd.h (select by name or by number)."""
    sel = SELECT.get(select, select)
    vol = np.asarray(vol)
    if sel == 0:
        return np.ones(vol.shape, bool)
    if sel == 1:
        return vol.astype(np.int64) > int(floor)
    m = np.asarray(mask)
    return (m != 0) if label < 0 else (m == label)


def ref_hist(vol, select="all", floor=0, label=-1, mask=None):
    vals = np.asarray(vol)[ref_selected(vol, select, floor, label, mask)].astype(np.int64)
    return np.bincount(vals + 32768, minlength=65536).astype(np.int64)


def ref_bbox(vol, select="all", floor=0, label=-1, mask=None):
    s = ref_selected(vol, select, floor, label, mask)
    s = s.reshape((1,) * (3 - s.ndim) + s.shape)
    if not s.any():
        return (s.shape[0], -1, s.shape[1], -1, s.shape[2], -1)
    out = []
    for ax in range(3):
        idx = np.nonzero(s.any(axis=tuple(a for a in range(3) if a != ax)))[0]
        out += [int(idx[0]), int(idx[-1])]
    return tuple(out)


def ref_stats(hist, pns=(), pd=PD):
    """The integers of vu_intensity_stats as a list of Python ints; pns: up to four numerators over pd."""
    h = [int(c) for c in np.asarray(hist).reshape(-1)]
    assert len(h) == 65536
    n = sum(h)
    out = [n] + [0] * (7 + 4 * len(pns))
    if n == 0:
        return out
    nz = [b for b, c in enumerate(h) if c]
    out[1], out[2] = nz[0] - 32768, nz[-1] - 32768
    out[3] = sum((b - 32768) * h[b] for b in nz)
    out[4] = sum((b - 32768) ** 2 * h[b] for b in nz)
    cum = np.cumsum(np.asarray(h, dtype=np.int64))

    def kth(k):                       # the k-th smallest, counted from 0: the first bin whose cumulative count exceeds k
        return int(np.searchsorted(cum, k, side="right")) - 32768

    for j, pn in enumerate(pns):
        k, r = divmod((n - 1) * int(pn), int(pd))
        out[8 + 4 * j:12 + 4 * j] = [k, r, kth(k), kth(min(k + 1, n - 1))]
    return out


def ref_window(vol, mode="percentile", lo=0.5, hi=99.5, k=3.0, select="all", floor=0, label=-1, mask=None):
    """(lo, hi) as IntensityNormalizer.window defines them, from the sorted selected values."""
    vals = sorted(int(v) for v in np.asarray(vol)[ref_selected(vol, select, floor, label, mask)].reshape(-1))
    n = len(vals)
    if n == 0:
        raise VuError("empty selection")
    if mode == "percentile":
        w = []
        for p in (lo, hi):
            kk, r = divmod((n - 1) * int(round(float(p) * 10 ** 4)), PD)
            a, b = vals[kk], vals[min(kk + 1, n - 1)]
            w.append(float(np.float32(float(a + Fraction((b - a) * r, PD)))))
    else:
        s, s2 = sum(vals), sum(v * v for v in vals)
        mean, std = float(Fraction(s, n)), math.sqrt(float(Fraction(n * s2 - s * s, n * n)))
        w = [float(np.float32(mean - float(k) * std)), float(np.float32(mean + float(k) * std))]
    if not w[1] > w[0]:
        w[1] = float(np.float32(w[0] + 1.0))
    return w[0], w[1]


def ct_like(shape, seed=0):
    """Half the voxels at -1024 (air), the rest normal around 40 with sigma 200."""
    rng = np.random.default_rng(seed)
    v = np.rint(rng.normal(40.0, 200.0, shape)).astype(np.int16)
    v[rng.random(shape) < 0.5] = -1024
    return v


# ---------------------------------------------------------------- the restatements on their own
PERCENTS = (0.0, 0.5, 50.0, 99.5, 100.0)


@pytest.mark.parametrize("n", [1, 2, 3, 1000])
def test_ref_stats_against_a_sort(n):
    rng = np.random.default_rng(n)
    vals = rng.integers(-32768, 32768, n).astype(np.int16)
    if n >= 3:
        vals[:2] = (-32768, 32767)
    if n == 1000:
        vals[10:300] = 17                                                     # a heavy bin: ranks inside one bin
    srt = np.sort(vals.astype(np.int64))
    pns = [int(round(p * 10 ** 4)) for p in PERCENTS]
    for chunk in (pns[:4], pns[1:]):
        st = ref_stats(ref_hist(vals), chunk)
        assert st[:8] == [n, int(srt[0]), int(srt[-1]), int(srt.sum()), int((srt * srt).sum()), 0, 0, 0]
        for j, pn in enumerate(chunk):
            k, r = divmod((n - 1) * pn, PD)
            assert st[8 + 4 * j:12 + 4 * j] == [k, r, int(srt[k]), int(srt[min(k + 1, n - 1)])]
    every = ref_hist(vals)                                                    # every order statistic, one at a time
    cum = np.cumsum(every)
    for k in range(n):
        assert int(np.searchsorted(cum, k, side="right")) - 32768 == int(srt[k])


def test_ref_stats_empty_and_selections():
    assert ref_stats(np.zeros(65536, np.int64), (5000, 995000)) == [0] * 16
    vol = np.array([[[-5, 0, 3], [7, 0, -5]]], np.int16)
    mask = np.array([[[0, 1, 2], [2, 0, 1]]], np.uint8)
    assert ref_hist(vol).sum() == 6 and ref_hist(vol, "above", 0).sum() == 2 and ref_hist(vol, "above", -5).sum() == 4
    assert ref_hist(vol, "mask", mask=mask).sum() == 4 and ref_hist(vol, "mask", label=2, mask=mask)[32768 + 3] == 1
    assert ref_hist(vol, "mask", label=7, mask=mask).sum() == 0
    assert ref_bbox(vol) == (0, 0, 0, 1, 0, 2) and ref_bbox(vol, "above", 3) == (0, 0, 1, 1, 0, 0)
    assert ref_bbox(vol, "mask", label=7, mask=mask) == (1, -1, 2, -1, 3, -1)
    assert ref_bbox(vol[0], "above", 6) == (0, 0, 1, 1, 0, 0)


# ---------------------------------------------------------------- vu_intensity_rank
def _rank(N, pn, pd):
    k, r = C.c_ulonglong(123), C.c_uint(456)
    rc = _lib.lib().vu_intensity_rank(N, pn, pd, C.byref(k), C.byref(r))
    return rc, k.value, r.value


def test_rank_against_python_integers():
    for N in (1, 2, 2 ** 32 - 1, 1000, 16777216):
        for pn, pd in ((0, PD), (PD, PD), (1, PD), (5000, PD), (500000, PD), (995000, PD), (999999, PD), (0, 1), (1, 1), (2, 3), (3, 7)):
            rc, k, r = _rank(N, pn, pd)
            assert rc == 0 and (k, r) == divmod((N - 1) * pn, pd), (N, pn, pd)


def test_rank_refusals():
    L = _lib.lib()
    for N, pn, pd in ((0, 1, 2), (2 ** 32, 1, 2), (2 ** 40, 1, 2), (5, 1, 0), (5, 3, 2), (5, 1, PD + 1), (5, PD + 1, PD + 1)):
        rc, k, r = _rank(N, pn, pd)
        assert rc == -1 and (k, r) == (123, 456) and L.vu_last_error().decode(), (N, pn, pd)
    k, r = C.c_ulonglong(0), C.c_uint(0)
    assert L.vu_intensity_rank(5, 1, 2, None, C.byref(r)) == -1 and L.vu_intensity_rank(5, 1, 2, C.byref(k), None) == -1


# ---------------------------------------------------------------- C entries: every refusal, before any launch
def hist_refusals():
    """(keyword overrides, a word of the message) for vu_intensity_hist; the GPU tests run the same list on real buffers."""
    return [(dict(vol=None), "null"), (dict(hist=None), "null"), (dict(select=-1), "select"), (dict(select=3), "select"),
            (dict(select=2, mask=None), "mask"), (dict(label=256), "label"), (dict(D=0), "at least 1"), (dict(H=-2), "at least 1"),
            (dict(W=0), "at least 1"), (dict(D=1024, H=2048, W=2048), "2^32"), (dict(D=65536, H=65536, W=1), "2^32"),
            (dict(D=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1), "2^32"), (dict(hist_off=2), "aligned"), (dict(bbox_off=2), "aligned")]


def stats_refusals():
    return [(dict(hist=None), "null"), (dict(stats=None), "null"), (dict(nq=-1), "nq"), (dict(nq=5), "nq"), (dict(pn=None), "pn"),
            (dict(pd=None), "pn"), (dict(pns=(1, 2, 3, 4), pds=(PD, PD, 0, PD)), "quantile"), (dict(pns=(1, 2, 3, 4), pds=(PD, PD, PD + 1, PD)), "quantile"),
            (dict(pns=(1, 7, 3, 4), pds=(PD, 6, PD, PD)), "quantile"), (dict(hist_off=2), "aligned"), (dict(stats_off=4), "aligned")]


def call_hist(p_vol, p_mask, p_hist, p_bbox, **kw):
    """vu_intensity_hist on integer addresses (None = NULL) with the overrides of `hist_refusals` -> (rc, message)."""
    a = dict(vol=p_vol, mask=p_mask, hist=p_hist, bbox=p_bbox, D=2, H=8, W=12, select=0, floor=0, label=-1, hist_off=0, bbox_off=0)
    a.update(kw)
    p = lambda v, off=0: None if v is None else C.c_void_p(v + off)    # noqa: E731
    L = _lib.lib()
    rc = L.vu_intensity_hist(p(a["vol"]), p(a["mask"]), p(a["hist"], a["hist_off"]), p(a["bbox"], a["bbox_off"]), a["D"], a["H"], a["W"],
                             a["select"], a["floor"], a["label"], kw.get("stream"))
    return rc, L.vu_last_error().decode()


def call_stats(p_hist, p_stats, **kw):
    a = dict(hist=p_hist, stats=p_stats, nq=4, pns=(0, 5000, 500000, PD), pds=(PD,) * 4, pn=True, pd=True, hist_off=0, stats_off=0)
    a.update(kw)
    pn, pd = (C.c_uint * 4)(*a["pns"]), (C.c_uint * 4)(*a["pds"])
    p = lambda v, off=0: None if v is None else C.c_void_p(v + off)    # noqa: E731
    L = _lib.lib()
    rc = L.vu_intensity_stats(p(a["hist"], a["hist_off"]), pn if a["pn"] else None, pd if a["pd"] else None, a["nq"],
                              p(a["stats"], a["stats_off"]), kw.get("stream"))
    return rc, L.vu_last_error().decode()


def test_c_entry_argument_errors():
    L = _lib.lib()
    g = [C.c_int(0) for _ in range(3)]
    assert L.vu_intensity_geometry(*(C.byref(v) for v in g)) == 0
    base, bins, V = (v.value for v in g)
    assert bins >= 0 and -32768 <= base and base + bins <= 32768 and V >= 64 and V % 8 == 0
    for miss in range(3):
        assert L.vu_intensity_geometry(*(None if i == miss else C.byref(g[i]) for i in range(3))) == -1
    P = 1 << 24                                   # distinct, aligned fake addresses: every check returns before they are used
    for kw, word in hist_refusals():
        rc, msg = call_hist(P, 2 * P, 3 * P, 4 * P, **kw)
        assert rc == -1 and word in msg, (kw, msg)
    for kw, word in stats_refusals():
        rc, msg = call_stats(3 * P, 5 * P, **kw)
        assert rc == -1 and word in msg, (kw, msg)


# ---------------------------------------------------------------- windows
def norm_window(n, vol, mask=None):
    """IntensityNormalizer.window without a device: its host arithmetic on the restated integers."""
    h = ref_hist(vol, n.select, n.floor, n.label, mask)
    return n.window_from(ref_stats(h, n.pn))


@pytest.mark.parametrize("kind", ["uniform", "ct", "small", "two"])
def test_percentile_window_against_numpy(kind):
    rng = np.random.default_rng(5)
    vol = {"uniform": lambda: rng.integers(-32768, 32768, (4, 50, 50)).astype(np.int16), "ct": lambda: ct_like((4, 50, 50), 3),
           "small": lambda: rng.integers(-2000, 2000, (1, 3, 5)).astype(np.int16),
           "two": lambda: np.array([[-32768, 32767]], np.int16)}[kind]()
    for lo, hi in ((0.5, 99.5), (0.0, 100.0), (2.5, 50.0), (33.3333, 66.6667), (49.9999, 50.0001)):
        for select, floor in (("all", 0), ("above", int(np.median(vol)))):
            n = IntensityNormalizer("percentile", lo, hi, select=select, floor=floor)
            vals = vol[ref_selected(vol, select, floor)].astype(np.float64)
            got = norm_window(n, vol)
            assert got == ref_window(vol, "percentile", lo, hi, select=select, floor=floor)
            assert all(float(np.float32(g)) == g for g in got)
            q = [n.pn[0] / 10 ** 4, n.pn[1] / 10 ** 4]
            want = np.percentile(vals, q, method="linear")
            st = ref_stats(ref_hist(vol, select, floor), n.pn)
            exact = [float(st[10 + 4 * j] + Fraction((st[11 + 4 * j] - st[10 + 4 * j]) * st[9 + 4 * j], PD)) for j in range(2)]
            assert abs(exact[0] - want[0]) <= 1e-9 and abs(exact[1] - want[1]) <= 1e-9, (exact, want)
            if np.float32(want[1]) > np.float32(want[0]):
                assert got == (float(np.float32(exact[0])), float(np.float32(exact[1])))


def test_zscore_window_against_numpy():
    rng = np.random.default_rng(9)
    vol = np.rint(rng.normal(300.0, 200.0, (10, 100, 100))).astype(np.int16)           # 10^5 voxels
    f = vol.astype(np.float64)
    for k in (1.0, 3.0, 2.5):
        n = IntensityNormalizer("zscore", k=k)
        lo, hi = norm_window(n, vol)
        assert (lo, hi) == ref_window(vol, "zscore", k=k)
        d = n.stats_dict(ref_stats(ref_hist(vol), n.pn))
        assert abs(d["mean"] - f.mean()) <= 1e-6 * abs(f.mean()) and abs(d["std"] - f.std()) <= 1e-6 * f.std()
        assert d["n"] == vol.size and d["min"] == vol.min() and d["max"] == vol.max() and d["sum"] == int(f.sum())
        wlo, whi = f.mean() - k * f.std(), f.mean() + k * f.std()
        assert abs(lo - wlo) <= 1e-6 * abs(wlo) and abs(hi - whi) <= 1e-6 * abs(whi)
    above = IntensityNormalizer("zscore", k=2.0, select="above", floor=300)
    g = f[f > 300]
    lo, hi = norm_window(above, vol)
    assert abs(lo - (g.mean() - 2 * g.std())) <= 1e-6 * abs(g.mean() - 2 * g.std()) and abs(hi - (g.mean() + 2 * g.std())) <= 1e-6 * hi


def test_degenerate_and_empty_windows():
    const = np.full((2, 5, 7), -321, np.int16)
    one = np.array([[5, -7, 900]], np.int16)
    for mode in ("percentile", "zscore"):
        n = IntensityNormalizer(mode)
        assert norm_window(n, const) == (-321.0, -320.0) == ref_window(const, mode)
        single = IntensityNormalizer(mode, select="above", floor=5)                      # N = 1: the voxel 900
        assert norm_window(single, one) == (900.0, 901.0) == ref_window(one, mode, select="above", floor=5)
        empty = IntensityNormalizer(mode, select="above", floor=900)
        with pytest.raises(VuError, match="empty"):
            norm_window(empty, one)
        with pytest.raises(VuError):
            ref_window(one, mode, select="above", floor=900)
    top = np.full((3, 3), 32767, np.int16)
    assert norm_window(IntensityNormalizer(), top) == (32767.0, 32768.0)
    m = np.array([[0, 2, 0]], np.uint8)
    assert norm_window(IntensityNormalizer(select="mask", label=2), one, m) == (-7.0, -6.0)


def test_constructor_refusals():
    bad = [dict(mode="otsu"), dict(mode=None), dict(lo=-0.1), dict(hi=100.5), dict(lo=50, hi=50), dict(lo=60, hi=40), dict(lo="1"),
           dict(hi=None), dict(lo=True), dict(lo=float("nan")), dict(k=0), dict(k=-1.0), dict(k=float("inf")), dict(k=float("nan")),
           dict(k="3"), dict(k=True), dict(select="fg"), dict(select=1), dict(floor=0.5), dict(floor=True), dict(floor=2 ** 31),
           dict(label=256), dict(label=1.0), dict(label=True)]
    for kw in bad:
        with pytest.raises(VuError):
            IntensityNormalizer(**kw)
    n = IntensityNormalizer("zscore", 1, 99, 2, "above", np.int16(-5), np.int64(3))
    assert (n.mode, n.lo, n.hi, n.k, n.select, n.floor, n.label, n.pn) == ("zscore", 1.0, 99.0, 2.0, "above", -5, 3, (10000, 990000))
    assert IntensityNormalizer(lo=0.00004, hi=99.99996).pn == (0, 10 ** 6)                # rounded to 1e-4 percent
    with pytest.raises(VuError, match="mask"):                                          # before any device is asked for
        IntensityNormalizer(select="mask").window(np.zeros((4, 4), np.int16))
    with pytest.raises(VuError):
        IntensityNormalizer().window(np.zeros((4, 4), np.float32))
    with pytest.raises(VuError):
        IntensityNormalizer(select="mask").window(np.zeros((4, 4), np.int16), np.zeros((4, 5), np.uint8))


# ---------------------------------------------------------------- a (lo, hi) pair builds what it always built
class _Model:
    im_size, num_channels = 32, 1


def test_pair_windows_pass_through():
    s = TiledSegmenter(_Model(), overlap=8)
    assert s.window == (-1024.0, 1024.0) and s.normalizer is None
    s = TiledSegmenter(_Model(), overlap=8, window=(-100, 300.1))
    assert s.window == (-100.0, float(np.float32(300.1))) and s.normalizer is None
    assert (s.T, s.overlap, s.batch, s.threshold, s.label, s.ensemble, s.zthr) == (32, 8, 64, 0.5, -1, 1, 0.0)
    assert s.clean is None and s.surface is None and s.resample is None
    for w in ((5, 5), (7, 3)):
        with pytest.raises(VuError, match="hi > lo"):
            TiledSegmenter(_Model(), overlap=8, window=w)
        with pytest.raises(VuError, match="hi > lo"):
            SegmentationPatchTransform(32, window=w)
    with pytest.raises(VuError, match="hi > lo"):
        s(np.zeros((40, 40), np.int16), window=(3, 3))
    t = SegmentationPatchTransform(32, 4, train=True, window=(0, 500.3), ls=0.1, fg=0.25, label=2, seed=5)
    assert t.window == (0.0, float(np.float32(500.3))) and t.normalizer is None
    assert (t.patch, t.per_volume, t.train, t.ls, t.fg, t.label, t.device, t.last_crops) == (32, 4, True, 0.1, 0.25, 2, "cuda", None)
    assert SegmentationPatchTransform(32).window == (-1024.0, 1024.0)
    n = IntensityNormalizer()
    sn, tn = TiledSegmenter(_Model(), overlap=8, window=n), SegmentationPatchTransform(32, window=n)
    assert sn.normalizer is n and sn.window is None and tn.normalizer is n and tn.window is None
    vol, msk = np.zeros((2, 40, 40), np.int16), np.zeros((2, 40, 40), np.uint8)
    with pytest.raises(VuError, match="windows"):                                       # one pair per volume, checked before any launch
        t(vol, msk, windows=[(0, 1), (0, 1)])
    with pytest.raises(VuError, match="hi > lo"):
        t(vol, msk, windows=[(4, 4)])
