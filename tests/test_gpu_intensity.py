"""Per-volume intensity statistics on the MI355X (csrc/vu_intensity.hip, segment.IntensityNormalizer) against the numpy
restatements of test_intensity_cpu.py.  Everything goes through the C ABI into sentinel-filled hist, bbox and stats; every integer
is compared exactly and every case runs twice and must give the same bits.  Shapes sit around the kernel's own geometry
(vu_intensity_geometry: V voxels per workgroup step; the edges of the LDS sub-histogram), W covers the 16-byte path and its tail,
and one case reads a volume one element into a larger allocation (scalar loads).  End to end: IntensityNormalizer equals
ref_window exactly; TiledSegmenter / SegmentationPatchTransform with a normalizer equal the same objects with the measured pair,
bit for bit; a pair or windows= launches no intensity kernel; run_segmentation measures every volume exactly once."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from test_gpu_segment import small_model
from test_intensity_cpu import (PD, SELECT, call_hist, call_stats, ct_like, hist_refusals, ref_bbox, ref_hist, ref_stats, ref_window,
                                stats_refusals)
from vit_unet.torch import _lib
from vit_unet.torch._lib import VuError, check, lib, ptr
from vit_unet.torch.dataset import SegmentationPatchTransform
from vit_unet.torch.segment import IntensityNormalizer, TiledSegmenter

pytestmark = pytest.mark.gpu
DEV = "cuda"
PNS = (0, 5000, 500000, PD)               # 0, 0.5, 50 and 100 percent


@functools.lru_cache(maxsize=None)
def geometry():
    g = [C.c_int(0) for _ in range(3)]
    check(lib().vu_intensity_geometry(*(C.byref(v) for v in g)))
    return tuple(v.value for v in g)                                    # lds_base, lds_bins, V


def st():
    return _lib.stream_ptr()


def run_hist(vol, select=0, floor=0, label=-1, mask=None, bbox=True, vol_dev=None):
    """vu_intensity_hist into sentinel-filled buffers, twice -> (hist int64, bbox tuple or None)."""
    v = torch.from_numpy(np.ascontiguousarray(vol)).to(DEV) if vol_dev is None else vol_dev
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
    shape = (1,) * (3 - vol.ndim) + tuple(vol.shape)
    outs = []
    for sentinel in (-1, 0x5a5a5a5a):
        hist = torch.full((65536,), sentinel, dtype=torch.int32, device=DEV)
        box = torch.full((6,), sentinel, dtype=torch.int32, device=DEV) if bbox else None
        check(lib().vu_intensity_hist(ptr(v), ptr(m), ptr(hist), ptr(box), *shape, SELECT.get(select, select), int(floor), int(label), st()))
        outs.append((hist.cpu().numpy().view(np.uint32).astype(np.int64), None if box is None else tuple(box.cpu().tolist())))
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
    return outs[0]


def run_stats(hist, pns=PNS, pd=PD):
    """vu_intensity_stats on a host histogram, twice -> the (8 + 4 nq) integers as a list."""
    h = torch.from_numpy(np.asarray(hist, dtype=np.int64).astype(np.uint32).view(np.int32)).to(DEV)
    nq = len(pns)
    outs = []
    for sentinel in (-1, 0x5a5a5a5a5a5a):
        stats = torch.full((8 + 4 * nq + 2,), sentinel, dtype=torch.int64, device=DEV)       # two guard words behind
        pn, pdv = (C.c_uint * max(nq, 1))(*pns), (C.c_uint * max(nq, 1))(*([pd] * nq))
        check(lib().vu_intensity_stats(ptr(h), pn, pdv, nq, ptr(stats), st()))
        s = stats.cpu().tolist()
        assert s[-2:] == [sentinel, sentinel]
        outs.append(s[:-2])
    assert outs[0] == outs[1]
    return outs[0]


def check_volume(vol, select=0, floor=0, label=-1, mask=None, stats=True):
    h, box = run_hist(vol, select, floor, label, mask)
    want = ref_hist(vol, select, floor, label, mask)
    assert np.array_equal(h, want), (int(np.abs(h - want).sum()), np.nonzero(h != want)[0][:8])
    assert box == ref_bbox(vol, select, floor, label, mask)
    if stats:
        assert run_stats(h) == ref_stats(want, PNS)


# ---------------------------------------------------------------- 1. shapes around the geometry
@functools.lru_cache(maxsize=None)
def shapes():
    V = geometry()[2]
    s = [(1, 1, n) for n in (V - 1, V, V + 1)] + [(1, 2 * V + 3, 1), (5, 41, V // 41 + 1)]    # about 5 V
    s += [(3, 5, w) for w in (1, 7, 8, 9, 13)] + [(2, 700, w) for w in (7, 8, 9, 13)]           # the 16-byte path and its tail
    s += [(1, 37, 64), (29, 1, 33), (4, V // 8, 3)]                                           # D = 1, H = 1
    return tuple(s)


NSHAPES = 17


def test_shape_list_is_complete():
    V = geometry()[2]
    assert len(shapes()) == NSHAPES
    n = [int(np.prod(s)) for s in shapes()]
    assert {V - 1, V, V + 1, 2 * V + 3} <= set(n) and any(4.5 * V < k < 5.5 * V for k in n)


def values(shape, kind):
    base, bins, _ = geometry()
    rng = np.random.default_rng(len(kind) + sum(shape))
    if kind == "constant":
        return np.full(shape, -1024, np.int16)
    if kind == "two":
        return rng.choice(np.array([0, 777], np.int16), shape)
    if kind == "edges":                                       # each side of each edge of the LDS range
        e = [min(max(v, -32768), 32767) for v in (base - 1, base, base + bins - 1, base + bins)]
        return rng.choice(np.array(e, np.int16), shape)
    if kind == "extremes":
        return rng.choice(np.array([-32768, 32767], np.int16), shape)
    if kind == "uniform":
        return rng.integers(-32768, 32768, shape).astype(np.int16)
    return ct_like(shape, 4)


KINDS = ("constant", "two", "edges", "extremes", "uniform", "ct")


@pytest.mark.parametrize("k", range(NSHAPES), ids=[f"s{k}" for k in range(NSHAPES)])
def test_hist_bbox_stats_exact(k):
    shape = shapes()[k]
    for kind in KINDS:
        vol = values(shape, kind)
        check_volume(vol, stats=kind in ("uniform", "ct", "edges"))
        if kind in ("two", "ct"):
            check_volume(vol, "above", floor=int(np.median(vol)), stats=False)


def test_offset_volume_pointer_takes_the_scalar_path():
    V = geometry()[2]
    shape = (2, V // 16 + 3, 9)
    n = int(np.prod(shape))
    for kind in ("uniform", "ct"):
        vol = values(shape, kind)
        buf = torch.full((n + 2,), 12345, dtype=torch.int16, device=DEV)
        buf[1:n + 1].copy_(torch.from_numpy(vol).reshape(-1))
        h, box = run_hist(vol, vol_dev=buf[1:n + 1].view(shape))
        assert np.array_equal(h, ref_hist(vol)) and box == ref_bbox(vol)
        b = buf.cpu()
        assert int(b[0]) == 12345 and int(b[-1]) == 12345 and np.array_equal(b[1:n + 1].view(shape).numpy(), vol)
        mask = (np.random.default_rng(1).random(shape) < 0.3).astype(np.uint8)
        mb = torch.zeros(n + 1, dtype=torch.uint8, device=DEV)                # an aligned volume with a mask off by one byte
        mb[1:].copy_(torch.from_numpy(mask).reshape(-1))
        hist = torch.full((65536,), -1, dtype=torch.int32, device=DEV)
        check(lib().vu_intensity_hist(ptr(torch.from_numpy(vol).to(DEV)), C.c_void_p(mb.data_ptr() + 1), ptr(hist), None, *shape, 2, 0, -1, st()))
        assert np.array_equal(hist.cpu().numpy().view(np.uint32).astype(np.int64), ref_hist(vol, "mask", mask=mask))


# ---------------------------------------------------------------- 2. selection
def test_floor_is_strict_and_at_the_lds_edges():
    base, bins, V = geometry()
    shape = (3, 50, V // 64 + 5)
    vol = values(shape, "edges")
    for floor in sorted({int(v) for v in np.unique(vol)} | {base - 1, base, base + bins - 1, base + bins, -40000, 40000}):
        check_volume(vol, "above", floor=floor, stats=False)
    ct = values(shape, "ct")
    for floor in (-1024, -1025, 40, 0):
        check_volume(ct, "above", floor=floor)


def test_mask_labels():
    V = geometry()[2]
    for shape in ((3, 50, V // 64 + 5), (2, 64, 128)):
        vol = values(shape, "ct")
        mask = np.random.default_rng(8).integers(0, 3, shape).astype(np.uint8)
        for label in (-1, 1, 2, 7):
            check_volume(vol, "mask", label=label, mask=mask)


def test_empty_selection_and_null_bbox():
    shape = (2, 30, 40)
    vol = values(shape, "ct")
    h, box = run_hist(vol, "above", floor=32767)
    assert not h.any() and box == (2, -1, 30, -1, 40, -1)
    assert run_stats(h) == [0] * 24
    h, box = run_hist(vol, "mask", label=7, mask=np.ones(shape, np.uint8))
    assert not h.any() and box == (2, -1, 30, -1, 40, -1)
    h, box = run_hist(vol, bbox=False)
    assert box is None and np.array_equal(h, ref_hist(vol))


def test_single_voxel_bbox():
    V = geometry()[2]
    for shape in ((3, 40, V // 32 + 7), (2, 5, 8)):
        D, H, W = shape
        spots = [(z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)] + [(D // 2, H // 2, W // 2)]
        for z, y, x in spots:
            vol = np.zeros(shape, np.int16)
            vol[z, y, x] = 5
            h, box = run_hist(vol, "above", floor=0)
            assert box == (z, z, y, y, x, x) and h[32768 + 5] == 1 and h.sum() == 1
        vol = np.zeros(shape, np.int16)
        vol[0, 1, 2], vol[D - 1, H - 2, 1] = 9, 9
        assert run_hist(vol, "above", floor=8)[1] == (0, D - 1, 1, H - 2, 1, 2)


# ---------------------------------------------------------------- 3. statistics
def test_stats_cases():
    h = np.zeros(65536, np.int64)
    h[32768 - 30000], h[32768 + 30000] = 4, 4                    # the median falls between two populated bins far apart
    assert run_stats(h) == ref_stats(h, PNS) and run_stats(h)[16:20] == [3, 500000, -30000, 30000]
    assert run_stats(h, ()) == ref_stats(h, ()) and len(run_stats(h, ())) == 8
    one = np.zeros(65536, np.int64)
    one[32768 - 7] = 1                                           # N = 1
    assert run_stats(one) == ref_stats(one, PNS) == [1, -7, -7, -7, 49, 0, 0, 0] + [0, 0, -7, -7] * 4
    ends = np.zeros(65536, np.int64)
    ends[0], ends[65535], ends[63], ends[64] = 2 ** 32 - 1, 1, 5, 6          # a full counter; bins across two threads' ranges
    for pns, pd in ((PNS, PD), ((1, 2, 3), 3), ((0, 1), 1), ((999999,), PD)):
        assert run_stats(ends, pns, pd) == ref_stats(ends, pns, pd)
    rng = np.random.default_rng(3)
    dense = rng.integers(0, 300, 65536)
    assert run_stats(dense, (1, 333333, 666667, 999999)) == ref_stats(dense, (1, 333333, 666667, 999999))
    hb = torch.zeros(65536 + 1, dtype=torch.int32, device=DEV)                 # a histogram that is only 4-byte aligned
    hb[1:].copy_(torch.from_numpy(dense.astype(np.int32)))
    stats = torch.full((24,), -1, dtype=torch.int64, device=DEV)
    pn, pdv = (C.c_uint * 4)(*PNS), (C.c_uint * 4)(*([PD] * 4))
    check(lib().vu_intensity_stats(C.c_void_p(hb.data_ptr() + 4), pn, pdv, 4, ptr(stats), st()))
    assert stats.cpu().tolist() == ref_stats(dense, PNS)


# ---------------------------------------------------------------- 4. refusals launch nothing
def kernel_counts(fn):
    """The launch profiler's kernel tags of one call, with their counts."""
    L = lib()
    check(L.vu_prof_enable(st()))
    fn()
    return {k: v["count"] for k, v in json.loads(L.vu_prof_report().decode()).items()}


def intensity_launches(fn):
    return sum(c for k, c in kernel_counts(fn).items() if "intensity_hist_kernel" in k)


def test_refusals_launch_nothing():
    vol = torch.zeros(2 * 8 * 12, dtype=torch.int16, device=DEV)
    mask = torch.zeros(2 * 8 * 12, dtype=torch.uint8, device=DEV)
    hist = torch.full((65536 + 1,), -1, dtype=torch.int32, device=DEV)
    bbox = torch.full((8,), -1, dtype=torch.int32, device=DEV)
    stats = torch.full((26,), -1, dtype=torch.int64, device=DEV)
    seen = []

    def all_refusals():
        for kw, word in hist_refusals():
            seen.append((call_hist(vol.data_ptr(), mask.data_ptr(), hist.data_ptr(), bbox.data_ptr(), stream=st(), **kw), word))
        for kw, word in stats_refusals():
            seen.append((call_stats(hist.data_ptr(), stats.data_ptr(), stream=st(), **kw), word))

    assert kernel_counts(all_refusals) == {}
    assert len(seen) == len(hist_refusals()) + len(stats_refusals())
    for (rc, msg), word in seen:
        assert rc == -1 and word in msg, msg
    torch.cuda.synchronize()
    assert bool((hist == -1).all()) and bool((bbox == -1).all()) and bool((stats == -1).all())


# ---------------------------------------------------------------- 5. end to end
def test_normalizer_equals_the_restatement():
    rng = np.random.default_rng(12)
    vol = (np.abs(rng.normal(0, 600, (3, 40, 52))) * (rng.random((3, 40, 52)) < 0.6)).astype(np.int16)       # MR-like: air at 0
    mask = np.zeros(vol.shape, np.uint8)
    mask[:, 8:30, 10:40] = 1
    mask[1, 20:35, 30:50] = 2
    cases = [dict(), dict(lo=2.5, hi=97.5, select="above", floor=0), dict(mode="zscore", k=2.0, select="above"),
             dict(select="mask"), dict(mode="zscore", select="mask", label=2)]
    for kw in cases:
        n = IntensityNormalizer(**kw)
        m = mask if n.select == "mask" else None
        want = ref_window(vol, mask=m, **kw)
        assert n.window(vol, m) == want and n.window(torch.from_numpy(vol).to(DEV), None if m is None else torch.from_numpy(m).to(DEV)) == want
        assert n.window([vol, vol[1]], None if m is None else [m, m[1]]) == [want, ref_window(vol[1], mask=None if m is None else m[1], **kw)]
        assert np.array_equal(n.hist(vol, m).cpu().numpy(), ref_hist(vol, n.select, n.floor, n.label, m))
        assert n.bbox(vol, m) == ref_bbox(vol, n.select, n.floor, n.label, m)
        d, r = n.stats(vol, m), ref_stats(ref_hist(vol, n.select, n.floor, n.label, m), n.pn)
        assert [d["n"], d["min"], d["max"], d["sum"], d["sumsq"]] == r[:5] and d["quantiles"] == [tuple(r[8:12]), tuple(r[12:16])]
    with pytest.raises(VuError, match="empty"):
        IntensityNormalizer(select="above", floor=32767).window(vol)
    assert IntensityNormalizer().window(np.full((4, 9), 77, np.int16)) == (77.0, 78.0)
    assert IntensityNormalizer().bbox(vol[0]) == (0, 0, 0, 39, 0, 51)


def same_result(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k


def test_segmenter_and_patches_with_a_normalizer():
    m, _, _ = small_model(torch.float32)
    rng = np.random.default_rng(31)
    vol = (np.abs(rng.normal(0, 900, (3, 40, 52))) * (rng.random((3, 40, 52)) < 0.7)).astype(np.int16)
    truth = np.zeros(vol.shape, dtype=np.uint8)
    truth[:, 8:30, 10:40] = 1
    kw = dict(overlap=8, batch=8)
    for nkw in (dict(select="above", floor=0), dict(mode="zscore", select="mask")):
        n = IntensityNormalizer(**nkw)
        pair = ref_window(vol, mask=truth if n.select == "mask" else None, **nkw)
        sn, sp = TiledSegmenter(m, window=n, **kw), TiledSegmenter(m, window=pair, **kw)
        same_result(sn.score(vol, truth), sp.score(vol, truth))
        assert intensity_launches(lambda: sn.score(vol, truth)) == 1
        assert intensity_launches(lambda: sp.score(vol, truth)) == 0
        assert intensity_launches(lambda: sn.score(vol, truth, window=pair)) == 0
        same_result(sn.score(vol, truth, window=(-5.0, 300.0)), TiledSegmenter(m, window=(-5.0, 300.0), **kw).score(vol, truth))
        rn, rp = TiledSegmenter(m, window=n, resample=(None, 1, 1), **kw), TiledSegmenter(m, window=pair, resample=(None, 1, 1), **kw)
        same_result(rn.score(vol, truth, spacing=(2, 1.5, 0.75)), rp.score(vol, truth, spacing=(2, 1.5, 0.75)))
        if n.select != "mask":
            assert torch.equal(sn(vol, "logits"), sp(vol, "logits")) and torch.equal(sn(vol), sp(vol))
            assert torch.equal(rn(vol, "logits", spacing=(2, 1.5, 0.75)), rp(vol, "logits", spacing=(2, 1.5, 0.75)))
            both = sn([vol, vol[0]], "logits")
            assert torch.equal(both[0], sp(vol, "logits"))
            assert torch.equal(both[1], TiledSegmenter(m, window=ref_window(vol[0], **nkw), **kw)(vol[0], "logits"))
            assert torch.equal(m.segment(vol, "logits", window=n, **kw), sp(vol, "logits"))
        else:
            with pytest.raises(VuError, match="mask"):
                sn(vol)
        # training patches: the same crops under the measured window and under the pair
        crops = [np.array([[0, 3, 5, 0], [2, 8, 20, 5]])]
        tn = SegmentationPatchTransform(32, 2, train=True, window=n, seed=1)
        tp = SegmentationPatchTransform(32, 2, train=True, window=pair, seed=1)
        a, b = tn(vol, truth, crops=crops), tp(vol, truth, crops=crops)
        assert torch.equal(a["x"], b["x"]) and torch.equal(a["y"], b["y"])
        assert intensity_launches(lambda: tn(vol, truth, crops=crops)) == 1
        assert intensity_launches(lambda: tn(vol, truth, crops=crops, windows=[pair])) == 0
        assert intensity_launches(lambda: tp(vol, truth, crops=crops)) == 0
        c = tn(vol, truth, crops=crops, windows=[pair])
        assert torch.equal(c["x"], b["x"]) and torch.equal(c["y"], b["y"])


def test_run_segmentation_measures_every_volume_once(tmp_path, monkeypatch):
    from vit_unet.torch.run import run_segmentation
    rng = np.random.default_rng(22)
    shapes3 = [(2, 40, 48), (2, 44, 40), (3, 36, 50)]
    vols = [(np.abs(rng.normal(0, 300 * (k + 1), s)) * (rng.random(s) < 0.7)).astype(np.int16) for k, s in enumerate(shapes3)]
    truths = []
    for k, s in enumerate(shapes3):
        tr = np.zeros(s, np.uint8)
        tr[:, 5 + k:25 + k, 8:30] = 1
        truths.append(tr)
    n = IntensityNormalizer(select="above", floor=0)
    calls, run_hist_was = [], IntensityNormalizer.run_hist

    def counted(self, vol, mask=None, bbox=False):
        calls.append(tuple(vol.shape))
        return run_hist_was(self, vol, mask, bbox)

    monkeypatch.setattr(IntensityNormalizer, "run_hist", counted)         # every measurement goes through this one launch site
    res = run_segmentation(vols, truths, n_epochs=1, folds=2, model_string="lite", batch_size=4, im_size=32, crops_per_volume=2,
                           fg=0.5, dtype=torch.float32, folder=str(tmp_path / "models"), seed=1, window=n)
    assert calls == shapes3
    assert res["windows"] == [ref_window(v, select="above", floor=0) for v in vols]
    assert sorted(len(d) for d in res["dice"]) == [1, 2] and 0.0 <= res["dice_mean"] <= 1.0
