"""Volume resampling on the GPU (csrc/vu_resample.hip, segment.VolumeResampler, TiledSegmenter(resample=)).

Through the C ABI with sentinel-filled outputs, against the restatements of tests/test_resample_cpu.py: int16 and uint8 results
EXACTLY, float32 results bit for bit, masks and counts exactly.  The shapes are built around the kernels' own tile
(vu_resample_geometry: tx x ty x tz outputs a workgroup): one short of it, exactly it, one more, two tiles and three, along each
axis; identity, strong reduction, lengths of one, Wo % 4 == 0 (vector stores) and != 0 (scalar ones), and pointers offset by one
element inside a larger allocation whose other bytes must stay as they were.  Two runs of every entry give the same bits.
End to end: VolumeResampler on host and device inputs and lists; TiledSegmenter(resample=) against the chain assembled by
hand - the restatement to the working grid, the segmenter's own native run there (the same call, so bit for bit), the
restatement back, threshold and counts in numpy - with and without clean= and surface=; resample=None is today's segmenter key
for key and bit for bit and launches no resampling kernel; dice_tiled(resample=) and a two-fold run_segmentation(spacings=,
resample=)."""
import ctypes as C
import functools
import json
import math

import numpy as np
import pytest
import torch

from test_gpu_segment import small_model
from test_resample_cpu import ref_mask_counts, ref_resample_f32, ref_resample_i16, ref_resample_u8
from vit_unet.torch import _lib, functions as F
from vit_unet.torch._lib import check, lib, ptr
from vit_unet.torch.segment import (MaskCleaner, SurfaceDistance, TiledSegmenter, VolumeResampler, dice_from_counts, iou_from_counts,
                                    logit_threshold)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def geometry():
    g = [C.c_int(0) for _ in range(3)]
    check(lib().vu_resample_geometry(*(C.byref(v) for v in g)))
    return tuple(v.value for v in g)                                    # tx, ty, tz


def st():
    return _lib.stream_ptr()


@functools.lru_cache(maxsize=None)
def shapes():
    tx, ty, tz = geometry()
    s = [((3, 9, 13), (3, 9, 13)), ((2, 8, 16), (2, 8, 16)),                             # identity, scalar and vector stores
         ((5, 7, 9), (7, 5, 13)), ((1, 6, 6), (1, 9, 4)), ((1, 5, 7), (4, 5, 7)), ((4, 5, 7), (1, 5, 7)),   # D = 1 both ways
         ((4, 1, 6), (4, 5, 7)), ((4, 5, 1), (3, 4, 9)), ((2, 1, 5), (3, 4, 1)),          # a length of one on every axis
         ((3, 64, 64), (3, 3, 100)), ((4, 33, 17), (9, 33, 40))]                         # strong reduction; one axis kept
    s += [((2, 3, 50), (2, 3, w)) for w in (tx - 1, tx, tx + 1, 2 * tx + 3)]
    s += [((2, 5, 6), (2, h, 8)) for h in (ty - 1, ty, ty + 1, 2 * ty + 3)]
    s += [((2, 3, 5), (d, 4, 8)) for d in (tz, tz + 1, 2 * tz + 3)]
    s += [((3, 20, 300), (2, 2 * ty + 3, 2 * tx + 4))]                                   # several workgroups on every axis, reducing
    return tuple(s)


def ids(n):
    return [f"s{k}" for k in range(n)]


NSHAPES = 23


def test_shape_list_is_complete():
    assert len(shapes()) == NSHAPES
    assert any(o[2] % 4 == 0 for _, o in shapes()) and any(o[2] % 4 != 0 for _, o in shapes())


@functools.lru_cache(maxsize=None)
def data_i16(ishape, kind):
    rng = np.random.default_rng(sum(ishape) + len(kind))
    if kind == "random":
        v = rng.integers(-32768, 32768, ishape).astype(np.int16)
        v.reshape(-1)[:2] = (-32768, 32767)
    elif kind == "constant":
        v = np.full(ishape, -1234, np.int16)
    elif kind == "ramp":
        v = ((np.arange(int(np.prod(ishape)), dtype=np.int64) * 37) % 65536 - 32768).astype(np.int16).reshape(ishape)
    else:                                                                # extreme: a -32768 / 32767 checkerboard
        z, y, x = np.indices(ishape)
        v = np.where((z + y + x) % 2 == 0, -32768, 32767).astype(np.int16)
    return v


def run_i16(vol, oshape):
    d = torch.from_numpy(np.array(vol)).to(DEV)
    out = torch.full(oshape, -12345, dtype=torch.int16, device=DEV)
    check(lib().vu_resample_i16(ptr(d), ptr(out), *vol.shape, *oshape, st()))
    return out.cpu().numpy()


def run_u8(m, oshape):
    d = torch.from_numpy(np.array(m)).to(DEV)
    out = torch.full(oshape, 0, dtype=torch.uint8, device=DEV)
    check(lib().vu_resample_u8_nearest(ptr(d), ptr(out), *m.shape, *oshape, st()))
    return out.cpu().numpy()


def run_f32(z, oshape, truth=None, zthr=0.0, label=-1, want=("out", "mask", "counts")):
    """vu_resample_f32 into sentinel-filled outputs -> (out, mask, counts), None for what was not asked for."""
    L = lib()
    d = torch.from_numpy(np.array(z)).to(DEV)
    t = None if truth is None else torch.from_numpy(np.array(truth)).to(DEV)
    Do = oshape[0]
    out = torch.full(oshape, float("nan"), dtype=torch.float32, device=DEV) if "out" in want else None
    mask = torch.full(oshape, 7, dtype=torch.uint8, device=DEV) if "mask" in want else None
    counts = torch.full((Do, 3), -1, dtype=torch.int64, device=DEV) if "counts" in want else None
    nbytes = int(L.vu_resample_f32_scratch_bytes(*oshape)) if counts is not None else 0
    scratch = torch.full((max(nbytes // 4, 1),), -1, dtype=torch.int32, device=DEV) if counts is not None else None
    check(L.vu_resample_f32(ptr(d), ptr(t), ptr(out), ptr(mask), ptr(counts), ptr(scratch), nbytes, *z.shape, *oshape, float(zthr),
                            int(label), st()))
    return tuple(None if a is None else a.cpu().numpy() for a in (out, mask, counts))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- 1. int16
@pytest.mark.parametrize("k", range(NSHAPES), ids=ids(NSHAPES))
def test_resample_i16_exact(k):
    ishape, oshape = shapes()[k]
    for kind in ("random", "constant", "ramp", "extreme"):
        vol = data_i16(ishape, kind)
        want = ref_resample_i16(vol, oshape)
        got = run_i16(vol, oshape)
        assert np.array_equal(got, want), (kind, int(np.abs(got.astype(np.int64) - want).max()))
        if ishape == oshape:
            assert np.array_equal(got, vol)


def offset_case(dtype_t, fill, ishape, oshape, data, launch):
    """Input and output one element into larger allocations: (output, the guard elements before and behind it)."""
    ni, no = int(np.prod(ishape)), int(np.prod(oshape))
    ib = torch.zeros(ni + 2, dtype=dtype_t, device=DEV)
    ib[1:ni + 1].copy_(torch.from_numpy(np.array(data)).reshape(-1))
    ob = torch.full((no + 2,), fill, dtype=dtype_t, device=DEV)
    launch(ib[1:ni + 1].view(ishape), ob[1:no + 1].view(oshape))
    o = ob.cpu()
    return o[1:no + 1].view(oshape).numpy(), o[0], o[-1]


@pytest.mark.parametrize("ishape,oshape", [((2, 8, 16), (3, 9, 20)), ((2, 5, 9), (2, 7, 132)), ((2, 8, 16), (2, 8, 16))])
def test_resample_offset_pointers(ishape, oshape):
    L = lib()
    vol = data_i16(ishape, "random")
    got, lo, hi = offset_case(torch.int16, -12345, ishape, oshape, vol,
                              lambda i, o: check(L.vu_resample_i16(ptr(i), ptr(o), *ishape, *oshape, st())))
    assert np.array_equal(got, ref_resample_i16(vol, oshape)) and lo == -12345 and hi == -12345
    m = (vol.astype(np.int64) & 255).astype(np.uint8)
    got, lo, hi = offset_case(torch.uint8, 77, ishape, oshape, m,
                              lambda i, o: check(L.vu_resample_u8_nearest(ptr(i), ptr(o), *ishape, *oshape, st())))
    assert np.array_equal(got, ref_resample_u8(m, oshape)) and lo == 77 and hi == 77
    z = (vol.astype(np.float32) / np.float32(4096.0))
    no = int(np.prod(oshape))
    truth = torch.zeros(no + 2, dtype=torch.uint8, device=DEV)                      # offset as well
    truth[1::3] = 1
    mb = torch.full((no + 2,), 7, dtype=torch.uint8, device=DEV)
    counts = torch.full((oshape[0], 3), -1, dtype=torch.int64, device=DEV)
    nbytes = int(L.vu_resample_f32_scratch_bytes(*oshape))
    scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=DEV)
    tv, mv = truth[1:no + 1].view(oshape), mb[1:no + 1].view(oshape)
    got, lo, hi = offset_case(torch.float32, float("nan"), ishape, oshape, z,
                              lambda i, o: check(L.vu_resample_f32(ptr(i), ptr(tv), ptr(o), ptr(mv), ptr(counts), ptr(scratch), nbytes,
                                                                   *ishape, *oshape, 0.25, -1, st())))
    want = ref_resample_f32(z, oshape)
    wm, wc = ref_mask_counts(want, tv.cpu().numpy(), 0.25, -1)
    assert np.array_equal(bits(got), bits(want)) and math.isnan(float(lo)) and math.isnan(float(hi))
    assert np.array_equal(mv.cpu().numpy(), wm) and int(mb[0]) == 7 and int(mb[-1]) == 7
    assert np.array_equal(counts.cpu().numpy(), wc)


# ---------------------------------------------------------------- 2. uint8 nearest
@pytest.mark.parametrize("k", range(NSHAPES), ids=ids(NSHAPES))
def test_resample_u8_exact(k):
    ishape, oshape = shapes()[k]
    m = np.random.default_rng(k).integers(0, 256, ishape).astype(np.uint8)
    got = run_u8(m, oshape)
    assert np.array_equal(got, ref_resample_u8(m, oshape))
    assert set(np.unique(got)) <= set(np.unique(m))
    two = (m % 2 * 255).astype(np.uint8)                                  # a {0, 255} mask stays one
    assert np.array_equal(run_u8(two, oshape), ref_resample_u8(two, oshape))


# ---------------------------------------------------------------- 3. float32, mask, counts
@functools.lru_cache(maxsize=None)
def logits(ishape):
    z = (np.random.default_rng(sum(ishape)).standard_normal(ishape) * 3).astype(np.float32)
    return z


@pytest.mark.parametrize("k", range(NSHAPES), ids=ids(NSHAPES))
def test_resample_f32_bit_exact(k):
    ishape, oshape = shapes()[k]
    z = logits(ishape)
    want = ref_resample_f32(z, oshape)
    zthr = (0.0, logit_threshold(0.3))[k % 2]
    label = (-1, 2)[k // 2 % 2]
    truth = np.random.default_rng(k).integers(0, 4, oshape).astype(np.uint8)
    wm, wc = ref_mask_counts(want, truth, zthr, label)
    out, mask, counts = run_f32(z, oshape, truth, zthr, label)
    assert np.array_equal(bits(out), bits(want))
    assert np.array_equal(mask, wm) and np.array_equal(counts, wc)
    if ishape == oshape:
        assert np.array_equal(bits(out), bits(z))


@pytest.mark.parametrize("ishape,oshape", [((5, 7, 9), (7, 5, 13)), ((3, 20, 300), (2, 19, 260))])
def test_resample_f32_outputs_thresholds_labels_truths(ishape, oshape):
    z = np.array(logits(ishape))
    thr3 = logit_threshold(0.3)
    z[:, :3, :4] = 0.0                                                   # constant patches: outputs exactly at either threshold
    z[:, -3:, -4:] = thr3
    want = ref_resample_f32(z, oshape)
    assert (want == 0.0).any() and (want == np.float32(thr3)).any()
    rng = np.random.default_rng(5)
    truths = {"random": rng.integers(0, 4, oshape).astype(np.uint8), "zeros": np.zeros(oshape, np.uint8), "ones": np.ones(oshape, np.uint8)}
    for zthr in (0.0, thr3):
        for label in (-1, 1, 2):
            for name, truth in truths.items():
                wm, wc = ref_mask_counts(want, truth, zthr, label)
                assert wm[want == np.float32(zthr)].all()                # a value at the threshold is inside the mask
                for sel in (("out",), ("mask",), ("counts",), ("out", "mask", "counts")):
                    out, mask, counts = run_f32(z, oshape, truth, zthr, label, want=sel)
                    assert (out is None) == ("out" not in sel) and (mask is None) == ("mask" not in sel)
                    if out is not None:
                        assert np.array_equal(bits(out), bits(want)), (zthr, label, name, sel)
                    if mask is not None:
                        assert np.array_equal(mask, wm), (zthr, label, name, sel)
                    if counts is not None:
                        assert np.array_equal(counts, wc), (zthr, label, name, sel)
    out, mask, counts = run_f32(z, oshape, None, 0.0, -1, want=("out", "mask"))       # no truth at all
    assert counts is None and np.array_equal(bits(out), bits(want)) and np.array_equal(mask, ref_mask_counts(want, truths["zeros"], 0.0, -1)[0])


def test_two_runs_are_bit_equal():
    for ishape, oshape in (((3, 64, 64), (3, 3, 100)), ((4, 33, 17), (9, 33, 40)), ((3, 20, 300), (2, 19, 260))):
        vol, z = data_i16(ishape, "random"), logits(ishape)
        m = (vol.astype(np.int64) & 255).astype(np.uint8)
        truth = (np.arange(int(np.prod(oshape))) % 3).astype(np.uint8).reshape(oshape)
        assert run_i16(vol, oshape).tobytes() == run_i16(vol, oshape).tobytes()
        assert run_u8(m, oshape).tobytes() == run_u8(m, oshape).tobytes()
        a, b = run_f32(z, oshape, truth, 0.1, 1), run_f32(z, oshape, truth, 0.1, 1)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------- 4. VolumeResampler
def test_volume_resampler_class():
    r = VolumeResampler((None, 1, 1))
    vol = data_i16((3, 20, 300), "random")
    sp = (2.5, 1.5, 0.75)
    oshape = r.out_shape(vol.shape, sp)
    assert oshape == (3, 30, 225)
    want = ref_resample_i16(vol, oshape)
    got = r.image(vol, sp)                                               # numpy, host
    assert got.is_cuda and got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(r.image(torch.from_numpy(np.array(vol)), sp).cpu().numpy(), want)          # torch, host
    assert np.array_equal(r.image(torch.from_numpy(np.array(vol)).to(DEV), sp).cpu().numpy(), want)  # torch, device
    one = r.image(vol[1], sp[1:])                                        # a slice with (sy, sx)
    assert tuple(one.shape) == oshape[1:] and np.array_equal(one.cpu().numpy(), ref_resample_i16(vol[1:2], (1,) + oshape[1:])[0])
    m = (vol.astype(np.int64) % 5 * 50).astype(np.uint8)                 # labels 0, 50, ..., 200
    lab = r.labels(m, sp)
    assert lab.dtype == torch.uint8 and np.array_equal(lab.cpu().numpy(), ref_resample_u8(m, oshape))
    assert set(np.unique(lab.cpu().numpy())) <= set(np.unique(m))
    both = r.image([vol, vol[:2]], [sp, (1, 3, 1)])                      # a list, one spacing each
    assert isinstance(both, list) and np.array_equal(both[0].cpu().numpy(), want)
    assert np.array_equal(both[1].cpu().numpy(), ref_resample_i16(vol[:2], (2, 60, 300)))
    same = r.labels([m, m], sp)                                          # a list, one spacing for all
    assert all(np.array_equal(x.cpu().numpy(), ref_resample_u8(m, oshape)) for x in same)
    all3 = VolumeResampler((1.25, 1, 1))                                 # z as well
    o3 = all3.out_shape(vol.shape, sp)
    assert o3 == (6, 30, 225) and np.array_equal(all3.image(vol, sp).cpu().numpy(), ref_resample_i16(vol, o3))
    # the way back
    z = logits(oshape)
    truth = (m > 60).astype(np.uint8)
    back = ref_resample_f32(z, vol.shape)
    wm, wc = ref_mask_counts(back, truth, 0.5, -1)
    res = r.logits_to(z, vol.shape, truth=truth, zthr=0.5)
    assert set(res) == {"logits", "mask", "counts"} and res["counts"].dtype == torch.int64
    assert np.array_equal(bits(res["logits"].cpu().numpy()), bits(back)) and np.array_equal(res["mask"].cpu().numpy(), wm)
    assert np.array_equal(res["counts"].cpu().numpy(), wc)
    res = r.logits_to([torch.from_numpy(np.array(z)).to(DEV), z[0]], [vol.shape, vol.shape[1:]])
    assert set(res[0]) == {"logits", "mask"} and np.array_equal(bits(res[0]["logits"].cpu().numpy()), bits(back))
    assert tuple(res[1]["mask"].shape) == vol.shape[1:]
    assert np.array_equal(bits(res[1]["logits"].cpu().numpy()), bits(ref_resample_f32(z[:1], (1,) + vol.shape[1:])[0]))


# ---------------------------------------------------------------- 5. end to end
def kernel_tags(fn):
    """The launch profiler's kernel tags of one call."""
    L = lib()
    check(L.vu_prof_enable(st()))
    fn()
    return set(json.loads(L.vu_prof_report().decode()))


def same_result(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k


def test_segmenter_with_and_without_resampling():
    m, _, _ = small_model(torch.float32)
    vol = np.random.default_rng(31).integers(-1500, 1500, (3, 40, 52)).astype(np.int16)
    truth = np.zeros(vol.shape, dtype=np.uint8)
    truth[:, 8:30, 10:40] = 1
    truth[1, 20:35, 30:50] = 2
    sp, kw = (2, 1.5, 0.75), dict(overlap=8, batch=8)
    plain = TiledSegmenter(m, **kw)
    # resample=None: today's segmenter, key for key and bit for bit, and nothing new is launched
    base = plain.score(vol, truth)
    same_result(TiledSegmenter(m, resample=None, **kw).score(vol, truth), base)
    assert torch.equal(TiledSegmenter(m, resample=None, **kw)(vol, "logits"), plain(vol, "logits"))
    assert not any("resample" in t for t in kernel_tags(lambda: TiledSegmenter(m, resample=None, **kw).score(vol, truth)))
    # the chain by hand: restatement to the working grid, the segmenter's own native run there, restatement back
    r = VolumeResampler((None, 1, 1))
    wshape = r.out_shape(vol.shape, sp)
    assert wshape == (3, 60, 39)
    work = ref_resample_i16(vol, wshape)
    zw = plain(work, "logits").cpu().numpy()
    zn = ref_resample_f32(zw, vol.shape)
    # a threshold inside the logits' range, so that the mask has structure whatever the weights are
    thr = float(1.0 / (1.0 + np.exp(-np.float64(np.median(zn)))))
    s = TiledSegmenter(m, threshold=thr, resample=(None, 1, 1), **kw)
    wm, wc = ref_mask_counts(zn, truth, s.zthr, -1)
    assert 0 < wm.sum() < wm.size
    tags = kernel_tags(lambda: s.score(vol, truth, spacing=sp))
    assert {"resample_i16_kernel", "resample_f32_kernel"} <= tags
    res = s.score(vol, truth, spacing=sp)
    assert set(res) == set(base) and np.array_equal(res["mask"].cpu().numpy(), wm) and np.array_equal(res["counts"].numpy(), wc)
    p, t, b = (int(c) for c in wc.sum(0))
    assert res["dice"] == dice_from_counts(p, t, b) and res["iou"] == iou_from_counts(p, t, b)
    assert np.array_equal(bits(s(vol, "logits", spacing=sp).cpu().numpy()), bits(zn))
    assert torch.equal(s(vol, "prob", spacing=sp), torch.sigmoid(torch.from_numpy(zn).to(DEV)))
    assert np.array_equal(s(vol, "mask", spacing=sp).cpu().numpy(), wm)
    assert np.array_equal(m.segment(vol, spacing=sp, threshold=thr, resample=(None, 1, 1), **kw).cpu().numpy(), wm)
    both = s([vol, vol[0]], "mask", spacing=[sp, sp])                                   # a list; a single slice
    assert np.array_equal(both[0].cpu().numpy(), wm) and tuple(both[1].shape) == vol.shape[1:]
    # label rule 2, through the same pass
    s2 = TiledSegmenter(m, threshold=thr, label=2, resample=r, **kw)
    assert np.array_equal(s2.score(vol, truth, spacing=sp)["counts"].numpy(), ref_mask_counts(zn, truth, s.zthr, 2)[1])
    # the same chain on the device from the public pieces
    dz = r.logits_to(plain(r.image(vol, sp), "logits"), vol.shape, truth=truth, zthr=s.zthr)
    assert np.array_equal(dz["mask"].cpu().numpy(), wm) and np.array_equal(dz["counts"].cpu().numpy(), wc)
    assert F.dice_tiled(m, [(vol, truth, sp)], threshold=thr, resample=(None, 1, 1), **kw).tolist() == [res["dice"]]
    assert F.iou_tiled(m, [(vol, truth, sp)], threshold=thr, resample=r, **kw).tolist() == [res["iou"]]
    # clean= and surface= work on the native-grid mask exactly as without a resampler
    cleaner, sd = MaskCleaner(8, min_size=4, keep_largest=True, fill_holes=True), SurfaceDistance(2, (1, 1, 1), tolerance=2.0)
    rc = TiledSegmenter(m, threshold=thr, resample=r, clean=cleaner, **kw).score(vol, truth, spacing=sp)
    cm = cleaner(wm).cpu().numpy()
    assert np.array_equal(rc["mask"].cpu().numpy(), cm) and np.array_equal(rc["raw_counts"].numpy(), wc)
    assert np.array_equal(rc["counts"].numpy(), ref_mask_counts(cm.astype(np.float32), truth, 0.5, -1)[1])
    rs = TiledSegmenter(m, threshold=thr, resample=r, surface=sd, **kw).score(vol, truth, spacing=sp)
    assert np.array_equal(rs["mask"].cpu().numpy(), wm) and set(rs) == set(base) | {"surface"}
    want = sd.score(wm, truth)
    assert torch.equal(rs["surface"]["stats"], want["stats"]) and rs["surface"]["hd95"] == want["hd95"]
    rcs = TiledSegmenter(m, threshold=thr, resample=r, clean=cleaner, surface=sd, **kw).score(vol, truth, spacing=sp)
    assert torch.equal(rcs["surface"]["stats"], sd.score(cm, truth)["stats"])
    assert F.hd95_tiled(m, [(vol, truth, sp)], threshold=thr, surface=sd, resample=r, **kw).tolist() == [want["hd95"]]
    assert F.assd_tiled(m, [(vol, truth, sp)], threshold=thr, surface=sd, resample=r, **kw).tolist() == [want["assd"]]
    assert F.nsd_tiled(m, [(vol, truth, sp)], threshold=thr, surface=sd, resample=r, **kw).tolist() == [want["nsd"]]


def test_run_segmentation_with_resampling(tmp_path):
    from vit_unet.torch.run import run_segmentation
    rng = np.random.default_rng(22)
    shapes3, spacings = [(2, 40, 48), (2, 44, 40), (3, 36, 50)], [(2, 1, 1), (2, 1.25, 1.25), (3, 0.9, 0.8)]
    vols = [rng.integers(-1500, 1500, s).astype(np.int16) for s in shapes3]
    truths = []
    for k, s in enumerate(shapes3):
        tr = np.zeros(s, np.uint8)
        tr[:, 5 + k:25 + k, 8:30] = 1
        truths.append(tr)
    res = run_segmentation(vols, truths, n_epochs=1, folds=2, model_string="lite", batch_size=4, im_size=32, crops_per_volume=2,
                           fg=0.5, dtype=torch.float32, folder=str(tmp_path / "models"), seed=1, spacings=spacings,
                           resample=(None, 1, 1))
    assert sorted(len(d) for d in res["dice"]) == [1, 2] and 0.0 <= res["dice_mean"] <= 1.0
    assert all(((d >= 0.0) & (d <= 1.0)).all() for d in res["dice"])
    with pytest.raises(AssertionError):
        run_segmentation(vols, truths, n_epochs=1, folds=2, im_size=32, folder=str(tmp_path / "models"), spacings=spacings)
