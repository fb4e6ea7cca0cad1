"""Segmentation mask clean-up on the GPU (csrc/vu_segclean.hip, segment.MaskCleaner, TiledSegmenter(clean=)).

Everything is integer arithmetic, so every comparison is EXACT, through the C ABI with sentinel-filled outputs, against the
flood-fill restatements of tests/test_segclean_cpu.py:
  vu_cc_label    labels and sizes == ref_label, conn 4 / 8 (fg 0 and 1) and 6 / 26, on masks built around the kernel's own tile
                 (vu_cc_tile): structures on tile borders and corners, long chains across many tiles, the worst LDS convergence
  vu_seg_clean   out, counts and stats == ref_clean / numpy counts over min_size x keep_largest x fill_holes; overflow == 0
  two runs of the same call are bit-equal
End to end: TiledSegmenter(clean=None) is today's segmenter bit for bit, with a cleaner the mask is ref_clean of the raw mask,
dice_tiled(clean=) agrees and a two-fold run_segmentation(clean=) finishes."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from test_gpu_segment import small_model, volume_i16
from test_segclean_cpu import ref_clean, ref_counts, ref_label
from vit_unet.torch import _lib, functions as F
from vit_unet.torch._lib import check, lib, ptr
from vit_unet.torch.segment import MaskCleaner, TiledSegmenter, dice_from_counts, iou_from_counts

pytestmark = pytest.mark.gpu
DEV = "cuda"


def tile():
    th, tw = C.c_int(0), C.c_int(0)
    check(lib().vu_cc_tile(C.byref(th), C.byref(tw)))
    return th.value, tw.value


def st():
    return _lib.stream_ptr()


# ---------------------------------------------------------------- masks, by name (built once, never changed)
def serpentine(H, W):
    """A one-pixel-wide path that fills the slice: every other row is full, the rows between hold one pixel at alternating ends."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[0::2] = 1
    m[1::4, W - 1] = 1
    m[3::4, 0] = 1
    return m


def spiral(H, W):
    """A one-pixel-wide rectangular spiral with one-pixel gaps, wound inwards from the top-left corner."""
    m = np.zeros((H, W), dtype=np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1
    while True:
        moved = False
        for _ in range(2):                                  # go on, or turn right once
            ny, nx = y + dy, x + dx
            ay, ax = ny + dy, nx + dx                       # the pixel after the next must be free too (keeps the gap)
            if 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
                y, x, moved = ny, nx, True
                m[y, x] = 1
                break
            dy, dx = dx, -dy
        if not moved:
            return m


@functools.lru_cache(maxsize=None)
def case(name):
    th, tw = tile()
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "zeros":
        return np.zeros((2, th + 3, tw + 5), dtype=np.uint8)
    if name == "ones":
        return np.full((2, th + 3, tw + 5), 255, dtype=np.uint8)
    if name == "last_pixel":
        m = np.zeros((2, th + 1, tw + 1), dtype=np.uint8)
        m[-1, -1, -1] = 1
        return m
    if name == "checkerboard":
        yy, xx = np.mgrid[0:2 * th + 1, 0:tw + 3]
        return ((yy + xx) % 2).astype(np.uint8)[None]
    if name == "odd_w":
        return (rng.random((3, 37, 45)) < 0.5).astype(np.uint8)
    if name == "w_mod_4":
        return (rng.random((2, th + 8, 2 * tw)) < 0.45).astype(np.uint8)
    if name == "small_slice":
        return (rng.random((1, 8, 8)) < 0.5).astype(np.uint8)
    if name == "serpentine":
        return serpentine(3 * th, 3 * tw)[None]
    if name == "serpentine_t":                                # columns instead of rows: the chain crosses horizontal tile borders
        return np.ascontiguousarray(serpentine(3 * tw, 3 * th).T)[None]
    if name == "spiral":
        return spiral(th, tw)[None]
    if name == "corner":                                     # two blobs that meet only diagonally through a tile corner, both ways
        m = np.zeros((2, 2 * th, 2 * tw), dtype=np.uint8)
        m[0, th - 4:th, tw - 6:tw] = 1
        m[0, th:th + 3, tw:tw + 5] = 1
        m[1, th - 4:th, tw:tw + 6] = 1
        m[1, th:th + 3, tw - 5:tw] = 1
        return m
    if name == "random20":
        return (rng.random((2, 2 * th + 5, 2 * tw + 7)) < 0.2).astype(np.uint8)
    if name == "random60":
        return (rng.random((2, 2 * th + 5, 2 * tw + 7)) < 0.6).astype(np.uint8) * 3
    if name == "twins":                                      # two slices with identical content get independent labels
        s = (rng.random((th + 2, tw + 2)) < 0.55).astype(np.uint8)
        return np.stack([s, s])
    # ---- volumes
    if name == "through_z":                                  # two bars in slice 0 joined only by a bridge in slice 1
        m = np.zeros((3, th + 2, tw + 2), dtype=np.uint8)
        m[0, 2, :] = 1
        m[0, th, :] = 1
        m[1, 2:th + 1, tw] = 1
        m[2, 5, 5] = 1
        return m
    if name == "diag3d":                                     # joined only through a 3-D diagonal across a tile corner
        m = np.zeros((3, 2 * th, 2 * tw), dtype=np.uint8)
        m[0, th - 3:th, tw - 3:tw] = 1
        m[1, th:th + 3, tw:tw + 3] = 1
        m[1, 0, 2 * tw - 1] = 1
        m[2, 1, 2 * tw - 2] = 1
        return m
    if name == "hollow_box":
        m = np.zeros((5, th + 4, tw + 4), dtype=np.uint8)
        m[1:4, 2:th + 2, 2:tw + 2] = 1
        m[2, 3:th + 1, 3:tw + 1] = 0
        return m
    if name == "random3d":
        return (rng.random((5, 2 * th + 3, 2 * tw + 5)) < 0.35).astype(np.uint8)
    if name == "random3d_dense":
        return (rng.random((4, th + 3, tw + 5)) < 0.8).astype(np.uint8)
    # ---- clean-up
    if name == "tie":                                        # three components of 6 pixels, one of 5, one pixel; slice 1: two of 4
        m = np.zeros((2, th + 4, tw + 9), dtype=np.uint8)
        m[0, 1:3, 10:13] = 1
        m[0, 1:4, tw - 1:tw + 1] = 1
        m[0, th - 1:th + 1, 3:6] = 1
        m[0, th + 2, 20:25] = 1
        m[0, 8, 30] = 1
        m[1, 5:7, tw + 2:tw + 4] = 1
        m[1, 5:7, 2:4] = 1
        return m
    if name == "holes":                                      # a hole open to the border, a ring around a small blob, a closed hole
        m = np.zeros((1, 2 * th + 2, tw + 12), dtype=np.uint8)
        m[0, 0:6, 2:9] = 1
        m[0, 0:5, 4:7] = 0                                   # open to the top edge
        m[0, th - 5:th + 6, tw - 7:tw + 6] = 1               # a ring across a tile corner ...
        m[0, th - 3:th + 4, tw - 5:tw + 4] = 0
        m[0, th, tw - 1:tw + 1] = 1                          # ... whose hole holds a 2-pixel blob
        m[0, th + 8:th + 14, 3:12] = 1
        m[0, th + 10:th + 12, 5:9] = 0                       # closed
        m[0, th + 9, 4] = 0
        m[0, th + 10, 5 - 1] = 1
        return m
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def label_ref(name, conn, fg):
    return ref_label(case(name), conn, fg)


def run_label(mask, conn, fg, with_sizes=True):
    """One vu_cc_label into sentinel-filled outputs -> (labels, sizes or None, overflow word), on the host."""
    L = lib()
    D, H, W = mask.shape
    d = torch.from_numpy(mask).to(DEV)
    labels = torch.full((D, H, W), -7, dtype=torch.int32, device=DEV)
    sizes = torch.full((D, H, W), 0x5a5a5a5a, dtype=torch.int32, device=DEV) if with_sizes else None
    nbytes = int(L.vu_cc_scratch_bytes(D, H, W))
    scratch = torch.full(((nbytes + 3) // 4,), -1, dtype=torch.int32, device=DEV)
    check(L.vu_cc_label(ptr(d), ptr(labels), ptr(sizes), ptr(scratch), nbytes, D, H, W, conn, fg, st()), "vu_cc_label")
    torch.cuda.synchronize()
    assert torch.equal(d.cpu(), torch.from_numpy(mask))                       # the input is left alone
    return labels.cpu().numpy(), (sizes.cpu().numpy().view(np.uint32) if with_sizes else None), int(scratch[0])


SLICE_CASES = ["zeros", "ones", "last_pixel", "checkerboard", "odd_w", "w_mod_4", "small_slice", "serpentine", "serpentine_t",
               "spiral", "corner", "random20", "random60", "twins"]
VOLUME_CASES = ["through_z", "diag3d", "hollow_box", "random3d", "random3d_dense"]


# ---------------------------------------------------------------- 1. labelling
@pytest.mark.parametrize("fg", [1, 0])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", SLICE_CASES)
def test_cc_label_slices(name, conn, fg):
    mask = case(name)
    want_l, want_s = label_ref(name, conn, fg)
    got_l, got_s, ovf = run_label(mask, conn, fg)
    assert ovf == 0
    assert np.array_equal(got_l, want_l), np.argwhere(got_l != want_l)[:5]
    assert np.array_equal(got_s, want_s), np.argwhere(got_s != want_s)[:5]


def test_cc_label_known_structures():
    th, tw = tile()
    n4 = lambda name, fg=1: int((label_ref(name, 4, fg)[1] != 0).sum())
    n8 = lambda name, fg=1: int((label_ref(name, 8, fg)[1] != 0).sum())
    H, W = case("checkerboard").shape[1:]
    assert n4("checkerboard") == (H * W) // 2 and n8("checkerboard") == 1     # the most components / one component
    assert n4("serpentine") == 1 and n8("serpentine") == 1 and int(label_ref("serpentine", 4, 1)[1][0, 0, 0]) == int(case("serpentine").sum())
    assert n4("spiral") == 1 and case("spiral").sum() > th * tw // 3
    assert n8("corner") == 2 and n4("corner") == 4                             # one component a slice under 8, two under 4
    l = label_ref("twins", 8, 1)[0]
    assert np.array_equal(l[1][l[1] >= 0], l[0][l[0] >= 0] + l[0].size)        # independent labels: slice 1 = slice 0 + H W
    assert n8("ones") == 2 and n8("zeros") == 0 and n8("zeros", 0) == 2 and n8("last_pixel") == 1


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("name", VOLUME_CASES)
def test_cc_label_volumes(name, conn):
    mask = case(name)
    for fg in ((1, 0) if name in ("hollow_box", "random3d_dense") else (1,)):
        want_l, want_s = label_ref(name, conn, fg)
        got_l, got_s, ovf = run_label(mask, conn, fg)
        assert ovf == 0
        assert np.array_equal(got_l, want_l), (fg, np.argwhere(got_l != want_l)[:5])
        assert np.array_equal(got_s, want_s), (fg, np.argwhere(got_s != want_s)[:5])
    n = lambda c: int((label_ref(name, c, 1)[1] != 0).sum())
    if name == "through_z":
        assert n(6) == 2 and int((label_ref(name, 4, 1)[1] != 0).sum()) == 4    # the bars are one component only through z
    if name == "diag3d":
        assert n(26) == 2 and n(6) == 4
    if name == "hollow_box":
        assert int((label_ref(name, 6, 0)[1] != 0).sum()) == 2                  # the outside and the cavity


def test_cc_label_without_sizes_and_unaligned_buffers():
    mask = case("random60")
    want_l, want_s = label_ref("random60", 8, 1)
    got_l, got_s, ovf = run_label(mask, 8, 1, with_sizes=False)
    assert ovf == 0 and got_s is None and np.array_equal(got_l, want_l)
    # a mask one byte and labels / sizes one word off their allocation: the scalar paths of a W % 4 == 0 shape
    m = case("w_mod_4")
    D, H, W = m.shape
    buf = torch.zeros(m.size + 1, dtype=torch.uint8, device=DEV)
    buf[1:].copy_(torch.from_numpy(m).reshape(-1))
    lab = torch.full((m.size + 1,), -7, dtype=torch.int32, device=DEV)
    siz = torch.full((m.size + 1,), -7, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(4, dtype=torch.int32, device=DEV)
    check(lib().vu_cc_label(ptr(buf[1:]), ptr(lab[1:]), ptr(siz[1:]), ptr(scratch), 16, D, H, W, 4, 1, st()))
    want_l, want_s = label_ref("w_mod_4", 4, 1)
    assert int(lab[0]) == -7 and int(siz[0]) == -7 and int(scratch[0]) == 0
    assert np.array_equal(lab[1:].cpu().numpy().reshape(m.shape), want_l)
    assert np.array_equal(siz[1:].cpu().numpy().view(np.uint32).reshape(m.shape), want_s)


# ---------------------------------------------------------------- 2. clean-up
def run_clean(mask, conn, min_size, keep, fill, truth=None, label=-1, alias=False, stats=True):
    L = lib()
    D, H, W = mask.shape
    U = 1 if conn in (6, 26) else D
    d = torch.from_numpy(mask).to(DEV)
    out = d if alias else torch.full((D, H, W), 0xAA, dtype=torch.uint8, device=DEV)
    t = torch.from_numpy(truth).to(DEV) if truth is not None else None
    counts = torch.full((D, 3), -1, dtype=torch.int64, device=DEV) if truth is not None else None
    sts = torch.full((U, 4), -1, dtype=torch.int64, device=DEV) if stats else None
    nbytes = int(L.vu_seg_clean_scratch_bytes(D, H, W))
    scratch = torch.full(((nbytes + 15) // 16 * 4,), -1, dtype=torch.int32, device=DEV)
    check(L.vu_seg_clean(ptr(d), ptr(t), ptr(out), ptr(counts), ptr(sts), ptr(scratch), nbytes, D, H, W, conn, min_size, keep, fill,
                         label, st()), "vu_seg_clean")
    torch.cuda.synchronize()
    if not alias:
        assert torch.equal(d.cpu(), torch.from_numpy(mask))
    return (out.cpu().numpy(), counts.cpu().numpy() if counts is not None else None, sts.cpu().numpy() if stats else None)


@functools.lru_cache(maxsize=None)
def clean_ref(name, conn, min_size, keep, fill):
    return ref_clean(case(name), conn, min_size, bool(keep), bool(fill))


@functools.lru_cache(maxsize=None)
def truth_of(name):
    m = case(name)
    rng = np.random.default_rng(m.size)
    return ((rng.random(m.shape) < 0.5) * rng.integers(1, 4, m.shape)).astype(np.uint8)


# (mask, conn): an exact size tie, holes (open, closed, a ring around a blob), odd W, long chains, both volume connectivities
CLEAN_CASES = [("tie", 4), ("tie", 8), ("holes", 8), ("holes", 4), ("odd_w", 8), ("random60", 4), ("serpentine", 8), ("corner", 4),
               ("hollow_box", 26), ("hollow_box", 6), ("random3d_dense", 6), ("random3d", 26), ("zeros", 8), ("ones", 4)]


@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("min_size", [0, 5])
@pytest.mark.parametrize("name,conn", CLEAN_CASES)
def test_seg_clean(name, conn, min_size, keep, fill):
    mask = case(name)
    want, want_stats = clean_ref(name, conn, min_size, keep, fill)
    truth = truth_of(name)
    k = CLEAN_CASES.index((name, conn)) + min_size + keep + fill
    label = -1 if k % 2 == 0 else 2                                            # both truth rules
    alias = k % 3 == 0                                                         # out aliasing mask
    out, counts, stats = run_clean(mask, conn, min_size, keep, fill, truth, label, alias=alias)
    assert np.array_equal(out, want), np.argwhere(out != want)[:5]
    assert np.array_equal(counts, ref_counts(want, truth, label))
    assert np.array_equal(stats, want_stats), (stats, want_stats)
    assert (stats[:, 3] == 0).all()
    # no truth, no stats: the same mask
    out2, c2, s2 = run_clean(mask, conn, min_size, keep, fill, stats=False)
    assert c2 is None and s2 is None and np.array_equal(out2, want)


def test_seg_clean_known_answers():
    tie = clean_ref("tie", 4, 0, 1, 0)
    th, tw = tile()
    assert tie[1].tolist() == [[5, 1, 6, 0], [2, 1, 4, 0]]
    assert tie[0][0].sum() == 6 and tie[0][0, 1:3, 10:13].all()                # the tie goes to the smallest root
    assert tie[0][1].sum() == 4 and tie[0][1, 5:7, 2:4].all()
    assert clean_ref("tie", 4, 7, 1, 0)[0].sum() == 0                          # nothing left: the unit stays empty
    h0, h5 = clean_ref("holes", 8, 0, 0, 1)[0][0], clean_ref("holes", 8, 5, 0, 1)[0][0]
    raw = case("holes")[0]
    assert not h0[0:5, 4:7].any()                                              # open to the border: not filled
    assert h0[th - 3:th + 4, tw - 5:tw + 4].all() and h5[th - 3:th + 4, tw - 5:tw + 4].all()   # with or without the blob
    assert h0[th + 10:th + 12, 5:9].all() and h0.sum() > raw.sum()


def test_two_runs_are_bit_equal():
    for name, conn in (("random60", 8), ("serpentine", 4), ("random3d", 26)):
        mask = case(name)
        a, b = run_label(mask, conn, 1), run_label(mask, conn, 1)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 0
        truth = truth_of(name)
        a, b = run_clean(mask, conn, 5, 1, 1, truth), run_clean(mask, conn, 5, 1, 1, truth)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 3. MaskCleaner
def test_mask_cleaner():
    mask = case("holes")
    want, want_stats = clean_ref("holes", 8, 5, 1, 1)
    c = MaskCleaner(8, min_size=5, keep_largest=True, fill_holes=True)
    got = c(mask)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(c(torch.from_numpy(mask[0]).to(DEV)).cpu().numpy(), want[0])       # (H,W), on the device
    assert [np.array_equal(g.cpu().numpy(), want) for g in c([mask, mask])] == [True, True]
    labels, sizes = MaskCleaner(4).labels(case("odd_w"))
    wl, ws = label_ref("odd_w", 4, 1)
    assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), wl) and np.array_equal(sizes.cpu().numpy(), ws.astype(np.int64))
    truth = truth_of("holes")
    res = c.score(mask, truth, label=2)
    counts = ref_counts(want, truth, 2)
    assert np.array_equal(res["mask"].cpu().numpy(), want) and np.array_equal(res["counts"].numpy(), counts)
    assert np.array_equal(res["stats"].numpy(), want_stats)
    assert res["dice"] == dice_from_counts(*counts.sum(0)) and res["iou"] == iou_from_counts(*counts.sum(0))
    v = MaskCleaner(26, fill_holes=True)(case("hollow_box"))
    assert np.array_equal(v.cpu().numpy(), clean_ref("hollow_box", 26, 0, 0, 1)[0]) and int(v.sum()) > int(case("hollow_box").sum())


# ---------------------------------------------------------------- 4. end to end
def test_segmenter_with_and_without_a_cleaner():
    m, _, _ = small_model(torch.float32)
    vol = volume_i16(3, 70, 90, seed=4)
    vol = (vol // 24).astype(np.int16)                                        # inside the window: a mask with structure
    truth = np.zeros(vol.shape, dtype=np.uint8)
    truth[:, 10:50, 20:70] = 1
    kw = dict(overlap=8, batch=8)
    plain = TiledSegmenter(m, **kw)
    raw = plain(vol)
    base = plain.score(vol, truth)
    none = TiledSegmenter(m, clean=None, **kw)
    assert torch.equal(none(vol), raw) and torch.equal(none.score(vol, truth)["mask"], raw)
    assert torch.equal(none.score(vol, truth)["counts"], base["counts"]) and set(none.score(vol, truth)) == set(base)
    rawn = raw.cpu().numpy()
    assert 0 < rawn.sum() < rawn.size
    for cleaner in (MaskCleaner(8, min_size=4, keep_largest=True, fill_holes=True), MaskCleaner(6, min_size=3, fill_holes=True)):
        want, want_stats = ref_clean(rawn, cleaner.connectivity, cleaner.min_size, cleaner.keep_largest, cleaner.fill_holes)
        s = TiledSegmenter(m, clean=cleaner, **kw)
        assert np.array_equal(s(vol).cpu().numpy(), want)
        res = s.score(vol, truth)
        counts = ref_counts(want, truth, -1)
        assert np.array_equal(res["mask"].cpu().numpy(), want) and np.array_equal(res["counts"].numpy(), counts)
        assert torch.equal(res["raw_counts"], base["counts"]) and np.array_equal(res["stats"].numpy(), want_stats)
        assert res["dice"] == dice_from_counts(*counts.sum(0)) and res["iou"] == iou_from_counts(*counts.sum(0))
        assert F.dice_tiled(m, [(vol, truth)], clean=cleaner, **kw).tolist() == [res["dice"]]
        assert F.iou_tiled(m, [(vol, truth)], clean=cleaner, **kw).tolist() == [res["iou"]]
        assert np.array_equal(m.segment(vol, clean=cleaner, **kw).cpu().numpy(), want)
        for output in ("logits", "prob"):
            with pytest.raises(_lib.VuError):
                s(vol, output)
    assert F.dice_tiled(m, [(vol, truth)], **kw).tolist() == [base["dice"]]


def test_run_segmentation_with_a_cleaner(tmp_path):
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
                           clean=MaskCleaner(8, min_size=3, keep_largest=True, fill_holes=True))
    assert [len(d) for d in res["dice"]] == [2, 2] and all(((d >= 0.0) & (d <= 1.0)).all() for d in res["dice"])
    assert 0.0 <= res["dice_mean"] <= 1.0 and np.isfinite(res["dice_std"])
