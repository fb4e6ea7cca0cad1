"""Whole-slice / volume segmentation, host side (no GPU): Dice and IoU from integer counts, the logit threshold, every argument
error of `segment.TiledSegmenter` and of the C entry points vu_tile_gather_i16 / vu_seg_blend that is decided on the host
(before any launch; the pointers below are never dereferenced), and the numpy restatement - window numbering across the
slices of a volume, mask and counts from the float64 blend - that tests/test_gpu_segment.py holds the HIP kernels against."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_restore_cpu import ref_axis, ref_blend, ref_src
from vit_unet.torch import _lib
from vit_unet.torch import model as M
from vit_unet.torch.segment import TiledSegmenter, dice_from_counts, iou_from_counts, logit_threshold


# ---------------------------------------------------------------- numpy restatement (independent of the C code)
def ref_nt(H, W, T, overlap):
    return len(ref_axis(H, T, overlap)) * len(ref_axis(W, T, overlap))


def ref_volume_windows(vol, T, overlap, g0=0, n=None):
    """(D,H,W) volume -> windows [g0, g0 + n) as (n,T,T), numbered over the whole volume: g = z nt + t, t = ty nx + tx."""
    D, H, W = vol.shape
    oys, oxs = ref_axis(H, T, overlap), ref_axis(W, T, overlap)
    nt = len(oys) * len(oxs)
    n = D * nt - g0 if n is None else n
    out = []
    for g in range(g0, g0 + n):
        z, t = divmod(g, nt)
        oy, ox = oys[t // len(oxs)], oxs[t % len(oxs)]
        out.append(vol[z][ref_src(H, T, oy)][:, ref_src(W, T, ox)])
    return np.stack(out)


def ref_truth_pixels(truth, label):
    return truth != 0 if label < 0 else truth == label


def ref_counts(mask, truth, label):
    """(nz,H,W) mask (0 / 1) and truth labels -> (nz,3) int64: mask pixels, truth pixels, both."""
    m, t = mask.astype(bool), ref_truth_pixels(truth, label)
    return np.stack([m.sum((1, 2)), t.sum((1, 2)), (m & t).sum((1, 2))], axis=1).astype(np.int64)


def ref_seg_blend(tiles, nz, H, W, T, overlap, zthr):
    """tiles (nz nt,1,T,T) -> (z (nz,H,W) float64: the float64 blend of every slice, mask = z >= zthr as uint8)."""
    nt = ref_nt(H, W, T, overlap)
    assert tiles.shape == (nz * nt, 1, T, T)
    z = np.stack([ref_blend(tiles[s * nt:(s + 1) * nt], H, W, T, overlap)[0] for s in range(nz)])
    return z, (z >= zthr).astype(np.uint8)


# ---------------------------------------------------------------- 1. Dice / IoU from counts, the threshold
def test_dice_and_iou_from_counts():
    assert dice_from_counts(0, 0, 0) == 1.0 and iou_from_counts(0, 0, 0) == 1.0          # empty against empty
    assert dice_from_counts(5, 7, 0) == 0.0 and iou_from_counts(5, 7, 0) == 0.0          # disjoint
    assert dice_from_counts(0, 7, 0) == 0.0 and iou_from_counts(3, 0, 0) == 0.0          # one side empty
    assert dice_from_counts(4, 4, 4) == 1.0 and iou_from_counts(4, 4, 4) == 1.0
    assert dice_from_counts(3, 5, 2) == 0.5 and iou_from_counts(3, 5, 2) == 2 / 6
    assert dice_from_counts(10, 30, 10) == 0.5 and iou_from_counts(10, 30, 10) == 10 / 30
    big = 3 * 2 ** 40                                                                    # beyond int32 and float32
    assert dice_from_counts(big, big, big) == 1.0 and iou_from_counts(2 * big, big, big) == 0.5
    c = torch.tensor([[3, 5, 2], [1, 1, 0]]).sum(0)                                      # as score() calls them
    assert dice_from_counts(*(int(v) for v in c)) == 0.4


def test_logit_threshold_values():
    assert logit_threshold(0.5) == 0.0 and math.copysign(1.0, logit_threshold(0.5)) == 1.0
    assert logit_threshold(0.3) == float(np.float32(math.log(0.3 / 0.7))) and abs(logit_threshold(0.3) + 0.8472979) < 1e-6
    assert logit_threshold(0.9) == float(np.float32(math.log(0.9 / (1 - 0.9)))) and abs(logit_threshold(0.9) - 2.1972246) < 1e-6
    for thr in (0.5, 0.3, 0.9):                                                          # a float32 value, as the C call takes it
        assert logit_threshold(thr) == C.c_float(logit_threshold(thr)).value
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(_lib.VuError, match="threshold"):
            logit_threshold(bad)


# ---------------------------------------------------------------- 2. argument errors
def seg_model(channels=1):
    return M.HViT_UNet(1, 1, 1, "conv", 32, 8, channels, 16, 2, 0., 0., 0.)


def test_segmenter_argument_errors():
    m = seg_model()
    for kw, word in ((dict(window=(100.0, 100.0)), "window"), (dict(window=(5.0, -5.0)), "window"), (dict(threshold=0.0), "threshold"),
                     (dict(threshold=1.0), "threshold"), (dict(threshold=-2), "threshold"), (dict(overlap=17), "overlap"),
                     (dict(overlap=-1), "overlap"), (dict(batch=0), "batch"), (dict(label=256), "label"), (dict(ensemble=3), "ensemble")):
        with pytest.raises(_lib.VuError, match=word):
            TiledSegmenter(m, **{"overlap": 8, **kw})       # the default overlap of 32 is for im_size 224
    with pytest.raises(_lib.VuError, match="channel"):
        TiledSegmenter(seg_model(3), overlap=8)
    s = TiledSegmenter(m, overlap=16, batch=4, window=(-1000, 2000), threshold=0.3, label=2, ensemble=2)
    assert (s.T, s.overlap, s.batch, s.window, s.label, s.ensemble) == (32, 16, 4, (-1000.0, 2000.0), 2, 2)
    assert s.zthr == logit_threshold(0.3) and TiledSegmenter(m, overlap=8).zthr == 0.0
    vol = np.zeros((2, 40, 40), np.int16)
    for bad in (vol.astype(np.float32), vol.astype(np.uint8), torch.zeros(40, 40), np.zeros((1, 2, 40, 40), np.int16),
                np.zeros(40, np.int16), "volume"):
        with pytest.raises(_lib.VuError, match="int16"):
            s(bad)
    with pytest.raises(_lib.VuError, match="output"):
        s(vol, output="labels")
    for truth in (np.zeros((2, 40, 41), np.uint8), np.zeros((40, 40), np.uint8), np.zeros((3, 40, 40), np.uint8)):
        with pytest.raises(_lib.VuError, match="shape"):
            s.score(vol, truth)
    with pytest.raises(_lib.VuError, match="uint8"):
        s.score(vol, np.zeros((2, 40, 40), np.int16))
    # a CPU model: refused at the call, no fallback - directly, through score and through the convenience entries
    with pytest.raises(_lib.VuError, match="cuda"):
        s(vol)
    with pytest.raises(_lib.VuError, match="cuda"):
        s.score(vol, np.zeros((2, 40, 40), np.uint8))
    with pytest.raises(_lib.VuError, match="cuda"):
        m.segment(vol[0], overlap=8)
    from vit_unet.torch import functions as F
    with pytest.raises(_lib.VuError, match="cuda"):
        F.dice_tiled(m, [(vol, np.zeros((2, 40, 40), np.uint8))], overlap=8)
    with pytest.raises(_lib.VuError, match="channel"):
        F.iou_tiled(seg_model(3), [], overlap=8)


def test_c_entry_argument_errors():
    """Everything here is refused by host code before a launch: the pointers are made up and never read."""
    L = _lib.lib()
    p, q, r = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 26)
    D, H, W, T, ov = 3, 83, 121, 32, 8
    nt = ref_nt(H, W, T, ov)
    assert nt == 20
    gather = [(lambda: L.vu_tile_gather_i16(p, q, D, H, W, T, ov, 0, 4, 100.0, 100.0, None), "hi > lo"),
              (lambda: L.vu_tile_gather_i16(p, q, D, H, W, T, ov, 0, 4, 5.0, -5.0, None), "hi > lo"),
              (lambda: L.vu_tile_gather_i16(p, q, D, H, W, T, ov, D * nt - 3, 4, -1024.0, 1024.0, None), "outside"),   # one too many
              (lambda: L.vu_tile_gather_i16(p, q, D, H, W, T, ov, D * nt, 1, -1024.0, 1024.0, None), "outside"),
              (lambda: L.vu_tile_gather_i16(p, q, D, H, W, T, ov, -1, 2, -1024.0, 1024.0, None), "outside"),
              (lambda: L.vu_tile_gather_i16(p, q, D, H, W, T, ov, 0, 0, -1024.0, 1024.0, None), "outside"),
              (lambda: L.vu_tile_gather_i16(p, q, 0, H, W, T, ov, 0, 1, -1024.0, 1024.0, None), "empty"),
              (lambda: L.vu_tile_gather_i16(None, q, D, H, W, T, ov, 0, 4, -1024.0, 1024.0, None), "null"),
              (lambda: L.vu_tile_gather_i16(p, None, D, H, W, T, ov, 0, 4, -1024.0, 1024.0, None), "null"),
              (lambda: L.vu_tile_gather_i16(p, q, D, H, W, T, 17, 0, 4, -1024.0, 1024.0, None), "overlap"),
              (lambda: L.vu_tile_gather_i16(p, q, D, H, 0, T, ov, 0, 4, -1024.0, 1024.0, None), "empty"),
              (lambda: L.vu_tile_gather_i16(p, q, D, H, W, 0, 0, 0, 4, -1024.0, 1024.0, None), "window")]
    big = 1 << 20
    blend = [(lambda: L.vu_seg_blend(p, None, None, q, r, r, big, D, H, W, T, ov, 0.0, -1, None), "truth"),          # counts without truth
             (lambda: L.vu_seg_blend(p, None, None, None, None, None, 0, D, H, W, T, ov, 0.0, -1, None), "null"),      # no output
             (lambda: L.vu_seg_blend(None, None, q, None, None, None, 0, D, H, W, T, ov, 0.0, -1, None), "null"),
             (lambda: L.vu_seg_blend(p, None, p, None, None, None, 0, D, H, W, T, ov, 0.0, -1, None), "alias"),
             (lambda: L.vu_seg_blend(p, None, None, C.c_void_p((1 << 20) + 100), None, None, 0, D, H, W, T, ov, 0.0, -1, None), "alias"),
             (lambda: L.vu_seg_blend(p, q, None, None, r, None, 0, D, H, W, T, ov, 0.0, -1, None), "scratch"),
             (lambda: L.vu_seg_blend(p, q, None, None, r, r, 8, D, H, W, T, ov, 0.0, -1, None), "scratch"),
             (lambda: L.vu_seg_blend(p, q, None, q, None, None, 0, 0, H, W, T, ov, 0.0, -1, None), "slice"),
             (lambda: L.vu_seg_blend(p, q, None, q, None, None, 0, D, H, W, T, ov, 0.0, 256, None), "label"),
             (lambda: L.vu_seg_blend(p, q, None, q, None, None, 0, D, H, W, T, ov, float("nan"), -1, None), "threshold"),
             (lambda: L.vu_seg_blend(p, q, None, q, None, None, 0, D, H, W, T, 17, 0.0, -1, None), "overlap")]
    for i, (call, word) in enumerate(gather + blend):
        assert call() < 0, i
        assert word in L.vu_last_error().decode(), (i, L.vu_last_error())


def test_scratch_bytes():
    L = _lib.lib()
    assert L.vu_seg_blend_scratch_bytes(0, 10, 10) == 0 and L.vu_seg_blend_scratch_bytes(1, 0, 10) == 0
    # one block of 256 threads owns 1024 pixel slots (quads of a row); 3 uint32 per block and slice
    for nz, H, W in ((1, 7, 9), (3, 83, 121), (2, 512, 512), (5, 1, 4097)):
        blocks = -(-(H * ((W + 3) // 4)) // 256)
        assert L.vu_seg_blend_scratch_bytes(nz, H, W) == nz * blocks * 12, (nz, H, W)


# ---------------------------------------------------------------- 3. the restatement itself
def test_window_numbering_across_slices():
    D, H, W, T, ov = 3, 83, 121, 32, 8
    vol = np.random.default_rng(0).integers(-32768, 32768, (D, H, W)).astype(np.int16)
    nt = ref_nt(H, W, T, ov)
    win = ref_volume_windows(vol, T, ov)
    assert win.shape == (D * nt, T, T) and win.dtype == np.int16
    oys, oxs = ref_axis(H, T, ov), ref_axis(W, T, ov)
    for g in (0, 7, nt - 1, nt, nt + 5, 2 * nt + 19):
        z, t = divmod(g, nt)
        oy, ox = oys[t // len(oxs)], oxs[t % len(oxs)]
        assert np.array_equal(win[g], vol[z, oy:oy + T, ox:ox + T])                      # L > T: plain crops
    assert np.array_equal(ref_volume_windows(vol, T, ov, nt - 3, 7), win[nt - 3:nt + 4])  # a range across a slice boundary
    assert np.array_equal(ref_volume_windows(vol, T, ov, D * nt - 1, 1), win[-1:])
    small = vol[:2, :7, :9]                                                              # both axes reflected, one window a slice
    w2 = ref_volume_windows(small, T, ov)
    assert w2.shape == (2, T, T)
    for z in range(2):
        assert np.array_equal(w2[z], small[z][ref_src(7, T, 0)][:, ref_src(9, T, 0)])
        assert np.array_equal(w2[z][:7, :9], small[z]) and w2[z][7, 0] == small[z][5, 0] and w2[z][0, 9] == small[z][0, 7]


@pytest.mark.parametrize("thr", [0.5, 0.3])
def test_mask_and_counts_from_the_float64_blend(thr):
    nz, H, W, T, ov = 2, 37, 45, 32, 8
    rng = np.random.default_rng(3)
    nt = ref_nt(H, W, T, ov)
    tiles = rng.uniform(-1, 1, (nz * nt, 1, T, T)).astype(np.float32)
    truth = rng.integers(0, 3, (nz, H, W)).astype(np.uint8)
    zthr = logit_threshold(thr)
    z, mask = ref_seg_blend(tiles, nz, H, W, T, ov, zthr)
    assert z.shape == (nz, H, W) and mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 1}
    if thr == 0.5:                                                                       # logit >= 0 <=> sigmoid >= 0.5
        assert np.array_equal(mask.astype(bool), 1 / (1 + np.exp(-z)) >= 0.5)
    for label in (-1, 1, 2):
        c = ref_counts(mask, truth, label)
        assert c.shape == (nz, 3) and c.dtype == np.int64
        t = ref_truth_pixels(truth, label)
        for s in range(nz):
            assert c[s].tolist() == [int(mask[s].sum()), int(t[s].sum()), int((mask[s].astype(bool) & t[s]).sum())]
        assert (c[:, 2] <= np.minimum(c[:, 0], c[:, 1])).all()
    assert np.array_equal(ref_counts(mask, truth, -1)[:, 1], ref_counts(mask, truth, 1)[:, 1] + ref_counts(mask, truth, 2)[:, 1])
    # constant windows: every logit is the constant, the mask is all or nothing
    ones = np.full_like(tiles, 0.25)
    assert ref_seg_blend(ones, nz, H, W, T, ov, 0.0)[1].all() and not ref_seg_blend(ones, nz, H, W, T, ov, 0.5)[1].any()


def test_left_out_share_of_the_mask_check_is_small():
    """tests/test_gpu_segment.py compares masks only where |z_ref - zthr| > 2e-6 max|v|; with uniform(-1,1) windows that
    leaves out far less than the 1 % per slice it allows."""
    for (D, H, W, ov), T in (((3, 83, 121, 8), 32), ((2, 20, 70, 5), 32), ((3, 37, 45, 8), 32)):
        nt = ref_nt(H, W, T, ov)
        tiles = np.random.default_rng(D + H).uniform(-1, 1, (D * nt, 1, T, T)).astype(np.float32)
        for thr in (0.5, 0.3):
            zthr = logit_threshold(thr)
            z, _ = ref_seg_blend(tiles, D, H, W, T, ov, zthr)
            near = np.abs(z - zthr) <= 2e-6 * np.abs(tiles).max()
            assert near.reshape(D, -1).mean(1).max() <= 1e-3
