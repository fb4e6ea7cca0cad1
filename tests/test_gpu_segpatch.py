"""Segmentation training patches with foreground sampling on the GPU (csrc/vu_segpatch.hip, dataset.SegmentationPatchTransform,
run.run_segmentation).

Everything the three kernels compute is integer or single-rounded float32 arithmetic, so every comparison is EXACT, through
the C ABI with pre-filled outputs, against the numpy restatements of tests/test_segpatch_cpu.py:
  vu_fg_index          == the numpy cumulative sum of the per-row foreground counts
  vu_segpatch_draw     == ref_draw of the same words; every crop inside the volume; every foreground crop holds its pixel
  vu_patch_pairs_i16   x and y bit-equal to ref_patches_i16 (the oracle's seg_prepare arithmetic on numpy-cut, numpy-turned crops)
End to end: the transform against the restatements of its own words, two fused Dice steps on patch batches, and a two-fold
run_segmentation on synthetic volumes."""
import itertools

import numpy as np
import pytest
import torch

from test_gpu_segment import small_model, volume_i16
from test_segpatch_cpu import clamp_table, ref_draw, ref_fg, ref_fg_index, ref_patches_i16, sparse_mask, words
from vit_unet.torch import _lib
from vit_unet.torch import functions as F
from vit_unet.torch._lib import check, lib, ptr
from vit_unet.torch.dataset import ImageFitter, SegmentationBatchTransform, SegmentationPatchTransform

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
WINDOWS = [(-1024.0, 1024.0), (-1000.0, 2000.0)]


def st():
    return _lib.stream_ptr()


def multi_mask(D, H, W, seed):
    """Labels {0,1,2,3}, about a fifth of the pixels set."""
    m = sparse_mask(D, H, W, seed, values=(1, 2, 3), share=0.2)
    assert set(np.unique(m).tolist()) == {0, 1, 2, 3} or m.size < 200
    return m


def _two_empty_slices():
    m = multi_mask(4, 33, 64, 4)
    m[0] = 0
    m[2] = 0
    return m


def _last_pixel():
    m = np.zeros((3, 37, 45), np.uint8)
    m[-1, -1, -1] = 2
    return m


# name -> mask volume: the scalar path (odd W); the 4-byte path; one tiny slice; empty slices between full ones; everything /
# nothing set; one pixel at the very end; more than 65536 rows, so that a block of the scan takes a second round of 256 rows
MASKS = {
    "3x37x45": lambda: multi_mask(3, 37, 45, 1),
    "2x20x72": lambda: multi_mask(2, 20, 72, 2),
    "1x8x8": lambda: multi_mask(1, 8, 8, 3),
    "4x33x64-empty-slices": _two_empty_slices,
    "all-foreground": lambda: np.full((2, 20, 72), 2, np.uint8),
    "all-background": lambda: np.zeros((3, 37, 45), np.uint8),
    "last-pixel": _last_pixel,
    "130x512x8-long": lambda: multi_mask(130, 512, 8, 5),
}
DRAW_MASKS = [k for k in MASKS if k != "130x512x8-long"]


def run_index(dmask, label):
    """One vu_fg_index call on a (D,H,W) uint8 device tensor -> the (D H + 1) index as a device int32 tensor (uint32 bits)."""
    L = lib()
    D, H, W = dmask.shape
    nbytes = L.vu_fg_index_bytes(D, H)
    scratch = torch.full((nbytes // 4,), -1, dtype=torch.int32, device=DEV)
    index = torch.full((D * H + 1,), -1, dtype=torch.int32, device=DEV)
    check(L.vu_fg_index(ptr(dmask), ptr(index), ptr(scratch), nbytes, D, H, W, label, st()), "vu_fg_index")
    return index


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------- 1. index
@pytest.mark.parametrize("label", [-1, 2])
@pytest.mark.parametrize("name", list(MASKS))
def test_fg_index_is_the_cumulative_sum(name, label):
    mask = MASKS[name]()
    D, H, W = mask.shape
    ref = ref_fg_index(mask, label)
    assert ref[-1] == ref_fg(mask, label).sum()
    d = torch.from_numpy(mask).to(DEV)
    got = run_index(d, label)
    assert np.array_equal(as_u32(got), ref)
    assert torch.equal(run_index(d, label), got)                                # a second run: the same bits
    # a mask that starts one byte into its buffer (byte loads whatever W is), the byte before it set
    buf = torch.full((mask.size + 1,), 2, dtype=torch.uint8, device=DEV)
    buf[1:].copy_(d.reshape(-1))
    assert np.array_equal(as_u32(run_index(buf[1:].view(D, H, W), label)), ref)


# ---------------------------------------------------------------- 2. draw
def hand_words(thresh, seed):
    """0 and 0xffffffff in every column (together and one column at a time), the branch word just below / at / just above
    the threshold, the ranks of the first and the last foreground pixel, 64 seeded rows."""
    rows = [[0, 0, 0, 0], [0xffffffff] * 4]
    fill = words(8, seed + 1)
    for c in range(4):
        for k, v in enumerate((0, 0xffffffff)):
            r = fill[2 * c + k].tolist()
            r[c] = v
            rows.append(r)
    for w0 in (max(thresh - 1, 0), thresh, min(thresh + 1, 0xffffffff)):
        rows.append([w0, 0x9e3779b9, 0x12345678, 5])
    rows += [[0, 0, 0x80008000, 1], [0, 0xffffffff, 0x80008000, 2], [0, 0, 0xffffffff, 3], [0, 0xffffffff, 0, 4]]
    return np.concatenate([np.array(rows, dtype=np.uint64).astype(np.uint32), words(64, seed)])


def run_draw(dmask, index, rnd, T, thresh, label):
    D, H, W = dmask.shape
    n = len(rnd)
    dr = torch.from_numpy(np.ascontiguousarray(rnd).view(np.int32)).to(DEV)
    crops = torch.full((n, 4), -77, dtype=torch.int32, device=DEV)
    check(lib().vu_segpatch_draw(ptr(dmask), ptr(index), ptr(dr), ptr(crops), n, D, H, W, T, thresh, label, st()), "vu_segpatch_draw")
    return crops.cpu().numpy()


@pytest.mark.parametrize("T", [8, 6])
@pytest.mark.parametrize("name", DRAW_MASKS)
def test_draw_equals_the_restatement(name, T):
    mask = MASKS[name]()
    D, H, W = mask.shape
    d = torch.from_numpy(mask).to(DEV)
    for label, thresh in ((-1, 1 << 31), (2, 1 << 31), (-1, 0), (2, 0xffffffff)):
        rnd = hand_words(thresh, seed=T + H)
        index = run_index(d, label)
        ref_index = ref_fg_index(mask, label)
        assert np.array_equal(as_u32(index), ref_index)
        want, picks = ref_draw(mask, ref_index, rnd, T, thresh, label)
        got = run_draw(d, index, rnd, T, thresh, label)
        assert np.array_equal(got, want), (label, thresh, np.nonzero((got != want).any(1))[0])
        assert (got[:, 0] >= 0).all() and (got[:, 0] < D).all() and (got[:, 1] >= 0).all() and (got[:, 1] <= H - T).all()
        assert (got[:, 2] >= 0).all() and (got[:, 2] <= W - T).all() and (got[:, 3] >= 0).all() and (got[:, 3] <= 7).all()
        fg = ref_fg(mask, label)
        for (z, y0, x0, _), pk in zip(got, picks):
            if pk is not None:                                                  # the crop holds its foreground pixel
                assert z == pk[0] and y0 <= pk[1] < y0 + T and x0 <= pk[2] < x0 + T and fg[pk]
        nfg = sum(p is not None for p in picks)
        if ref_index[-1] == 0 or thresh == 0:
            assert nfg == 0                                                     # no foreground / fg_thresh 0: the uniform branch only
        else:
            assert nfg >= 8 and (thresh == 0xffffffff or nfg < len(rnd))        # both branches occur
        assert np.array_equal(run_draw(d, index, rnd, T, thresh, label), got)   # a second run: the same table


# ---------------------------------------------------------------- 3. cut
# (H, W, T): odd sizes with T % 4 == 0; W % 4 == 0; T % 4 != 0; the slice is the patch; T = 33 crosses the 32-tile edge with a
# partial tile (2 x 2 tiles, three of them partial)
CUT_SHAPES = [(37, 45, 8), (20, 72, 8), (9, 9, 6), (8, 8, 8), (40, 48, 33)]


def cut_table(D, H, W, T, seed):
    """48 crops: every op at the four corner origins and at two seeded ones; slices in turn, the first crop in slice 0."""
    rng = np.random.default_rng(seed)
    rows = []
    for op in range(8):
        for y0, x0 in ((0, 0), (0, W - T), (H - T, 0), (H - T, W - T), tuple(rng.integers(0, (H - T + 1, W - T + 1))),
                       tuple(rng.integers(0, (H - T + 1, W - T + 1)))):
            rows.append((len(rows) % D, int(y0), int(x0), op))
    return np.array(rows, dtype=np.int32)


def run_cut(vol, mask, x, y, D, H, W, T, table, lo=-1024.0, hi=1024.0, ls=0.0, label=-1):
    d = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(DEV)
    check(lib().vu_patch_pairs_i16(ptr(vol), ptr(mask), ptr(x), ptr(y), D, H, W, T, ptr(d), len(table), lo, hi, ls, label, st()),
          "vu_patch_pairs_i16")


def nan_batch(n, T):
    return torch.full((n, 1, T, T), NAN, device=DEV)


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("H,W,T", CUT_SHAPES)
def test_patch_pairs_i16_bit_exact(H, W, T, D):
    vol = volume_i16(D, H, W, seed=H + W + D)                                   # vol[0, 0, :2] = -32768, 32767: inside crop 0
    masks = {-1: sparse_mask(D, H, W, H, share=0.3), 2: multi_mask(D, H, W, W)}
    table = cut_table(D, H, W, T, seed=H * W)
    n = len(table)
    assert tuple(table[0]) == (0, 0, 0, 0) and sorted(set(table[:, 3].tolist())) == list(range(8)) and set(table[:, 0].tolist()) == set(range(D))
    dv = torch.from_numpy(vol).to(DEV)
    dm = {k: torch.from_numpy(m).to(DEV) for k, m in masks.items()}
    for (lo, hi), ls, label in itertools.product(WINDOWS, (0.0, 0.1), (-1, 2)):
        rx, ry = ref_patches_i16(vol, masks[label], T, table, lo, hi, ls, label)
        assert rx.min() == 0.0 and rx.max() == 1.0 and len(np.unique(ry)) == 2  # both clips, both label levels
        x, y = nan_batch(n, T), nan_batch(n, T)
        run_cut(dv, dm[label], x, y, D, H, W, T, table, lo, hi, ls, label)
        assert torch.equal(x.cpu(), torch.from_numpy(rx)), (lo, hi, ls, label)
        assert torch.equal(y.cpu(), torch.from_numpy(ry)), (lo, hi, ls, label)
    lo, hi, ls, label = -1000.0, 2000.0, 0.1, 2
    # each pair omitted in turn: the other side carries the same bits
    x1, y1 = nan_batch(n, T), nan_batch(n, T)
    run_cut(dv, None, x1, None, D, H, W, T, table, lo, hi, ls, label)
    run_cut(None, dm[label], None, y1, D, H, W, T, table, lo, hi, ls, label)
    assert torch.equal(x1, x) and torch.equal(y1, y)
    # outputs offset by one float (not 16-byte aligned: scalar stores), the float before untouched
    bx, by = torch.full((n * T * T + 1,), NAN, device=DEV), torch.full((n * T * T + 1,), NAN, device=DEV)
    run_cut(dv, dm[label], bx[1:].view(n, 1, T, T), by[1:].view(n, 1, T, T), D, H, W, T, table, lo, hi, ls, label)
    assert torch.equal(bx[1:].view(n, 1, T, T), x) and torch.equal(by[1:].view(n, 1, T, T), y)
    assert torch.isnan(bx[0]) and torch.isnan(by[0])
    # the documented clamp: an out-of-range table gives what its clamped form gives
    wild = np.array([[-5, -5, W, 11], [D, H, -1, 8 + 6], [D + 7, 1 << 30, -(1 << 30), -1], [-(1 << 31), 0, 0, 1 << 20]], dtype=np.int64)
    tame = clamp_table(wild, D, H, W, T)
    assert tame[0].tolist() == [0, 0, W - T, 3] and tame[1].tolist() == [D - 1, H - T, 0, 6] and tame[2, 3] == 7
    x2, y2, x3, y3 = nan_batch(4, T), nan_batch(4, T), nan_batch(4, T), nan_batch(4, T)
    run_cut(dv, dm[label], x2, y2, D, H, W, T, wild.astype(np.int32), lo, hi, ls, label)
    run_cut(dv, dm[label], x3, y3, D, H, W, T, tame, lo, hi, ls, label)
    assert torch.equal(x2, x3) and torch.equal(y2, y3) and torch.isfinite(x2).all() and torch.isfinite(y2).all()
    r3 = ref_patches_i16(vol, masks[label], T, tame, lo, hi, ls, label)
    assert torch.equal(x3.cpu(), torch.from_numpy(r3[0])) and torch.equal(y3.cpu(), torch.from_numpy(r3[1]))


@pytest.mark.parametrize("T", [8, 33])
def test_patch_of_a_patch_sized_slice_is_the_validation_transform(T):
    vol = volume_i16(1, T, T, seed=T)
    mask = sparse_mask(1, T, T, T, share=0.4)
    for (lo, hi), ls in itertools.product(WINDOWS, (0.0, 0.1)):
        x, y = nan_batch(1, T), nan_batch(1, T)
        run_cut(torch.from_numpy(vol).to(DEV), torch.from_numpy(mask).to(DEV), x, y, 1, T, T, T, np.zeros((1, 4), np.int32), lo, hi, ls, -1)
        want = SegmentationBatchTransform(T, train=False, window=(lo, hi), ls=ls)(vol, mask)
        assert torch.equal(x, want["x"]) and torch.equal(y, want["y"])


# ---------------------------------------------------------------- 4. SegmentationPatchTransform
def test_transform_on_two_volumes_of_different_sizes():
    T, P, seed = 8, 6, 11
    vols = [volume_i16(3, 40, 48, seed=1), volume_i16(1, 37, 45, seed=2)[0]]   # a volume and one (H,W) slice
    masks = [multi_mask(3, 40, 48, 7), multi_mask(1, 37, 45, 8)[0]]
    kw = dict(window=(-1000.0, 2000.0), ls=0.1, fg=0.5, label=2)
    t = SegmentationPatchTransform(T, per_volume=P, seed=seed, **kw)
    got = t(vols, masks)
    assert got["x"].shape == (2 * P, 1, T, T) and got["y"].shape == (2 * P, 1, T, T)
    assert got["x"].dtype == torch.float32 and got["x"].is_cuda and len(t.last_crops) == 2
    host = SegmentationPatchTransform(T, per_volume=P, seed=seed, **kw)         # the same words, drawn on the host
    nfg = 0
    for b in range(2):
        v3, m3 = vols[b].reshape((-1,) + vols[b].shape[-2:]), masks[b].reshape((-1,) + masks[b].shape[-2:])
        want, picks = ref_draw(m3, ref_fg_index(m3, 2), host.draw_words(P), T, host.fg_thresh, 2)
        nfg += sum(p is not None for p in picks)
        assert t.last_crops[b].shape == (P, 4) and t.last_crops[b].dtype == torch.int32 and t.last_crops[b].is_cuda
        assert np.array_equal(t.last_crops[b].cpu().numpy(), want)
        rx, ry = ref_patches_i16(v3, m3, T, want, -1000.0, 2000.0, 0.1, 2)
        assert torch.equal(got["x"][b * P:(b + 1) * P].cpu(), torch.from_numpy(rx))     # the patches of volume 0 come first
        assert torch.equal(got["y"][b * P:(b + 1) * P].cpu(), torch.from_numpy(ry))
    assert 0 < nfg < 2 * P                                                      # this seed takes both branches
    # the same seed again, from host torch and device torch inputs: the same bits
    for conv in (torch.from_numpy, lambda a: torch.from_numpy(a).to(DEV)):
        g2 = SegmentationPatchTransform(T, per_volume=P, seed=seed, **kw)([conv(a) for a in vols], [conv(a) for a in masks])
        assert torch.equal(g2["x"], got["x"]) and torch.equal(g2["y"], got["y"])
    nxt = t(vols, masks)                                                        # the generator moves on
    assert not torch.equal(nxt["x"], got["x"])
    # crops= replaces the draw
    table = [np.array([[2, 32, 40, 5], [0, 0, 0, 0]]), np.array([[0, 29, 37, 7], [0, 3, 5, 2]])]
    e = SegmentationPatchTransform(T, per_volume=2, seed=0, **kw)(vols, masks, crops=table)
    for b in range(2):
        v3, m3 = vols[b].reshape((-1,) + vols[b].shape[-2:]), masks[b].reshape((-1,) + masks[b].shape[-2:])
        rx, ry = ref_patches_i16(v3, m3, T, table[b], -1000.0, 2000.0, 0.1, 2)
        assert torch.equal(e["x"][2 * b:2 * b + 2].cpu(), torch.from_numpy(rx)) and torch.equal(e["y"][2 * b:2 * b + 2].cpu(), torch.from_numpy(ry))
    # train=False: one centred crop of the middle slice, op 0, no draw
    v = SegmentationPatchTransform(T, per_volume=P, train=False, **kw)
    val = v(vols, masks)
    assert val["x"].shape == (2, 1, T, T)
    assert [c.cpu().tolist() for c in v.last_crops] == [[[1, 16, 20, 0]], [[0, 14, 18, 0]]]
    rx, ry = ref_patches_i16(vols[0], masks[0], T, [(1, 16, 20, 0)], -1000.0, 2000.0, 0.1, 2)
    assert torch.equal(val["x"][:1].cpu(), torch.from_numpy(rx)) and torch.equal(val["y"][:1].cpu(), torch.from_numpy(ry))


def test_full_foreground_share_gives_no_empty_target():
    """fg = 1.0: every crop is placed around a foreground pixel, so with ls = 0 every target patch has a non-zero sum -
    by construction, not by chance; fg = 0.0 on the same volume leaves most targets empty."""
    T, P = 8, 32
    mask = np.zeros((4, 64, 80), np.uint8)
    mask[2, 50:53, 70:74] = 1                                                   # 12 foreground pixels in 20480
    vol = volume_i16(4, 64, 80, seed=3)
    full = SegmentationPatchTransform(T, per_volume=P, fg=1.0, seed=5)(vol, mask)
    sums = full["y"].sum(dim=(1, 2, 3)).cpu().numpy()
    assert (sums >= 1.0).all(), sums
    none = SegmentationPatchTransform(T, per_volume=P, fg=0.0, seed=5)
    assert none.fg_thresh == 0
    empty = none(vol, mask)["y"].sum(dim=(1, 2, 3)).cpu().numpy()
    assert (empty == 0).sum() > P // 2
    want, picks = ref_draw(mask, ref_fg_index(mask, -1), SegmentationPatchTransform(T, seed=5).draw_words(P), T, 0, -1)
    assert all(p is None for p in picks) and np.array_equal(none.last_crops[0].cpu().numpy(), want)


# ---------------------------------------------------------------- 5. training
def test_dice_steps_on_patch_batches(tmp_path):
    m, _, _ = small_model(torch.float32)
    m.train()
    vol = np.random.default_rng(1).integers(-1500, 1500, (3, 40, 48)).astype(np.int16)
    mask = np.zeros((3, 40, 48), np.uint8)
    mask[:, 10:30, 12:36] = 1
    t = SegmentationPatchTransform(32, per_volume=8, seed=4)
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    fitter = ImageFitter(m, loss=F.DiceLoss(), lr=1e-3, folder=str(tmp_path), seed=3)
    assert fitter._fused_kind() == "dice"
    losses = []
    for _ in range(2):
        b = t(vol, mask)
        assert b["x"].shape == (8, 1, 32, 32) and b["y"].shape == (8, 1, 32, 32)
        losses.append(fitter._train_batch(*fitter.unpack(b)))
    assert fitter._fused is not None                                            # the fused HIP step ran, not autograd
    assert np.isfinite(losses).all() and all(0.0 <= v <= 1.0 for v in losses), losses
    changed = [k for k, v in m.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert len(changed) > len(before) // 2, changed
    assert all(torch.isfinite(v).all() for v in m.parameters())


def test_run_segmentation(tmp_path):
    from vit_unet.torch.run import run_segmentation
    rng = np.random.default_rng(21)
    vols = [rng.integers(-1500, 1500, (2, 40, 48)).astype(np.int16) for _ in range(4)]
    truths = []
    for k in range(4):
        tr = np.zeros((2, 40, 48), np.uint8)
        tr[:, 5 + k:25 + k, 8:30] = 1
        truths.append(tr)
    folder = tmp_path / "models"
    res = run_segmentation(vols, truths, n_epochs=1, folds=2, model_string="lite", batch_size=4, im_size=32, crops_per_volume=2,
                           fg=0.5, dtype=torch.float32, folder=str(folder), seed=1)
    assert [len(d) for d in res["dice"]] == [2, 2] and len(res["history"]) == 2 and all(len(h) == 1 for h in res["history"])
    assert all(((d >= 0.0) & (d <= 1.0)).all() for d in res["dice"])
    assert 0.0 <= res["dice_mean"] <= 1.0 and np.isfinite(res["dice_std"])
    assert all(np.isfinite(h[0]["train"]) and np.isfinite(h[0]["val"]) for h in res["history"])
    assert (folder / "best-checkpoint.bin").exists() and (folder / "last-checkpoint.bin").exists()
    with pytest.raises(AssertionError):
        run_segmentation(vols, truths, batch_size=6, crops_per_volume=4)       # 4 does not divide 6
