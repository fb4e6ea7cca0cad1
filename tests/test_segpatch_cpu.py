"""Segmentation training patches with foreground sampling, host side (no GPU): the numpy restatements of the three entries
of csrc/vu_segpatch.hip, written from the formulas of include/vit_unet_amd.h, that tests/test_gpu_segpatch.py holds the HIP
kernels against; the random words `SegmentationPatchTransform` draws; and every argument error the C entries and the
transform report before any GPU call."""
import ctypes as C

import numpy as np
import pytest
import torch

import vit_unet_oracle as O
from test_patch_cpu import ref_dihedral
from vit_unet.torch import _lib
from vit_unet.torch.dataset import SegmentationBatchTransform, SegmentationDataset, SegmentationPatchTransform


# ---------------------------------------------------------------- numpy restatement (the definition of the header)
def ref_fg(mask, label):
    """A foreground pixel is mask != 0 when label < 0 and mask == label when 0 <= label <= 255."""
    return mask != 0 if label < 0 else mask == label


def ref_fg_index(mask, label):
    """(D,H,W) uint8 -> (D H + 1) uint32: index[r] = foreground pixels in rows [0, r) of the volume taken as D H rows."""
    D, H, W = mask.shape
    index = np.zeros(D * H + 1, dtype=np.uint32)
    index[1:] = np.cumsum(ref_fg(mask, label).reshape(D * H, W).sum(axis=1, dtype=np.uint64)).astype(np.uint32)
    return index


def ref_draw(mask, index, rnd, T, fg_thresh, label):
    """(n,4) uint32 words -> ((n,4) int32 crops (z, y0, x0, op), [the (z, y, x) of the foreground pixel of every foreground
    crop, None for the others]).  Python integers throughout: the header's formulas as they stand."""
    D, H, W = mask.shape
    total = int(index[D * H])
    fg = ref_fg(mask, label).reshape(D * H, W)
    crops, picks = np.zeros((len(rnd), 4), dtype=np.int32), []
    for i, (w0, w1, w2, w3) in enumerate([[int(v) for v in row] for row in rnd]):
        hy, hx = w2 >> 16, w2 & 0xffff
        if w0 < fg_thresh and total > 0:
            r = (w1 * total) >> 32
            q = int(np.searchsorted(index, r, side="right")) - 1              # index[q] <= r < index[q+1]
            assert int(index[q]) <= r < int(index[q + 1])
            z, y = divmod(q, H)
            x = int(np.flatnonzero(fg[q])[r - int(index[q])])
            oy, ox = (hy * T) >> 16, (hx * T) >> 16
            y0, x0 = min(max(y - oy, 0), H - T), min(max(x - ox, 0), W - T)
            picks.append((z, y, x))
        else:
            z = (w1 * D) >> 32
            y0, x0 = (hy * (H - T + 1)) >> 16, (hx * (W - T + 1)) >> 16
            picks.append(None)
        crops[i] = (z, y0, x0, w3 & 7)
    return crops, picks


def ref_patches_i16(vol, mask, T, crops, lo=-1024.0, hi=1024.0, ls=0.0, label=-1):
    """(D,H,W) int16 / uint8, [(z, y0, x0, op)] -> x, y (n,1,T,T) float32: D_op of the crop under the intensity window
    (every operation rounded once in float32) and of t (1 - ls) + ls / 2 with t the foreground rule.  Either input may be
    None."""
    f = np.float32
    rng_ = f(hi) - f(lo)
    keep, floor_ = f(1.0) - f(ls), f(0.5) * f(ls)
    xs, ys = [], []
    for z, y0, x0, op in crops:
        if vol is not None:
            p = vol[z, y0:y0 + T, x0:x0 + T].astype(f)
            xs.append(np.ascontiguousarray(ref_dihedral(np.clip((p - f(lo)) / rng_, f(0), f(1)), op))[None])
        if mask is not None:
            t = ref_fg(mask[z, y0:y0 + T, x0:x0 + T], label).astype(f)
            ys.append(np.ascontiguousarray(ref_dihedral(t * keep + floor_, op))[None])
    return (np.stack(xs) if xs else None), (np.stack(ys) if ys else None)


def clamp_table(table, D, H, W, T):
    """What the cut kernel makes of any table: z to [0, D-1], y0 to [0, H-T], x0 to [0, W-T], op & 7."""
    t = np.asarray(table, dtype=np.int64)
    return np.stack([np.clip(t[:, 0], 0, D - 1), np.clip(t[:, 1], 0, H - T), np.clip(t[:, 2], 0, W - T), t[:, 3] & 7], axis=1).astype(np.int32)


def sparse_mask(D, H, W, seed, values=(1,), share=0.05):
    """A label volume with about `share` foreground, drawn from `values`."""
    rng = np.random.default_rng(seed)
    m = np.zeros((D, H, W), dtype=np.uint8)
    on = rng.random((D, H, W)) < share
    m[on] = rng.choice(np.asarray(values, dtype=np.uint8), size=int(on.sum()))
    return m


def words(n, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, (n, 4), dtype=np.uint64).astype(np.uint32)


# ---------------------------------------------------------------- 1. the restatement itself
@pytest.mark.parametrize("label", [-1, 2])
def test_foreground_pick_is_flatnonzero_indexing(label):
    D, H, W, T = 3, 37, 45, 8
    mask = sparse_mask(D, H, W, seed=1, values=(1, 2, 3))
    index = ref_fg_index(mask, label)
    flat = np.flatnonzero(ref_fg(mask, label).reshape(-1))
    assert index[0] == 0 and index[-1] == len(flat) > 0 and (np.diff(index.astype(np.int64)) >= 0).all()
    rnd = words(200, seed=2)
    rnd[0, 1], rnd[1, 1] = 0, 0xffffffff                                       # the first and the last foreground pixel
    crops, picks = ref_draw(mask, index, rnd, T, 2 ** 32 - 1, label)
    assert picks[0] == tuple(int(v) for v in np.unravel_index(flat[0], mask.shape))
    assert picks[1] == tuple(int(v) for v in np.unravel_index(flat[-1], mask.shape))
    seen = 0
    for i, pk in enumerate(picks):
        if pk is None:
            assert rnd[i, 0] == 0xffffffff                                      # only a word AT the threshold is no foreground crop
            continue
        seen += 1
        r = (int(rnd[i, 1]) * len(flat)) >> 32
        assert np.ravel_multi_index(pk, mask.shape) == flat[r]
        z, y0, x0, op = crops[i]
        assert z == pk[0] and y0 <= pk[1] < y0 + T and x0 <= pk[2] < x0 + T    # the pixel lies inside its crop
        assert 0 <= y0 <= H - T and 0 <= x0 <= W - T and op == rnd[i, 3] & 7
    assert seen >= 199


def test_uniform_branch_and_empty_volume():
    D, H, W, T = 2, 20, 72, 6
    rnd = words(300, seed=3)
    rnd[0], rnd[1] = 0, 0xffffffff
    for mask, thresh in ((np.zeros((D, H, W), np.uint8), 2 ** 32 - 1), (sparse_mask(D, H, W, 4), 0)):
        crops, picks = ref_draw(mask, ref_fg_index(mask, -1), rnd, T, thresh, -1)
        assert all(p is None for p in picks)                                    # total == 0 / fg_thresh == 0: never foreground
        assert crops[0].tolist() == [0, 0, 0, 0] and crops[1].tolist() == [D - 1, H - T, W - T, 7]
        assert (crops[:, 0] >= 0).all() and (crops[:, 0] < D).all() and (crops[:, 1] <= H - T).all() and (crops[:, 2] <= W - T).all()
        assert set(crops[:, 3].tolist()) == set(range(8)) and set(crops[:, 0].tolist()) == {0, 1}
    # the pixel stays inside the crop at every offset word, the corners of the slice included
    mask = np.zeros((1, 9, 9), np.uint8)
    for y, x in ((0, 0), (8, 8), (0, 8), (4, 4)):
        mask[:] = 0
        mask[0, y, x] = 1
        for w2 in (0, 0xffffffff, 0x0000ffff, 0xffff0000, 0x80008000):
            crops, picks = ref_draw(mask, ref_fg_index(mask, -1), np.array([[0, 12345, w2, 0]], np.uint32), 6, 1, -1)
            assert picks[0] == (0, y, x)
            assert crops[0, 1] <= y < crops[0, 1] + 6 and crops[0, 2] <= x < crops[0, 2] + 6 and 0 <= crops[0, 1] <= 3 and 0 <= crops[0, 2] <= 3


def test_ref_patches_is_the_oracle_without_resize_and_warp():
    """For a {0,1} mask and label < 0 the restatement is the oracle's seg_prepare of the numpy-cut crops, bit for bit."""
    rng = np.random.default_rng(5)
    D, H, W, T = 2, 20, 24, 8
    vol = rng.integers(-32768, 32768, (D, H, W)).astype(np.int16)
    mask = sparse_mask(D, H, W, 6, share=0.4)
    crops = [(0, 0, 0, 0), (1, 12, 16, 0), (1, 3, 5, 0)]
    for lo, hi, ls in ((-1024.0, 1024.0, 0.0), (-1000.0, 2000.0, 0.1)):
        x, y = ref_patches_i16(vol, mask, T, crops, lo, hi, ls)
        cut_v = np.stack([vol[z, a:a + T, b:b + T] for z, a, b, _ in crops])
        cut_m = np.stack([mask[z, a:a + T, b:b + T] for z, a, b, _ in crops])
        ox, oy = O.seg_prepare(cut_v, cut_m, T, None, lo, hi, ls)
        assert x.dtype == np.float32 and y.dtype == np.float32 and x.shape == (3, 1, T, T)
        assert np.array_equal(x, ox.numpy()) and np.array_equal(y, oy.numpy())
    x5, y5 = ref_patches_i16(vol, mask, T, [(1, 3, 5, 5)])
    x0, y0 = ref_patches_i16(vol, mask, T, [(1, 3, 5, 0)])
    assert np.array_equal(x5[0, 0], x0[0, 0].T) and np.array_equal(y5[0, 0], y0[0, 0].T)      # op 5 is the transpose
    assert clamp_table([[-5, -1, 99, 11], [7, 99, -3, 8 + 6]], D, H, W, T).tolist() == [[0, 0, W - T, 3], [D - 1, H - T, 0, 6]]


# ---------------------------------------------------------------- 2. the transform's words and arguments
def test_draw_words_and_threshold():
    a = SegmentationPatchTransform(32, per_volume=5, seed=7)
    wa = a.draw_words(5)
    assert wa.shape == (5, 4) and wa.dtype == np.uint32
    assert np.array_equal(wa, SegmentationPatchTransform(32, per_volume=5, seed=7).draw_words(5))
    assert not np.array_equal(wa, SegmentationPatchTransform(32, per_volume=5, seed=8).draw_words(5))
    assert not np.array_equal(wa, a.draw_words(5))                              # the generator moves on
    b = SegmentationPatchTransform(32, seed=7)
    assert np.array_equal(np.concatenate([b.draw_words(2), b.draw_words(3)]), wa)
    big = SegmentationPatchTransform(32, seed=1).draw_words(256)
    assert big.max() > 0xf0000000 and big.min() < 0x10000000                    # full 32-bit words
    assert SegmentationPatchTransform(32, fg=0.0).fg_thresh == 0
    assert SegmentationPatchTransform(32, fg=0.5).fg_thresh == 2 ** 31
    assert SegmentationPatchTransform(32, fg=1.0).fg_thresh == 2 ** 32 - 1
    assert SegmentationPatchTransform(32).fg_thresh == 2 ** 31 and SegmentationPatchTransform(32).per_volume == 8
    v = SegmentationPatchTransform(32, per_volume=5, train=False)
    assert v.per_volume == 1 and v.last_crops is None


def test_transform_refuses_before_any_launch():
    for kw in (dict(patch=0), dict(per_volume=0), dict(window=(5.0, 5.0)), dict(window=(1.0, -1.0)), dict(ls=1.0), dict(ls=-0.1),
               dict(fg=1.5), dict(fg=-0.1), dict(label=256), dict(patch=65536)):
        with pytest.raises(_lib.VuError):
            SegmentationPatchTransform(**{"patch": 8, **kw})
    t = SegmentationPatchTransform(8, per_volume=2, seed=0)
    vol, mask = np.zeros((2, 20, 24), np.int16), np.zeros((2, 20, 24), np.uint8)
    ok = [np.array([[0, 0, 0, 0], [1, 12, 16, 7]])]
    for call in (lambda: t(vol, mask[:, :, :23], crops=ok),                     # mismatched pair
                 lambda: t(vol[:, :7], mask[:, :7], crops=ok),                  # smaller than a patch
                 lambda: t(vol.astype(np.int32), mask, crops=ok),               # wrong dtypes
                 lambda: t(vol, mask.astype(np.int16), crops=ok),
                 lambda: t([vol, vol], [mask], crops=ok),
                 lambda: t([], [], crops=ok),
                 lambda: t(vol[0, 0], mask[0, 0], crops=ok),                    # one line is no slice
                 lambda: t(vol, mask, crops=ok + ok),                           # a table too many
                 lambda: t(vol, mask, crops=[np.zeros((3, 4), np.int32)]),      # table of another shape
                 lambda: t(vol, mask, crops=[np.zeros((2, 3), np.int32)]),
                 lambda: t(vol, mask, crops=[np.zeros((2, 4), np.float32)]),
                 lambda: t(vol, mask, crops=[np.array([[2, 0, 0, 0], [0, 0, 0, 0]])]),
                 lambda: t(vol, mask, crops=[np.array([[0, 13, 0, 0], [0, 0, 0, 0]])]),
                 lambda: t(vol, mask, crops=[np.array([[0, 0, 17, 0], [0, 0, 0, 0]])]),
                 lambda: t(vol, mask, crops=[np.array([[0, 0, 0, 8], [0, 0, 0, 0]])]),
                 lambda: t(vol, mask, crops=[np.array([[0, 0, 0, 0], [0, -1, 0, 0]])])):
        with pytest.raises(_lib.VuError):
            call()
    with pytest.raises(_lib.VuError, match="no CPU fallback"):
        SegmentationPatchTransform(8, per_volume=2, device="cpu")(vol, mask, crops=ok)
    assert t.last_crops is None                                                 # nothing ran


def test_dataset_accepts_the_patch_transform():
    import pandas as pd
    df = pd.DataFrame({"image": ["a", "b"], "mask": ["ma", "mb"], "mask_index": [0, 1]})
    kw = dict(read_image=lambda p: np.zeros((40, 48), np.int16), read_mask=lambda p, i: np.zeros((40, 48), np.uint8))
    ds = SegmentationDataset(df, augments=SegmentationPatchTransform(32, per_volume=2, seed=1), **kw)
    assert len(ds) == 2 and ds[0]["x"].shape == (40, 48) and isinstance(ds.augments, SegmentationPatchTransform)
    SegmentationDataset(df, augments=SegmentationBatchTransform(32, train=False), **kw)
    SegmentationDataset(df, **kw)
    for bad in (object(), "patch", lambda a, b: None):
        with pytest.raises(TypeError):
            SegmentationDataset(df, augments=bad, **kw)
    test_ds = SegmentationDataset(df, augments=SegmentationPatchTransform(32, per_volume=2), is_test=True, **kw)
    with pytest.raises(_lib.VuError, match="is_test"):
        test_ds.transform([test_ds[0]])


# ---------------------------------------------------------------- 3. argument errors of the C entries (before any GPU call)
def _host_buffers():
    u8, i16, f, u32 = (C.c_uint8 * 4096)(), (C.c_int16 * 4096)(), (C.c_float * 4096)(), (C.c_uint32 * 4096)()
    return [C.cast(b, C.c_void_p) for b in (u8, i16, f, u32)] + [(u8, i16, f, u32)]


def _refused(L, cases):
    for call, word in cases:
        assert call() < 0, word
        assert word in L.vu_last_error().decode(), (word, L.vu_last_error())


def test_fg_index_argument_errors():
    L = _lib.lib()
    # the checks return before any pointer is used: host buffers stand in for device memory
    m_, _, _, w_, keep = _host_buffers()
    assert L.vu_fg_index_bytes(3, 37) >= 4 * 3 * 37 and L.vu_fg_index_bytes(0, 5) == 0 and L.vu_fg_index_bytes(5, -1) == 0
    need = L.vu_fg_index_bytes(2, 16)

    def fi(mask=m_, index=w_, scratch=w_, nbytes=need, D=2, H=16, W=16, label=-1):
        return L.vu_fg_index(mask, index, scratch, nbytes, D, H, W, label, None)

    odd = C.c_void_p(C.addressof(keep[3]) + 2)
    _refused(L, ((lambda: fi(mask=None), "null"), (lambda: fi(index=None), "null"), (lambda: fi(scratch=None), "null"),
                 (lambda: fi(nbytes=need - 1), "scratch"), (lambda: fi(nbytes=0), "scratch"), (lambda: fi(scratch=odd), "scratch"),
                 (lambda: fi(index=odd), "aligned"), (lambda: fi(D=0), "empty"), (lambda: fi(H=0), "empty"), (lambda: fi(W=-1), "empty"),
                 (lambda: fi(label=256), "label"), (lambda: fi(D=65536, H=256, W=256), "too large"),
                 (lambda: fi(D=1 << 20, H=1 << 11, W=1), "too large")))


def test_segpatch_draw_argument_errors():
    L = _lib.lib()
    m_, _, _, w_, keep = _host_buffers()
    base = C.addressof(keep[3])
    rnd, crops, off4 = C.c_void_p(base + 1024), C.c_void_p(base + 2048), C.c_void_p(base + 4)

    def dr(mask=m_, index=w_, r=rnd, c=crops, n=4, D=2, H=16, W=16, T=8, thresh=1 << 31, label=-1):
        return L.vu_segpatch_draw(mask, index, r, c, n, D, H, W, T, thresh, label, None)

    _refused(L, ((lambda: dr(mask=None), "null"), (lambda: dr(index=None), "null"), (lambda: dr(r=None), "null"),
                 (lambda: dr(c=None), "null"), (lambda: dr(n=0), "no crop"), (lambda: dr(T=0), "patch size"),
                 (lambda: dr(H=7), "smaller"), (lambda: dr(W=7), "smaller"), (lambda: dr(H=65536), "65535"),
                 (lambda: dr(W=65536, D=1), "65535"), (lambda: dr(D=0), "empty"), (lambda: dr(label=300), "label"),
                 (lambda: dr(D=1 << 16, H=1 << 10, W=1 << 10), "too large"), (lambda: dr(r=off4), "aligned"),
                 (lambda: dr(c=off4), "aligned")))


def test_patch_pairs_i16_argument_errors():
    L = _lib.lib()
    m_, v_, f_, w_, keep = _host_buffers()
    y_ = C.c_void_p(C.addressof(keep[2]) + 8192)

    def pp(vol=v_, mask=m_, x=f_, y=y_, D=2, H=16, W=16, T=8, crops=w_, n=4, lo=-1024.0, hi=1024.0, ls=0.0, label=-1):
        return L.vu_patch_pairs_i16(vol, mask, x, y, D, H, W, T, crops, n, lo, hi, ls, label, None)

    _refused(L, ((lambda: pp(H=7), "smaller"), (lambda: pp(W=7), "smaller"), (lambda: pp(n=0), "no crop"), (lambda: pp(T=0), "patch size"),
                 (lambda: pp(crops=None), "null"), (lambda: pp(vol=None, mask=None, x=None, y=None), "null"),
                 (lambda: pp(vol=None), "null"), (lambda: pp(y=None), "null"), (lambda: pp(x=None), "null"),
                 (lambda: pp(mask=None), "null"), (lambda: pp(hi=-1024.0), "hi > lo"), (lambda: pp(lo=5.0, hi=4.0), "hi > lo"),
                 (lambda: pp(ls=1.0), "smoothing"), (lambda: pp(ls=-0.5), "smoothing"), (lambda: pp(label=256), "label"),
                 (lambda: pp(D=0), "empty"), (lambda: pp(D=1 << 16, H=1 << 10, W=1 << 10), "too large"),
                 (lambda: pp(crops=C.c_void_p(C.addressof(keep[3]) + 4)), "aligned"),
                 (lambda: pp(n=1 << 30, T=64, H=64, W=64), "launch too large")))
