"""Segmentation mask clean-up, host side (no GPU): the plain numpy / Python restatements of `vu_cc_label` and `vu_seg_clean`,
written from the text of include/vit_unet_amd.h, that tests/test_gpu_segclean.py holds the HIP kernels against; their answers
on small hand-written arrays; and every argument error `MaskCleaner` and the C entries report before any GPU call."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_segment_cpu import ref_counts  # noqa: F401  (re-exported for the GPU tests)
from vit_unet.torch import _lib
from vit_unet.torch.segment import MaskCleaner, TiledSegmenter


# ---------------------------------------------------------------- the definition of the header, restated
def neighbours(conn):
    """Offsets (dz, dy, dx) of the connectivity: 4 / 8 inside a slice, 6 / 26 in the volume."""
    if conn == 4:
        return [(0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    if conn == 8:
        return [(0, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
    if conn == 6:
        return [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    assert conn == 26
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]


DUAL = {8: 4, 4: 8, 26: 6, 6: 26}


def ref_label(mask, conn, fg=1):
    """(D,H,W) uint8 -> labels int32 (-1 unlabelled, else the smallest linear index of the component), sizes uint32 (the pixel
    count at the smallest index, 0 elsewhere).  A raster-order flood fill: the first pixel met is the smallest index."""
    mask = np.asarray(mask)
    D, H, W = mask.shape
    sel = (mask != 0) if fg else (mask == 0)
    labels = np.full((D, H, W), -1, dtype=np.int32)
    sizes = np.zeros((D, H, W), dtype=np.uint32)
    nb = neighbours(conn)
    for z, y, x in zip(*np.nonzero(sel)):               # np.nonzero lists in raster order
        if labels[z, y, x] >= 0:
            continue
        root = (int(z) * H + int(y)) * W + int(x)
        labels[z, y, x] = root
        stack, n = [(int(z), int(y), int(x))], 0
        while stack:
            cz, cy, cx = stack.pop()
            n += 1
            for dz, dy, dx in nb:
                qz, qy, qx = cz + dz, cy + dy, cx + dx
                if 0 <= qz < D and 0 <= qy < H and 0 <= qx < W and sel[qz, qy, qx] and labels[qz, qy, qx] < 0:
                    labels[qz, qy, qx] = root
                    stack.append((qz, qy, qx))
        sizes[z, y, x] = n
    return labels, sizes


def ref_clean(mask, conn, min_size=0, keep_largest=False, fill_holes=False):
    """The four steps of vu_seg_clean -> (out uint8 {0,1}, stats (U,4) int64: found, kept, largest, overflow = 0)."""
    mask = np.asarray(mask)
    D, H, W = mask.shape
    vol = conn in (6, 26)
    units = [slice(0, D)] if vol else [slice(z, z + 1) for z in range(D)]
    labels, sizes = ref_label(mask, conn, 1)                                   # 1. label the foreground
    out = np.zeros((D, H, W), dtype=np.uint8)
    stats = np.zeros((len(units), 4), dtype=np.int64)
    flat_sizes = sizes.reshape(-1)
    for u, sl in enumerate(units):
        lab = labels[sl]
        roots = np.unique(lab[lab >= 0])
        stats[u, 0] = len(roots)
        stats[u, 2] = max((int(flat_sizes[r]) for r in roots), default=0)
        kept = [int(r) for r in roots if int(flat_sizes[r]) >= min_size]       # 2. drop size < min_size
        if keep_largest and kept:                                              # 3. largest, ties to the smallest root
            kept = [min(kept, key=lambda r: (-int(flat_sizes[r]), r))]
        stats[u, 1] = len(kept)
        out[sl] = np.isin(lab, kept) & (lab >= 0)
    if fill_holes:                                                             # 4. background components off every border
        bl, _ = ref_label(out, DUAL[conn], 0)
        for sl in units:
            lab = bl[sl]
            faces = [lab[:, 0, :], lab[:, -1, :], lab[:, :, 0], lab[:, :, -1]] + ([lab[0], lab[-1]] if vol else [])
            border = np.unique(np.concatenate([f.reshape(-1) for f in faces]))
            out[sl] |= ((lab >= 0) & ~np.isin(lab, border)).astype(np.uint8)
    return out, stats


def arr(rows):
    """One slice from strings of '#' and '.'."""
    return np.array([[c == "#" for c in r] for r in rows], dtype=np.uint8)[None]


# ---------------------------------------------------------------- known answers
def test_two_pixels_touching_diagonally():
    m = arr(["#..",
             ".#.",
             "..."])
    l4, s4 = ref_label(m, 4)
    l8, s8 = ref_label(m, 8)
    assert l4[0].tolist() == [[0, -1, -1], [-1, 4, -1], [-1, -1, -1]] and s4[0, 0, 0] == 1 and s4[0, 1, 1] == 1 and s4.sum() == 2
    assert l8[0].tolist() == [[0, -1, -1], [-1, 0, -1], [-1, -1, -1]] and s8[0, 0, 0] == 2 and s8.sum() == 2
    lb, sb = ref_label(m, 4, fg=0)                     # the background is one 4-connected piece of 7 pixels rooted at index 1
    assert (lb[0][m[0] == 0] == 1).all() and (lb[0][m[0] != 0] == -1).all() and sb[0, 0, 1] == 7
    # min_size 2 drops both pixels under 4, none under 8
    assert ref_clean(m, 4, min_size=2)[0].sum() == 0 and ref_clean(m, 8, min_size=2)[0].sum() == 2
    # through z: the same two pixels in neighbouring slices
    v = np.zeros((2, 3, 3), dtype=np.uint8)
    v[0, 0, 0] = v[1, 1, 1] = 1
    assert ref_label(v, 6)[1].sum() == 2 and ref_label(v, 6)[0][1, 1, 1] == 13
    assert ref_label(v, 26)[0][1, 1, 1] == 0 and ref_label(v, 26)[1][0, 0, 0] == 2
    assert ref_label(v, 8)[0][1, 1, 1] == 13           # per-slice units never join across z


def test_ring_with_a_hole():
    m = arr([".....",
             ".###.",
             ".#.#.",
             ".###.",
             "....."])
    out, stats = ref_clean(m, 8, fill_holes=True)
    assert out[0, 2, 2] == 1 and out.sum() == 9 and stats.tolist() == [[1, 1, 8, 0]]
    assert np.array_equal(ref_clean(m, 8)[0], m)
    # a diamond ring: closed under 8 (background 4: the hole is cut off), open under 4 (background 8 leaks through the corners)
    d = arr([".....",
             "..#..",
             ".#.#.",
             "..#..",
             "....."])
    assert ref_clean(d, 8, fill_holes=True)[0][0, 2, 2] == 1
    assert ref_clean(d, 4, fill_holes=True)[0][0, 2, 2] == 0 and ref_clean(d, 4)[1].tolist() == [[4, 4, 1, 0]]
    # a ring whose hole holds a small blob: min_size drops the blob, then the whole inside is filled
    r = arr(["#####",
             "#...#",
             "#.#.#",
             "#...#",
             "#####"])
    out, stats = ref_clean(r, 8, min_size=2, fill_holes=True)
    assert out.sum() == 25 and stats.tolist() == [[2, 1, 16, 0]]
    out, _ = ref_clean(r, 8, fill_holes=True)
    assert out.sum() == 25                             # blob kept, the ring-shaped hole around it filled


def test_hole_open_to_the_border():
    m = arr(["###",
             "#.#",
             "#.#"])
    assert np.array_equal(ref_clean(m, 8, fill_holes=True)[0], m)
    m2 = arr(["####",
              "#..#",
              "####"])
    assert ref_clean(m2, 8, fill_holes=True)[0].sum() == 12
    # a closed box in 3-D is a hole of the volume; the same box cut open by the first slice is not
    v = np.ones((3, 3, 3), dtype=np.uint8)
    v[1, 1, 1] = 0
    assert ref_clean(v, 26, fill_holes=True)[0].sum() == 27 and ref_clean(v, 6, fill_holes=True)[0].sum() == 27
    v[0, 1, 1] = 0
    assert ref_clean(v, 26, fill_holes=True)[0].sum() == 25
    # per-slice units: the middle slice's centre is a hole of that slice alone
    assert ref_clean(v, 8, fill_holes=True)[0][1, 1, 1] == 1 and ref_clean(v, 8, fill_holes=True)[0][0, 1, 1] == 1


def test_size_tie_goes_to_the_smallest_root():
    m = arr(["##.##",
             ".....",
             "##..."])
    out, stats = ref_clean(m, 4, keep_largest=True)
    assert out[0].tolist() == [[1, 1, 0, 0, 0], [0] * 5, [0] * 5] and stats.tolist() == [[3, 1, 2, 0]]
    out, stats = ref_clean(m, 4, min_size=3, keep_largest=True)
    assert out.sum() == 0 and stats.tolist() == [[3, 0, 2, 0]]          # an empty unit stays empty
    e = np.zeros((2, 3, 3), dtype=np.uint8)
    out, stats = ref_clean(e, 8, keep_largest=True, fill_holes=True)
    assert out.sum() == 0 and stats.tolist() == [[0, 0, 0, 0]] * 2       # an empty slice has no enclosed background


# ---------------------------------------------------------------- argument errors, before any GPU call
def test_mask_cleaner_constructor_errors():
    for bad in (0, 5, 18, "8", None):
        with pytest.raises(_lib.VuError, match="connectivity"):
            MaskCleaner(connectivity=bad)
    for bad in (-1, 1 << 32, 2.5, True, "3"):
        with pytest.raises(_lib.VuError, match="min_size"):
            MaskCleaner(min_size=bad)
    c = MaskCleaner(26, min_size=np.int64(7), keep_largest=1, fill_holes=0)
    assert (c.connectivity, c.min_size, c.keep_largest, c.fill_holes) == (26, 7, True, False)


def test_mask_cleaner_call_errors():
    c = MaskCleaner()
    with pytest.raises(_lib.VuError, match="uint8"):
        c(np.zeros((4, 4), dtype=np.int16))
    with pytest.raises(_lib.VuError, match="uint8"):
        c(np.zeros((1, 2, 4, 4), dtype=np.uint8))
    with pytest.raises(_lib.VuError, match="empty"):
        c(np.zeros((0, 4), dtype=np.uint8))
    for vol in (np.zeros((4, 4), dtype=np.uint8), np.zeros((1, 4, 4), dtype=np.uint8)):
        with pytest.raises(_lib.VuError, match="needs a"):
            MaskCleaner(6)(vol)
        with pytest.raises(_lib.VuError, match="needs a"):
            MaskCleaner(26).labels(vol)
    with pytest.raises(_lib.VuError, match="shape"):
        c.score(np.zeros((4, 4), dtype=np.uint8), np.zeros((4, 5), dtype=np.uint8))
    with pytest.raises(_lib.VuError, match="label"):
        c.score(np.zeros((4, 4), dtype=np.uint8), np.zeros((4, 4), dtype=np.uint8), label=256)


class _Model:
    im_size, num_channels = 32, 1


def test_tiled_segmenter_clean_argument_errors():
    with pytest.raises(_lib.VuError, match="MaskCleaner"):
        TiledSegmenter(_Model(), overlap=8, clean="largest")
    s = TiledSegmenter(_Model(), overlap=8, clean=MaskCleaner(26))
    vol = np.zeros((2, 40, 40), dtype=np.int16)
    for output in ("logits", "prob"):
        with pytest.raises(_lib.VuError, match="refused"):
            s(vol, output)
    with pytest.raises(_lib.VuError, match="needs a"):
        s(vol[0])
    with pytest.raises(_lib.VuError, match="needs a"):
        s.score(vol[:1], np.zeros((1, 40, 40), dtype=np.uint8))
    assert TiledSegmenter(_Model(), overlap=8).clean is None


def _rc(fn, *a):
    rc = fn(*a)
    return rc, _lib.lib().vu_last_error().decode()


def test_c_entry_argument_errors():
    """Every refusal of the header, with fake (never dereferenced) pointers: the checks run before any launch."""
    L = _lib.lib()
    th, tw = C.c_int(0), C.c_int(0)
    assert L.vu_cc_tile(C.byref(th), C.byref(tw)) == 0 and th.value > 0 and tw.value > 0 and tw.value % 4 == 0
    assert L.vu_cc_tile(None, C.byref(tw)) == -1
    D, H, W = 2, 8, 12
    N = D * H * W
    P = 1 << 20                                   # distinct, aligned, non-overlapping fake addresses
    mask, labels, sizes, scratch, out, truth, counts, stats = (C.c_void_p(P * (i + 1)) for i in range(8))
    need = L.vu_cc_scratch_bytes(D, H, W)
    assert need >= 4 and L.vu_cc_scratch_bytes(0, H, W) == 0

    def label(mask=mask, labels=labels, sizes=sizes, scratch=scratch, nbytes=need, D=D, H=H, W=W, conn=8, fg=1):
        return _rc(L.vu_cc_label, mask, labels, sizes, scratch, nbytes, D, H, W, conn, fg, None)

    for kw, text in [(dict(conn=5), "connectivity"), (dict(conn=0), "connectivity"), (dict(conn=18), "connectivity"),
                     (dict(conn=6, D=1), "single slice"), (dict(conn=26, D=1), "single slice"),
                     (dict(D=0), "empty"), (dict(H=-1), "empty"), (dict(W=0), "empty"),
                     (dict(D=2048, H=1024, W=1024), "2^31"), (dict(fg=2), "fg"), (dict(fg=-1), "fg"),
                     (dict(mask=None), "null"), (dict(labels=None), "null"), (dict(scratch=None), "null"),
                     (dict(nbytes=need - 1), "scratch"), (dict(scratch=C.c_void_p(P * 4 + 2)), "scratch"),
                     (dict(labels=C.c_void_p(P * 2 + 2)), "aligned"), (dict(sizes=C.c_void_p(P * 3 + 1)), "aligned"),
                     (dict(labels=C.c_void_p(P + 4)), "overlap"), (dict(sizes=C.c_void_p(P * 2 + 8)), "overlap"),
                     (dict(scratch=C.c_void_p(P * 2 + 4)), "overlap")]:
        rc, msg = label(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)

    need = L.vu_seg_clean_scratch_bytes(D, H, W)
    assert need >= 8 * N and L.vu_seg_clean_scratch_bytes(D, 0, W) == 0 and L.vu_seg_clean_scratch_bytes(2048, 1024, 1024) == 0
    scr = C.c_void_p(P * 16)

    def clean(mask=mask, truth=truth, out=out, counts=counts, stats=stats, scratch=scr, nbytes=need, D=D, H=H, W=W, conn=8,
              min_size=0, keep=0, fill=0, label=-1):
        return _rc(L.vu_seg_clean, mask, truth, out, counts, stats, scratch, nbytes, D, H, W, conn, min_size, keep, fill, label, None)

    for kw, text in [(dict(conn=7), "connectivity"), (dict(conn=6, D=1), "single slice"), (dict(conn=26, D=1), "single slice"),
                     (dict(D=0), "empty"), (dict(D=2048, H=1024, W=1024), "2^31"), (dict(label=256), "label"),
                     (dict(keep=2), "keep_largest"), (dict(fill=-1), "fill_holes"),
                     (dict(mask=None), "null"), (dict(out=None), "null"), (dict(scratch=None), "null"),
                     (dict(truth=None), "together"), (dict(counts=None), "together"),
                     (dict(nbytes=need - 1), "scratch"), (dict(scratch=C.c_void_p(P * 16 + 8)), "scratch"),
                     (dict(counts=C.c_void_p(P * 7 + 4)), "aligned"), (dict(stats=C.c_void_p(P * 8 + 4)), "aligned"),
                     (dict(out=C.c_void_p(P + 1)), "out is the mask itself"), (dict(scratch=C.c_void_p(P - 16)), "overlap"),
                     (dict(out=C.c_void_p(P * 6 + 16)), "overlap"), (dict(stats=C.c_void_p(P * 16 + 64)), "overlap")]:
        rc, msg = clean(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
