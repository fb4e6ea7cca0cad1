"""Device-side input pipeline of the denoising runs (reference: vit_unet/torch/dataset.py:44-73 and
the albumentations transforms of run_denoising.py:52-59).

The reference decodes, resizes, augments and normalises every image on the host
(`DenoisingDataset.__getitem__`, two DataLoader workers); at the GPU path's step rate that is the
bottleneck.  Here the host only decodes (PNG -> uint8 HWC, out of scope) and draws the augmentation
parameters; `DenoisingBatchTransform` runs resize -> ShiftScaleRotate -> Normalize -> /255 -> CHW
for the whole batch with the HIP kernels of csrc/vu_data.hip (C ABI `vu_denoise_prepare`) and
returns the `{'x','y'}` dict `ImageFitter.unpack` expects.  `DenoisingPatchTransform` is the
native-resolution recipe instead of the resize: random aligned crops of the pair, each under one
of the eight flips / rotations of the square (csrc/vu_patch.hip, C ABI `vu_patch_pairs_u8`).
`SegmentationPatchTransform` is the same recipe for int16 volumes and their label masks, with crops drawn on the
device so that a chosen share holds foreground (csrc/vu_segpatch.hip).
No CPU fallback.
"""
from __future__ import annotations

import math
import random
from typing import Dict, List, Optional

import numpy as np
import torch

from ._lib import VuError, check, lib, ptr, stream_ptr
from .fitter import ImageFitter  # noqa: F401  (the reference keeps ImageFitter in this module)


def shift_scale_rotate_matrices(B: int, im, shift_limit: float = 0.2, scale_limit: float = 0.2,
                                rotate_limit: float = 20.0, rng: Optional[random.Random] = None) -> np.ndarray:
    """Per-image forward 2x3 matrices of albumentations.ShiftScaleRotate(p=1.0) as
    run_denoising.py:53 configures it: angle ~ U(-rotate_limit, rotate_limit) degrees,
    scale ~ U(1 - scale_limit, 1 + scale_limit), dx, dy ~ U(-shift_limit, shift_limit) (fractions of
    the image size); rotation about (w/2 - 0.5, h/2 - 0.5)."""
    rng = rng or random
    out = np.zeros((B, 2, 3), dtype=np.float64)
    h, w = (im, im) if isinstance(im, int) else im
    cx, cy = w / 2.0 - 0.5, h / 2.0 - 0.5
    for b in range(B):
        angle = rng.uniform(-rotate_limit, rotate_limit)
        scale = rng.uniform(1.0 - scale_limit, 1.0 + scale_limit)
        dx, dy = rng.uniform(-shift_limit, shift_limit), rng.uniform(-shift_limit, shift_limit)
        a = scale * math.cos(math.radians(angle))
        s = scale * math.sin(math.radians(angle))
        out[b] = [[a, s, (1 - a) * cx - s * cy + dx * w], [-s, a, s * cx + (1 - a) * cy + dy * h]]
    return out


def invert_affine(fwd: np.ndarray) -> np.ndarray:
    """(B,2,3) forward matrices -> (B,2,3) inverse matrices, the way cv2.warpAffine inverts them."""
    M = np.asarray(fwd, dtype=np.float64).reshape(-1, 2, 3)
    out = np.empty_like(M)
    for b in range(M.shape[0]):
        m = M[b]
        D = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
        D = 1.0 / D if D != 0 else 0.0
        i00, i11 = m[1, 1] * D, m[0, 0] * D
        i01, i10 = m[0, 1] * (-D), m[1, 0] * (-D)
        out[b] = [[i00, i01, -i00 * m[0, 2] - i01 * m[1, 2]], [i10, i11, -i10 * m[0, 2] - i11 * m[1, 2]]]
    return out


class DenoisingBatchTransform:
    """`train=True`: run_denoising.py:52-55 (ShiftScaleRotate + Normalize); `train=False`: :57-59
    (Normalize only).  Call with decoded uint8 batches (B,H,W,C) (numpy or torch, host or device);
    returns {'x': (B,C,im,im) float32, 'y': ...} on the device."""

    def __init__(self, im_size: int = 224, train: bool = True, mean: float = 0.456, std: float = 0.224,
                 device="cuda", seed: Optional[int] = None):
        self.im_size, self.train, self.mean, self.std, self.device = int(im_size), bool(train), float(mean), float(std), device
        self.rng = random.Random(seed)

    def _u8(self, a) -> torch.Tensor:
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        assert t.dtype == torch.uint8 and t.dim() == 4, "expected a (B,H,W,C) uint8 batch"
        return t.to(self.device, non_blocking=True).contiguous()

    def __call__(self, noisy, clean, matrices: Optional[np.ndarray] = None) -> Dict[str, torch.Tensor]:
        n, c = self._u8(noisy), self._u8(clean)
        assert n.shape == c.shape, f"noisy {tuple(n.shape)} and clean {tuple(c.shape)} differ"
        B, H, W, Cn = n.shape
        im = self.im_size
        L = lib()
        x = torch.empty(B, Cn, im, im, dtype=torch.float32, device=n.device)
        y = torch.empty_like(x)
        nb = L.vu_denoise_prepare_scratch_bytes(B, im, Cn)
        scratch = torch.empty(max(nb, 1), dtype=torch.uint8, device=n.device)
        minv = None
        if self.train:
            fwd = matrices if matrices is not None else shift_scale_rotate_matrices(B, im, rng=self.rng)
            assert np.asarray(fwd).shape == (B, 2, 3), "matrices must be (B,2,3)"
            minv = torch.from_numpy(invert_affine(fwd).reshape(B, 6)).to(n.device)
        check(L.vu_denoise_prepare(ptr(n), ptr(c), ptr(x), ptr(y), ptr(scratch), scratch.numel(), ptr(minv), B, H, W, Cn, im,
                                   self.mean, self.std, stream_ptr(n.device)), "vu_denoise_prepare")
        return {"x": x, "y": y}


def dihedral_inverse(op: int) -> int:
    """The op (0..7) that undoes dihedral op `op` (include/vit_unet_amd.h: vu_dihedral_inverse; host code, no GPU)."""
    inv = lib().vu_dihedral_inverse(int(op))
    if inv < 0:
        raise VuError(f"a dihedral op is in 0 .. 7 (got {op})")
    return inv


class DenoisingPatchTransform:
    """Native-resolution training patches: `per_image` aligned crops of `patch` x `patch` pixels out of every noisy / clean
    pair, each under one of the eight dihedral ops (op & 3 counter-clockwise quarter turns after a left-right flip when
    op & 4), normalised like the validation transform of `DenoisingBatchTransform` (Normalize on noisy, /255 on both) - no
    resize anywhere.  Call with `(noisy, clean)`: (B,H,W,C) uint8 batches or lists of (H,W,C) uint8 images whose sizes may
    differ from pair to pair (numpy or torch, host or device); returns {'x','y'} (B*per_image,C,patch,patch) float32 on the
    device, the patches of image 0 first.

    `train=True` draws (y0, x0, op) per patch from the transform's own `random.Random(seed)`; `train=False` is ONE centred
    crop per image (y0 = (H-T)//2, x0 = (W-T)//2) with op 0.  `crops=` (B,per_image,3) replaces the draw.  Out-of-range
    table entries, mismatched pairs and images smaller than a patch are refused here, before any launch (the kernel itself
    clamps what it is given).  One `vu_patch_pairs_u8` call per pair, into slices of one output tensor."""

    def __init__(self, patch: int = 224, per_image: int = 8, train: bool = True, mean: float = 0.456, std: float = 0.224,
                 device="cuda", seed: Optional[int] = None):
        self.patch, self.train = int(patch), bool(train)
        self.per_image = int(per_image) if self.train else 1
        if self.patch < 1 or self.per_image < 1:
            raise VuError(f"patch and per_image must be at least 1 (got {patch}, {per_image})")
        if not float(std) > 0:
            raise VuError(f"std must be positive (got {std})")
        self.mean, self.std, self.device = float(mean), float(std), device
        self.rng = random.Random(seed)

    def draw(self, sizes) -> np.ndarray:
        """The (B,per_image,3) int32 crop table for images of `sizes` = [(H,W), ...] (host code, no GPU)."""
        T = self.patch
        out = np.zeros((len(sizes), self.per_image, 3), dtype=np.int32)
        for b, (H, W) in enumerate(sizes):
            if H < T or W < T:
                raise VuError(f"image {b} ({H} x {W}) is smaller than a patch of {T}")
            for p in range(self.per_image):
                if self.train:
                    out[b, p] = (self.rng.randint(0, H - T), self.rng.randint(0, W - T), self.rng.randint(0, 7))
                else:
                    out[b, p] = ((H - T) // 2, (W - T) // 2, 0)
        return out

    def _images(self, a) -> List[torch.Tensor]:
        if isinstance(a, np.ndarray) or torch.is_tensor(a):
            assert a.ndim == 4, "expected a (B,H,W,C) uint8 batch or a list of (H,W,C) uint8 images"
        out = []
        for im in a:
            t = torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else im
            assert torch.is_tensor(t) and t.dtype == torch.uint8 and t.dim() == 3, "expected (H,W,C) uint8 images"
            out.append(t.to(self.device, non_blocking=True).contiguous())
        return out

    def __call__(self, noisy, clean, crops=None) -> Dict[str, torch.Tensor]:
        ns, cs = self._images(noisy), self._images(clean)
        assert len(ns) == len(cs) and len(ns) > 0, f"{len(ns)} noisy and {len(cs)} clean images"
        T, P = self.patch, self.per_image
        for b, (n, c) in enumerate(zip(ns, cs)):
            assert n.shape == c.shape, f"pair {b}: noisy {tuple(n.shape)} and clean {tuple(c.shape)} differ"
            assert n.shape[2] == ns[0].shape[2], f"pair {b}: {n.shape[2]} channels, pair 0 has {ns[0].shape[2]}"
            if n.shape[0] < T or n.shape[1] < T:
                raise VuError(f"image {b} ({n.shape[0]} x {n.shape[1]}) is smaller than a patch of {T}")
        B, Cn = len(ns), int(ns[0].shape[2])
        if not 1 <= Cn <= 4:
            raise VuError(f"1 to 4 channels (got {Cn})")
        if crops is None:
            table = self.draw([(int(n.shape[0]), int(n.shape[1])) for n in ns])
        else:
            table = np.asarray(crops.cpu() if torch.is_tensor(crops) else crops)
            assert table.shape == (B, P, 3), f"crops must be ({B},{P},3), got {table.shape}"
            assert np.issubdtype(table.dtype, np.integer), "crops must be integers"
            for b, n in enumerate(ns):
                t = table[b]
                if (t < 0).any() or (t[:, 0] > n.shape[0] - T).any() or (t[:, 1] > n.shape[1] - T).any() or (t[:, 2] > 7).any():
                    raise VuError(f"crops[{b}] leaves the image ({n.shape[0]} x {n.shape[1]}, patch {T}) or names an op outside 0 .. 7")
            table = np.ascontiguousarray(table, dtype=np.int32)
        dev = ns[0].device
        L, st = lib(), stream_ptr(dev)
        d = torch.from_numpy(table).to(dev)
        x = torch.empty(B * P, Cn, T, T, dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        for b in range(B):
            H, W = int(ns[b].shape[0]), int(ns[b].shape[1])
            check(L.vu_patch_pairs_u8(ptr(ns[b]), ptr(cs[b]), ptr(x[b * P:(b + 1) * P]), ptr(y[b * P:(b + 1) * P]), H, W, Cn, T,
                                      ptr(d[b]), P, self.mean, self.std, st), "vu_patch_pairs_u8")
        return {"x": x, "y": y}


class SegmentationBatchTransform:
    """Device-side scaling / augmentation for SegmentationDataset batches (the reference leaves both
    to the caller's `augments`, dataset.py:32-36): resize to `im_size` (bilinear slice, nearest
    mask) -> ShiftScaleRotate when `train` -> intensity window `window` -> [0,1]; mask ->
    label (1 - ls) + ls / 2.  Call with image (B,H,W) int16 and mask (B,H,W) uint8 (either may be
    None); returns {'x': (B,1,h,w) float32, 'y': ...} on the device (C ABI `vu_seg_prepare`)."""

    def __init__(self, im_size=(128, 128), train: bool = True, window=(-1024.0, 1024.0), ls: float = 0.0,
                 device="cuda", seed: Optional[int] = None):
        self.im_size = (int(im_size), int(im_size)) if isinstance(im_size, int) else (int(im_size[0]), int(im_size[1]))
        self.train, self.window, self.ls, self.device = bool(train), (float(window[0]), float(window[1])), float(ls), device
        self.rng = random.Random(seed)

    def _dev(self, a, dtype) -> Optional[torch.Tensor]:
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        assert t.dtype == dtype and t.dim() == 3, f"expected a (B,H,W) {dtype} batch, got {t.dtype} {tuple(t.shape)}"
        return t.to(self.device, non_blocking=True).contiguous()

    def __call__(self, image, mask=None, matrices: Optional[np.ndarray] = None) -> Dict[str, torch.Tensor]:
        i, m = self._dev(image, torch.int16), self._dev(mask, torch.uint8)
        ref = i if i is not None else m
        assert ref is not None, "nothing to transform"
        assert i is None or m is None or i.shape == m.shape, "image and mask shapes differ"
        B, H, W = ref.shape
        oh, ow = self.im_size
        L = lib()
        x = torch.empty(B, 1, oh, ow, dtype=torch.float32, device=ref.device) if i is not None else None
        y = torch.empty(B, 1, oh, ow, dtype=torch.float32, device=ref.device) if m is not None else None
        scratch = torch.empty(max(L.vu_seg_prepare_scratch_bytes(B, oh, ow), 2), dtype=torch.uint8, device=ref.device)
        minv = None
        if self.train:
            fwd = matrices if matrices is not None else shift_scale_rotate_matrices(B, (oh, ow), rng=self.rng)
            assert np.asarray(fwd).shape == (B, 2, 3), "matrices must be (B,2,3)"
            minv = torch.from_numpy(invert_affine(fwd).reshape(B, 6)).to(ref.device)
        check(L.vu_seg_prepare(ptr(i), ptr(m), ptr(x), ptr(y), ptr(scratch), scratch.numel(), ptr(minv), B, H, W, oh, ow,
                               self.window[0], self.window[1], self.ls, stream_ptr(ref.device)), "vu_seg_prepare")
        out = {}
        if x is not None:
            out["x"] = x
        if y is not None:
            out["y"] = y
        return out


class SegmentationPatchTransform:
    """Native-resolution segmentation training patches: `per_volume` crops of `patch` x `patch` pixels of single slices out
    of every int16 volume and its uint8 label mask, each under one of the eight dihedral ops of `DenoisingPatchTransform`,
    the slice under the intensity window `window` and the mask as label (1 - ls) + ls / 2 exactly as
    `SegmentationBatchTransform(train=False)` gives them - no resize anywhere.  A foreground pixel is mask != 0 (`label` < 0)
    or mask == label.  Call with `(image, mask)`: one (H,W) / (D,H,W) int16 volume and its uint8 mask, or lists of them whose
    sizes may differ (numpy or torch, host or device); returns {'x','y'} (sum per_volume,1,patch,patch) float32 on the device,
    the patches of volume 0 first.

    `train=True`: the crops are drawn ON THE DEVICE (C ABI `vu_fg_index`, `vu_segpatch_draw`) from `draw_words(per_volume)`,
    four uint32 words per crop out of the transform's own `random.Random(seed)`: with probability `fg` a crop is placed
    around a uniformly chosen foreground pixel of the volume (which then lies inside it), otherwise (and when the volume has
    no foreground) uniformly; the formulas are in include/vit_unet_amd.h.  The host never waits for the device.
    `train=False` is ONE centred crop of the middle slice (z = D//2, y0 = (H-T)//2, x0 = (W-T)//2) with op 0 and launches no
    draw.  `crops=` - one (per_volume,4) integer table (z, y0, x0, op) per volume - replaces the draw and is checked on the
    host.  `last_crops` keeps the device tables of the last call (a list, one (per_volume,4) int32 tensor per volume).
    `window` may be a `segment.IntensityNormalizer` instead of a (lo, hi) pair: every volume of a call is then measured (its mask
    is the mask of select "mask"), which waits for the device once per volume; `windows=` - one (lo, hi) per volume, e.g. measured
    once before training - replaces the measurement (or the constructor's pair): no statistics launch and no wait.
    Argument errors raise `VuError` before any launch (the cut itself clamps what it is given)."""

    def __init__(self, patch: int = 224, per_volume: int = 8, train: bool = True, window=(-1024.0, 1024.0), ls: float = 0.0,
                 fg: float = 0.5, label: int = -1, device="cuda", seed: Optional[int] = None):
        self.patch, self.train = int(patch), bool(train)
        self.per_volume = int(per_volume) if self.train else 1
        if self.patch < 1 or self.per_volume < 1:
            raise VuError(f"patch and per_volume must be at least 1 (got {patch}, {per_volume})")
        if self.patch > 65535:
            raise VuError(f"a patch has at most 65535 pixels a side (got {patch})")
        from .segment import IntensityNormalizer, window_pair
        self.normalizer = window if isinstance(window, IntensityNormalizer) else None
        lo_hi = None if self.normalizer is not None else window_pair(window)
        if not 0.0 <= float(ls) < 1.0:
            raise VuError(f"label smoothing must be in [0,1) (got {ls})")
        if not 0.0 <= float(fg) <= 1.0:
            raise VuError(f"fg, the share of foreground crops, must be in [0,1] (got {fg})")
        if int(label) > 255:
            raise VuError(f"label must be negative (any non-zero mask value) or 0 .. 255 (got {label})")
        self.window, self.ls, self.fg, self.label, self.device = lo_hi, float(ls), float(fg), int(label), device
        self.rng = random.Random(seed)
        self.last_crops: Optional[List[torch.Tensor]] = None

    @property
    def fg_thresh(self) -> int:
        """A crop is a foreground crop when its first random word is below this (0: never)."""
        return min(int(self.fg * 2 ** 32), 2 ** 32 - 1)

    def draw_words(self, n: int) -> np.ndarray:
        """The next (n,4) uint32 words of the transform's generator (host code, no GPU): per crop the branch word, the rank /
        slice word, the two 16-bit offsets and the op word."""
        return np.array([[self.rng.getrandbits(32) for _ in range(4)] for _ in range(int(n))], dtype=np.uint32).reshape(int(n), 4)

    def _volumes(self, a, dtype, what) -> List[torch.Tensor]:
        if isinstance(a, np.ndarray) or torch.is_tensor(a):
            a = [a]
        if not isinstance(a, (list, tuple)) or len(a) == 0:
            raise VuError(f"expected one (H,W) or (D,H,W) {dtype} {what} or a non-empty list of them")
        out = []
        for v in a:
            t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
            if not torch.is_tensor(t) or t.dim() not in (2, 3) or t.dtype != dtype or t.numel() == 0:
                got = f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else type(v).__name__
                raise VuError(f"expected (H,W) or (D,H,W) {dtype} {what}s, got {got}")
            out.append(t.reshape((-1,) + tuple(t.shape[-2:])))
        return out

    def _check_table(self, crops, b, shape) -> np.ndarray:
        D, H, W = shape
        T, P = self.patch, self.per_volume
        t = np.asarray(crops.cpu() if torch.is_tensor(crops) else crops)
        if t.shape != (P, 4) or not np.issubdtype(t.dtype, np.integer):
            raise VuError(f"crops[{b}] must be an integer table of shape ({P},4), got {t.dtype} {t.shape}")
        if (t < 0).any() or (t[:, 0] > D - 1).any() or (t[:, 1] > H - T).any() or (t[:, 2] > W - T).any() or (t[:, 3] > 7).any():
            raise VuError(f"crops[{b}] leaves the volume ({D} x {H} x {W}, patch {T}) or names an op outside 0 .. 7")
        return np.ascontiguousarray(t, dtype=np.int32)

    def __call__(self, image, mask, crops=None, windows=None) -> Dict[str, torch.Tensor]:
        vs, ms = self._volumes(image, torch.int16, "volume"), self._volumes(mask, torch.uint8, "mask")
        if len(vs) != len(ms):
            raise VuError(f"{len(vs)} volumes and {len(ms)} masks")
        T, P, B = self.patch, self.per_volume, len(vs)
        shapes = []
        for b, (v, m) in enumerate(zip(vs, ms)):
            if v.shape != m.shape:
                raise VuError(f"pair {b}: volume {tuple(v.shape)} and mask {tuple(m.shape)} differ")
            D, H, W = (int(s) for s in v.shape)
            if H < T or W < T:
                raise VuError(f"volume {b} ({H} x {W} slices) is smaller than a patch of {T}")
            if H > 65535 or W > 65535 or D * H * W >= 2 ** 32:
                raise VuError(f"volume {b} ({D} x {H} x {W}) is too large (65535 a side, below 2^32 pixels)")
            shapes.append((D, H, W))
        tables = None
        if crops is not None:
            if len(crops) != B:
                raise VuError(f"crops must hold one ({P},4) table per volume ({B}), got {len(crops)}")
            tables = [self._check_table(c, b, shapes[b]) for b, c in enumerate(crops)]
        elif not self.train:
            tables = [np.array([[D // 2, (H - T) // 2, (W - T) // 2, 0]], dtype=np.int32) for D, H, W in shapes]
        if windows is not None:
            from .segment import window_pair
            if not isinstance(windows, (list, tuple)) or len(windows) != B:
                raise VuError(f"windows must hold one (lo, hi) per volume ({B})")
            windows = [window_pair(w, f"windows[{b}]") for b, w in enumerate(windows)]
        if not str(self.device).startswith("cuda"):
            raise VuError("SegmentationPatchTransform runs on the MI355X only (device 'cuda'; no CPU fallback)")
        vs = [v.to(self.device, non_blocking=True).contiguous() for v in vs]
        ms = [m.to(self.device, non_blocking=True).contiguous() for m in ms]
        dev = vs[0].device
        L, st = lib(), stream_ptr(dev)
        if windows is None:
            windows = [self.window] * B if self.normalizer is None else [self.normalizer.window(vs[b], ms[b]) for b in range(B)]
        x = torch.empty(B * P, 1, T, T, dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        self.last_crops = []
        for b, (D, H, W) in enumerate(shapes):
            if tables is not None:
                d = torch.from_numpy(tables[b]).to(dev)
            else:
                words = torch.from_numpy(self.draw_words(P).view(np.int32)).to(dev)
                index = torch.empty(D * H + 1, dtype=torch.int32, device=dev)
                nbytes = int(L.vu_fg_index_bytes(D, H))
                scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
                d = torch.empty(P, 4, dtype=torch.int32, device=dev)
                check(L.vu_fg_index(ptr(ms[b]), ptr(index), ptr(scratch), nbytes, D, H, W, self.label, st), "vu_fg_index")
                check(L.vu_segpatch_draw(ptr(ms[b]), ptr(index), ptr(words), ptr(d), P, D, H, W, T, self.fg_thresh, self.label, st),
                      "vu_segpatch_draw")
            self.last_crops.append(d)
            lo, hi = windows[b]
            check(L.vu_patch_pairs_i16(ptr(vs[b]), ptr(ms[b]), ptr(x[b * P:(b + 1) * P]), ptr(y[b * P:(b + 1) * P]), D, H, W, T, ptr(d),
                                       P, lo, hi, self.ls, self.label, st), "vu_patch_pairs_i16")
        return {"x": x, "y": y}


def _read_png_bgr(path: str) -> np.ndarray:
    """cv2.imread(path) without OpenCV: decoded 8-bit pixels, HWC, BGR channel order."""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


class DenoisingDataset(torch.utils.data.Dataset):
    """dataset.py:44-73, host half only: an item is the DECODED pair {'x': noisy, 'y': clean} as
    (H,W,3) uint8 BGR arrays.  The reference's per-item resize / augment / normalise / CHW steps run
    per batch on the GPU: pass a `DenoisingBatchTransform` as `augments` and iterate with
    `DeviceBatches` (or call `dataset.augments(noisy_batch, clean_batch)` yourself).  `read` replaces
    the decoder (default: PIL in cv2.imread's BGR order)."""

    def __init__(self, img_names, augments=None, clean_folder='/ssid/clean/', noisy_folder='/ssid/noisy/', im_size=224,
                 read=None):
        import os
        self._join = os.path.join
        self.img_names, self.augments = img_names, augments
        self.clean_folder, self.noisy_folder, self.im_size = clean_folder, noisy_folder, im_size
        self.read = read or _read_png_bgr
        if augments is not None and not isinstance(augments, (DenoisingBatchTransform, DenoisingPatchTransform)):
            raise TypeError("augments must be a DenoisingBatchTransform (the albumentations pipeline of "
                            "run_denoising.py:52-59 runs on the device here), a DenoisingPatchTransform or None")

    def __getitem__(self, idx):
        name = self.img_names[idx]
        return {'x': self.read(self._join(self.noisy_folder, name) + '.png'),
                'y': self.read(self._join(self.clean_folder, name) + '.png')}

    def __len__(self):
        return len(self.img_names)

    def transform(self, items) -> Dict[str, torch.Tensor]:
        """A list of items -> one device batch {'x','y'} (B,3,im,im) float32 (a `DenoisingPatchTransform` takes all items at
        once, whatever their sizes, and gives B * per_image patches)."""
        if isinstance(self.augments, DenoisingPatchTransform):
            return self.augments([np.asarray(it['x']) for it in items], [np.asarray(it['y']) for it in items])
        t = self.augments or DenoisingBatchTransform(im_size=self.im_size, train=False)
        return _batched(items, lambda xs, ys: t(np.stack(xs), np.stack(ys)))


class SegmentationDataset(torch.utils.data.Dataset):
    """dataset.py:9-41, host half only: an item is {'x': DICOM slice (H,W) int16, 'y': mask plane
    (H,W) uint8 labels} as read (`read_image(path)` / `read_mask(path, index)`; defaults: pydicom
    pixel_array and nibabel get_fdata()[:, :, index], imported lazily).  Scaling / augmentation runs
    per batch on the GPU: `augments` is a `SegmentationBatchTransform` (default: resize to `im_size`,
    label smoothing `ls`, no warp) or a `SegmentationPatchTransform` (native-resolution crops with foreground
    sampling; it needs the masks, so not with `is_test`).  `is_test`: items carry no mask."""

    def __init__(self, df, augments=None, is_test=False, data_folder='output', im_size=(128, 128), ls=0.0,
                 read_image=None, read_mask=None):
        self.df, self.augments, self.is_test = df, augments, is_test
        self.data_folder, self.im_size, self.ls = data_folder, im_size, ls
        self.read_image, self.read_mask = read_image or self._dicom, read_mask or self._nifti
        if augments is not None and not isinstance(augments, (SegmentationBatchTransform, SegmentationPatchTransform)):
            raise TypeError("augments must be a SegmentationBatchTransform, a SegmentationPatchTransform or None")

    @staticmethod
    def _dicom(path):
        import pydicom
        a = np.asarray(pydicom.read_file(path).pixel_array)
        # the device pipeline takes int16 slices (vu_seg_prepare): unsigned 16-bit DICOM (PixelRepresentation = 0) values
        # >= 32768 would wrap negative in the cast - refuse them instead of silently windowing wrapped intensities
        if a.dtype != np.int16 and a.size and (int(a.max()) > 32767 or int(a.min()) < -32768):
            raise ValueError(f"{path}: pixel values outside the int16 range ({a.dtype}, max {int(a.max())}): pass a `read_image` "
                             "that applies RescaleSlope / RescaleIntercept (or shifts the range) and returns int16")
        return a.astype(np.int16)

    @staticmethod
    def _nifti(path, index):
        import nibabel as nib
        return np.asarray(nib.load(path).get_fdata()[:, :, index]).astype(np.uint8)

    def __getitem__(self, idx):
        row = self.df.loc[idx]
        item = {'x': self.read_image(row['image'])}
        if not self.is_test:
            item['y'] = self.read_mask(row['mask'], row['mask_index'])
        return item

    def __len__(self):
        return len(self.df)

    def transform(self, items) -> Dict[str, torch.Tensor]:
        """A list of items -> one device batch (a `SegmentationPatchTransform` takes all items at once, whatever their sizes,
        and gives len(items) * per_volume patches)."""
        if isinstance(self.augments, SegmentationPatchTransform):
            if self.is_test:
                raise VuError("a SegmentationPatchTransform draws its crops from the masks: not with is_test")
            return self.augments([np.asarray(it['x']) for it in items], [np.asarray(it['y']) for it in items])
        t = self.augments or SegmentationBatchTransform(im_size=self.im_size, train=False, ls=self.ls)
        if self.is_test:
            return _batched(items, lambda xs, ys: t(np.stack(xs), None), with_y=False)
        return _batched(items, lambda xs, ys: t(np.stack(xs), np.stack(ys)))


def _batched(items, fn, with_y=True):
    """Items of one source size go through `fn` together; mixed sizes are grouped (order kept)."""
    groups = {}
    for i, it in enumerate(items):
        groups.setdefault(np.asarray(it['x']).shape, []).append(i)
    parts, order = [], []
    for idxs in groups.values():
        parts.append(fn([np.asarray(items[i]['x']) for i in idxs], [np.asarray(items[i]['y']) for i in idxs] if with_y else None))
        order += idxs
    if len(parts) == 1:
        return parts[0]
    inv = torch.as_tensor(np.argsort(order), device=parts[0]['x'].device)
    return {k: torch.cat([p[k] for p in parts]).index_select(0, inv) for k in parts[0]}


class DeviceBatches:
    """The DataLoader of run_denoising.py:60-75 for the device pipeline: host workers decode items
    (`num_workers` DataLoader workers, identity collate), the dataset's batch transform runs on the
    GPU, and what comes out is the {'x','y'} dict `ImageFitter.unpack` takes."""

    def __init__(self, dataset, batch_size=1, shuffle=False, num_workers=0, drop_last=False):
        self.dataset = dataset
        self.loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers,
                                                  drop_last=drop_last, collate_fn=list)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for items in self.loader:
            yield self.dataset.transform(items)
