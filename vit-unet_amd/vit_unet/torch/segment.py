"""Whole-slice and volume segmentation: sliding-window inference for the 1-channel segmentation configuration.

The segmentation twin of `restore.TiledRestorer`.  `HViT_UNet.forward` resizes anything that is not `im_size` x
`im_size`, which is the wrong operation for a label mask; `TiledSegmenter` takes a trained segmentation model and an int16
slice (H,W) or volume (D,H,W), covers every slice with the window plan of `restore.tile_plan`, runs the model's eval
forward on batches of windows and blends the window logits back, ending in a uint8 label mask and - against a truth
volume - the integer overlap counts that Dice and IoU are made of.  Cutting (with the intensity window of
`SegmentationBatchTransform`), blending, thresholding and counting are the HIP kernels of csrc/vu_segtile.hip (C ABI
`vu_tile_gather_i16`, `vu_seg_blend`; documented in include/vit_unet_amd.h); the model call in the middle is the
unchanged `vu_model_forward` path.  No CPU fallback.

`MaskCleaner` is the stage after the threshold: connected components on the device (csrc/vu_segclean.hip, C ABI
`vu_cc_label`, `vu_seg_clean`) - drop small components, keep the largest, fill enclosed holes - on a mask that never leaves
the GPU.  `TiledSegmenter(clean=MaskCleaner(...))` returns and scores the cleaned mask.

`SurfaceDistance` adds the boundary metrics organ segmentation is reported with - Hausdorff distance, HD95, average symmetric
surface distance, surface Dice - from an exact integer Euclidean distance transform on the device (csrc/vu_segdist.hip, C ABI
`vu_edt_sq`, `vu_mask_surface`, `vu_surface_dist`); `TiledSegmenter(surface=SurfaceDistance(...))` scores the final mask with
them.

`VolumeResampler` is the step around all of it: volumes and label masks of any voxel size are brought to one working spacing
before patches and windows, and logits are brought back to the volume's own grid before the threshold (csrc/vu_resample.hip,
C ABI `vu_resample_i16`, `vu_resample_u8_nearest`, `vu_resample_f32`); `TiledSegmenter(resample=VolumeResampler(...))` does
both around the model and thresholds, cleans, counts and measures on the native grid.

`IntensityNormalizer` replaces the fixed intensity window by one measured per volume: the exact int16 histogram of the volume
(all voxels, those above a floor, or those of a mask) on the device, and from its integers a percentile or mean +- k std window
formed on the host in exact rational arithmetic (csrc/vu_intensity.hip, C ABI `vu_intensity_hist`, `vu_intensity_stats`).
Every `window=` of this package that takes a (lo, hi) pair also takes one.
"""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import numpy as np
import torch

from ._lib import VuError, check, lib, ptr, stream_ptr
from .restore import TiledRestorer


def dice_from_counts(pred: int, true: int, both: int) -> float:
    """2 both / (pred + true); 1.0 when both sets are empty."""
    den = int(pred) + int(true)
    return 1.0 if den == 0 else 2.0 * int(both) / den


def iou_from_counts(pred: int, true: int, both: int) -> float:
    """both / (pred + true - both); 1.0 when both sets are empty."""
    den = int(pred) + int(true) - int(both)
    return 1.0 if den == 0 else int(both) / den


def logit_threshold(threshold: float) -> float:
    """The logit that belongs to a probability threshold: float32(log(thr / (1 - thr))), computed in float64; exactly 0 for 0.5."""
    thr = float(threshold)
    if not 0.0 < thr < 1.0:
        raise VuError(f"threshold must be inside (0, 1) (got {threshold})")
    return float(np.float32(math.log(thr / (1.0 - thr))))


class MaskCleaner:
    """`c = MaskCleaner(connectivity=8, min_size=0, keep_largest=False, fill_holes=False); clean = c(mask)`.

    mask (H,W) or (D,H,W) uint8 (numpy or torch, host or device; a list / tuple gives a list); any non-zero value is
    foreground.  connectivity 4 / 8 labels every slice on its own, 6 / 26 the whole (D,H,W) volume (refused for a single
    slice).  The steps and their order are those of `vu_seg_clean` (include/vit_unet_amd.h): label, drop components smaller
    than `min_size`, keep the largest remaining one per unit (ties to the smallest index), fill the background components
    that touch no border of their unit (labelled with the dual connectivity).
      cleaner(mask)                 the cleaned {0,1} uint8 mask of the input's shape, on the device
      cleaner.labels(mask)          (labels int32: -1 on background, else the smallest linear index of the component;
                                    sizes int64: the component's pixel count at that index, 0 elsewhere), both of mask's shape
      cleaner.score(mask, truth, label=-1)   {"mask", "counts" (D,3) int64 on the host, "dice", "iou", "stats" (U,4) int64 on the
                                    host: components found, kept, largest size, overflow}; raises VuError on a non-zero overflow
    No CPU fallback: the mask is moved to 'cuda'.  Argument errors raise `VuError` before any launch."""

    def __init__(self, connectivity: int = 8, min_size: int = 0, keep_largest: bool = False, fill_holes: bool = False):
        if connectivity not in (4, 8, 6, 26):
            raise VuError(f"connectivity must be 4 or 8 (slice by slice), 6 or 26 (the volume) (got {connectivity!r})")
        if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)) or not 0 <= int(min_size) <= 0xffffffff:
            raise VuError(f"min_size must be an integer in 0 .. 2^32 - 1 (got {min_size!r})")
        self.connectivity, self.min_size = int(connectivity), int(min_size)
        self.keep_largest, self.fill_holes = bool(keep_largest), bool(fill_holes)

    def _mask(self, mask, what="mask"):
        m = TiledSegmenter._volume(mask, torch.uint8, what)
        if self.connectivity in (6, 26) and (m.dim() == 2 or m.shape[0] == 1):
            raise VuError(f"connectivity {self.connectivity} needs a (D,H,W) volume with D >= 2 (got {tuple(m.shape)}); a slice takes 4 or 8")
        if m.numel() > 0x7fffffff:
            raise VuError(f"{what} {tuple(m.shape)} exceeds 2^31 - 1 pixels")
        return m

    @staticmethod
    def _to_device(t):
        if not torch.cuda.is_available():
            raise VuError("MaskCleaner runs on the MI355X only (no CPU fallback)")
        return (t if t.is_cuda else t.to("cuda", non_blocking=True)).contiguous()

    def __call__(self, mask):
        if isinstance(mask, (list, tuple)):
            return [self(m) for m in mask]
        m = self._mask(mask)
        shape = tuple(m.shape)
        m = self._to_device(m).reshape((-1,) + shape[-2:])
        with torch.cuda.device(m.device):
            return self.run(m, None)["mask"].reshape(shape)

    def labels(self, mask):
        if isinstance(mask, (list, tuple)):
            return [self.labels(m) for m in mask]
        m = self._mask(mask)
        shape = tuple(m.shape)
        m = self._to_device(m).reshape((-1,) + shape[-2:])
        L = lib()
        D, H, W = (int(s) for s in m.shape)
        with torch.cuda.device(m.device):
            labels = torch.empty(D, H, W, dtype=torch.int32, device=m.device)
            sizes = torch.empty(D, H, W, dtype=torch.int32, device=m.device)
            nbytes = int(L.vu_cc_scratch_bytes(D, H, W))
            scratch = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=m.device)
            check(L.vu_cc_label(ptr(m), ptr(labels), ptr(sizes), ptr(scratch), nbytes, D, H, W, self.connectivity, 1,
                                stream_ptr(m.device)), "vu_cc_label")
            if int(scratch[0]) != 0:
                raise VuError("vu_cc_label: an iteration cap was reached (overflow): the labels are not valid")
        return labels.reshape(shape), sizes.reshape(shape).to(torch.int64)

    def score(self, mask, truth, label: int = -1):
        if int(label) > 255:
            raise VuError(f"label must be negative (any non-zero truth) or 0 .. 255 (got {label})")
        m, t = self._mask(mask), TiledSegmenter._volume(truth, torch.uint8, "truth")
        if tuple(m.shape) != tuple(t.shape):
            raise VuError(f"the truth {tuple(t.shape)} does not have the mask's shape {tuple(m.shape)}")
        shape = tuple(m.shape)
        m = self._to_device(m).reshape((-1,) + shape[-2:])
        t = t.to(m.device, non_blocking=True).contiguous().reshape(m.shape)
        with torch.cuda.device(m.device):
            res = self.run(m, t, int(label))
        return self.finish(res, shape)

    @staticmethod
    def finish(res, shape):
        """Host side of a scored `run`: counts and stats to the host, the overflow check, Dice and IoU of the whole volume."""
        counts, stats = res["counts"].cpu(), res["stats"].cpu()
        if int(stats[:, 3].max()) != 0:
            raise VuError("vu_seg_clean: an iteration cap was reached (overflow): the cleaned mask is not valid")
        pred, true, both = (int(c) for c in counts.sum(0))
        return {"mask": res["mask"].reshape(shape), "counts": counts, "dice": dice_from_counts(pred, true, both),
                "iou": iou_from_counts(pred, true, both), "stats": stats}

    def run(self, mask: torch.Tensor, truth, label: int = -1, out=None):
        """One vu_seg_clean on a (D,H,W) uint8 device mask (and truth): {"mask", "stats" (U,4) int64 and, with a truth,
        "counts" (D,3) int64}, all on the device.  `out` may be `mask` itself."""
        L = lib()
        D, H, W = (int(s) for s in mask.shape)
        if self.connectivity in (6, 26) and D == 1:
            raise VuError(f"connectivity {self.connectivity} needs a volume with D >= 2 (got one slice); a slice takes 4 or 8")
        dev = mask.device
        U = 1 if self.connectivity in (6, 26) else D
        res = {"mask": torch.empty(D, H, W, dtype=torch.uint8, device=dev) if out is None else out,
               "stats": torch.empty(U, 4, dtype=torch.int64, device=dev)}
        if truth is not None:
            res["counts"] = torch.empty(D, 3, dtype=torch.int64, device=dev)
        nbytes = int(L.vu_seg_clean_scratch_bytes(D, H, W))
        scratch = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.int32, device=dev)
        check(L.vu_seg_clean(ptr(mask), ptr(truth), ptr(res["mask"]), ptr(res.get("counts")), ptr(res["stats"]), ptr(scratch),
                             nbytes, D, H, W, self.connectivity, self.min_size, int(self.keep_largest), int(self.fill_holes),
                             int(label), stream_ptr(dev)), "vu_seg_clean")
        return res


NO_SITE = 0xffffffff   # vu_edt_sq / vu_surface_dist: no site in this unit


def surface_metrics(stats, sums, order, qnum: int, qden: int) -> dict:
    """The float64 part of the surface metrics, on the host, from the per-unit integers of `vu_surface_dist`
    (include/vit_unet_amd.h): stats (U,6), sums (U,2), order (U,3,2), and the quantile qnum / qden they were selected for.
    Per unit, with P and T the two surfaces:
      hd             sqrt(max(max d(P->T), max d(T->P)))
      hd95           sqrt(a) + (sqrt(b) - sqrt(a)) frac over the pooled set (order[u,2] = (a, b)), n = |P| + |T|,
                     frac = (qnum (n - 1) mod qden) / qden: numpy.percentile(..., method="linear"), MedPy's definition
      hd95_directed  the larger of the same interpolation over d(P->T) and over d(T->P): MONAI's definition
      assd           (sum P->T + sum T->P) / (|P| + |T|)
      nsd            (within P->T + within T->P) / (|P| + |T|)
    A unit with both surfaces empty gives 0, 0, 0, 0 and nsd 1; one with exactly one surface empty inf, inf, inf, inf and nsd 0.
    Returns the per-unit float64 arrays "hd_units", "hd95_units", "hd95_directed_units", "assd_units", "nsd_units", "units" =
    the number of units that are not both-empty, and "hd", "hd95", "hd95_directed", "assd", "nsd" = the means over those
    units (the values of a both-empty unit when there is no other)."""
    st = np.asarray(stats).astype(np.int64).reshape(-1, 6)
    sm = np.asarray(sums, dtype=np.float64).reshape(-1, 2)
    od = np.asarray(order).astype(np.int64).reshape(-1, 3, 2)
    qnum, qden = int(qnum), int(qden)
    if not (1 <= qden and 0 <= qnum <= qden):
        raise VuError(f"the quantile needs 0 <= qnum <= qden, qden >= 1 (got {qnum} / {qden})")
    U = st.shape[0]
    if sm.shape[0] != U or od.shape[0] != U:
        raise VuError(f"stats, sums and order disagree on the number of units ({U}, {sm.shape[0]}, {od.shape[0]})")
    names = ("hd", "hd95", "hd95_directed", "assd", "nsd")
    per = {k: np.zeros(U, dtype=np.float64) for k in names}

    def interp(pair, n):
        a, b = math.sqrt(int(pair[0])), math.sqrt(int(pair[1]))
        frac = ((qnum * (n - 1)) % qden) / qden
        return a + (b - a) * frac

    live = np.zeros(U, dtype=bool)
    for u in range(U):
        n_p, n_t = int(st[u, 0]), int(st[u, 1])
        if n_p == 0 and n_t == 0:
            per["nsd"][u] = 1.0
            continue
        live[u] = True
        if n_p == 0 or n_t == 0:
            for k in names[:4]:
                per[k][u] = math.inf
            continue
        n = n_p + n_t
        per["hd"][u] = math.sqrt(max(int(st[u, 2]), int(st[u, 3])))
        per["hd95"][u] = interp(od[u, 2], n)
        per["hd95_directed"][u] = max(interp(od[u, 0], n_p), interp(od[u, 1], n_t))
        per["assd"][u] = (float(sm[u, 0]) + float(sm[u, 1])) / n
        per["nsd"][u] = (int(st[u, 4]) + int(st[u, 5])) / n
    out = {k + "_units": v for k, v in per.items()}
    out["units"] = int(live.sum())
    for k in names:
        out[k] = float(per[k][live].mean()) if live.any() else (1.0 if k == "nsd" else 0.0)
    return out


class SurfaceDistance:
    """`sd = SurfaceDistance(dims=2, spacing=(1, 1, 1), tolerance=1.0, percentile=95.0); res = sd.score(mask, truth)`.

    Boundary metrics of a mask against a truth, from the exact squared Euclidean distance transform of `vu_edt_sq` on the
    device.  dims 2 treats every slice as a unit, dims 3 the whole (D,H,W) volume (refused for a single slice).  `spacing` =
    (sz, sy, sx): positive integers in a unit of the caller's choice (tenths of a millimetre, say); distances come out in that
    unit, `tolerance` (of the surface Dice) is given in it and enters as tol2 = floor(tolerance^2) - exact, because squared
    distances are integers.  `percentile` becomes qnum / qden = Fraction(percentile / 100).limit_denominator(10000).
    Inputs as `MaskCleaner`: (H,W) or (D,H,W) uint8, numpy or torch, host or device; lists give lists.
      sd.edt(mask, fg=True)            int64 of mask's shape: squared distance to the nearest pixel with mask != 0 (fg) or
                                       mask == 0 (not fg) of the same unit, -1 where the unit has none
      sd.surface(mask, label=-1)       uint8: the foreground pixels with an axis neighbour in the background or outside the unit
      sd.score(mask, truth, label=-1)  {"stats" (U,6) int64, "sums" (U,2) float64, "order" (U,3,2) int64 on the host, as
                                       `vu_surface_dist` defines them} plus everything `surface_metrics` returns: "hd", "hd95",
                                       "hd95_directed", "assd", "nsd", their "*_units" arrays and "units"
    No CPU fallback: the mask is moved to 'cuda'.  Argument errors raise `VuError` before any launch."""

    def __init__(self, dims: int = 2, spacing=(1, 1, 1), tolerance: float = 1.0, percentile: float = 95.0):
        if isinstance(dims, bool) or dims not in (2, 3):
            raise VuError(f"dims must be 2 (slice by slice) or 3 (the volume) (got {dims!r})")
        try:
            sp = tuple(spacing)
        except TypeError:
            sp = ()
        if len(sp) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= 0x7fffffff for v in sp):
            raise VuError(f"spacing must be three positive integers (sz, sy, sx) (got {spacing!r})")
        if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float, np.integer, np.floating)) \
                or not math.isfinite(float(tolerance)) or float(tolerance) < 0.0:
            raise VuError(f"tolerance must be a finite number >= 0 (got {tolerance!r})")
        if isinstance(percentile, bool) or not isinstance(percentile, (int, float, np.integer, np.floating)) \
                or not 0.0 <= float(percentile) <= 100.0:
            raise VuError(f"percentile must be a number in 0 .. 100 (got {percentile!r})")
        self.dims, self.spacing = int(dims), tuple(int(v) for v in sp)
        self.tolerance, self.percentile = float(tolerance), float(percentile)
        t = Fraction(self.tolerance)
        self.tol2 = min(int(math.floor(t * t)), 0x7fffffff)   # no squared distance is larger
        q = (Fraction(self.percentile) / 100).limit_denominator(10000)
        self.qnum, self.qden = int(q.numerator), int(q.denominator)

    def _mask(self, mask, what="mask"):
        m = TiledSegmenter._volume(mask, torch.uint8, what)
        self._check_shape(tuple(m.shape))
        return m

    def _check_shape(self, shape):
        if self.dims == 3 and (len(shape) == 2 or shape[0] == 1):
            raise VuError(f"dims 3 needs a (D,H,W) volume with D >= 2 (got {tuple(shape)}); a slice takes dims 2")
        D, H, W = (1,) * (3 - len(shape)) + tuple(int(v) for v in shape)
        if D * H * W > 0x7fffffff:
            raise VuError(f"{tuple(shape)} exceeds 2^31 - 1 pixels")
        sz, sy, sx = self.spacing
        far = (sy * (H - 1)) ** 2 + (sx * (W - 1)) ** 2 + ((sz * (D - 1)) ** 2 if self.dims == 3 else 0)
        if far > 0x7fffffff:
            raise VuError(f"the largest squared distance of {tuple(shape)} at spacing {self.spacing} is {far} > 2^31 - 1: use a coarser unit")

    @staticmethod
    def _to_device(t):
        if not torch.cuda.is_available():
            raise VuError("SurfaceDistance runs on the MI355X only (no CPU fallback)")
        return (t if t.is_cuda else t.to("cuda", non_blocking=True)).contiguous()

    def edt(self, mask, fg: bool = True):
        if isinstance(mask, (list, tuple)):
            return [self.edt(m, fg) for m in mask]
        m = self._mask(mask)
        shape = tuple(m.shape)
        m = self._to_device(m).reshape((-1,) + shape[-2:])
        L = lib()
        D, H, W = (int(v) for v in m.shape)
        with torch.cuda.device(m.device):
            d2 = torch.empty(D, H, W, dtype=torch.int32, device=m.device)
            nbytes = int(L.vu_edt_scratch_bytes(D, H, W, self.dims))
            scratch = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.int32, device=m.device)
            check(L.vu_edt_sq(ptr(m), ptr(d2), ptr(scratch), nbytes, D, H, W, self.dims, int(bool(fg)), *self.spacing,
                              stream_ptr(m.device)), "vu_edt_sq")
        return d2.reshape(shape).to(torch.int64)   # 0xffffffff -> -1, every distance < 2^31 unchanged

    def surface(self, mask, label: int = -1):
        if isinstance(mask, (list, tuple)):
            return [self.surface(m, label) for m in mask]
        if int(label) > 255:
            raise VuError(f"label must be negative (any non-zero pixel) or 0 .. 255 (got {label})")
        m = self._mask(mask)
        shape = tuple(m.shape)
        m = self._to_device(m).reshape((-1,) + shape[-2:])
        D, H, W = (int(v) for v in m.shape)
        with torch.cuda.device(m.device):
            surf = torch.empty(D, H, W, dtype=torch.uint8, device=m.device)
            check(lib().vu_mask_surface(ptr(m), ptr(surf), D, H, W, self.dims, int(label), stream_ptr(m.device)), "vu_mask_surface")
        return surf.reshape(shape)

    def score(self, mask, truth, label: int = -1):
        if isinstance(mask, (list, tuple)):
            return [self.score(m, t, label) for m, t in zip(mask, truth)]
        if int(label) > 255:
            raise VuError(f"label must be negative (any non-zero truth) or 0 .. 255 (got {label})")
        m, t = self._mask(mask), TiledSegmenter._volume(truth, torch.uint8, "truth")
        if tuple(m.shape) != tuple(t.shape):
            raise VuError(f"the truth {tuple(t.shape)} does not have the mask's shape {tuple(m.shape)}")
        shape = tuple(m.shape)
        m = self._to_device(m).reshape((-1,) + shape[-2:])
        t = t.to(m.device, non_blocking=True).contiguous().reshape(m.shape)
        with torch.cuda.device(m.device):
            res = self.run(m, t, int(label))
        return self.finish(res)

    def finish(self, res) -> dict:
        """Host side of a `run`: the integers to the host and the float64 metrics of `surface_metrics`."""
        stats = res["stats"].cpu()
        sums = res["sums"].cpu()
        order = res["order"].cpu().to(torch.int64) & 0xffffffff
        out = {"stats": stats, "sums": sums, "order": order}
        out.update(surface_metrics(stats.numpy(), sums.numpy(), order.numpy(), self.qnum, self.qden))
        return out

    def run(self, mask: torch.Tensor, truth: torch.Tensor, label: int = -1, maps: bool = False):
        """One vu_surface_dist on (D,H,W) uint8 device tensors: {"stats" (U,6) int64, "sums" (U,2) float64, "order" (U,3,2)
        int32 holding the uint32 bits} on the device; with `maps` also "dist_pt" / "dist_tp" (D,H,W) int32 bits."""
        L = lib()
        D, H, W = (int(v) for v in mask.shape)
        self._check_shape((D, H, W))
        dev = mask.device
        U = 1 if self.dims == 3 else D
        res = {"stats": torch.empty(U, 6, dtype=torch.int64, device=dev), "sums": torch.empty(U, 2, dtype=torch.float64, device=dev),
               "order": torch.empty(U, 3, 2, dtype=torch.int32, device=dev)}
        if maps:
            res["dist_pt"] = torch.empty(D, H, W, dtype=torch.int32, device=dev)
            res["dist_tp"] = torch.empty(D, H, W, dtype=torch.int32, device=dev)
        nbytes = int(L.vu_surface_dist_scratch_bytes(D, H, W, self.dims))
        scratch = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.int32, device=dev)
        check(L.vu_surface_dist(ptr(mask), ptr(truth), ptr(res["stats"]), ptr(res["sums"]), ptr(res["order"]), ptr(res.get("dist_pt")),
                                ptr(res.get("dist_tp")), ptr(scratch), nbytes, D, H, W, self.dims, *self.spacing, int(label),
                                self.tol2, self.qnum, self.qden, stream_ptr(dev)), "vu_surface_dist")
        return res


class VolumeResampler:
    """`r = VolumeResampler(target_spacing=(None, 1.0, 1.0)); work = r.image(vol, spacing)`.

    Brings volumes of any voxel size to one working spacing and results back, on the device (csrc/vu_resample.hip, C ABI
    `vu_resample_i16`, `vu_resample_u8_nearest`, `vu_resample_f32`; arithmetic in include/vit_unet_amd.h).  `target_spacing` =
    (sz, sy, sx) in the unit of the caller's spacings; an entry may be None: that axis keeps its length ((None, s, s) is the
    natural choice for the 2-D model).  Every spacing becomes Fraction(x).limit_denominator(10000); a `spacing` argument is
    (sz, sy, sx) of the input, or (sy, sx) for an (H,W) input.
      r.out_shape(shape, spacing)   n_out = max(1, floor(n_in s_in / s_out + 1/2)) per axis, in exact rational arithmetic
      r.image(vol_i16, spacing)     the int16 volume on the working grid (trilinear, exact integer arithmetic), on the device
      r.labels(mask_u8, spacing)    the uint8 label mask on the working grid (nearest: no label value is invented)
      r.logits_to(z_f32, shape, truth=None, zthr=0.0, label=-1)
                                    float32 logits brought to `shape` (the native grid): {"logits", "mask" uint8 = logit >= zthr}
                                    and, with a `truth` uint8 of `shape`, "counts" (D,3) int64 on the device: mask pixels, truth
                                    pixels, both, per slice (`label` as in `TiledSegmenter`)
    Inputs are (H,W) or (D,H,W), numpy or torch, host or device; a list / tuple of inputs gives a list (with one spacing / shape
    for all, or a list of them).  No CPU fallback: inputs are moved to 'cuda'.  Argument errors raise `VuError` before any launch."""

    def __init__(self, target_spacing=(None, 1.0, 1.0)):
        try:
            sp = tuple(target_spacing)
        except TypeError:
            sp = ()
        if len(sp) != 3:
            raise VuError(f"target_spacing must be (sz, sy, sx), entries a positive number or None (got {target_spacing!r})")
        self.target = tuple(None if v is None else self._fraction(v, "target_spacing") for v in sp)

    @staticmethod
    def _fraction(v, what) -> Fraction:
        if isinstance(v, bool) or not isinstance(v, (int, float, Fraction, np.integer, np.floating)) or not math.isfinite(float(v)) \
                or float(v) <= 0.0:
            raise VuError(f"{what}: a spacing must be a finite number > 0 (got {v!r})")
        f = (Fraction(int(v)) if isinstance(v, np.integer) else Fraction(float(v)) if isinstance(v, np.floating) else Fraction(v))
        f = f.limit_denominator(10000)
        if f <= 0:
            raise VuError(f"{what}: the spacing {v!r} is below 1 / 10000")
        return f

    def _spacing(self, spacing, ndim):
        try:
            sp = tuple(spacing)
        except TypeError:
            sp = ()
        if len(sp) == 2 and ndim == 2:
            sp = (1,) + sp
        if len(sp) != 3:
            raise VuError(f"spacing must be (sz, sy, sx){' or (sy, sx)' if ndim == 2 else ''} (got {spacing!r})")
        return tuple(self._fraction(v, "spacing") for v in sp)

    def out_shape(self, shape, spacing):
        shape = tuple(int(n) for n in shape)
        if len(shape) not in (2, 3) or min(shape) < 1:
            raise VuError(f"expected an (H,W) or (D,H,W) shape of positive lengths (got {shape})")
        sp = self._spacing(spacing, len(shape))
        out = []
        for n, s, t in zip(shape, sp[3 - len(shape):], self.target[3 - len(shape):]):
            out.append(n if t is None else max(1, math.floor(Fraction(n) * s / t + Fraction(1, 2))))
        if math.prod(out) > 0x7fffffff:
            raise VuError(f"the resampled shape {tuple(out)} exceeds 2^31 - 1 elements")
        return tuple(out)

    @staticmethod
    def _to_device(t):
        if not torch.cuda.is_available():
            raise VuError("VolumeResampler runs on the MI355X only (no CPU fallback)")
        return (t if t.is_cuda else t.to("cuda", non_blocking=True)).contiguous()

    @staticmethod
    def _per_item(arg, n, is_one):
        """One argument for all n inputs, or a list of n of them."""
        if is_one(arg):
            return [arg] * n
        if not isinstance(arg, (list, tuple)) or len(arg) != n:
            raise VuError(f"expected one spacing / shape or a list of {n} of them (got {arg!r})")
        return list(arg)

    @staticmethod
    def _is_one(arg):
        return not isinstance(arg, (list, tuple)) or len(arg) == 0 or not isinstance(arg[0], (list, tuple))

    def _resample(self, a, spacing, dtype, what, entry):
        if isinstance(a, (list, tuple)):
            return [self._resample(v, s, dtype, what, entry) for v, s in zip(a, self._per_item(spacing, len(a), self._is_one))]
        v = TiledSegmenter._volume(a, dtype, what)
        if v.numel() > 0x7fffffff:
            raise VuError(f"{what} {tuple(v.shape)} exceeds 2^31 - 1 elements")
        oshape = self.out_shape(tuple(v.shape), spacing)
        v = self._to_device(v)
        with torch.cuda.device(v.device):
            return entry(v.reshape((-1,) + tuple(v.shape[-2:])), (1,) * (3 - len(oshape)) + oshape).reshape(oshape)

    def image(self, vol, spacing):
        return self._resample(vol, spacing, torch.int16, "volume", self.run_i16)

    def labels(self, mask, spacing):
        return self._resample(mask, spacing, torch.uint8, "mask", self.run_u8)

    def logits_to(self, z, shape, truth=None, zthr: float = 0.0, label: int = -1):
        if isinstance(z, (list, tuple)):
            shapes = self._per_item(shape, len(z), lambda s: not isinstance(s[0], (list, tuple)))
            truths = [None] * len(z) if truth is None else self._per_item(truth, len(z), lambda t: False)
            return [self.logits_to(a, s, t, zthr, label) for a, s, t in zip(z, shapes, truths)]
        if int(label) > 255:
            raise VuError(f"label must be negative (any non-zero truth) or 0 .. 255 (got {label})")
        if not math.isfinite(float(zthr)):
            raise VuError(f"zthr must be a finite logit (got {zthr!r})")
        v = TiledSegmenter._volume(z, torch.float32, "logit volume")
        shape = tuple(int(n) for n in shape)
        if len(shape) != v.dim() or min(shape) < 1 or math.prod(shape) > 0x7fffffff or v.numel() > 0x7fffffff:
            raise VuError(f"cannot bring logits of shape {tuple(v.shape)} to {shape}: same rank, 1 .. 2^31 - 1 elements")
        t = None
        if truth is not None:
            t = TiledSegmenter._volume(truth, torch.uint8, "truth")
            if tuple(t.shape) != shape:
                raise VuError(f"the truth {tuple(t.shape)} does not have the target shape {shape}")
        v = self._to_device(v)
        if t is not None:
            t = t.to(v.device, non_blocking=True).contiguous().reshape((-1,) + shape[-2:])
        with torch.cuda.device(v.device):
            res = self.run_f32(v.reshape((-1,) + tuple(v.shape[-2:])), (1,) * (3 - len(shape)) + shape, t, float(zthr), int(label))
        return {k: (a if k == "counts" else a.reshape(shape)) for k, a in res.items()}

    # ---- one launch each on (D,H,W) device tensors
    @staticmethod
    def run_i16(vol: torch.Tensor, oshape) -> torch.Tensor:
        out = torch.empty(oshape, dtype=torch.int16, device=vol.device)
        check(lib().vu_resample_i16(ptr(vol), ptr(out), *(int(n) for n in vol.shape), *oshape, stream_ptr(vol.device)), "vu_resample_i16")
        return out

    @staticmethod
    def run_u8(mask: torch.Tensor, oshape) -> torch.Tensor:
        out = torch.empty(oshape, dtype=torch.uint8, device=mask.device)
        check(lib().vu_resample_u8_nearest(ptr(mask), ptr(out), *(int(n) for n in mask.shape), *oshape, stream_ptr(mask.device)),
              "vu_resample_u8_nearest")
        return out

    @staticmethod
    def run_f32(z: torch.Tensor, oshape, truth=None, zthr: float = 0.0, label: int = -1, logits: bool = True, mask: bool = True):
        """One vu_resample_f32: {"logits" and / or "mask" of `oshape` and, with a truth, "counts" (Do,3) int64}, on the device."""
        L, dev = lib(), z.device
        Do, Ho, Wo = (int(n) for n in oshape)
        res = {}
        if logits:
            res["logits"] = torch.empty(Do, Ho, Wo, dtype=torch.float32, device=dev)
        if mask:
            res["mask"] = torch.empty(Do, Ho, Wo, dtype=torch.uint8, device=dev)
        scratch, nbytes = None, 0
        if truth is not None:
            res["counts"] = torch.empty(Do, 3, dtype=torch.int64, device=dev)
            nbytes = int(L.vu_resample_f32_scratch_bytes(Do, Ho, Wo))
            scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        check(L.vu_resample_f32(ptr(z), ptr(truth), ptr(res.get("logits")), ptr(res.get("mask")), ptr(res.get("counts")), ptr(scratch),
                                nbytes, *(int(n) for n in z.shape), Do, Ho, Wo, float(zthr), int(label), stream_ptr(dev)),
              "vu_resample_f32")
        return res


class IntensityNormalizer:
    """`n = IntensityNormalizer(mode="percentile", lo=0.5, hi=99.5, k=3.0, select="all", floor=0, label=-1); lo, hi = n.window(vol)`.

    A per-volume intensity window for volumes without an absolute scale (MR): x = clip((v - lo) / (hi - lo), 0, 1) with lo, hi
    measured on the volume itself.  `select` names the voxels that are measured: "all"; "above": v > `floor` (strict; floor 0 is
    the MR non-air rule); "mask": the foreground of the `mask` argument under `label` (mask != 0 when label < 0, mask == label
    when 0 .. 255).  The histogram (65536 bins, exact) and every integer come from the device (csrc/vu_intensity.hip; contract
    in include/vit_unet_amd.h); the window is formed on the host from those integers alone, in `fractions.Fraction` arithmetic, so
    it is a function of the volume and of nothing else:
      mode "percentile"  the `lo` and `hi` percentiles (percent, rounded to 1e-4 percent: pn = round(p 10^4), pd = 10^6) under
                         numpy's linear definition, q = v_k + (v_k1 - v_k) r / pd exactly, rounded once to float64, then to float32
      mode "zscore"      mean = sum / N and var = (N sumsq - sum^2) / N^2 exactly; std = math.sqrt(float(var));
                         lo / hi = float32(float(mean) -+ k std): x is the z-score clipped at +-k and mapped to [0, 1]
    If hi > lo does not hold after rounding (a constant volume, N = 1), hi = lo + 1.  An empty selection raises `VuError`.
      n.hist(vol, mask=None)    the device histogram, (65536,) int64 (hist[b] counts the value b - 32768)
      n.stats(vol, mask=None)   {"n", "min", "max", "sum", "sumsq" (exact ints), "mean", "std" (host floats; None when n = 0),
                                "quantiles": [(k, r, v_k, v_k1) for lo and hi]}
      n.bbox(vol, mask=None)    (z0, z1, y0, y1, x0, x1), the inclusive extent of the selected voxels ((D, -1, H, -1, W, -1) when none;
                                an (H,W) input counts as D = 1)
      n.window(vol, mask=None)  (lo, hi): Python floats that are exactly float32 values
    vol is (H,W) or (D,H,W) int16, mask uint8 of the same shape (needed for select "mask" only); numpy or torch, host or device; a
    list / tuple of volumes gives a list.  `window` and `stats` cost three small launches (clear, count, statistics) and one
    128-byte read-back: they wait for the device once per volume - measure a volume once and keep the numbers (`run_segmentation`
    does).  No CPU fallback: inputs are moved to 'cuda'.  Argument errors raise `VuError` before any launch."""

    SELECT = {"all": 0, "above": 1, "mask": 2}
    PD = 10 ** 6

    def __init__(self, mode: str = "percentile", lo: float = 0.5, hi: float = 99.5, k: float = 3.0, select: str = "all",
                 floor: int = 0, label: int = -1):
        num = (int, float, np.integer, np.floating)
        if mode not in ("percentile", "zscore"):
            raise VuError(f"mode must be 'percentile' or 'zscore' (got {mode!r})")
        if any(isinstance(p, bool) or not isinstance(p, num) for p in (lo, hi)) or not 0.0 <= float(lo) < float(hi) <= 100.0:
            raise VuError(f"lo and hi are percentages with 0 <= lo < hi <= 100 (got {lo!r}, {hi!r})")
        if isinstance(k, bool) or not isinstance(k, num) or not math.isfinite(float(k)) or float(k) <= 0.0:
            raise VuError(f"k must be a finite number > 0 (got {k!r})")
        if select not in self.SELECT:
            raise VuError(f"select must be one of {sorted(self.SELECT)} (got {select!r})")
        if isinstance(floor, bool) or not isinstance(floor, (int, np.integer)) or not -2 ** 31 <= int(floor) < 2 ** 31:
            raise VuError(f"floor must be an integer that fits int32 (got {floor!r})")
        if isinstance(label, bool) or not isinstance(label, (int, np.integer)) or not -2 ** 31 <= int(label) <= 255:
            raise VuError(f"label must be negative (any non-zero mask value) or 0 .. 255 (got {label!r})")
        self.mode, self.lo, self.hi, self.k = mode, float(lo), float(hi), float(k)
        self.select, self.floor, self.label = select, int(floor), int(label)
        self.pn = (int(round(self.lo * 10 ** 4)), int(round(self.hi * 10 ** 4)))

    @staticmethod
    def _to_device(t):
        if not torch.cuda.is_available():
            raise VuError("IntensityNormalizer runs on the MI355X only (no CPU fallback)")
        return (t if t.is_cuda else t.to("cuda", non_blocking=True)).contiguous()

    def _inputs(self, vol, mask):
        """(vol, mask or None) as (D,H,W) device tensors."""
        v = TiledSegmenter._volume(vol, torch.int16, "volume")
        if v.numel() >= 2 ** 32:
            raise VuError(f"volume {tuple(v.shape)} has 2^32 voxels or more")
        m = None
        if self.select == "mask":
            if mask is None:
                raise VuError("select='mask' measures the foreground of a mask: pass mask=")
            m = TiledSegmenter._volume(mask, torch.uint8, "mask")
            if tuple(m.shape) != tuple(v.shape):
                raise VuError(f"the mask {tuple(m.shape)} does not have the volume's shape {tuple(v.shape)}")
        v = self._to_device(v)
        v = v.reshape((-1,) + tuple(v.shape[-2:]))
        if m is not None:
            m = m.to(v.device, non_blocking=True).contiguous().reshape(v.shape)
        return v, m

    # ---- the launches, on (D,H,W) device tensors
    def run_hist(self, vol: torch.Tensor, mask=None, bbox: bool = False):
        """vu_intensity_hist: (hist (65536,) int32 holding the uint32 bits, bbox (6,) int32 or None), on the device."""
        dev = vol.device
        hist = torch.empty(65536, dtype=torch.int32, device=dev)
        box = torch.empty(6, dtype=torch.int32, device=dev) if bbox else None
        check(lib().vu_intensity_hist(ptr(vol), ptr(mask), ptr(hist), ptr(box), *(int(n) for n in vol.shape), self.SELECT[self.select],
                                      self.floor, self.label, stream_ptr(dev)), "vu_intensity_hist")
        return hist, box

    def run_stats(self, hist: torch.Tensor) -> torch.Tensor:
        """vu_intensity_stats with the lo and hi quantiles: (16,) int64 on the device."""
        stats = torch.empty(16, dtype=torch.int64, device=hist.device)
        pn, pd = (C.c_uint * 2)(*self.pn), (C.c_uint * 2)(self.PD, self.PD)
        check(lib().vu_intensity_stats(ptr(hist), pn, pd, 2, ptr(stats), stream_ptr(hist.device)), "vu_intensity_stats")
        return stats

    def _measure(self, vol, mask):
        v, m = self._inputs(vol, mask)
        with torch.cuda.device(v.device):
            return [int(x) for x in self.run_stats(self.run_hist(v, m)[0]).cpu().tolist()]

    # ---- the public calls
    def hist(self, vol, mask=None):
        if isinstance(vol, (list, tuple)):
            return [self.hist(v, m) for v, m in zip(vol, mask if mask is not None else [None] * len(vol))]
        v, m = self._inputs(vol, mask)
        with torch.cuda.device(v.device):
            return self.run_hist(v, m)[0].to(torch.int64) & 0xffffffff

    def bbox(self, vol, mask=None):
        if isinstance(vol, (list, tuple)):
            return [self.bbox(v, m) for v, m in zip(vol, mask if mask is not None else [None] * len(vol))]
        v, m = self._inputs(vol, mask)
        with torch.cuda.device(v.device):
            return tuple(int(x) for x in self.run_hist(v, m, bbox=True)[1].cpu().tolist())

    def stats(self, vol, mask=None):
        if isinstance(vol, (list, tuple)):
            return [self.stats(v, m) for v, m in zip(vol, mask if mask is not None else [None] * len(vol))]
        return self.stats_dict(self._measure(vol, mask))

    def window(self, vol, mask=None):
        if isinstance(vol, (list, tuple)):
            return [self.window(v, m) for v, m in zip(vol, mask if mask is not None else [None] * len(vol))]
        return self.window_from(self._measure(vol, mask))

    # ---- host arithmetic on the 16 integers of `run_stats`
    @staticmethod
    def stats_dict(st) -> dict:
        n, s, s2 = int(st[0]), int(st[3]), int(st[4])
        out = {"n": n, "min": int(st[1]), "max": int(st[2]), "sum": s, "sumsq": s2, "mean": None, "std": None,
               "quantiles": [tuple(int(x) for x in st[8 + 4 * j:12 + 4 * j]) for j in range(2)]}
        if n:
            out["mean"] = float(Fraction(s, n))
            out["std"] = math.sqrt(float(Fraction(n * s2 - s * s, n * n)))
        return out

    def window_from(self, st):
        """(lo, hi) from the 16 integers (N, min, max, sum, sumsq, 0, 0, 0, then k, r, v_k, v_k1 for lo and for hi)."""
        n = int(st[0])
        if n == 0:
            raise VuError(f"the selection ({self.select!r}) is empty: no voxel to measure the intensity window on")
        if self.mode == "percentile":
            lo, hi = (float(np.float32(float(Fraction(int(st[10 + 4 * j])) +
                                             Fraction((int(st[11 + 4 * j]) - int(st[10 + 4 * j])) * int(st[9 + 4 * j]), self.PD))))
                      for j in range(2))
        else:
            d = self.stats_dict(st)
            lo, hi = float(np.float32(d["mean"] - self.k * d["std"])), float(np.float32(d["mean"] + self.k * d["std"]))
        if not hi > lo:
            hi = float(np.float32(lo + 1.0))
        return lo, hi


def window_pair(window, what: str = "the intensity window"):
    """A (lo, hi) window as two Python floats that are float32 values; hi > lo or VuError."""
    try:
        lo, hi = float(np.float32(window[0])), float(np.float32(window[1]))
    except (TypeError, IndexError, ValueError):
        raise VuError(f"{what} must be a (lo, hi) pair or an IntensityNormalizer (got {window!r})") from None
    if not hi > lo:
        raise VuError(f"{what} must have hi > lo (got {window[0]} .. {window[1]})")
    return lo, hi


class TiledSegmenter:
    """`s = TiledSegmenter(model, overlap=32, batch=64); mask = s(vol)`.

    vol (H,W) or (D,H,W) int16 (numpy or torch, host or device; a list / tuple gives a list).  Every value goes through the
    intensity window `window` = (lo, hi): x = clip((v - lo) / (hi - lo), 0, 1), as `SegmentationBatchTransform` does.
      output="mask"    uint8 of the input's shape on the device: 1 where sigmoid(logit) >= threshold, i.e. logit >= zthr
      output="logits"  the blended float32 logits
      output="prob"    torch.sigmoid of the logits
    `score(vol, truth)`: truth uint8 of the same shape -> {"mask", "counts" (D,3) int64 on the host: mask pixels, truth
    pixels, both; "dice", "iou" of the whole volume, from the summed counts}.  A truth pixel is truth != 0 when `label` < 0,
    truth == label when 0 <= label <= 255.

    Execution order (fixed): with nt windows per slice, slices run in groups of G = max(1, batch // nt); the windows
    [g0, g0 + n) of a group (numbered over the volume, g = z nt + t) run in chunks of `batch`, the last at its own size:
    vu_tile_gather_i16, then the eval forward (running BatchNorm statistics, no dropout, under `torch.no_grad()`) into the
    group's output buffer; one vu_seg_blend per group.  `ensemble` in {1, 2, 4, 8} is `TiledRestorer`'s self-ensemble (the
    same op sets and vu_dihedral_f32 loop) on the logits; `ensemble=1` launches none of those kernels.  The model's mode,
    running statistics and counters are untouched.  Argument errors raise `VuError` before any launch; a model that is not on
    'cuda' is refused at the call, as `TiledRestorer` does.

    `clean`: a `MaskCleaner`.  After the last blend one `vu_seg_clean` runs on the whole thresholded volume, in place:
    output="mask" is the cleaned mask, `score` gives counts, Dice and IoU of the cleaned mask plus "stats" (the cleaner's) and
    "raw_counts" (those of the thresholded mask); "logits" / "prob" with a cleaner are refused.  `clean=None` launches nothing
    new.

    `surface`: a `SurfaceDistance`.  `score` then runs one `vu_surface_dist` on the final mask (after `clean`, if given)
    against the truth under `label` and adds "surface": the dict of `SurfaceDistance.score`.  `surface=None` launches nothing
    new and returns exactly the dicts above.

    `resample`: a `VolumeResampler` (or the target spacing of one).  `s(vol, output, spacing=)` and `s.score(vol, truth,
    spacing=)` then take the volume's own voxel size (sz, sy, sx) and run the model at the working spacing: one
    `vu_resample_i16` brings the volume to `resample.out_shape(vol.shape, spacing)`, the order above runs there for the
    logits, and one `vu_resample_f32` brings them back to the volume's own shape, where they are thresholded and - in
    `score` - counted against the native truth; `clean` and `surface` then work on that native-grid mask as before, and
    "logits" / "prob" are native-grid values.  A list of volumes takes one spacing for all or a list of them.  A resampler
    without a spacing and a spacing without a resampler are refused; `resample=None` launches nothing new and returns today's
    results bit for bit.

    `window`: a (lo, hi) pair or an `IntensityNormalizer`.  A normalizer measures every volume of a call - as passed, on its own
    grid, before any `resample=` (three small launches and one wait for the device) - and that window serves every gather of the
    call; with select "mask" the truth of `score` is the mask (a plain call has none and is refused).  `s(vol, ..., window=(lo, hi))`
    and `s.score(vol, truth, ..., window=(lo, hi))` override it for that call and launch no statistics (a list of volumes takes
    one pair for all or a list of pairs).  With a (lo, hi) pair nothing new is launched and every result is today's."""

    def __init__(self, model, overlap: int = 32, batch: int = 64, window=(-1024.0, 1024.0), threshold: float = 0.5,
                 label: int = -1, ensemble: int = 1, clean=None, surface=None, resample=None):
        T = int(model.im_size)
        if int(model.num_channels) != 1:
            raise VuError(f"a segmentation model has 1 channel (this one has {model.num_channels})")
        if not 0 <= int(overlap) <= T // 2:
            raise VuError(f"overlap must be in 0 .. im_size // 2 = {T // 2} (got {overlap})")
        if int(batch) < 1:
            raise VuError(f"batch must be at least 1 (got {batch})")
        self.normalizer = window if isinstance(window, IntensityNormalizer) else None
        lo_hi = None if self.normalizer is not None else window_pair(window)
        if int(label) > 255:
            raise VuError(f"label must be negative (any non-zero truth) or 0 .. 255 (got {label})")
        if ensemble not in TiledRestorer.ENSEMBLE_OPS:
            raise VuError(f"ensemble must be one of {sorted(TiledRestorer.ENSEMBLE_OPS)} (got {ensemble!r})")
        if clean is not None and not isinstance(clean, MaskCleaner):
            raise VuError(f"clean must be a MaskCleaner or None (got {type(clean).__name__})")
        if surface is not None and not isinstance(surface, SurfaceDistance):
            raise VuError(f"surface must be a SurfaceDistance or None (got {type(surface).__name__})")
        if resample is not None and not isinstance(resample, VolumeResampler):
            resample = VolumeResampler(resample)
        self.clean, self.surface, self.resample = clean, surface, resample
        self.zthr = logit_threshold(threshold)
        self.model, self.T, self.overlap, self.batch = model, T, int(overlap), int(batch)
        self.window, self.threshold, self.label, self.ensemble = lo_hi, float(threshold), int(label), int(ensemble)

    def _device(self) -> torch.device:
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise VuError("TiledSegmenter runs on the MI355X only: move the model to 'cuda' (no CPU fallback)")
        return dev

    @staticmethod
    def _volume(a, dtype, what):
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        if not torch.is_tensor(t) or t.dim() not in (2, 3) or t.dtype != dtype:
            got = f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else type(a).__name__
            raise VuError(f"expected one (H,W) or (D,H,W) {dtype} {what} (or a list of them), got {got}")
        if t.numel() == 0:
            raise VuError(f"empty {what} {tuple(t.shape)}")
        return t

    def __call__(self, vol, output: str = "mask", spacing=None, window=None):
        if isinstance(vol, (list, tuple)):
            ws = [None] * len(vol) if window is None else VolumeResampler._per_item(window, len(vol), VolumeResampler._is_one)
            if spacing is None:
                return [self(v, output, window=w) for v, w in zip(vol, ws)]
            return [self(v, output, s, w) for v, s, w in zip(vol, VolumeResampler._per_item(spacing, len(vol), VolumeResampler._is_one), ws)]
        if output not in ("mask", "logits", "prob"):
            raise VuError(f"output must be 'mask', 'logits' or 'prob' (got {output!r})")
        if window is not None:
            window = window_pair(window)
        if self.clean is not None and output != "mask":
            raise VuError(f"a cleaner works on the mask: output={output!r} with clean= is refused")
        v = self._volume(vol, torch.int16, "volume")
        self._check_clean(v)
        wshape = self._working_shape(tuple(v.shape), spacing)
        dev = self._device()
        shape = tuple(v.shape)
        v = v.to(dev, non_blocking=True).contiguous().reshape((-1,) + shape[-2:])
        win = self._window_of(v, None, window)
        with torch.no_grad():
            if output == "mask":
                m = (self._run(v, None, mask=True, window=win) if wshape is None
                     else self._run_resampled(v, wshape, None, mask=True, window=win))["mask"]
                if self.clean is not None:
                    m = self.clean.run(m, None, out=m)["mask"]
                return m.reshape(shape)
            z = (self._run(v, None, logits=True, window=win) if wshape is None
                 else self._run_resampled(v, wshape, None, logits=True, window=win))["logits"]
            z = z.reshape(shape)
            return z if output == "logits" else torch.sigmoid(z)

    def _working_shape(self, shape, spacing):
        """None without a resampler; else the (D,H,W) working-grid shape of a volume of `shape` and `spacing`."""
        if self.resample is None:
            if spacing is not None:
                raise VuError("a spacing= needs a resampler: TiledSegmenter(..., resample=VolumeResampler(...))")
            return None
        if spacing is None:
            raise VuError("this segmenter resamples to a working spacing: give the volume's own spacing=(sz, sy, sx)")
        w = self.resample.out_shape(shape, spacing)
        return (1,) * (3 - len(w)) + w

    def _window_of(self, vol: torch.Tensor, truth, window):
        """The (lo, hi) of one call: the per-call pair, else the constructor's pair, else the normalizer's measurement of the
        (D,H,W) device volume as passed (its truth is the mask of select "mask")."""
        if window is not None:
            return window_pair(window)
        if self.normalizer is None:
            return self.window
        return self.normalizer.window(vol, truth)

    def _run_resampled(self, vol: torch.Tensor, wshape, truth, logits: bool = False, mask: bool = False, window=None):
        """`_run` at the working spacing: vu_resample_i16 to `wshape`, the logits there, one vu_resample_f32 back to vol's
        shape -> what `_run` returns, on the native grid."""
        with torch.cuda.device(vol.device):
            work = VolumeResampler.run_i16(vol, wshape)
            z = self._run(work, None, logits=True, window=window)["logits"]
            return VolumeResampler.run_f32(z, tuple(vol.shape), truth, self.zthr, self.label, logits=logits, mask=mask)

    def score(self, vol, truth, spacing=None, window=None):
        if window is not None:
            window = window_pair(window)
        v, t = self._volume(vol, torch.int16, "volume"), self._volume(truth, torch.uint8, "truth")
        if tuple(v.shape) != tuple(t.shape):
            raise VuError(f"the truth {tuple(t.shape)} does not have the volume's shape {tuple(v.shape)}")
        self._check_clean(v)
        if self.surface is not None:
            self.surface._check_shape(tuple(v.shape))
        wshape = self._working_shape(tuple(v.shape), spacing)
        dev = self._device()
        shape = tuple(v.shape)
        v = v.to(dev, non_blocking=True).contiguous().reshape((-1,) + shape[-2:])
        t = t.to(dev, non_blocking=True).contiguous().reshape(v.shape)
        win = self._window_of(v, t, window)
        with torch.no_grad():
            res = self._run(v, t, mask=True, window=win) if wshape is None else self._run_resampled(v, wshape, t, mask=True, window=win)
            if self.clean is not None:
                raw = res["counts"].cpu()
                out = MaskCleaner.finish(self.clean.run(res["mask"], t, self.label, out=res["mask"]), shape)
                out["raw_counts"] = raw
            else:
                counts = res["counts"].cpu()
                pred, true, both = (int(c) for c in counts.sum(0))
                out = {"mask": res["mask"].reshape(shape), "counts": counts, "dice": dice_from_counts(pred, true, both),
                       "iou": iou_from_counts(pred, true, both)}
            if self.surface is not None:
                out["surface"] = self.surface.finish(self.surface.run(res["mask"], t, self.label))
        return out

    def _check_clean(self, v):
        c = self.clean
        if c is not None and c.connectivity in (6, 26) and (v.dim() == 2 or v.shape[0] == 1):
            raise VuError(f"connectivity {c.connectivity} needs a (D,H,W) volume with D >= 2 (got {tuple(v.shape)}); a slice takes 4 or 8")

    def _run(self, vol: torch.Tensor, truth, logits: bool = False, mask: bool = False, window=None):
        L, T, ov, m = lib(), self.T, self.overlap, self.model
        D, H, W = (int(s) for s in vol.shape)
        ny, nx = C.c_int(0), C.c_int(0)
        check(L.vu_tile_plan_count(H, W, T, ov, C.byref(ny), C.byref(nx)), "vu_tile_plan_count")
        nt = ny.value * nx.value
        G = max(1, self.batch // nt)
        dev, st = vol.device, stream_ptr(vol.device)
        lo, hi = window if window is not None else self._window_of(vol, truth, None)
        m._ensure_flat()
        outs = torch.empty(min(G, D) * nt, 1, T, T, dtype=torch.float32, device=dev)
        x = torch.empty(min(self.batch, outs.shape[0]), 1, T, T, dtype=torch.float32, device=dev)
        ops = TiledRestorer.ENSEMBLE_OPS[self.ensemble]
        if len(ops) > 1:
            xt, tmp = torch.empty_like(x), torch.empty_like(x)
        res = {}
        if logits:
            res["logits"] = torch.empty(D, H, W, dtype=torch.float32, device=dev)
        if mask:
            res["mask"] = torch.empty(D, H, W, dtype=torch.uint8, device=dev)
        scratch, nbytes = None, 0
        if truth is not None:
            res["counts"] = torch.empty(D, 3, dtype=torch.int64, device=dev)
            nbytes = int(L.vu_seg_blend_scratch_bytes(min(G, D), H, W))
            scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        for z0 in range(0, D, G):
            nz = min(G, D - z0)
            g0, nw = z0 * nt, nz * nt
            for c0 in range(0, nw, self.batch):
                n = min(self.batch, nw - c0)
                check(L.vu_tile_gather_i16(ptr(vol), ptr(x), D, H, W, T, ov, g0 + c0, n, lo, hi, st), "vu_tile_gather_i16")
                if len(ops) == 1:
                    m._run_forward(x[:n], False, 0, out=outs[c0:c0 + n])
                    continue
                for k, op in enumerate(ops):
                    check(L.vu_dihedral_f32(ptr(x), ptr(xt), n, 1, T, op, 0, 1.0, st), "vu_dihedral_f32")
                    m._run_forward(xt[:n], False, 0, out=tmp[:n])
                    check(L.vu_dihedral_f32(ptr(tmp), ptr(outs[c0:c0 + n]), n, 1, T, L.vu_dihedral_inverse(op), int(k > 0),
                                            1.0 / len(ops) if k == len(ops) - 1 else 1.0, st), "vu_dihedral_f32")
            sl = slice(z0, z0 + nz)
            check(L.vu_seg_blend(ptr(outs), ptr(truth[sl]) if truth is not None else None,
                                 ptr(res["logits"][sl]) if logits else None, ptr(res["mask"][sl]) if mask else None,
                                 ptr(res["counts"][sl]) if truth is not None else None, ptr(scratch), nbytes, nz, H, W, T, ov,
                                 self.zthr, self.label, st), "vu_seg_blend")
        return res
