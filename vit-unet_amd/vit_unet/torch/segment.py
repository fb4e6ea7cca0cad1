"""Whole-slice and volume segmentation: sliding-window inference for the 1-channel segmentation configuration.

The segmentation twin of `restore.TiledRestorer`.  `HViT_UNet.forward` resizes anything that is not `im_size` x
`im_size`, which is the wrong operation for a label mask; `TiledSegmenter` takes a trained segmentation model and an int16
slice (H,W) or volume (D,H,W), covers every slice with the window plan of `restore.tile_plan`, runs the model's eval
forward on batches of windows and blends the window logits back, ending in a uint8 label mask and - against a truth
volume - the integer overlap counts that Dice and IoU are made of.  Cutting (with the intensity window of
`SegmentationBatchTransform`), blending, thresholding and counting are the HIP kernels of csrc/vu_segtile.hip (C ABI
`vu_tile_gather_i16`, `vu_seg_blend`; documented in include/vit_unet_amd.h); the model call in the middle is the
unchanged `vu_model_forward` path.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math

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
    'cuda' is refused at the call, as `TiledRestorer` does."""

    def __init__(self, model, overlap: int = 32, batch: int = 64, window=(-1024.0, 1024.0), threshold: float = 0.5,
                 label: int = -1, ensemble: int = 1):
        T = int(model.im_size)
        if int(model.num_channels) != 1:
            raise VuError(f"a segmentation model has 1 channel (this one has {model.num_channels})")
        if not 0 <= int(overlap) <= T // 2:
            raise VuError(f"overlap must be in 0 .. im_size // 2 = {T // 2} (got {overlap})")
        if int(batch) < 1:
            raise VuError(f"batch must be at least 1 (got {batch})")
        lo, hi = float(np.float32(window[0])), float(np.float32(window[1]))
        if not hi > lo:
            raise VuError(f"the intensity window must have hi > lo (got {window[0]} .. {window[1]})")
        if int(label) > 255:
            raise VuError(f"label must be negative (any non-zero truth) or 0 .. 255 (got {label})")
        if ensemble not in TiledRestorer.ENSEMBLE_OPS:
            raise VuError(f"ensemble must be one of {sorted(TiledRestorer.ENSEMBLE_OPS)} (got {ensemble!r})")
        self.zthr = logit_threshold(threshold)
        self.model, self.T, self.overlap, self.batch = model, T, int(overlap), int(batch)
        self.window, self.threshold, self.label, self.ensemble = (lo, hi), float(threshold), int(label), int(ensemble)

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

    def __call__(self, vol, output: str = "mask"):
        if isinstance(vol, (list, tuple)):
            return [self(v, output) for v in vol]
        if output not in ("mask", "logits", "prob"):
            raise VuError(f"output must be 'mask', 'logits' or 'prob' (got {output!r})")
        v = self._volume(vol, torch.int16, "volume")
        dev = self._device()
        shape = tuple(v.shape)
        v = v.to(dev, non_blocking=True).contiguous().reshape((-1,) + shape[-2:])
        with torch.no_grad():
            if output == "mask":
                return self._run(v, None, mask=True)["mask"].reshape(shape)
            z = self._run(v, None, logits=True)["logits"].reshape(shape)
            return z if output == "logits" else torch.sigmoid(z)

    def score(self, vol, truth):
        v, t = self._volume(vol, torch.int16, "volume"), self._volume(truth, torch.uint8, "truth")
        if tuple(v.shape) != tuple(t.shape):
            raise VuError(f"the truth {tuple(t.shape)} does not have the volume's shape {tuple(v.shape)}")
        dev = self._device()
        shape = tuple(v.shape)
        v = v.to(dev, non_blocking=True).contiguous().reshape((-1,) + shape[-2:])
        t = t.to(dev, non_blocking=True).contiguous().reshape(v.shape)
        with torch.no_grad():
            res = self._run(v, t, mask=True)
        counts = res["counts"].cpu()
        pred, true, both = (int(c) for c in counts.sum(0))
        return {"mask": res["mask"].reshape(shape), "counts": counts, "dice": dice_from_counts(pred, true, both),
                "iou": iou_from_counts(pred, true, both)}

    def _run(self, vol: torch.Tensor, truth, logits: bool = False, mask: bool = False):
        L, T, ov, m = lib(), self.T, self.overlap, self.model
        D, H, W = (int(s) for s in vol.shape)
        ny, nx = C.c_int(0), C.c_int(0)
        check(L.vu_tile_plan_count(H, W, T, ov, C.byref(ny), C.byref(nx)), "vu_tile_plan_count")
        nt = ny.value * nx.value
        G = max(1, self.batch // nt)
        dev, st = vol.device, stream_ptr(vol.device)
        lo, hi = self.window
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
