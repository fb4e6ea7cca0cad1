"""Metrics / losses next to the model (reference: vit_unet/torch/functions.py:7-19, README.md:85-101).

`psnr(model, dataloader)` keeps the reference signature but computes the metric on the device with
the HIP kernels of csrc/vu_metrics.hip (10*log10(R^2/MSE) per image, data_range 1.0 = what
scikit-image infers for float targets in [0,1]) and transfers one vector per batch instead of the
whole output tensor.  `ssim_batch` / `dice_loss` are the two other measures the README names;
`dice_loss` is differentiable (its backward is the HIP gradient kernel).  No CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from ._lib import check, lib, ptr, stream_ptr


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


def psnr_batch(target: torch.Tensor, out: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """Per-image PSNR of two (B, ...) GPU tensors -> (B,) float32 on the device."""
    assert target.shape == out.shape, f"shape mismatch {tuple(target.shape)} vs {tuple(out.shape)}"
    t, o = _f32(target), _f32(out)
    B = t.shape[0]
    P = t.numel() // max(B, 1)
    L = lib()
    res = torch.empty(B, dtype=torch.float32, device=t.device)
    part = torch.empty(max(1, L.vu_psnr_partials_floats(B)), dtype=torch.float32, device=t.device)
    check(L.vu_psnr(ptr(t), ptr(o), ptr(res), ptr(part), B, P, float(data_range), stream_ptr(t.device)), "vu_psnr")
    return res


def ssim_batch(target: torch.Tensor, out: torch.Tensor, data_range: float = 1.0, win_size: int = 7) -> torch.Tensor:
    """Per-image mean SSIM (channels averaged) of two (B,C,H,W) GPU tensors -> (B,) float32."""
    assert target.shape == out.shape and target.dim() == 4, "ssim_batch takes two (B,C,H,W) tensors"
    t, o = _f32(target), _f32(out)
    B, Cn, H, W = t.shape
    L = lib()
    res = torch.empty(B, dtype=torch.float32, device=t.device)
    part = torch.empty(max(1, L.vu_ssim_partials_floats(B, Cn, H, W, win_size)), dtype=torch.float32, device=t.device)
    check(L.vu_ssim(ptr(t), ptr(o), ptr(res), ptr(part), B, Cn, H, W, int(win_size), float(data_range),
                    stream_ptr(t.device)), "vu_ssim")
    return res


def psnr(model, dataloader, device="cuda"):
    score = []
    with torch.no_grad():
        for batch in dataloader:
            x = batch["x"].to(device).float()
            y = batch["y"].to(device).float()
            score.append(psnr_batch(y, model(x)).cpu().numpy())
    return np.concatenate(score) if score else np.zeros(0)


def ssim(model, dataloader, device="cuda"):
    """Same calling convention as `psnr` (the README lists SSIM beside PSNR)."""
    score = []
    with torch.no_grad():
        for batch in dataloader:
            x = batch["x"].to(device).float()
            y = batch["y"].to(device).float()
            score.append(ssim_batch(y, model(x)).cpu().numpy())
    return np.concatenate(score) if score else np.zeros(0)


def _tiled_scores(model, pairs, overlap, batch, score, ensemble=1):
    """Full-resolution metric over (noisy_u8, clean_u8) pairs of (H,W,C) images: the restorer's float image against clean / 255
    (what `DenoisingBatchTransform` gives the model as target), one (1,C,H,W) call of `score` per pair."""
    from .restore import TiledRestorer
    r = TiledRestorer(model, overlap=overlap, batch=batch, ensemble=ensemble)
    res = []
    for noisy, clean in pairs:
        out = r(noisy, output="f32")
        c = torch.from_numpy(np.ascontiguousarray(clean)) if isinstance(clean, np.ndarray) else clean
        assert c.dtype == torch.uint8 and c.dim() == 3, "expected (H,W,C) uint8 clean images"
        y = (c.to(out.device).permute(2, 0, 1).double() / 255.0).float().contiguous()
        res.append(score(y[None], out[None]).cpu().numpy())
    return np.concatenate(res) if res else np.zeros(0)


def psnr_tiled(model, pairs, overlap: int = 32, batch: int = 64, ensemble: int = 1):
    """`psnr` at full resolution: every pair of (H,W,C) uint8 images goes through sliding-window inference
    (restore.TiledRestorer, with its self-ensemble when `ensemble` > 1) instead of a resize to im_size.  Returns one
    value per pair."""
    return _tiled_scores(model, pairs, overlap, batch, psnr_batch, ensemble)


def ssim_tiled(model, pairs, overlap: int = 32, batch: int = 64, ensemble: int = 1):
    """`ssim` at full resolution (see `psnr_tiled`)."""
    return _tiled_scores(model, pairs, overlap, batch, ssim_batch, ensemble)


def _scored(s, pairs):
    """`s.score` over (volume, truth) pairs; with a resampler every item is (volume, truth, spacing): the volume's own voxel size
    rides along as the item's third entry."""
    for vol, truth, *sp in pairs:
        if len(sp) > 1:
            raise ValueError(f"expected (volume, truth) or (volume, truth, spacing) items, got {2 + len(sp)} entries")
        yield s.score(vol, truth, spacing=sp[0]) if sp else s.score(vol, truth)


def _tiled_overlap(model, pairs, key, **kw):
    from .segment import TiledSegmenter
    s = TiledSegmenter(model, **kw)
    return np.array([r[key] for r in _scored(s, pairs)], dtype=np.float64)


def dice_tiled(model, pairs, overlap: int = 32, batch: int = 64, window=(-1024.0, 1024.0), threshold: float = 0.5,
               label: int = -1, ensemble: int = 1, clean=None, resample=None):
    """Hard Dice at full resolution over (volume_i16, truth_u8) pairs of (H,W) slices or (D,H,W) volumes: every volume goes
    through sliding-window inference (segment.TiledSegmenter) instead of a resize to im_size; the mask is sigmoid(logit) >=
    `threshold`, a truth pixel is truth != 0 (`label` < 0) or truth == label.  Returns one value per pair, from the
    integer counts of the whole volume (1.0 when mask and truth are both empty).  `clean`: a segment.MaskCleaner applied to
    the thresholded mask before it is counted.  `resample`: a segment.VolumeResampler (or its target spacing); the items are
    then (volume, truth, spacing) triples, the model runs at the working spacing and the mask is counted on the volume's own
    grid (see `TiledSegmenter`).  None launches nothing new.  `window`: a (lo, hi) pair for all volumes, or a
    segment.IntensityNormalizer, which measures every volume before its inference pass (with select "mask" the truth is the
    mask); the same holds for `iou_tiled`, `hd95_tiled`, `assd_tiled` and `nsd_tiled`."""
    return _tiled_overlap(model, pairs, "dice", overlap=overlap, batch=batch, window=window, threshold=threshold, label=label,
                          ensemble=ensemble, clean=clean, resample=resample)


def iou_tiled(model, pairs, overlap: int = 32, batch: int = 64, window=(-1024.0, 1024.0), threshold: float = 0.5,
              label: int = -1, ensemble: int = 1, clean=None, resample=None):
    """Intersection over union at full resolution (see `dice_tiled`)."""
    return _tiled_overlap(model, pairs, "iou", overlap=overlap, batch=batch, window=window, threshold=threshold, label=label,
                          ensemble=ensemble, clean=clean, resample=resample)


def _tiled_surface(model, pairs, key, surface, **kw):
    from ._lib import VuError
    from .segment import SurfaceDistance, TiledSegmenter
    if not isinstance(surface, SurfaceDistance):
        raise VuError(f"surface must be a segment.SurfaceDistance (got {type(surface).__name__})")
    s = TiledSegmenter(model, surface=surface, **kw)
    return np.array([r["surface"][key] for r in _scored(s, pairs)], dtype=np.float64)


def hd95_tiled(model, pairs, overlap: int = 32, batch: int = 64, window=(-1024.0, 1024.0), threshold: float = 0.5,
               label: int = -1, ensemble: int = 1, surface=None, clean=None, resample=None):
    """Percentile Hausdorff distance (the percentile of `surface`, 95 by default) at full resolution over (volume_i16,
    truth_u8) pairs, beside `dice_tiled`: the mask of sliding-window inference, after `clean` if given, against the truth
    under `label`, measured by `surface` (a segment.SurfaceDistance: units, spacing, tolerance, percentile; required).
    One value per pair, in the spacing's unit: the pooled-set definition ("hd95" of segment.surface_metrics).  `resample`: as
    in `dice_tiled` (items are (volume, truth, spacing) triples; the boundary is measured on the volume's own grid)."""
    return _tiled_surface(model, pairs, "hd95", surface, overlap=overlap, batch=batch, window=window, threshold=threshold,
                          label=label, ensemble=ensemble, clean=clean, resample=resample)


def assd_tiled(model, pairs, overlap: int = 32, batch: int = 64, window=(-1024.0, 1024.0), threshold: float = 0.5,
               label: int = -1, ensemble: int = 1, surface=None, clean=None, resample=None):
    """Average symmetric surface distance at full resolution (see `hd95_tiled`)."""
    return _tiled_surface(model, pairs, "assd", surface, overlap=overlap, batch=batch, window=window, threshold=threshold,
                          label=label, ensemble=ensemble, clean=clean, resample=resample)


def nsd_tiled(model, pairs, overlap: int = 32, batch: int = 64, window=(-1024.0, 1024.0), threshold: float = 0.5,
              label: int = -1, ensemble: int = 1, surface=None, clean=None, resample=None):
    """Surface Dice at the tolerance of `surface`, at full resolution (see `hd95_tiled`)."""
    return _tiled_surface(model, pairs, "nsd", surface, overlap=overlap, batch=batch, window=window, threshold=threshold,
                          label=label, ensemble=ensemble, clean=clean, resample=resample)


class _Dice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, target, apply_sigmoid):
        x, t = inp.detach().float().contiguous(), _f32(target)
        L = lib()
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        part = torch.empty(L.vu_dice_partials_floats(), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        check(L.vu_dice_loss(ptr(x), ptr(t), ptr(dx), ptr(loss), ptr(part), x.numel(), int(apply_sigmoid), 1.0,
                             stream_ptr(x.device)), "vu_dice_loss")
        ctx.save_for_backward(dx)
        ctx.in_dtype, ctx.in_shape = inp.dtype, inp.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return (dx * g).reshape(ctx.in_shape).to(ctx.in_dtype), None, None


def dice_loss(input: torch.Tensor, target: torch.Tensor, apply_sigmoid: bool = False):
    """README.md:91-101 (smooth = 1, flattened).  `apply_sigmoid=True` is the segmentation head of
    BASELINE config 5: `input` are the model's logits."""
    assert input.numel() == target.numel(), "dice_loss: input and target sizes differ"
    return _Dice.apply(input, target, apply_sigmoid)


class DiceLoss(torch.nn.Module):
    """Criterion object for `ImageFitter(model, loss=DiceLoss())`: Dice on sigmoid(model output) (the
    segmentation configuration, BASELINE config 5).  With `apply_sigmoid=True` the fitter runs the
    fused HIP step (`TrainStep(loss="dice")`)."""

    def __init__(self, apply_sigmoid: bool = True):
        super().__init__()
        self.apply_sigmoid = bool(apply_sigmoid)

    def forward(self, input, target):
        return dice_loss(input, target, apply_sigmoid=self.apply_sigmoid)
