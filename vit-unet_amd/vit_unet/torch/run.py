"""K-fold denoising run: the counterpart of `run_denoising.py:16-122` without W&B, fire and file
decoding (those stay with the caller) - per fold: build the preset model, `AdamW`, `ImageFitter`,
`fit(train, val, n_epochs, callbacks)`, reload `best-checkpoint.bin`, per-image PSNR of the test
split.  The loaders feed decoded uint8 HWC images through the device-side input pipeline
(`dataset.DenoisingBatchTransform`: train transform on the training split, validation transform on
the test split, run_denoising.py:52-59).  `patch_train=True` is the native-resolution recipe instead:
random crops under flips / rotations for training (`dataset.DenoisingPatchTransform`), a centred crop
for the validation loss, and the per-fold score from whole test images through sliding-window inference
(`functions.psnr_tiled`, with its self-ensemble when `ensemble` > 1).

`run_segmentation` is the same loop for the 1-channel segmentation configuration, at native resolution throughout:
K-fold over int16 volumes, training patches with foreground sampling (`dataset.SegmentationPatchTransform`), the fused
Dice step (`ImageFitter(model, loss=DiceLoss())`), the validation loss on centred crops and the per-fold score from whole
test volumes (`functions.dice_tiled`)."""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import functions as fn
from . import model as models
from .dataset import DenoisingBatchTransform, DenoisingPatchTransform, ImageFitter, SegmentationPatchTransform


def kfold_indices(n: int, folds: int, seed: Optional[int] = None):
    """sklearn.model_selection.KFold(folds, shuffle=True).split: the first n % folds folds get one
    extra sample; yields (train_idx, test_idx) with sorted indices."""
    assert 2 <= folds <= n, f"cannot split {n} samples into {folds} folds"
    perm = np.random.RandomState(seed).permutation(n)
    sizes = np.full(folds, n // folds)
    sizes[: n % folds] += 1
    stop = np.cumsum(sizes)
    for f in range(folds):
        test = np.sort(perm[stop[f] - sizes[f]: stop[f]])
        mask = np.ones(n, bool)
        mask[test] = False
        yield np.nonzero(mask)[0], test


class BatchLoader:
    """Minimal stand-in for the reference's DataLoader over DenoisingDataset: batches of decoded uint8
    images -> {'x','y'} device tensors via the device pipeline.  Re-iterable (one pass per epoch)."""

    def __init__(self, noisy: np.ndarray, clean: np.ndarray, idx: Sequence[int], batch_size: int, transform,
                 shuffle: bool, seed: int = 0):
        self.noisy, self.clean, self.idx, self.bs, self.tf, self.shuffle = noisy, clean, np.asarray(idx), batch_size, transform, shuffle
        self.rs = np.random.RandomState(seed)

    def __len__(self):
        return (len(self.idx) + self.bs - 1) // self.bs

    def __iter__(self):
        order = self.rs.permutation(self.idx) if self.shuffle else self.idx
        for i in range(0, len(order), self.bs):
            sel = order[i:i + self.bs]
            yield self.tf(self.noisy[sel], self.clean[sel])


def run_denoising(noisy: np.ndarray, clean: np.ndarray, n_epochs: int = 5, folds: int = 5, model_string: str = "lite",
                  lr: float = 1e-4, batch_size: int = 8, im_size: int = 224, folder: str = "models", seed: int = 0,
                  dtype=torch.bfloat16, callbacks: Optional[List[Callable[[int, Dict], None]]] = None,
                  verbose: bool = False, patch_train: bool = False, crops_per_image: int = 8, ensemble: int = 1) -> Dict:
    """noisy / clean: (n,H,W,3) uint8 decoded images (what `cv2.imread` returns for the SIDD pairs).
    Returns {'psnr': [per-fold arrays], 'psnr_mean', 'psnr_std', 'history'} (run_denoising.py:113-119).
    `patch_train`: train on `crops_per_image` random im_size patches per image at native resolution (`batch_size` then
    counts patches: batch_size // crops_per_image images per step) and score whole images with `psnr_tiled(ensemble=)`."""
    assert len(clean) == len(noisy), f"Clean length {len(clean)} is not equal to Noisy length {len(noisy)}"
    if patch_train:
        assert crops_per_image >= 1 and batch_size % crops_per_image == 0, \
            f"batch_size {batch_size} (patches) must be a multiple of crops_per_image {crops_per_image}"
    results, histories = [], []
    for fold, (train_idx, test_idx) in enumerate(kfold_indices(len(noisy), folds, seed)):
        if verbose:
            print(f"FOLD {fold}: Training on {len(train_idx)} samples and testing on {len(test_idx)} samples")
        if patch_train:
            train = BatchLoader(noisy, clean, train_idx, batch_size // crops_per_image,
                                DenoisingPatchTransform(im_size, crops_per_image, train=True, seed=seed + fold), shuffle=True,
                                seed=seed + fold)
            test = BatchLoader(noisy, clean, test_idx, batch_size, DenoisingPatchTransform(im_size, train=False), shuffle=False)
        else:
            train = BatchLoader(noisy, clean, train_idx, batch_size, DenoisingBatchTransform(im_size, train=True, seed=seed + fold),
                                shuffle=True, seed=seed + fold)
            test = BatchLoader(noisy, clean, test_idx, batch_size, DenoisingBatchTransform(im_size, train=False), shuffle=False)
        model = models.get_vit_unet(model_string, dtype=dtype)
        model.to("cuda")
        criterion = torch.nn.MSELoss()
        optimizer = torch.optim.AdamW(model.parameters(), lr=lr)
        fitter = ImageFitter(model, loss=criterion, optimizer=optimizer, device="cuda", folder=folder, seed=seed + fold)
        cbs = [(lambda log, f=fold, cb=cb: cb(f, log)) for cb in (callbacks or [])]
        histories.append(fitter.fit(train, test, n_epochs=n_epochs, callbacks=cbs, verbose=verbose))
        fitter.load(os.path.join(folder, "best-checkpoint.bin"))
        model = fitter.model
        model.eval()
        if patch_train:
            score = fn.psnr_tiled(model, ((noisy[i], clean[i]) for i in test_idx), overlap=min(32, im_size // 2), ensemble=ensemble)
        else:
            score = fn.psnr(model, test)
        if verbose:
            print(f"FOLD {fold}: Mean PSNR {np.mean(score)}")
        results.append(score)
    # run_denoising.py:109-112: np.mean(results) / np.std(results) over the list of per-fold score arrays, i.e. over ALL
    # per-image scores of all folds (not the spread of the fold means)
    allv = np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1) for r in results])
    return {"psnr": results, "psnr_mean": float(allv.mean()), "psnr_std": float(allv.std()), "history": histories}


class VolumeLoader:
    """`BatchLoader` for volumes whose sizes may differ: lists of (D,H,W) int16 volumes and uint8 label masks -> {'x','y'}
    patch batches via a `SegmentationPatchTransform`, `per_step` volumes a batch.  Re-iterable (one pass per epoch)."""

    def __init__(self, volumes, truths, idx: Sequence[int], per_step: int, transform, shuffle: bool, seed: int = 0, windows=None):
        self.volumes, self.truths, self.idx, self.bs, self.tf, self.shuffle = volumes, truths, np.asarray(idx), per_step, transform, shuffle
        self.rs = np.random.RandomState(seed)
        self.windows = windows      # one (lo, hi) per volume, measured beforehand: the transform then measures nothing

    def __len__(self):
        return (len(self.idx) + self.bs - 1) // self.bs

    def __iter__(self):
        order = self.rs.permutation(self.idx) if self.shuffle else self.idx
        for i in range(0, len(order), self.bs):
            sel = order[i:i + self.bs]
            if self.windows is None:
                yield self.tf([self.volumes[k] for k in sel], [self.truths[k] for k in sel])
            else:
                yield self.tf([self.volumes[k] for k in sel], [self.truths[k] for k in sel], windows=[self.windows[k] for k in sel])


def run_segmentation(volumes, truths, n_epochs: int = 5, folds: int = 5, model_string: str = "lite", lr: float = 1e-4,
                     batch_size: int = 8, im_size: int = 224, folder: str = "models", seed: int = 0, dtype=torch.bfloat16,
                     callbacks: Optional[List[Callable[[int, Dict], None]]] = None, verbose: bool = False,
                     crops_per_volume: int = 8, fg: float = 0.5, window=(-1024.0, 1024.0), label: int = -1, ls: float = 0.0,
                     ensemble: int = 1, model_kwargs: Optional[Dict] = None, clean=None, surface=None, spacings=None,
                     resample=None) -> Dict:
    """volumes / truths: sequences of (D,H,W) (or (H,W)) int16 volumes and uint8 label masks of the same shapes; sizes may
    differ from volume to volume, every slice at least im_size x im_size.  K-fold over the volumes; per fold a 1-channel
    preset model (`model_kwargs` overrides preset fields, e.g. patch_size) trains on `crops_per_volume` im_size patches per
    volume, a share `fg` of them around foreground (`batch_size` counts patches: batch_size // crops_per_volume volumes per
    step), validates on one centred crop per test volume and is scored by the hard Dice of its whole test volumes
    (`functions.dice_tiled(window=, label=, ensemble=, clean=)`; `clean` is a segment.MaskCleaner or None).
    Returns {'dice': [per-fold arrays], 'dice_mean', 'dice_std', 'history'}, mean / std over all per-volume scores.
    `surface`: a segment.SurfaceDistance; the same inference pass then also measures every test volume's boundary and the
    result gains 'hd95', 'assd', 'nsd' (per-fold arrays) and their '_mean' / '_std'.  None (default) launches nothing new.
    `spacings` (one (sz, sy, sx) voxel size per volume) and `resample` (a segment.VolumeResampler or its target spacing), given
    together: every volume and its truth are resampled once on the device to the working spacing (trilinear / nearest) and the
    training and validation patches are cut from those (every resampled slice at least im_size x im_size); the test volumes are
    scored on their own grids by `TiledSegmenter(resample=)`.  Without them nothing changes.
    `window`: a (lo, hi) pair or a segment.IntensityNormalizer.  A normalizer measures every volume ONCE, before the folds, as
    passed (on its own grid; with select "mask" its truth is the mask); the stored windows then serve the training patches, the
    validation crops and the scoring of that volume, so the epoch loop launches no statistics and never waits on their account.
    The result gains 'windows', the list of (lo, hi)."""
    assert len(volumes) == len(truths), f"{len(volumes)} volumes and {len(truths)} truths"
    assert (spacings is None) == (resample is None), "spacings= and resample= go together"
    work_volumes, work_truths = volumes, truths
    if resample is not None:
        from .segment import VolumeResampler
        assert len(spacings) == len(volumes), f"{len(volumes)} volumes and {len(spacings)} spacings"
        if not isinstance(resample, VolumeResampler):
            resample = VolumeResampler(resample)
        work_volumes = resample.image(list(volumes), [tuple(s) for s in spacings])
        work_truths = resample.labels(list(truths), [tuple(s) for s in spacings])
    assert crops_per_volume >= 1 and batch_size % crops_per_volume == 0, \
        f"batch_size {batch_size} (patches) must be a multiple of crops_per_volume {crops_per_volume}"
    from .segment import IntensityNormalizer
    windows = window.window(list(volumes), list(truths)) if isinstance(window, IntensityNormalizer) else None
    results, histories = [], []
    surf = {"hd95": [], "assd": [], "nsd": []}
    for fold, (train_idx, test_idx) in enumerate(kfold_indices(len(volumes), folds, seed)):
        if verbose:
            print(f"FOLD {fold}: Training on {len(train_idx)} volumes and testing on {len(test_idx)} volumes")
        train = VolumeLoader(work_volumes, work_truths, train_idx, batch_size // crops_per_volume,
                             SegmentationPatchTransform(im_size, crops_per_volume, train=True, window=window, ls=ls, fg=fg, label=label,
                                                        seed=seed + fold), shuffle=True, seed=seed + fold, windows=windows)
        test = VolumeLoader(work_volumes, work_truths, test_idx, batch_size,
                            SegmentationPatchTransform(im_size, train=False, window=window, ls=ls, label=label), shuffle=False,
                            windows=windows)
        model = models.get_vit_unet(model_string, dtype=dtype, **{**(model_kwargs or {}), "num_channels": 1, "im_size": im_size})
        model.to("cuda")
        optimizer = torch.optim.AdamW(model.parameters(), lr=lr)
        fitter = ImageFitter(model, loss=fn.DiceLoss(), optimizer=optimizer, device="cuda", folder=folder, seed=seed + fold)
        cbs = [(lambda log, f=fold, cb=cb: cb(f, log)) for cb in (callbacks or [])]
        histories.append(fitter.fit(train, test, n_epochs=n_epochs, callbacks=cbs, verbose=verbose))
        fitter.load(os.path.join(folder, "best-checkpoint.bin"))
        model = fitter.model
        model.eval()
        if surface is None and resample is None and windows is None:
            score = fn.dice_tiled(model, ((volumes[i], truths[i]) for i in test_idx), overlap=min(32, im_size // 2), window=window,
                                  label=label, ensemble=ensemble, clean=clean)
        elif surface is None and windows is None:
            score = fn.dice_tiled(model, ((volumes[i], truths[i], tuple(spacings[i])) for i in test_idx), overlap=min(32, im_size // 2),
                                  window=window, label=label, ensemble=ensemble, clean=clean, resample=resample)
        else:   # one inference pass per volume for Dice and the boundary metrics, under the volume's stored window if measured
            from .segment import TiledSegmenter
            seg = TiledSegmenter(model, overlap=min(32, im_size // 2), window=window, label=label, ensemble=ensemble, clean=clean,
                                 surface=surface, resample=resample)
            scored = [seg.score(volumes[i], truths[i], **({} if resample is None else {"spacing": tuple(spacings[i])}),
                                **({} if windows is None else {"window": windows[i]})) for i in test_idx]
            score = np.array([r["dice"] for r in scored], dtype=np.float64)
            if surface is not None:
                for k in surf:
                    surf[k].append(np.array([r["surface"][k] for r in scored], dtype=np.float64))
        if verbose:
            print(f"FOLD {fold}: Mean Dice {np.mean(score)}")
        results.append(score)
    allv = np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1) for r in results])
    out = {"dice": results, "dice_mean": float(allv.mean()), "dice_std": float(allv.std()), "history": histories}
    if windows is not None:
        out["windows"] = windows
    if surface is not None:
        for k, v in surf.items():
            a = np.concatenate(v)
            with np.errstate(invalid="ignore"):   # an empty mask or truth gives inf: the mean is inf, the spread undefined
                out.update({k: v, k + "_mean": float(a.mean()), k + "_std": float(a.std())})
    return out
