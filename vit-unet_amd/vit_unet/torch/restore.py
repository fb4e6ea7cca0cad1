"""Whole-image restoration: sliding-window inference at the model's own resolution.

`HViT_UNet.forward` takes `im_size` x `im_size` images and resizes anything else (the reference's
Resize, model.py:376), so a photograph could only be denoised as a thumbnail.  `TiledRestorer`
covers an H x W image with T x T windows (T = `model.im_size`) that overlap by `overlap` pixels,
runs the model's eval forward on batches of windows and blends the window outputs back into an
H x W image with a separable ramp weight, normalised per pixel.  Cutting and blending are the HIP
kernels of csrc/vu_tile.hip (C ABI `vu_tile_gather_u8` / `_f32`, `vu_tile_blend`; the plan and the
weights are documented in include/vit_unet_amd.h); the model call in the middle is the unchanged
`vu_model_forward` path.  `ensemble=K` is the self-ensemble: every window is restored under K of the
eight flips / rotations of the square and the K results, turned back, are averaged before the blend
(csrc/vu_patch.hip, C ABI `vu_dihedral_f32`).  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Tuple

import numpy as np
import torch

from ._lib import VuError, check, lib, ptr, stream_ptr


def tile_plan(H: int, W: int, T: int, overlap: int) -> Tuple[List[int], List[int]]:
    """(origins_y, origins_x) of the window plan of an H x W image (the C plan: vu_tile_plan_count / _axis; host code, no
    GPU).  Window t = ty * len(origins_x) + tx starts at (origins_y[ty], origins_x[tx])."""
    L = lib()
    ny, nx = C.c_int(0), C.c_int(0)
    check(L.vu_tile_plan_count(int(H), int(W), int(T), int(overlap), C.byref(ny), C.byref(nx)), "vu_tile_plan_count")
    out = []
    for length, n in ((H, ny.value), (W, nx.value)):
        arr = (C.c_int * n)()
        got = check(L.vu_tile_plan_axis(int(length), int(T), int(overlap), arr, n), "vu_tile_plan_axis")
        assert got == n, (got, n)
        out.append(list(arr))
    return out[0], out[1]


class TiledRestorer:
    """`r = TiledRestorer(model, overlap=32, batch=64); out = r(img)`.

    img (H,W,C) uint8 (numpy or torch, host or device), as decoded: normalised like the validation transform
        (`DenoisingBatchTransform(train=False)`: Normalize(mean, std), /255) -> (H,W,C) uint8 on the device,
        clamp(floor(255 out + 0.5)); `output="f32"` gives the (C,H,W) float32 image before quantisation instead.
    img (C,H,W) float32 device tensor: windows are cut unchanged (the caller normalises) -> (C,H,W) float32.
    A list / tuple of images is processed one after the other and gives a list.

    The eval forward (running BatchNorm statistics, no dropout) runs under `torch.no_grad()` whatever mode the model is
    in; neither the mode nor the running statistics are touched.  Windows run in chunks of `batch`, the last chunk at
    its own size; all window outputs of one image are kept (nt C T^2 floats) and blended in one launch.

    `ensemble` in {1, 2, 4, 8}: the dihedral ops (0,), (0, 4), (0, 1, 2, 3), (0 .. 7) (op & 3 counter-clockwise quarter
    turns after a left-right flip when op & 4).  Per chunk and op, in this order: transform the windows, run the eval
    forward, add the output under the inverse op to the chunk's slot (the first op stores, the last one also scales by
    1 / K).  K forwards and 2 K transform launches per chunk; `ensemble=1` launches none of them and is today's path."""

    ENSEMBLE_OPS = {1: (0,), 2: (0, 4), 4: (0, 1, 2, 3), 8: (0, 1, 2, 3, 4, 5, 6, 7)}

    def __init__(self, model, overlap: int = 32, batch: int = 64, mean: float = 0.456, std: float = 0.224, ensemble: int = 1):
        T = int(model.im_size)
        if not 0 <= int(overlap) <= T // 2:
            raise VuError(f"overlap must be in 0 .. im_size // 2 = {T // 2} (got {overlap})")
        if int(batch) < 1:
            raise VuError(f"batch must be at least 1 (got {batch})")
        if not float(std) > 0:
            raise VuError(f"std must be positive (got {std})")
        self.model, self.T, self.overlap, self.batch = model, T, int(overlap), int(batch)
        if ensemble not in self.ENSEMBLE_OPS:
            raise VuError(f"ensemble must be one of {sorted(self.ENSEMBLE_OPS)} (got {ensemble!r})")
        self.mean, self.std, self.ensemble = float(mean), float(std), int(ensemble)

    def _device(self) -> torch.device:
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise VuError("TiledRestorer runs on the MI355X only: move the model to 'cuda' (no CPU fallback)")
        return dev

    def __call__(self, img, output=None):
        if isinstance(img, (list, tuple)):
            return [self(i, output) for i in img]
        dev = self._device()
        t = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
        if not torch.is_tensor(t) or t.dim() != 3:
            raise VuError("expected one (H,W,C) uint8 or (C,H,W) float32 image (or a list of them)")
        Cn = int(self.model.num_channels)
        if t.dtype == torch.uint8:
            H, W, ch = t.shape
            t = t.to(dev, non_blocking=True).contiguous()
            output = output or "u8"
        elif t.dtype == torch.float32:
            if not t.is_cuda:
                raise VuError("a float32 image must already be on the GPU (got a CPU tensor); there is no CPU fallback")
            ch, H, W = t.shape
            t = t.detach().contiguous()
            output = output or "f32"
        else:
            raise VuError(f"expected a uint8 (H,W,C) or float32 (C,H,W) image, got {t.dtype}")
        if ch != Cn:
            raise VuError(f"the image has {ch} channels, the model {Cn}")
        if output not in ("u8", "f32"):
            raise VuError(f"output must be 'u8' or 'f32' (got {output!r})")
        with torch.no_grad():
            return self._restore(t, int(H), int(W), Cn, output)

    def _restore(self, img: torch.Tensor, H: int, W: int, Cn: int, output: str) -> torch.Tensor:
        L, T, ov, m = lib(), self.T, self.overlap, self.model
        ny, nx = C.c_int(0), C.c_int(0)
        check(L.vu_tile_plan_count(H, W, T, ov, C.byref(ny), C.byref(nx)), "vu_tile_plan_count")
        nt = ny.value * nx.value
        dev, st = img.device, stream_ptr(img.device)
        m._ensure_flat()
        outs = torch.empty(nt, Cn, T, T, dtype=torch.float32, device=dev)
        x = torch.empty(min(self.batch, nt), Cn, T, T, dtype=torch.float32, device=dev)
        ops = self.ENSEMBLE_OPS[self.ensemble]
        if len(ops) > 1:
            xt, scratch = torch.empty_like(x), torch.empty_like(x)
        for t0 in range(0, nt, self.batch):
            n = min(self.batch, nt - t0)
            if img.dtype == torch.uint8:
                check(L.vu_tile_gather_u8(ptr(img), ptr(x), H, W, Cn, T, ov, t0, n, self.mean, self.std, st), "vu_tile_gather_u8")
            else:
                check(L.vu_tile_gather_f32(ptr(img), ptr(x), H, W, Cn, T, ov, t0, n, st), "vu_tile_gather_f32")
            if len(ops) == 1:
                m._run_forward(x[:n], False, 0, out=outs[t0:t0 + n])
                continue
            for k, op in enumerate(ops):
                check(L.vu_dihedral_f32(ptr(x), ptr(xt), n, Cn, T, op, 0, 1.0, st), "vu_dihedral_f32")
                m._run_forward(xt[:n], False, 0, out=scratch[:n])
                check(L.vu_dihedral_f32(ptr(scratch), ptr(outs[t0:t0 + n]), n, Cn, T, L.vu_dihedral_inverse(op), int(k > 0),
                                        1.0 / len(ops) if k == len(ops) - 1 else 1.0, st), "vu_dihedral_f32")
        if output == "u8":
            res = torch.empty(H, W, Cn, dtype=torch.uint8, device=dev)
            check(L.vu_tile_blend(ptr(outs), None, ptr(res), H, W, Cn, T, ov, st), "vu_tile_blend")
        else:
            res = torch.empty(Cn, H, W, dtype=torch.float32, device=dev)
            check(L.vu_tile_blend(ptr(outs), ptr(res), None, H, W, Cn, T, ov, st), "vu_tile_blend")
        return res
