"""Cost of volume resampling (csrc/vu_resample.hip) on one MI355X: vu_resample_i16, vu_resample_u8_nearest and vu_resample_f32
(logits, mask and counts in one call) on a resident 64 x 512 x 512 volume, next to a plain copy of a tensor of the OUTPUT's byte
size (the memory floor: no resampling writes less).

Three in-plane ratios, the slice count kept: a 0.6 mm acquisition brought to 1.0 mm (512 -> 307), a 1.4 mm one (512 -> 717) and the
identity.  The float32 entry is timed on the way back, from the working grid to 512 x 512.

  *_ms        the whole call, mean of timed repetitions between two device events after untimed warm-up ones, three rounds
              alternating with the copy
  *_copy_ms   out.copy_(other) on a tensor of the entry's output size and type, timed the same way; *_over_copy = call / copy
Prints one JSON line per ratio; --out also writes them to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-unet_amd"))

import torch  # noqa: E402

from vit_unet.torch._lib import check, lib, ptr, stream_ptr  # noqa: E402
from vit_unet.torch.segment import VolumeResampler  # noqa: E402

ROUNDS = 3


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure(name, native, spacing, a):
    L, st = lib(), stream_ptr()
    work = VolumeResampler((None, 1, 1)).out_shape(native, spacing)
    g = torch.Generator(device="cuda").manual_seed(7)
    vol = torch.randint(-1024, 3072, native, generator=g, device="cuda", dtype=torch.int16)
    lab = torch.randint(0, 4, native, generator=g, device="cuda", dtype=torch.uint8)
    z = torch.randn(work, generator=g, device="cuda")
    vol_w, lab_w = torch.empty(work, dtype=torch.int16, device="cuda"), torch.empty(work, dtype=torch.uint8, device="cuda")
    z_n, mask_n = torch.empty(native, dtype=torch.float32, device="cuda"), torch.empty(native, dtype=torch.uint8, device="cuda")
    counts = torch.empty(native[0], 3, dtype=torch.int64, device="cuda")
    nbytes = int(L.vu_resample_f32_scratch_bytes(*native))
    scratch = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
    calls = {
        "i16": (lambda: check(L.vu_resample_i16(ptr(vol), ptr(vol_w), *native, *work, st), "vu_resample_i16"), vol_w),
        "u8": (lambda: check(L.vu_resample_u8_nearest(ptr(lab), ptr(lab_w), *native, *work, st), "vu_resample_u8_nearest"), lab_w),
        "f32": (lambda: check(L.vu_resample_f32(ptr(z), ptr(lab), ptr(z_n), ptr(mask_n), ptr(counts), ptr(scratch), nbytes, *work, *native,
                                                0.0, -1, st), "vu_resample_f32"), z_n),
    }
    res = {"ratio": name, "spacing": list(spacing), "native": list(native), "working": list(work), "warmup": a.warmup, "reps": a.reps,
           "rounds": ROUNDS, "form": "direct gathers, fused x / y / z stages in registers"}
    runs = {k: [] for k in calls}
    copies = {k: [] for k in calls}
    for _ in range(ROUNDS):                                  # alternate, so that a drift of the machine hits everything
        for k, (fn, out) in calls.items():
            other = torch.empty_like(out)
            runs[k].append(timed(fn, a.warmup, a.reps))
            copies[k].append(timed(lambda: other.copy_(out), a.warmup, a.reps))
    torch.cuda.synchronize()
    for k, (_, out) in calls.items():
        ms, cp = sum(runs[k]) / ROUNDS, sum(copies[k]) / ROUNDS
        res.update({f"{k}_ms": ms, f"{k}_ms_runs": runs[k], f"{k}_copy_ms": cp, f"{k}_copy_ms_runs": copies[k],
                    f"{k}_over_copy": ms / cp, f"{k}_out_bytes": out.numel() * out.element_size()})
    res["mask_pixels"] = int(counts[:, 0].sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="64,512,512")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench.py measures on the GPU; none found (no CPU fallback)")
    native = tuple(int(v) for v in a.shape.split(","))
    lines = []
    for name, spacing in (("0.6 -> 1.0", (1.0, 0.6, 0.6)), ("1.4 -> 1.0", (1.0, 1.4, 1.4)), ("identity", (1.0, 1.0, 1.0))):
        lines.append(json.dumps(measure(name, native, spacing, a)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
