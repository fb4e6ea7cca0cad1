"""Cost of the native-resolution patch gather and of the self-ensemble (csrc/vu_patch.hip) on one MI355X.  Inputs and
outputs stay on the device; every figure is the mean of `--reps` timed repetitions between two device events after
`--warmup` untimed ones, and the per-op figures are taken in `--rounds` passes over all eight ops so that a drift of the
machine hits every op alike (the mean over the rounds is reported, the per-round values are kept beside it).

  patch_us[op]     vu_patch_pairs_u8: one batch of `--patches` (64) crops of T x T x 3 (T = 224) out of one `--height` x
                   `--width` (3000 x 4000) noisy / clean pair, every crop under the same op, origins drawn once from a seed;
                   beside it the ratio to op 0 and the achieved bytes/s against the minimal traffic (2 n C T^2 bytes read,
                   8 n C T^2 written)
  dihedral_us[op]  vu_dihedral_f32 on (patches,3,T,T), copy form; minimal traffic 8 n C T^2 bytes; dihedral_acc_us: the
                   accumulate-and-scale form of the last ensemble op (12 n C T^2 bytes)
  restore_ms[K]    TiledRestorer(img) on one height x width image, Base bf16, overlap 32, batch 64, ensemble 1 and 8
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-unet_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vit_unet.torch import model as M  # noqa: E402
from vit_unet.torch._lib import check, lib, ptr, stream_ptr  # noqa: E402
from vit_unet.torch.restore import TiledRestorer  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--patch", type=int, default=224)
    ap.add_argument("--patches", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", default="base")
    ap.add_argument("--restore-reps", type=int, default=2)
    ap.add_argument("--no-restore", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("patch_bench.py measures on the GPU; none found (no CPU fallback)")
    H, W, T, n, Cn = a.height, a.width, a.patch, a.patches, 3
    L, st = lib(), stream_ptr()
    torch.manual_seed(0)
    noisy = torch.randint(0, 256, (H, W, Cn), dtype=torch.uint8, device="cuda")
    clean = torch.randint(0, 256, (H, W, Cn), dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(0)
    origins = np.stack([rng.integers(0, H - T + 1, n), rng.integers(0, W - T + 1, n)], axis=1)
    tables = [torch.from_numpy(np.concatenate([origins, np.full((n, 1), op)], axis=1).astype(np.int32)).to("cuda") for op in range(8)]
    x = torch.empty(n, Cn, T, T, device="cuda")
    y = torch.empty_like(x)
    src = torch.rand(n, Cn, T, T, device="cuda")
    elems = float(n) * Cn * T * T
    res = {"H": H, "W": W, "C": Cn, "T": T, "patches": n, "warmup": a.warmup, "reps": a.reps, "rounds": a.rounds,
           "patch_bytes": 10.0 * elems, "dihedral_bytes": 8.0 * elems, "dihedral_acc_bytes": 12.0 * elems}

    def patch(op):
        check(L.vu_patch_pairs_u8(ptr(noisy), ptr(clean), ptr(x), ptr(y), H, W, Cn, T, ptr(tables[op]), n, 0.456, 0.224, st),
              "vu_patch_pairs_u8")

    def dihedral(op, acc=0, scale=1.0):
        check(L.vu_dihedral_f32(ptr(src), ptr(x), n, Cn, T, op, acc, scale, st), "vu_dihedral_f32")

    for name, fn in (("patch", patch), ("dihedral", dihedral), ("dihedral_acc", lambda op: dihedral(op, 1, 0.125))):
        runs = [[1e3 * timed(lambda: fn(op), a.warmup, a.reps) for op in range(8)] for _ in range(a.rounds)]
        mean = [sum(r[op] for r in runs) / a.rounds for op in range(8)]
        res[f"{name}_us"], res[f"{name}_us_rounds"] = mean, runs
        res[f"{name}_vs_op0"] = [m / mean[0] for m in mean]
        res[f"{name}_TBps"] = [res[f"{name}_bytes"] / (m * 1e-6) / 1e12 for m in mean]
    if not a.no_restore:
        m = M.get_vit_unet(a.model, dtype=torch.bfloat16).to("cuda").eval()
        assert m.im_size == T and m.num_channels == Cn, "the restorer figures use the model's own window size"
        r1, r8 = TiledRestorer(m, overlap=32, batch=64), TiledRestorer(m, overlap=32, batch=64, ensemble=8)
        t1, t8 = [], []
        for _ in range(2):            # alternate the two
            t1.append(timed(lambda: r1(noisy), 1, a.restore_reps))
            t8.append(timed(lambda: r8(noisy), 1, a.restore_reps))
        res["model"], res["restore_ms"] = a.model, {"1": sum(t1) / 2, "8": sum(t8) / 2}
        res["restore_ms_runs"] = {"1": t1, "8": t8}
        res["restore_8_vs_1"] = res["restore_ms"]["8"] / res["restore_ms"]["1"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
