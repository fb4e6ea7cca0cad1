"""Cost of the segmentation patch pipeline (csrc/vu_segpatch.hip) on one MI355X.  Inputs and outputs stay on the device;
every figure is the mean of `--reps` timed repetitions between two device events after `--warmup` untimed ones, taken in
`--rounds` passes over all figures so that a drift of the machine hits every one alike (the mean over the rounds is
reported, the per-round values are kept beside it).

  index_us     vu_fg_index on a `--depth` x `--height` x `--width` (64 x 512 x 512) uint8 mask with one ellipsoid of
               foreground; minimal traffic D H W mask bytes read + 12 D H bytes of row counts and index
  draw_us      vu_segpatch_draw of `--patches` (64) crops, all of them foreground crops (fg_thresh = 2^32 - 1: the search and
               the row walk run for every crop); traffic is the words, the table and at most one mask row per crop
  cut_us[op]   vu_patch_pairs_i16: `--patches` crops of T x T (T = 224) out of the int16 volume and the mask, every crop
               under the same op, origins drawn once from a seed; minimal traffic 3 n T^2 bytes read, 8 n T^2 written
Beside each time the achieved bytes/s against that minimal traffic.  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-unet_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vit_unet.torch._lib import check, lib, ptr, stream_ptr  # noqa: E402


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
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--patch", type=int, default=224)
    ap.add_argument("--patches", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segpatch_bench.py measures on the GPU; none found (no CPU fallback)")
    D, H, W, T, n = a.depth, a.height, a.width, a.patch, a.patches
    L, st = lib(), stream_ptr()
    torch.manual_seed(0)
    vol = torch.randint(-1500, 1500, (D, H, W), dtype=torch.int16, device="cuda")
    z, y, x = torch.meshgrid(torch.arange(D, device="cuda"), torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    mask = ((((z - D / 2) / (D / 4)) ** 2 + ((y - H / 2) / (H / 8)) ** 2 + ((x - W / 2) / (W / 8)) ** 2) <= 1.0).to(torch.uint8).contiguous()
    del z, y, x
    nbytes = int(L.vu_fg_index_bytes(D, H))
    scratch = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
    index = torch.empty(D * H + 1, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(0)
    words = torch.from_numpy(rng.integers(0, 2 ** 32, (n, 4), dtype=np.uint64).astype(np.uint32).view(np.int32)).to("cuda")
    drawn = torch.empty(n, 4, dtype=torch.int32, device="cuda")
    origins = np.stack([rng.integers(0, D, n), rng.integers(0, H - T + 1, n), rng.integers(0, W - T + 1, n)], axis=1)
    tables = [torch.from_numpy(np.concatenate([origins, np.full((n, 1), op)], axis=1).astype(np.int32)).to("cuda") for op in range(8)]
    xo = torch.empty(n, 1, T, T, device="cuda")
    yo = torch.empty_like(xo)

    def index_fn():
        check(L.vu_fg_index(ptr(mask), ptr(index), ptr(scratch), nbytes, D, H, W, -1, st), "vu_fg_index")

    def draw_fn():
        check(L.vu_segpatch_draw(ptr(mask), ptr(index), ptr(words), ptr(drawn), n, D, H, W, T, 0xffffffff, -1, st), "vu_segpatch_draw")

    def cut_fn(op):
        check(L.vu_patch_pairs_i16(ptr(vol), ptr(mask), ptr(xo), ptr(yo), D, H, W, T, ptr(tables[op]), n, -1024.0, 1024.0, 0.0, -1, st),
              "vu_patch_pairs_i16")

    index_fn()
    torch.cuda.synchronize()
    total = int(index[-1].item())
    res = {"D": D, "H": H, "W": W, "T": T, "patches": n, "warmup": a.warmup, "reps": a.reps, "rounds": a.rounds, "foreground": total,
           "index_bytes": float(D) * H * W + 12.0 * D * H, "draw_bytes": 32.0 * n + float(n) * W,
           "cut_bytes": 11.0 * n * T * T}
    idx_r, draw_r, cut_r = [], [], []
    for _ in range(a.rounds):
        idx_r.append(1e3 * timed(index_fn, a.warmup, a.reps))
        draw_r.append(1e3 * timed(draw_fn, a.warmup, a.reps))
        cut_r.append([1e3 * timed(lambda: cut_fn(op), a.warmup, a.reps) for op in range(8)])
    res["index_us"], res["index_us_rounds"] = sum(idx_r) / a.rounds, idx_r
    res["draw_us"], res["draw_us_rounds"] = sum(draw_r) / a.rounds, draw_r
    res["cut_us"], res["cut_us_rounds"] = [sum(r[op] for r in cut_r) / a.rounds for op in range(8)], cut_r
    res["index_TBps"] = res["index_bytes"] / (res["index_us"] * 1e-6) / 1e12
    res["draw_GBps"] = res["draw_bytes"] / (res["draw_us"] * 1e-6) / 1e9
    res["cut_TBps"] = [res["cut_bytes"] / (m * 1e-6) / 1e12 for m in res["cut_us"]]
    res["cut_vs_op0"] = [m / res["cut_us"][0] for m in res["cut_us"]]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
