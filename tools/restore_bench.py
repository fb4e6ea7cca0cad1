"""Cost of whole-image restoration (vit_unet/torch/restore.py) on one MI355X: Base bf16, one 4032 x 3024 x 3 image,
overlap 32, batch 64 by default.  Input and output stay on the device; every figure is the mean of `--reps` timed
repetitions between two device events after `--warmup` untimed ones.

  restorer_ms   TiledRestorer(img): gather + eval forwards + blend
  forwards_ms   the bare eval forwards over the same window batches (model(x) under no_grad; no restorer code involved):
                the yardstick
  gather_ms / blend_ms   the two kernels alone (the gather summed over the chunks), with achieved bytes/s against their
                minimal traffic (gather: H W C bytes read + 4 nt C T^2 written; blend: 4 nt C T^2 read + H W C written)
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-unet_amd"))

import torch  # noqa: E402

from vit_unet.torch import model as M  # noqa: E402
from vit_unet.torch._lib import check, lib, ptr, stream_ptr  # noqa: E402
from vit_unet.torch.restore import TiledRestorer, tile_plan  # noqa: E402


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
    ap.add_argument("--model", default="base")
    ap.add_argument("--height", type=int, default=3024)
    ap.add_argument("--width", type=int, default=4032)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("restore_bench.py measures on the GPU; none found (no CPU fallback)")
    torch.manual_seed(0)
    m = M.get_vit_unet(a.model, dtype=torch.bfloat16).to("cuda").eval()
    T, Cn, H, W, ov = m.im_size, m.num_channels, a.height, a.width, a.overlap
    oy, ox = tile_plan(H, W, T, ov)
    nt = len(oy) * len(ox)
    img = torch.randint(0, 256, (H, W, Cn), dtype=torch.uint8, device="cuda")
    r = TiledRestorer(m, overlap=ov, batch=a.batch)
    L, st = lib(), stream_ptr()
    chunks = [(t0, min(a.batch, nt - t0)) for t0 in range(0, nt, a.batch)]
    x = torch.rand(min(a.batch, nt), Cn, T, T, device="cuda")
    tiles = torch.rand(nt, Cn, T, T, device="cuda")
    out_u8 = torch.empty(H, W, Cn, dtype=torch.uint8, device="cuda")

    def forwards():
        with torch.no_grad():
            for _, n in chunks:
                m(x[:n])

    def gather():
        for t0, n in chunks:
            check(L.vu_tile_gather_u8(ptr(img), ptr(x), H, W, Cn, T, ov, t0, n, r.mean, r.std, st), "vu_tile_gather_u8")

    def blend():
        check(L.vu_tile_blend(ptr(tiles), None, ptr(out_u8), H, W, Cn, T, ov, st), "vu_tile_blend")

    res = {"model": a.model, "dtype": "bf16", "H": H, "W": W, "C": Cn, "T": T, "overlap": ov, "batch": a.batch, "windows": nt,
           "warmup": a.warmup, "reps": a.reps}
    # alternate the two end-to-end figures so that a drift of the machine hits both
    rs, fs = [], []
    for _ in range(3):
        rs.append(timed(lambda: r(img), a.warmup, a.reps))
        fs.append(timed(forwards, a.warmup, a.reps))
    res["restorer_ms"], res["forwards_ms"] = sum(rs) / 3, sum(fs) / 3
    res["restorer_ms_runs"], res["forwards_ms_runs"] = rs, fs
    res["ratio"] = res["restorer_ms"] / res["forwards_ms"]
    win_bytes, px = 4.0 * nt * Cn * T * T, float(H) * W * Cn
    res["gather_ms"], res["blend_ms"] = timed(gather, a.warmup, a.reps * 4), timed(blend, a.warmup, a.reps * 4)
    res["gather_bytes"], res["blend_bytes"] = px + win_bytes, win_bytes + px
    res["gather_TBps"] = res["gather_bytes"] / (res["gather_ms"] * 1e-3) / 1e12
    res["blend_TBps"] = res["blend_bytes"] / (res["blend_ms"] * 1e-3) / 1e12
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
