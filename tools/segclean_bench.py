"""Cost of the mask clean-up (csrc/vu_segclean.hip) on one MI355X: vu_seg_clean on a 64 x 512 x 512 uint8 mask, per phase and
as a whole, next to a plain 1-byte-per-pixel copy of the same mask (the memory floor: the least any pass over the mask moves).

Two inputs: `blobs`, smooth random blobs (a thresholded low-pass of white noise: what a segmentation model's mask looks like),
and `serpentine`, the worst case of tests/test_gpu_segclean.py (a one-pixel-wide path through a (3 th) x (3 tw) slice) tiled up
to the slice size: the longest union chains across tile borders and the slowest convergence inside a tile.  Each runs under
connectivity 8 (slice by slice) and 26 (the volume), with min_size, keep_largest and fill_holes all on (two labellings).

  whole_ms   the whole call with truth, counts and stats, mean of timed repetitions between two device events after untimed
             warm-up ones
  phases_ms  device time per launch from the library's own launch profiler (an event after every launch, behind a gate that lets
             the host run ahead), mean per call; label = foreground, holes = background of step 4
  copy_ms    out.copy_(mask) on the same buffers, timed the same way; whole_over_copy = whole_ms / copy_ms
Prints one JSON line per input and connectivity; --out also writes them to a file."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-unet_amd"))

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


def blobs(D, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(1, 1, D, H, W, generator=g, device="cuda")
    for _ in range(3):                                       # a box filter three times over: close to a Gaussian
        x = torch.nn.functional.avg_pool3d(x, (3, 9, 9), stride=1, padding=(1, 4, 4))
    return (x[0, 0] > x.std() * 0.5).to(torch.uint8).contiguous()


def serpentine(D, H, W):
    th, tw = C.c_int(0), C.c_int(0)
    check(lib().vu_cc_tile(C.byref(th), C.byref(tw)), "vu_cc_tile")
    h, w = 3 * th.value, 3 * tw.value
    s = torch.zeros(h, w, dtype=torch.uint8)
    s[0::2] = 1
    s[1::4, w - 1] = 1
    s[3::4, 0] = 1
    s = s.repeat((H + h - 1) // h, (W + w - 1) // w)[:H, :W]
    return s[None].repeat(D, 1, 1).contiguous().to("cuda")


def measure(name, mask, conn, a):
    L, st = lib(), stream_ptr()
    D, H, W = (int(v) for v in mask.shape)
    U = 1 if conn in (6, 26) else D
    g = torch.Generator(device="cuda").manual_seed(7)
    truth = (torch.rand(D, H, W, generator=g, device="cuda") < 0.3).to(torch.uint8)
    out = torch.empty_like(mask)
    counts = torch.empty(D, 3, dtype=torch.int64, device="cuda")
    stats = torch.empty(U, 4, dtype=torch.int64, device="cuda")
    nbytes = int(L.vu_seg_clean_scratch_bytes(D, H, W))
    scratch = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.int32, device="cuda")

    def clean():
        check(L.vu_seg_clean(ptr(mask), ptr(truth), ptr(out), ptr(counts), ptr(stats), ptr(scratch), nbytes, D, H, W, conn,
                             a.min_size, 1, 1, -1, st), "vu_seg_clean")

    res = {"input": name, "conn": conn, "D": D, "H": H, "W": W, "min_size": a.min_size, "keep_largest": 1, "fill_holes": 1,
           "foreground_share": float(mask.ne(0).float().mean()), "warmup": a.warmup, "reps": a.reps}
    ws, cs = [], []
    for _ in range(3):                                       # alternate, so that a drift of the machine hits both
        ws.append(timed(clean, a.warmup, a.reps))
        cs.append(timed(lambda: out.copy_(mask), a.warmup, a.reps))
    clean()
    torch.cuda.synchronize()
    res["stats_unit0"] = [int(v) for v in stats[0]]
    res["overflow"] = int(stats[:, 3].max())
    res["cleaned_share"] = float(out.float().mean())
    res["whole_ms"], res["copy_ms"] = sum(ws) / 3, sum(cs) / 3
    res["whole_ms_runs"], res["copy_ms_runs"] = ws, cs
    res["whole_over_copy"] = res["whole_ms"] / res["copy_ms"]
    check(L.vu_prof_enable(st), "vu_prof_enable")
    check(L.vu_prof_gate(20000), "vu_prof_gate")
    for _ in range(a.reps):
        clean()
    rep = json.loads(L.vu_prof_report().decode())
    res["phases_ms"] = {k.replace("vu_seg_clean/", ""): v["ms"] / a.reps for k, v in sorted(rep.items())}
    res["phases_sum_ms"] = sum(res["phases_ms"].values())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="64,512,512")
    ap.add_argument("--conn", default="8,26")
    ap.add_argument("--min-size", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segclean_bench.py measures on the GPU; none found (no CPU fallback)")
    D, H, W = (int(v) for v in a.shape.split(","))
    lines = []
    for name, mask in (("blobs", blobs(D, H, W, 3)), ("serpentine", serpentine(D, H, W))):
        for conn in (int(v) for v in a.conn.split(",")):
            lines.append(json.dumps(measure(name, mask, conn, a)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
