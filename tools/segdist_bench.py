"""Cost of the surface-distance metrics (csrc/vu_segdist.hip) on one MI355X: vu_edt_sq and vu_surface_dist on a resident
64 x 512 x 512 uint8 mask, per launch and as a whole, next to a plain 1-byte-per-pixel copy of the same mask (the memory floor:
the least any pass over the mask moves).

Two inputs: `blobs`, smooth random blobs (a thresholded low-pass of white noise: what a segmentation model's mask looks like),
and `sparse`, one site in 20000 pixels: the worst case of the pruned lower envelope, where every output walks far along its line
and no piece of a long line can be voted away.  Each runs under dims 2 (slice by slice) and dims 3 (the volume).  The truth of
vu_surface_dist is the mask moved by (1, 3, -2) pixels.

  edt_ms / dist_ms  the whole call, mean of timed repetitions between two device events after untimed warm-up ones, three rounds
                    alternating with the copy
  *_launches_ms     device time per launch from the library's own launch profiler (an event after every launch, behind a gate
                    that lets the host run ahead), mean per call
  copy_ms           out.copy_(mask) on the same buffers, timed the same way; *_over_copy = the call / copy_ms
Prints one JSON line per input and dims; --out also writes them to a file."""
import argparse
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


def sparse(D, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(D, H, W, generator=g, device="cuda") < 5e-5).to(torch.uint8).contiguous()


def profiled(fn, reps, prefix):
    L, st = lib(), stream_ptr()
    check(L.vu_prof_enable(st), "vu_prof_enable")
    check(L.vu_prof_gate(20000), "vu_prof_gate")
    for _ in range(reps):
        fn()
    rep = json.loads(L.vu_prof_report().decode())
    return {k.replace(prefix, ""): v["ms"] / reps for k, v in sorted(rep.items())}


def measure(name, mask, dims, a):
    L, st = lib(), stream_ptr()
    D, H, W = (int(v) for v in mask.shape)
    U = 1 if dims == 3 else D
    truth = torch.roll(mask, (1, 3, -2), (0, 1, 2)).contiguous()
    out = torch.empty_like(mask)
    dist2 = torch.empty(D, H, W, dtype=torch.int32, device="cuda")
    stats = torch.empty(U, 6, dtype=torch.int64, device="cuda")
    sums = torch.empty(U, 2, dtype=torch.float64, device="cuda")
    order = torch.empty(U, 3, 2, dtype=torch.int32, device="cuda")
    eb, sb = int(L.vu_edt_scratch_bytes(D, H, W, dims)), int(L.vu_surface_dist_scratch_bytes(D, H, W, dims))
    scratch = torch.empty((max(eb, sb) + 15) // 16 * 4, dtype=torch.int32, device="cuda")

    def edt():
        check(L.vu_edt_sq(ptr(mask), ptr(dist2), ptr(scratch), eb, D, H, W, dims, 1, 1, 1, 1, st), "vu_edt_sq")

    def dist():
        check(L.vu_surface_dist(ptr(mask), ptr(truth), ptr(stats), ptr(sums), ptr(order), None, None, ptr(scratch), sb, D, H, W, dims,
                                1, 1, 1, -1, 1, 19, 20, st), "vu_surface_dist")

    res = {"input": name, "dims": dims, "D": D, "H": H, "W": W, "spacing": [1, 1, 1], "tol2": 1, "quantile": [19, 20],
           "foreground_share": float(mask.ne(0).float().mean()), "warmup": a.warmup, "reps": a.reps}
    es, ds, cs = [], [], []
    for _ in range(3):                                       # alternate, so that a drift of the machine hits all three
        es.append(timed(edt, a.warmup, a.reps))
        ds.append(timed(dist, a.warmup, a.reps))
        cs.append(timed(lambda: out.copy_(mask), a.warmup, a.reps))
    torch.cuda.synchronize()
    res["stats_unit0"] = [int(v) for v in stats[0]]
    res["edt_max"] = int((dist2.to(torch.int64) & 0xffffffff).max())
    res["edt_ms"], res["dist_ms"], res["copy_ms"] = sum(es) / 3, sum(ds) / 3, sum(cs) / 3
    res["edt_ms_runs"], res["dist_ms_runs"], res["copy_ms_runs"] = es, ds, cs
    res["edt_over_copy"], res["dist_over_copy"] = res["edt_ms"] / res["copy_ms"], res["dist_ms"] / res["copy_ms"]
    res["edt_launches_ms"] = profiled(edt, a.reps, "vu_edt_sq/")
    res["dist_launches_ms"] = profiled(dist, a.reps, "vu_surface_dist/")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="64,512,512")
    ap.add_argument("--dims", default="2,3")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segdist_bench.py measures on the GPU; none found (no CPU fallback)")
    D, H, W = (int(v) for v in a.shape.split(","))
    lines = []
    for name, mask in (("blobs", blobs(D, H, W, 3)), ("sparse", sparse(D, H, W, 4))):
        for dims in (int(v) for v in a.dims.split(",")):
            lines.append(json.dumps(measure(name, mask, dims, a)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
