"""Cost of the per-volume intensity statistics (csrc/vu_intensity.hip) on one MI355X: vu_intensity_hist and vu_intensity_stats on a
resident 64 x 512 x 512 int16 volume, next to a plain device copy of the volume's 32 MiB in the same process (the memory floor of
one pass over the volume, the yardstick of the other segmentation benches).

Three inputs: uniform over the int16 range; CT-like (half the voxels at -1024, the rest normal around 40 with sigma 200); constant.
The in-tree library is the product form.  --variant tag=path (repeatable) times measurement builds of the same source in the same
run - tools/build_variant.sh <tag> vu_intensity.hip "-DVU_INTENSITY_DIRECT" (every count a global atomic),
"-DVU_INTENSITY_PEEL" (wave-uniform values peeled by ballot first), or both - each loaded as a library of its own beside the product;
every form's histogram is compared with torch.bincount before it is timed.

  *_ms        the whole call (clear + count for hist), mean of timed repetitions between two device events after untimed warm-up
              ones, three rounds alternating with the copy
  copy_ms     dst.copy_(vol), timed the same way; *_over_copy = call / copy
Prints one JSON line per input; --out also writes them to a file."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-unet_amd"))

import torch  # noqa: E402

from vit_unet.torch._lib import SIGNATURES, lib, ptr, stream_ptr  # noqa: E402

ROUNDS = 3
ENTRIES = ("vu_intensity_geometry", "vu_intensity_hist", "vu_intensity_stats", "vu_last_error")


def load_variant(path):
    L = C.CDLL(path)
    for name in ENTRIES:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = SIGNATURES[name]
    return L


def geometry(L):
    g = [C.c_int(0) for _ in range(3)]
    assert L.vu_intensity_geometry(*(C.byref(v) for v in g)) == 0
    return {"lds_base": g[0].value, "lds_bins": g[1].value, "voxels_per_block": g[2].value}


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


def make_input(kind, shape):
    g = torch.Generator(device="cuda").manual_seed(7)
    if kind == "uniform":
        return torch.randint(-32768, 32768, shape, generator=g, device="cuda", dtype=torch.int16)
    if kind == "constant":
        return torch.full(shape, -1024, device="cuda", dtype=torch.int16)
    v = torch.round(torch.randn(shape, generator=g, device="cuda") * 200.0 + 40.0).to(torch.int16)
    v[torch.rand(shape, generator=g, device="cuda") < 0.5] = -1024
    return v


def measure(kind, shape, forms, a):
    st = stream_ptr()
    vol = make_input(kind, shape)
    other = torch.empty_like(vol)
    want = torch.bincount(vol.reshape(-1).to(torch.int64) + 32768, minlength=65536)
    hist = torch.empty(65536, dtype=torch.int32, device="cuda")
    bbox = torch.empty(6, dtype=torch.int32, device="cuda")
    stats = torch.empty(16, dtype=torch.int64, device="cuda")
    pn, pd = (C.c_uint * 2)(5000, 995000), (C.c_uint * 2)(10 ** 6, 10 ** 6)

    def call(L, fn, *args):
        rc = fn(*args)
        if rc < 0:
            raise SystemExit(f"{kind}: rc={rc}: {L.vu_last_error().decode()}")

    calls = {}
    for tag, L in forms.items():
        calls[f"hist_{tag}"] = (lambda L=L: call(L, L.vu_intensity_hist, ptr(vol), None, ptr(hist), ptr(bbox), *shape, 0, 0, -1, st))
        calls[f"hist_nobox_{tag}"] = (lambda L=L: call(L, L.vu_intensity_hist, ptr(vol), None, ptr(hist), None, *shape, 0, 0, -1, st))
        calls[f"hist_{tag}"]()
        assert torch.equal(hist.to(torch.int64) & 0xffffffff, want), f"{kind}/{tag}: the histogram is wrong"
    P = forms["product"]
    calls["stats"] = lambda: call(P, P.vu_intensity_stats, ptr(hist), pn, pd, 2, ptr(stats), st)
    res = {"input": kind, "shape": list(shape), "bytes": vol.numel() * 2, "warmup": a.warmup, "reps": a.reps, "rounds": ROUNDS,
           "forms": {tag: geometry(L) for tag, L in forms.items()}}
    runs, copies = {k: [] for k in calls}, []
    for _ in range(ROUNDS):                                  # alternate, so that a drift of the machine hits everything
        for k, fn in calls.items():
            runs[k].append(timed(fn, a.warmup, a.reps))
        copies.append(timed(lambda: other.copy_(vol), a.warmup, a.reps))
    torch.cuda.synchronize()
    cp = sum(copies) / ROUNDS
    res.update({"copy_ms": cp, "copy_ms_runs": copies})
    for k in calls:
        ms = sum(runs[k]) / ROUNDS
        res.update({f"{k}_ms": ms, f"{k}_ms_runs": runs[k], f"{k}_over_copy": ms / cp})
    res["stats_first_words"] = stats[:5].cpu().tolist()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="64,512,512")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--variant", action="append", default=[], help="tag=path of a measurement build (tools/build_variant.sh)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("intensity_bench.py measures on the GPU; none found (no CPU fallback)")
    shape = tuple(int(v) for v in a.shape.split(","))
    forms = {"product": lib()}
    for v in a.variant:
        tag, path = v.split("=", 1)
        forms[tag] = load_variant(os.path.abspath(path))
    lines = []
    for kind in ("uniform", "ct", "constant"):
        lines.append(json.dumps(measure(kind, shape, forms, a)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
