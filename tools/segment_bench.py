"""Cost of whole-volume segmentation (vit_unet/torch/segment.py) on one MI355X: Base at 512 x 512 x 1 in bf16 (BASELINE.md
config 5's shape), volumes of 512 x 512 slices (one window a slice) and of 640 x 640 slices (four windows a slice), overlap
32.  Inputs and outputs stay on the device; every figure is the mean of timed repetitions between two device events after
untimed warm-up ones.

  segmenter_ms  TiledSegmenter.score(vol, truth): gather + eval forwards + blend with mask and counts (the copy of the
                (D,3) counts to the host included)
  forwards_ms   the bare eval forwards over the same window chunks (model(x) under no_grad; no segmenter code involved):
                the yardstick
  gather_ms / blend_ms   the two kernels alone on `--kernel-slices` slices (more than the 256 MiB last-level cache holds),
                in the segmenter's own chunks / groups, with achieved bytes/s against their minimal traffic (gather: 2 bytes
                read per slice pixel + 4 per window pixel written; blend: 4 per window pixel read, 1 truth byte read and 1
                mask byte written per slice pixel)
  unfused_ms    what vu_seg_blend (mask + counts) replaces, on the same windows: vu_tile_blend(out_f32) per slice, then `>=`
                and three sums per slice in torch
Prints one JSON line per volume shape; --out also writes them to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-unet_amd"))

import torch  # noqa: E402

from vit_unet.torch import model as M  # noqa: E402
from vit_unet.torch._lib import check, lib, ptr, stream_ptr  # noqa: E402
from vit_unet.torch.restore import tile_plan  # noqa: E402
from vit_unet.torch.segment import TiledSegmenter  # noqa: E402


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


def groups(D, nt, batch):
    """[(z0, nz, [(c0, n)])]: the segmenter's documented execution order."""
    G = max(1, batch // nt)
    out = []
    for z0 in range(0, D, G):
        nz = min(G, D - z0)
        out.append((z0, nz, [(c0, min(batch, nz * nt - c0)) for c0 in range(0, nz * nt, batch)]))
    return out


def measure(m, a, H, W, D):
    T, ov = m.im_size, a.overlap
    oy, ox = tile_plan(H, W, T, ov)
    nt = len(oy) * len(ox)
    L, st = lib(), stream_ptr()
    g = torch.Generator(device="cuda").manual_seed(H + W)
    vol = torch.randint(-1500, 1500, (D, H, W), generator=g, device="cuda").to(torch.int16)
    truth = (torch.rand(D, H, W, generator=g, device="cuda") < 0.1).to(torch.uint8)
    s = TiledSegmenter(m, overlap=ov, batch=a.batch)
    plan = groups(D, nt, a.batch)
    x = torch.rand(min(a.batch, plan[0][1] * nt), 1, T, T, device="cuda")

    def forwards():
        with torch.no_grad():
            for _, _, chunks in plan:
                for _, n in chunks:
                    m(x[:n])

    res = {"model": a.model, "dtype": "bf16", "D": D, "H": H, "W": W, "T": T, "overlap": ov, "batch": a.batch,
           "windows_per_slice": nt, "warmup": a.warmup, "reps": a.reps}
    # alternate the two end-to-end figures so that a drift of the machine hits both
    ss, fs = [], []
    for _ in range(3):
        ss.append(timed(lambda: s.score(vol, truth), a.warmup, a.reps))
        fs.append(timed(forwards, a.warmup, a.reps))
    res["segmenter_ms"], res["forwards_ms"] = sum(ss) / 3, sum(fs) / 3
    res["segmenter_ms_runs"], res["forwards_ms_runs"] = ss, fs
    res["ratio"] = res["segmenter_ms"] / res["forwards_ms"]
    del vol, truth

    # the kernels alone, on a volume that the last-level cache does not hold
    K = a.kernel_slices
    kplan = groups(K, nt, a.batch)
    G = kplan[0][1]
    vol = torch.randint(-1500, 1500, (K, H, W), generator=g, device="cuda").to(torch.int16)
    truth = (torch.rand(K, H, W, generator=g, device="cuda") < 0.1).to(torch.uint8)
    tiles = torch.randn(K * nt, 1, T, T, generator=g, device="cuda")
    mask = torch.empty(K, H, W, dtype=torch.uint8, device="cuda")
    counts = torch.empty(K, 3, dtype=torch.int64, device="cuda")
    nbytes = L.vu_seg_blend_scratch_bytes(G, H, W)
    scratch = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
    xk = torch.empty(K * nt, 1, T, T, device="cuda")       # every chunk to its own place: no rewriting of one cached buffer
    zf = torch.empty(K, H, W, device="cuda")

    def gather():
        for z0, _, chunks in kplan:
            for c0, n in chunks:
                g0 = z0 * nt + c0
                check(L.vu_tile_gather_i16(ptr(vol), ptr(xk[g0:g0 + n]), K, H, W, T, ov, g0, n, s.window[0], s.window[1], st),
                      "vu_tile_gather_i16")

    def blend():
        for z0, nz, _ in kplan:
            check(L.vu_seg_blend(ptr(tiles[z0 * nt:(z0 + nz) * nt]), ptr(truth[z0:z0 + nz]), None, ptr(mask[z0:z0 + nz]),
                                 ptr(counts[z0:z0 + nz]), ptr(scratch), nbytes, nz, H, W, T, ov, s.zthr, s.label, st), "vu_seg_blend")

    def unfused():
        for z in range(K):
            check(L.vu_tile_blend(ptr(tiles[z * nt:(z + 1) * nt]), ptr(zf[z]), None, H, W, 1, T, ov, st), "vu_tile_blend")
        mk = zf >= s.zthr
        tr = truth != 0
        return mk.sum((1, 2)), tr.sum((1, 2)), (mk & tr).sum((1, 2))

    # the two blends must agree before their times are compared
    blend()
    p, t, b = unfused()
    assert torch.equal(counts, torch.stack([p, t, b], 1)) and torch.equal(mask, (zf >= s.zthr).to(torch.uint8))
    kr = a.reps * 4
    res["kernel_slices"] = K
    res["gather_ms"] = timed(gather, a.warmup, kr)
    bs, us = [], []
    for _ in range(3):
        bs.append(timed(blend, a.warmup, kr))
        us.append(timed(unfused, a.warmup, kr))
    res["blend_ms"], res["unfused_ms"] = sum(bs) / 3, sum(us) / 3
    res["blend_ms_runs"], res["unfused_ms_runs"] = bs, us
    res["unfused_over_blend"] = res["unfused_ms"] / res["blend_ms"]
    win_bytes, px = 4.0 * K * nt * T * T, float(K) * H * W
    res["gather_bytes"], res["blend_bytes"] = 2.0 * px + win_bytes, win_bytes + 2.0 * px
    res["gather_TBps"] = res["gather_bytes"] / (res["gather_ms"] * 1e-3) / 1e12
    res["blend_TBps"] = res["blend_bytes"] / (res["blend_ms"] * 1e-3) / 1e12
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="base")
    ap.add_argument("--im-size", type=int, default=512)
    ap.add_argument("--sizes", default="512,640", help="comma-separated slice sizes (square slices)")
    ap.add_argument("--slices", type=int, default=32, help="slices of the end-to-end volume")
    ap.add_argument("--kernel-slices", type=int, default=256, help="slices of the volume the kernels alone are timed on")
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segment_bench.py measures on the GPU; none found (no CPU fallback)")
    torch.manual_seed(0)
    m = M.get_vit_unet(a.model, dtype=torch.bfloat16, im_size=a.im_size, num_channels=1).to("cuda").eval()
    lines = []
    for size in (int(v) for v in a.sizes.split(",")):
        lines.append(json.dumps(measure(m, a, size, size, a.slices)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
