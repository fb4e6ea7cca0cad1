#!/usr/bin/env python3
"""bench.py - images/sec of one ViT_UNet train step (forward + MSE + backward + gradient all-reduce +
AdamW) on N MI355X GPUs of one node, the metric BASELINE.json names.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus N ...      (outside torchrun: starts the N ranks itself as a child `python -m torch.distributed.run`)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One process per GPU (RANK / LOCAL_RANK / WORLD_SIZE from the environment), data parallel over
RCCL: every rank holds `--batch` images (weak scaling), gradients of the flat arena are summed in
buckets of at most 48 MB cut at backward-unit boundaries in reverse execution order, each all-reduced
on a side stream while the backward goes on (engine.dp_unit_buckets).  Inputs are synthetic and resident in HBM before the
timed region.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times exactly `--steps` steps, writes the last step's outputs if
`--dump-outputs DIR` is given, and prints the line (metric, value, unit, higher_is_better, dtype,
ms_per_step, ...).  With `--full` the line also carries what takes runs or checks of its own:
  sustained    - a second, longer timed region of the same step (clocks and thermals)
  host_input   - the same step fed from pinned host memory (PCIe-inclusive rates), N=1 only
  roofline     - the dominant kernel of the step, timed live with HIP events behind every launch
                 (vu_prof_enable) over extra instrumented steps; achieved = algorithmic flops (or
                 bytes) / launch time, against the MI355X dense bf16 MFMA peak (or HBM peak)
  parity       - the GPU eval forward against the CPU oracle, N=1 only
  cpu_baseline - the CPU oracle (torch CPU fp32 restatement of the reference) timed on this
                 host's cores on a bounded sample (B=8, a few iterations), N=1 only
Without `--full` these fields are null.

`--dump-outputs DIR` (rank 0): what the timed step left behind after its last timed step, as float32
.npy files - loss, output (the model's prediction), params and grads (the flat parameter / gradient
arenas after AdamW), bn_stats (BatchNorm running statistics).  An array of more than DUMP_CAP elements
is written as a fixed, seeded sample of DUMP_CAP elements (the same indices on every run).  Inputs,
weights and dropout masks are seeded, so two runs with the same arguments are comparable output for
output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "vit-unet_amd"))

import torch  # noqa: E402

TRAIN_GFLOP_PER_IMG = {"lite": 27.93, "base": 23.27, "large": 42.43, "seg512": 107.71}
MFMA_PEAK_TFLOPS = 2500.0      # dense bf16, MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0
DUMP_CAP = 3 << 20             # elements per dumped array (12 MB in float32; five arrays stay under 64 MB)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--model", default="base", choices=["lite", "base", "large", "seg512"],
                    help="seg512 = BASELINE config 5 shape: Base ctor at 512x512x1, Dice loss on a sigmoid head")
    ap.add_argument("--batch", type=int, default=64, help="images per GPU (weak scaling: the default mode)")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="strong scaling: this many images per step over ALL GPUs (BASELINE config 3: 64 over 2 / 4 GPUs)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--attn-operands", default=None, choices=["storage", "e4m3"],
                    help="what q, k, v are rounded to before the attention products; default: e4m3 for seg512 "
                         "(BASELINE config 5: fp8 attention operands), the storage dtype otherwise")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--force-graph", action="store_true", help="replay a hipGraph even where TrainStep.prefers_eager() says that "
                    "eager launches are faster (the low-priority dv sweep of the recompute attention's backward)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-host-input", action="store_true", help="skip the PCIe-inclusive legs (N=1 only)")
    ap.add_argument("--grad-wire", default="fp32", choices=["fp32", "bf16"], help="N > 1: dtype of the gradient buckets on the links")
    ap.add_argument("--collective", default="all_reduce", choices=["all_reduce", "rs_ag", "c_abi"],
                    help="N > 1: one all-reduce per gradient bucket, or reduce-scatter + all-gather (engine._sum_over_ranks)")
    ap.add_argument("--no-sustained", action="store_true", help="skip the second, longer timed region (profiler runs)")
    ap.add_argument("--sustained-s", type=float, default=8.0, help="length of the second timed region in seconds")
    ap.add_argument("--profile-steps", type=int, default=2)
    ap.add_argument("--dump-profile", default=None, help="--full: write the full per-kernel table (JSON) here")
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs of its own: sustained region, host-input legs, roofline, "
                         "parity against the CPU oracle, CPU baseline (each still switched off by its --no-* option)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the last timed step's outputs to DIR/<name>.npy (float32, large arrays sampled)")
    a = ap.parse_args()
    if a.dump_profile and not a.full:
        ap.error("--dump-profile needs --full (the per-kernel table comes from the roofline steps)")
    return a


def dump_sample(t: torch.Tensor, cap: int = DUMP_CAP, seed: int = 0) -> torch.Tensor:
    """`t` flattened, or a fixed, seeded, sorted sample of `cap` of its elements: one index drawn in each of `cap` equal
    strides of the flat array, so that the sample covers the whole tensor and is the same on every run."""
    t = t.detach().reshape(-1)
    n = t.numel()
    if n <= cap:
        return t
    g = torch.Generator(device="cpu").manual_seed(seed)
    lo = torch.arange(cap, dtype=torch.int64) * n // cap
    hi = (torch.arange(1, cap + 1, dtype=torch.int64) * n) // cap
    idx = lo + (torch.rand(cap, generator=g, dtype=torch.float64) * (hi - lo)).to(torch.int64)
    return t[idx.to(t.device)]


def dump_outputs(out_dir: str, ts, model) -> dict:
    """The arrays a caller of the timed step receives after its last step, as float32 .npy files (see the module docstring)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"loss": ts.loss, "output": ts._gout, "params": model._arena, "grads": model._garena, "bn_stats": model._bn}
    shapes = {}
    for i, (name, t) in enumerate(arrays.items()):
        v = dump_sample(t, seed=i).float().cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), v)
        shapes[name] = {"shape": list(t.shape), "written": int(v.size)}
    return shapes


def host_cores() -> int:
    """Cores this process may actually use: min(affinity mask, cgroup cpu quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except Exception:
        pass
    return max(1, n)


def cpu_baseline(model_name: str, threads: int):
    """The oracle's train step on the host cores: B=8, 1 warm-up + up to 2 timed iterations
    (stops after the first timed one if it took more than 15 s, so the default run stays short)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import vit_unet_oracle as O
    torch.set_num_threads(threads)
    cfg = O.Config(**O.PRESETS[model_name])
    w = O.make_weights(cfg, seed=0)
    names = [k for k, _ in O.param_shapes(cfg)]
    for k in names:
        w[k].requires_grad_(True)
    m = {k: torch.zeros_like(w[k]) for k in names}
    v = {k: torch.zeros_like(w[k]) for k in names}
    B = 8
    x, y = O.make_batch(cfg, B=B, seed=1234)
    times = []
    for it in range(3):
        t0 = time.perf_counter()
        out = O.forward(w, cfg, x, training=True, seed=None)      # torch-native dropout, as the reference
        loss = O.mse_loss(out, y)
        loss.backward()
        with torch.no_grad():
            for k in names:
                O.adamw_step(w[k], w[k].grad, m[k], v[k], it + 1)
                w[k].grad = None
        times.append(time.perf_counter() - t0)
        if it >= 1 and times[-1] > 15.0:
            break
    best = min(times[1:])
    return {"value": B / best, "unit": "images/s", "cores": threads, "kind": "port",
            "sample": f"oracle (torch CPU fp32) train step, {model_name}, B={B}, best of {len(times) - 1} after 1 warm-up",
            "s_per_step": best}


def eval_parity(model_name: str, dtype, B: int = 2, operands: str = "storage"):
    """error of the GPU forward against the CPU oracle (fp32) on the synthetic batch, and what it
    does to the metric the reference reports (functions.py:7-19 PSNR; README.md:91-101 Dice for the segmentation shape).
    Eval mode (running statistics), the oracle's deterministic weights (make_weights: every tensor non-trivial, running
    variances ~1e-4 as after training), full-size model.  The oracle is the checker here, nothing is timed."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import vit_unet_oracle as O
    from vit_unet.torch import model as M
    seg = model_name == "seg512"
    if seg:
        kw = dict(O.PRESETS["base"], im_size=512, num_channels=1)
    else:
        kw = dict(O.PRESETS[model_name])
    cfg = O.Config(**kw)
    w = O.make_weights(cfg, seed=0)
    if seg:
        g = torch.Generator().manual_seed(4321)
        x = torch.rand(B, 1, 512, 512, generator=g)
        y = (torch.rand(B, 1, 512, 512, generator=g) < 0.1).float()
    else:
        x, y = O.make_batch(cfg, B=B, seed=1234)
    m = M.HViT_UNet(dtype=dtype, attn_operands=operands, **kw)
    m.load_state_dict({k: v.clone().float() for k, v in w.items()})
    m = m.to("cuda").eval()
    with torch.no_grad():
        got = m(x.to("cuda")).float().cpu()
        ref = O.forward(w, cfg, x, training=False)           # fp32 everywhere, operands as stored: the reference's arithmetic

    def deltas(r):
        e = (got - r).abs()
        d = {"max_abs": e.max().item(), "max_rel": (e.max() / r.abs().max()).item(),
             "rms_rel": (e.pow(2).mean().sqrt() / r.pow(2).mean().sqrt()).item()}
        if seg:
            dg, dr = O.dice_loss(torch.sigmoid(got), y).item(), O.dice_loss(torch.sigmoid(r), y).item()
            d.update({"dice_gpu": dg, "dice_oracle": dr, "ddice": dg - dr})
        else:
            pg, pr = O.psnr(y, got), O.psnr(y, r)
            d.update({"psnr_gpu": pg.mean().item(), "psnr_oracle": pr.mean().item(), "dpsnr": (pg - pr).abs().max().item()})
        return d
    out = {"model": model_name, "B": B, "dtype": str(dtype).replace("torch.", ""), "attn_operands": operands,
           "mode": "eval forward vs fp32 CPU oracle"}
    out.update(deltas(ref))
    if dtype != torch.float32 or operands != "storage":
        # the same comparison against the oracle that rounds where this path rounds (bf16 where a tensor is stored, e4m3
        # operands): what is left is kernel error, the rest above is the number format
        with torch.no_grad():
            cfg_r = O.Config(**dict(kw, attn_operands=operands))
            ref_r = O.forward(w, cfg_r, x, training=False, storage=dtype if dtype != torch.float32 else None)
        out["vs_same_rounding_points"] = deltas(ref_r)
    del m
    return out


def self_launch(a) -> int:
    """`python bench.py --gpus N` with N > 1 (or VU_DP_FORCE=1) outside torchrun: start the N ranks as a CHILD process group
    (`python -m torch.distributed.run`, one rank per GPU over RCCL) before this process has made any GPU call, let rank 0's JSON
    line through on the inherited stdout, and return the child's exit code.  Never os.exec*: see the GPU box rules."""
    import socket
    import subprocess
    with socket.socket() as sk:                      # a free rendezvous port on the loopback interface
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def main():
    a = parse()
    if "WORLD_SIZE" not in os.environ and "RANK" not in os.environ and (a.gpus > 1 or os.environ.get("VU_DP_FORCE")):
        sys.exit(self_launch(a))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.global_batch:
        if a.global_batch % world:
            raise SystemExit(f"--global-batch {a.global_batch} is not a multiple of {world} ranks")
        a.batch = a.global_batch // world
    if a.gpus > 1 and world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} needs torchrun with {a.gpus} ranks (WORLD_SIZE={world})")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dp = world > 1 or bool(os.environ.get("VU_DP_FORCE"))     # VU_DP_FORCE=1: the RCCL path on one rank (under torchrun)
    if dp:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.distributed.init_process_group("nccl", device_id=dev)

    from vit_unet.torch import model as M
    from vit_unet.torch import _lib
    from vit_unet.torch.engine import TrainStep

    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    torch.manual_seed(0)                                   # identical initial weights on every rank
    seg = a.model == "seg512"
    operands = a.attn_operands or ("e4m3" if seg else "storage")
    if seg:
        model = M.get_vit_unet("base", dtype=dt, im_size=512, num_channels=1, attn_operands=operands).to(dev).train()
        g = torch.Generator(device="cpu").manual_seed(4321 + rank)
        x = torch.rand(a.batch, 1, 512, 512, generator=g)
        y = (torch.rand(a.batch, 1, 512, 512, generator=g) < 0.1).float()
    else:
        model = M.get_vit_unet(a.model, dtype=dt, attn_operands=operands).to(dev).train()
        g = torch.Generator(device="cpu").manual_seed(1234 + rank)
        y = torch.rand(a.batch, 3, 224, 224, generator=g)
        x = (y + 0.1 * torch.randn(y.shape, generator=g)).clamp(0, 1)
    x, y = x.to(dev), y.to(dev)
    if dp and a.collective == "c_abi":       # the library's own RCCL communicator (vu_dp_init) beside torch's process group
        from vit_unet.torch.engine import dp_c_abi_init
        dp_c_abi_init()
    ts = TrainStep(model, lr=1e-4, seed=1234 + rank, loss="dice" if seg else "mse",
                   grad_wire_dtype=torch.bfloat16 if a.grad_wire == "bf16" else None, collective=a.collective)
    # what the collective library itself reports, so that the driver can check "RCCL formed N ranks" against n_gpus
    comm = None
    if dp:
        comm = {"backend": torch.distributed.get_backend(), "ranks": torch.distributed.get_world_size(), "collective": a.collective,
                "buckets": len(ts._ubuckets), "bucket_mb": [round(sum(hi - lo for lo, hi in rs) * 4 / 2 ** 20, 1) for _, _, rs in ts._ubuckets]}
    # eager where the step has tails to fill (TrainStep.prefers_eager: Base at >= 40 images per GPU), a hipGraph elsewhere
    tail_overlap = ts.prefers_eager(a.batch) and not a.force_graph
    use_graph = not a.no_graph and not tail_overlap
    if use_graph and not dp:
        ts.capture(x, y)
        step = lambda: ts.replay()                          # noqa: E731  (inputs stay resident)
    elif use_graph:
        ts.capture_dp(x, y)                                 # one hipGraph per gradient bucket, collectives in between
        step = lambda: ts.replay()                          # noqa: E731
    else:
        step = lambda: ts.step(x, y)                        # noqa: E731

    def fence():
        torch.cuda.synchronize(dev)
        if dp:
            torch.distributed.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(a.warmup):
        step()
    fence()
    # the contract's clock: EXACTLY `steps` steps between two fences (barrier + device synchronize), max over ranks;
    # besides it, a HIP event after every step on the compute stream: the median per-step time
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(a.steps):
        step()
        evs[i + 1].record()
    fence()
    dt_s = time.perf_counter() - t0
    per_step = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(a.steps))
    med_ms = per_step[len(per_step) // 2]
    if dp:
        t = torch.tensor([dt_s], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt_s = t.item()
    dumped = None
    if a.dump_outputs and rank == 0:
        dumped = dump_outputs(a.dump_outputs, ts, model)      # before anything below runs another step
    loss = float(ts.loss.item())
    images = a.batch * world * a.steps
    value = images / dt_s
    # a short contract run (the driver's --steps 20 is 0.3 s of GPU work) says little about clocks and thermals: when the
    # timed region was under 2 s, a second, longer region of the same step is timed and reported beside it (`sustained`;
    # `value` / `steps` stay the contract's K steps)
    sustained = None
    if a.full and dt_s < a.sustained_s and not a.no_sustained:
        # (round 6: >= 8 s by default, so that a 5 s GPU-busy sampler beside the run sees the card working - the contract's
        # 20 steps are 0.2 s of a run whose wall clock is mostly the CPU baseline)
        n2 = int(min(4000, max(a.steps, a.sustained_s * 1.1 / (dt_s / a.steps))))
        fence()
        t1 = time.perf_counter()
        for _ in range(n2):
            step()
        fence()
        d2 = time.perf_counter() - t1
        if dp:
            t = torch.tensor([d2], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            d2 = t.item()
        sustained = {"steps": n2, "ms_per_step": d2 / n2 * 1e3, "value": a.batch * world * n2 / d2, "wall_s": d2}

    # PCIe-inclusive rates (never `value`): the same step fed from pinned host memory, (a) as the float32
    # CHW batch ImageFitter.unpack moves (dataset.py:78-91), (b) as decoded uint8 HWC images that the
    # device-side input pipeline (vu_denoise_prepare, train transform) turns into the batch
    host_in = None
    if a.full and rank == 0 and not dp and not a.no_host_input and not seg:
        from vit_unet.torch.dataset import DenoisingBatchTransform
        n_h = max(3, min(a.steps, 10))
        hx, hy = x.cpu().pin_memory(), y.cpu().pin_memory()
        hu = (y.cpu() * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().pin_memory()
        prep = DenoisingBatchTransform(224, train=True, seed=0)
        gx, gy = (ts._gx, ts._gy) if use_graph else (x, y)

        def step_f32():
            gx.copy_(hx, non_blocking=True)
            gy.copy_(hy, non_blocking=True)
            step()

        def step_u8():
            b = prep(hu, hu)
            gx.copy_(b["x"])
            gy.copy_(b["y"])
            step()
        host_in = {}
        for key, fn in (("float32_chw", step_f32), ("uint8_hwc_device_pipeline", step_u8)):
            fn()
            fence()
            t1 = time.perf_counter()
            for _ in range(n_h):
                fn()
            fence()
            host_in[key] = a.batch * n_h / (time.perf_counter() - t1)
        host_in["unit"] = "images/s"
        host_in["steps"] = n_h

    roof = None
    rep = None
    if a.full and not a.no_roofline:
        # extra instrumented steps: every rank runs them (they contain the gradient all-reduce), rank 0 with one HIP
        # event behind every launch on its compute stream
        L = _lib.lib()
        st = torch.cuda.current_stream(dev)
        torch.cuda.synchronize(dev)
        if rank == 0:
            L.vu_prof_enable(_lib.C.c_void_p(st.cuda_stream))
        # the gate holds the stream while the host enqueues the step, so an interval between two events is a launch, not a launch
        # plus the time the GPU waited for the eager host (16 images per GPU: ~390 launches of 5 - 20 us)
        gate_us = int(min(200000, 1300.0 * dt_s / a.steps * 1e3 + 3000))
        for _ in range(a.profile_steps):
            if rank == 0:
                _lib.check(L.vu_prof_gate(gate_us), "vu_prof_gate")
            ts.step(x, y)
        torch.cuda.synchronize(dev)
        if rank == 0:
            rep = json.loads(L.vu_prof_report().decode())
        if dp:
            torch.distributed.barrier()
    if rank == 0 and rep is not None:
        if True:
            if a.dump_profile:
                with open(a.dump_profile, "w") as f:
                    json.dump({k: dict(v, ms_per_step=v["ms"] / a.profile_steps) for k, v in
                               sorted(rep.items(), key=lambda kv: -kv[1]["ms"])}, f, indent=1)
            tot_ms = sum(v["ms"] for v in rep.values())
            top = sorted(rep.items(), key=lambda kv: -kv[1]["ms"])
            name, d = top[0]
            avg_s = d["ms"] / d["count"] * 1e-3
            if d["flops"] > 0:
                ach = d["flops"] / d["count"] / avg_s / 1e12
                strict = d.get("flops_strict", d["flops"]) / d["count"] / avg_s / 1e12
                roof = {"bound": "mfma", "achieved": ach, "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": ach / MFMA_PEAK_TFLOPS,
                        # SURVEY 8d's rule: the model's own products only (no recomputed logits / mixes, no padding)
                        "achieved_strict": strict, "frac_strict": strict / MFMA_PEAK_TFLOPS}
            else:
                ach = d["bytes"] / d["count"] / avg_s / 1e9
                roof = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS}
            traffic, tsrc = None, None
            try:      # HBM bytes per launch from the committed rocprofv3 --pmc passes (not collectable in-process)
                import glob
                for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic.json")))[::-1]:      # newest round first
                    pj = json.load(open(f))
                    wl = pj.get("workload", {"model": "base", "batch": 64})      # (the PMC passes run the default bench.py workload)
                    if wl.get("model") != a.model or wl.get("batch") != a.batch or wl.get("dtype", "bf16") != a.dtype:
                        continue          # counters of another workload say nothing about this launch: traffic stays null
                    # several template instances can share the name: the dominant launch is the one with most traffic
                    # (profiler tag -> kernel symbol: the fused delta + dq sweep of the 4-head form is an instantiation of flash_bwd_delta_kernel)
                    stem = name.split("<")[0].replace("flash_bwd_delta_dq_kernel", "flash_bwd_delta_kernel")
                    for sym, rec in pj["kernels"].items():
                        if stem in sym and rec.get("traffic_bytes") and rec["traffic_bytes"] > (traffic or 0):
                            traffic, tsrc = rec["traffic_bytes"], os.path.basename(f)
                    if traffic:
                        break
            except Exception:
                pass
            # the launch's bytes WITHOUT map-sized streams (q, k, v, dO, dq ... only): `traffic` minus this is what the probability
            # cache (design traffic, not algorithmic) and any re-reads cost
            roof["traffic_algorithmic"] = d.get("bytes_mapfree", d["bytes"]) / d["count"]
            roof.update({"traffic": traffic, "traffic_source": tsrc, "kernel": name, "avg_launch_us": avg_s * 1e6,
                         "launches_per_step": d["count"] / a.profile_steps,
                         "share_of_step": d["ms"] / tot_ms,
                         "step_mfma_frac": value / world * TRAIN_GFLOP_PER_IMG[a.model] / 1e3 / MFMA_PEAK_TFLOPS,
                         "top": [{"kernel": k, "ms_per_step": v["ms"] / a.profile_steps,
                                  "launches_per_step": v["count"] / a.profile_steps,
                                  "TFLOPs": (v["flops"] / (v["ms"] * 1e-3) / 1e12) if v["flops"] else None,
                                  "GBs": (v["bytes"] / (v["ms"] * 1e-3) / 1e9) if v["bytes"] else None}
                                 for k, v in top[:8]]})
    cpu, parity = None, None
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        parity = eval_parity(a.model, dt, B=1 if seg else 2, operands=operands)
        if not seg:
            cpu = cpu_baseline(a.model, host_cores())

    if rank == 0:
        shape, lossn = ("512x512x1", "Dice(sigmoid)") if seg else ("224x224x3", "MSELoss")
        mname = "Base@512" if seg else a.model.capitalize()
        out = {"metric": f"images/sec ({shape}) ViT_UNet-{mname} train step",
               "value": value, "unit": "images/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
               "ms_per_step": dt_s / a.steps * 1e3, "ms_per_step_median_hip_events": med_ms,
               "higher_is_better": True, "scaling": "strong" if a.global_batch else "weak",
               "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
               "config": {"workload": f"ViT_UNet-{mname} train step: forward + {lossn} + backward + "
                                      f"AdamW on synthetic " + ("CT-style 512x512x1 image/mask pairs" if seg else
                                                                "SIDD-style 224x224x3 noisy/clean pairs") + ", random-init weights",
                          "per_gpu_batch": a.batch, "global_batch": a.batch * world, "parallelism": f"dp{world}", "rccl_path": dp, "comm": comm, "grad_wire": a.grad_wire,
                          "hip_graph": use_graph, "tail_overlap": bool(not use_graph and ts.prefers_eager(a.batch)), "attn_operands": operands, "final_loss": loss},
               "roofline": roof, "cpu_baseline": cpu, "parity": parity, "host_input": host_in, "sustained": sustained,
               "workspace": model.workspace_report(a.batch), "full": a.full, "dumped_outputs": dumped}
        print(json.dumps(out), flush=True)
    if dp:
        # Leave without tearing the RCCL process group down: destroy_process_group() aborted intermittently in the GPU test
        # suite (the communicator's watchdog thread against captured graphs that still hold its stream), and an abort here
        # would turn a finished measurement into a failed run.  Every rank has passed the fences above and the line is out.
        torch.distributed.barrier()
        torch.cuda.synchronize()
        sys.stdout.flush(); sys.stderr.flush()
        os._exit(0)


if __name__ == "__main__":
    main()
