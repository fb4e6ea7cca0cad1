"""Multi-process tests of the data-parallel path.  They collect LAST (file name): a red multi-process rehearsal must never
again hide the per-op parity tests behind `pytest -x` (round 3: 507 tests unreached).  Each one starts child processes; the
parity tests proper are in the files that sort before this one, the hot-path ones first (tests/test_a_hotpath_gpu.py)."""
import os

import pytest

pytestmark = pytest.mark.gpu


def test_dp_path_one_rank_rccl_matches_single_gpu_step(golden_dir):
    """The data-parallel choreography (NCCL process group, bucketed all-reduces on the side stream, 1/world folded into
    AdamW, per-bucket hipGraphs) on ONE rank over RCCL (VU_DP_FORCE=1) must reproduce the plain single-GPU fused step.
    Runs in a child process (tests/dp_one_rank_worker.py): tearing an RCCL process group down inside a long-lived pytest
    process aborted intermittently in destroy_process_group (its watchdog thread against captured graphs that still hold
    the communicator's stream); the worker reports and leaves with os._exit, so no teardown runs at all."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VU_DP_FORCE="1")
    r = subprocess.run([sys.executable, os.path.join(here, "dp_one_rank_worker.py"), golden_dir],
                       capture_output=True, text=True, timeout=600, env=env)
    assert "DP_ONE_RANK_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_two_rank_data_parallel_rehearsal():
    """Two ranks of the real engine on this one GPU (fresh child processes under torch.distributed.run; gloo moves the
    CUDA buckets because RCCL cannot put two ranks on one device): every rank ends with bit-identical parameters, equal to
    a single-process reference that averages both ranks' autograd gradients and steps torch.optim.AdamW."""
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(root, "tools", "dp_rehearsal.py")],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("identical parameters across ranks: True") == 2
    # the same two ranks on the Base preset in bf16 (recompute attention at level 2, dropout on), one step: identical
    # parameters, and the all-reduced gradient arena is bit for bit the sum of the two ranks' stand-alone gradients
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(root, "tools", "dp_rehearsal.py"), "--base"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("identical parameters across ranks: True") == 2
    assert "bit for bit: True" in r.stdout


def test_c_abi_allreduce_matches_torch_on_two_gpus():
    """SURVEY 8b's comm entry points with MORE than one rank (round-5 advice: the one-rank test cannot tell a sum from a no-op):
    vu_dp_allreduce_bucket against torch.distributed.all_reduce on two GPUs, fp32 and bf16, bit for bit.  Needs two devices: skipped
    on the one-GPU boxes this suite normally runs on."""
    import socket
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    here = os.path.dirname(os.path.abspath(__file__))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(here, "dp_two_rank_cabi_worker.py")],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.count("C_ABI_OK") == 2, r.stdout[-2000:] + r.stderr[-3000:]


def test_ops_are_bit_reproducible_while_another_process_uses_the_gpu():
    """Round 4 root cause of the red rehearsal: with a SECOND PROCESS computing on the same GPU the q / k / v convolution
    forward (scalar-load weight path, csrc/vu_conv.hip) returned wrong values for whole waves in 4 - 10 % of its launches -
    invisible on an idle GPU.  tools/contention_ops.py runs every stand-alone op of a Base level back to back under such a load
    and compares each repetition's output bytes with the first; the weights now come through LDS and every op must be clean."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    # (round 4's counts - 45 s of load, 120 repetitions per op - under VU_SHARING_LONG=1; the default keeps the driver's suite inside
    # its 10 minutes.  The ops include the round-6 Toeplitz / Gram convolution kernels: the forward / data gradient at patch 16 and 8
    # take them by default, the weight gradient is in the list with a lent scratch slab.)
    load, iters = ("45", "120") if os.environ.get("VU_SHARING_LONG") else ("25", "60")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "contention_ops.py"), "--load", load, "--iters", iters],
                       capture_output=True, text=True, timeout=420, env=env)
    assert "CONTENTION_OPS CLEAN" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0


def test_four_head_recompute_attention_under_gpu_sharing():
    """The same check for the recompute attention op at Lite's two long-row levels (4 heads, d = 12 / 48) and at Base level 2
    (8 heads).  Round 4 found the 4-head backward NOT reproducible beside a load process: delta - and with it dq, dk - of 1 - 2 % of
    the 16-query tiles off in the last bits, everything else identical (tools/attn_ws_diff.py); the cause was traced to the rows
    of the transposed-mix table being prefetched from an LDS struct inside the head loop of the delta / dq / dk sweeps; with the
    table in registers every buffer is identical again."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", CONTENTION_ATTN_ONLY="1")
    # (VU_SHARING_LONG=1: round 4's 60 s / 30 repetitions.  The 8-head case runs the training forward + backward with the probability
    # cache on - the round-5 cached sweeps, their LDS-DMA rings included - because that is the op's default.)
    load, iters = ("60", "30") if os.environ.get("VU_SHARING_LONG") else ("30", "12")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "contention_ops.py"), "--load", load, "--iters", iters, "--B", "16", "--attn", "all"],
                       capture_output=True, text=True, timeout=420, env=env)
    assert "CONTENTION_OPS CLEAN" in r.stdout, r.stdout[-2000:]


def test_bench_launches_its_own_ranks_over_rccl():
    """`python bench.py --gpus N` as the driver calls it (no torchrun around it): bench.py starts its ranks itself as a child
    `python -m torch.distributed.run` before touching the GPU and relays rank 0's line.  On this one-GPU box: VU_DP_FORCE=1 sends
    --gpus 1 through that path - the line must report the RCCL process group it formed; and --gpus 2 must fail with the CHILD's
    error (no second device), not with a message about torchrun."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", VU_DP_FORCE="1")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--full",
                        "--no-cpu-baseline", "--no-host-input", "--no-sustained"], capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["config"]["rccl_path"] is True
    comm = out["config"]["comm"]
    assert comm["backend"] == "nccl" and comm["ranks"] == 1 and comm["buckets"] >= 1
    assert out["value"] > 0 and out["roofline"] is not None
    import torch
    if torch.cuda.device_count() == 1:
        env.pop("VU_DP_FORCE")
        r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline",
                             "--no-roofline"], capture_output=True, text=True, timeout=300, env=env)
        assert r2.returncode != 0
        assert "needs torchrun" not in (r2.stdout + r2.stderr)
