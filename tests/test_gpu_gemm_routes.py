"""Every kernel route of vu_gemm_launch (csrc/vu_gemm.hip) stand-alone, through the C ABI, in exact arithmetic.

The cases, their integer operands and the float64 reference come from tests/gemm_cases.py (its docstring has the argument for
exactness; tests/test_gemm_cases_cpu.py checks it).  For each case:
  * the launch profiler must name exactly the kernel the case records - one launch, nothing else (the tag shows neither the
    k-step nor the ring depth: those follow from K alone, see gemm_cases.py);
  * the result equals the reference bit for bit (fp32) or after one round-to-nearest-even (bf16): torch.equal, no tolerance;
  * the output lies inside a larger buffer: 64 sentinel elements in front and behind and the padding columns of every row
    (ldc > N) must keep their bit patterns - NaN for plain outputs, 12345.0 for accumulating ones;
  * A and B lie inside NaN: in front, behind and in the 8 padding elements of every row.  A NaN (or a 0 * NaN of a "zeroed"
    k-slot) that reached any sum would show in the result.
The FeedForward epilogues (GELU with its saved pre-activation, dropout, bias, the bias gradients' column sums) on the 32 x 32 and
32 x 64 routes follow at the end, against the oracle, with the bounds of the existing FeedForward tests.
"""
import ctypes as C
import json

import pytest
import torch

import gemm_cases as G
import vit_unet_oracle as O
from vit_unet.torch import _lib
from vit_unet.torch import model as M
from vit_unet.torch._lib import check, lib, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def serr(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def _profiled(fn):
    L = lib()
    torch.cuda.synchronize()
    L.vu_prof_enable(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    try:
        fn()
    finally:
        rep = json.loads(L.vu_prof_report().decode())      # (waits for the stream and switches the profiler off)
    return rep


@pytest.mark.parametrize("case", G.CASES, ids=[c.name for c in G.CASES])
def test_gemm_route_exact_with_guard_bands(case):
    a, b, base, bias = G.operands(case)
    ref = G.reference(case, a, b, base, bias)
    h = G.gemm_buffers(case, a, b, base, bias)
    A, Bm, Cb = h["A"].to(DEV), h["B"].to(DEV), h["C"].to(DEV)
    biasd = h["bias"].to(DEV) if case.bias else None
    code = _lib.DTYPE_CODE[case.tdtype]

    def call():
        check(lib().vu_gemm(code, case.c_float, ptr(A[h["offA"]:]), ptr(Bm[h["offB"]:]), ptr(Cb[h["offC"]:]), case.M, case.N, case.K,
                            h["sAm"], h["sAk"], h["sBk"], h["sBn"], case.ldc, case.Z1, case.Z2, h["sA1"], h["sA2"], h["sB1"], h["sB2"],
                            h["sC1"], h["sC2"], case.alpha, ptr(biasd[h["offBias"]:]) if case.bias else None, case.accumulate,
                            _lib.stream_ptr()))

    rep = _profiled(call)
    assert {k: v["count"] for k, v in rep.items()} == {case.tag: 1}, (case.name, list(rep))

    got = Cb.cpu()
    off, n = h["offC"], case.Z1 * case.Z2 * case.M * case.ldc
    sent = G.bits(torch.tensor([h["sentinel"]], dtype=case.out_dtype))[0]
    body = got[off:off + n].view(case.Z1, case.Z2, case.M, case.ldc)
    assert torch.equal(body[..., :case.N], ref), f"{case.name}: result differs from the exact reference in " \
        f"{(body[..., :case.N] != ref).sum().item()} of {ref.numel()} elements"
    assert bool((G.bits(got[:off]) == sent).all()), f"{case.name}: front guard written"
    assert bool((G.bits(got[off + n:]) == sent).all()), f"{case.name}: tail guard written"
    if case.ldc > case.N:
        assert bool((G.bits(body[..., case.N:]) == sent).all()), f"{case.name}: padding columns written"
    # the operands and the bias were only read
    assert torch.equal(G.bits(A.cpu()), G.bits(h["A"])) and torch.equal(G.bits(Bm.cpu()), G.bits(h["B"]))


# ---- FeedForward epilogues on the level-0 / level-1 routes -----------------------------------------------------------------------
@pytest.mark.parametrize("drop", [0.0, 0.3])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,D,hid", [(200, 3072, 128), (200, 768, 64)])
def test_feedforward_level0_level1_routes_vs_oracle(rows, D, hid, dt, drop):
    """vu_ff_forward / vu_ff_backward at the model's real level-0 (3072 -> 128) and level-1 (768 -> 64) widths, where the first
    product rides on the 32 x 32 / 32 x 64 tiles of the general kernel (bf16; fp32 storage has no such route and takes its
    128 x 128 / 64 x 64 tiles): GELU with its saved pre-activation, both dropout sites, the biases and the bias gradients' column
    sums against the oracle on the storage-rounded operands.  Bounds: those of test_feedforward_module_vs_golden (fp32),
    test_feedforward_fused_level2_vs_oracle (bf16, no dropout) and test_feedforward_linear_drop_vs_oracle (bf16 with dropout)."""
    B, N = 2, rows // 2
    gen = torch.Generator().manual_seed(D + hid)
    ff = M.FeedForward(D, hid, drop).to(DEV).train()
    x = torch.randn(B, N, D, generator=gen)
    dy = torch.randn(B, N, D, generator=gen).to(dt)
    xd = x.to(dt).to(DEV).requires_grad_(True)

    def run():
        out = ff(xd, seed=5, stream_id=2)
        out.backward(dy.to(DEV))
        run.out = out

    rep = _profiled(run)
    out = run.out
    assert not any("hipblaslt" in k or k.startswith("Cijk") for k in rep), rep.keys()
    t = "bf16" if dt == torch.bfloat16 else "f32"
    first = {(torch.bfloat16, 3072): "32x32", (torch.bfloat16, 768): "32x64", (torch.float32, 3072): "128x128", (torch.float32, 768): "64x64"}[(dt, D)]
    # x (rows, D) W1^T: hid >= 64 columns, so the launcher exchanges the operands; both are k-contiguous.  For bf16 no other product
    # of the layer can give this tag (fp32 has one tile for most shapes, its tag only shows the general kernel ran): the second forward product and dx have K = hid < 512, dh has an n-contiguous operand (a T in the
    # tag), and the weight gradients have a float output.
    assert rep.get(f"vu_gemm_kernel<{t},{t},NN,{first}>", {}).get("count", 0) >= 1, rep.keys()
    p = {"net.0.weight": ff.net[0].weight.detach().cpu().to(dt).float().requires_grad_(True),
         "net.0.bias": ff.net[0].bias.detach().cpu().clone().requires_grad_(True),
         "net.3.weight": ff.net[3].weight.detach().cpu().to(dt).float().requires_grad_(True),
         "net.3.bias": ff.net[3].bias.detach().cpu().clone().requires_grad_(True)}
    xr = x.to(dt).float().requires_grad_(True)
    ref = O.feed_forward(xr, p, "", training=True, linear_drop=drop, seed=5, stream=2, storage=dt)
    ref.backward(dy.float())
    if dt == torch.float32:
        ft, bt = 2e-5, 2e-4
    else:
        ft, bt = (1e-2, 2e-2) if drop == 0.0 else (3e-2, 5e-2)
    errs = {"out": serr(out.float(), ref), "dx": serr(xd.grad.float(), xr.grad)}
    for k, q in ff.net.named_parameters():
        errs[k] = serr(q.grad, p["net." + k].grad)
    print(f"feedforward rows {rows} D {D} hid {hid} {t} drop {drop}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    if drop > 0:
        assert (out == 0).float().mean().item() > 0.2                  # the output dropout really dropped
    assert errs["out"] < ft, errs
    for k, v in errs.items():
        assert k == "out" or v < bt, (k, errs)
