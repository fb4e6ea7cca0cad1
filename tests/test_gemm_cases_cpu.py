"""The GEMM route case table (tests/gemm_cases.py) checked on the CPU: the exactness precondition of every case, the float64
reference against an int64 recomputation, unique names, a tag on every case, and every tall-skinny class pair present."""
import re

import pytest
import torch

import gemm_cases as G

IDS = [c.name for c in G.CASES]


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_exactness_precondition(case):
    """|operands| <= OPERAND_MAX, |base| <= BASE_MAX, |bias| <= BIAS_MAX (the ranges operands() draws from): every partial sum of the product, in any order, and the finished element are
    integers (or halves, alpha = 0.5) below 2^24 in magnitude: fp32 accumulation cannot round."""
    assert case.alpha in (1.0, 0.5)
    assert case.K * G.OPERAND_MAX ** 2 * max(1.0, case.alpha) + G.BASE_MAX + G.BIAS_MAX < 2 ** 24
    a, b, base, bias = G.operands(case)
    for t, lim in ((a, G.OPERAND_MAX), (b, G.OPERAND_MAX), (base, G.BASE_MAX), (bias, G.BIAS_MAX)):
        if t is not None:
            assert t.abs().max().item() <= lim and torch.equal(t, t.round())
            assert torch.equal(t.to(case.tdtype).float(), t)             # exact in the storage type
    assert (base is not None) == bool(case.accumulate) and (bias is not None) == case.bias


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_reference_is_exact(case):
    """The float64 reference equals an int64 recomputation on a sample of rows and columns (first, last, a few inside); the value
    the test compares with is that integer result after ONE rounding to the output type."""
    a, b, base, bias = G.operands(case)
    g = torch.Generator().manual_seed(1)
    rows = torch.unique(torch.cat([torch.tensor([0, case.M - 1]), torch.randint(0, case.M, (6,), generator=g)]))
    cols = torch.unique(torch.cat([torch.tensor([0, case.N - 1]), torch.randint(0, case.N, (6,), generator=g)]))
    # (the reference is row by row: the sampled rows of A and of the base give the sampled rows of the result)
    ref = G.reference(case, a[:, :, rows], b, None if base is None else base[:, :, rows], bias)
    assert ref.shape == (case.Z1, case.Z2, len(rows), case.N) and ref.dtype == case.out_dtype
    ref = ref[:, :, :, cols]
    ai, bi = a.long()[:, :, rows, :], b.long()[:, :, :, cols]
    twice = 2 * (ai @ bi) if case.alpha == 1.0 else ai @ bi              # 2 x the exact value: an integer for alpha = 0.5 too
    if bias is not None:
        twice = twice + 2 * bias.long()[cols]
    if base is not None:
        twice = twice + 2 * base.long()[:, :, rows][:, :, :, cols]
    exact = twice.double() / 2
    assert exact.abs().max().item() < 2 ** 23
    assert torch.equal(exact.float().to(case.out_dtype), ref)
    if case.out_dtype == torch.float32:
        assert torch.equal(ref.double(), exact)


def test_names_unique_and_tags_present():
    assert len(set(IDS)) == len(IDS)
    pat = re.compile(r"^(vu_gemm_kernel<(bf16|f32),(bf16|f32),[NT][NT],\d+x\d+>|vu_tsgemm_kernel<\d+x\d+>|"
                     r"vu_pgemm_kernel<[NT],N\d+,K\d+>|bgemm_kernel<[NT][NT],(bf16|f32 acc),\d+x\d+>)$")
    for c in G.CASES:
        assert pat.match(c.tag), (c.name, c.tag)
        if c.scalar:
            assert c.tag.startswith("vu_gemm_kernel<"), c.name       # nothing but the general kernel takes unaligned operands
        assert c.ldc >= c.N and c.layout in ("NN", "NT", "TT") and c.dtype in ("bf16", "f32")


def test_every_tall_skinny_class_has_cases():
    """All sixteen VU_TS(...) instantiations of vu_tsgemm_try (192 x 192 twice: the one-tile 'halves' form and the several-tile
    form; its slab path for M, N > 192 needs the model executor), each with an odd and an even K, and each shape really inside its class."""
    pairs = [(32, 64), (64, 32), (64, 64), (128, 32), (32, 128), (128, 64), (64, 128), (128, 128), (192, 32), (32, 192),
             (192, 64), (64, 192), (192, 128), (128, 192), (192, 192)]
    ts = [c for c in G.CASES if c.ts_class is not None and not c.scalar]
    for c in ts:
        assert (G.ts_side_class(c.M), G.ts_side_class(c.N)) == c.ts_class, c.name
        assert c.M % 8 == 0 and c.N % 8 == 0 and c.K >= 1024 and not (c.M > 192 and c.N > 192), c.name
        assert c.dtype == "bf16" and c.c_float and c.accumulate and c.layout == "TT" and c.alpha == 1.0 and not c.bias
    for p in pairs:
        ks = {c.K for c in ts if c.ts_class == p}
        assert any(k % 2 for k in ks) and any(k % 256 == 0 for k in ks), (p, ks)
    tiles = {c.tag for c in ts if c.ts_class == (192, 192)}
    assert tiles == {"vu_tsgemm_kernel<192x96>", "vu_tsgemm_kernel<192x192>"}
    assert len({c.tag for c in ts}) == 16
