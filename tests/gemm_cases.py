"""Case table and exact reference for the GEMM route tests (tests/test_gemm_cases_cpu.py, tests/test_gpu_gemm_routes.py).

A helper module, not a conftest; it needs no GPU.

Exact arithmetic.  Operands are integers in {-2 .. 2}, the accumulate base integers in [-8, 8], the bias integers in [-4, 4],
alpha 1 or 0.5: all exact in bf16 and fp32.  With K <= 4100 every partial sum of a product, in any order, stays far below 2^24,
so fp32 accumulation is exact whatever the tile shape, k-split or atomic order: an fp32 result equals the float64 reference bit
for bit and a bf16 result is ONE round-to-nearest-even of an exactly known value.  No tolerance appears anywhere.

Routes.  Every case records the profiler tag of the kernel csrc/vu_gemm.hip (vu_gemm_launch) must pick for it.  The tile in the
tag is written down per case (derived by hand from launch_tiles, launch_layout and the three *_try functions); only the operand-form
letters are computed here, from the layout and the launcher's operand exchange (kernel_forms).  The k-step variant of the 32 x 64 and
32 x 32 routes is not in the tag: it follows K % 256, so those routes appear with K both ways.  Nor is the ring depth of the
64 x 64 tile (PD = 4 from K >= 512): ring64, quarter64 and plain64 assert the same "64x64".  A process-wide measurement switch
(VU_GEMM_RING, VU_GEMM_3232_BK, VU_GEMM_3264_BK) would therefore run the other variant unnoticed; the tests set none.
The scalar cases misalign A, B and C together (the bias stays aligned): forms with only one of vecA / vecB / vecC / vec8 cleared are
not covered here.

Layouts are the caller's, as in test_gemm_forms:
  NT: A (M, K) k-contiguous, B stored (N, K) k-contiguous;  NN: B stored (K, N) n-contiguous;  TT: A stored (K, M), B stored (K, N).
The tag's letters are the KERNEL's: T = the operand is row-contiguous (k-major image), after the exchange A <-> B where it happens.
"""
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

OPERAND_MAX, BASE_MAX, BIAS_MAX = 2, 8, 4      # |values| of operands(): what the exactness precondition is stated in
GUARD = 64              # sentinel elements in front of and behind every buffer (a multiple of 8: 16-byte alignment is kept)
ACC_SENTINEL = 12345.0  # guard value of accumulate outputs (plain outputs: NaN)


@dataclass(frozen=True)
class Case:
    name: str
    dtype: str                      # storage: "bf16" | "f32"
    c_float: int                    # 1: fp32 C on bf16 storage (fp32 storage: every C is fp32)
    layout: str                     # "NN" | "NT" | "TT" (caller's orientation, see above)
    M: int
    N: int
    K: int
    Z1: int
    Z2: int
    alpha: float
    bias: bool
    accumulate: int
    ldc: int
    tag: str                        # the one profiler tag the call must produce
    scalar: bool = False            # A, B and C start one element past a 16-byte boundary: no vector access anywhere
    ts_class: Optional[Tuple[int, int]] = None      # tall-skinny cases: the VU_TS(...) class pair
    note: str = ""

    @property
    def tdtype(self):
        return torch.bfloat16 if self.dtype == "bf16" else torch.float32

    @property
    def out_dtype(self):
        return torch.float32 if (self.c_float or self.dtype == "f32") else torch.bfloat16


def cdiv(a, b):
    return (a + b - 1) // b


def exchanged(M, N, Z, accumulate):
    """launch_layout: the operands change places (the kernel computes C^T) when the original N >= 64, except for products that may
    split K (accumulate with fewer than 512 tiles of 128 x 128)."""
    return N >= 64 and not (accumulate and cdiv(M, 128) * cdiv(N, 128) * Z < 512)


def kernel_forms(layout, swapped):
    ta, tb = {"NN": (False, True), "NT": (False, False), "TT": (True, True)}[layout]
    if swapped:
        ta, tb = tb, ta
    return ("T" if ta else "N") + ("T" if tb else "N")


def general_tag(dtype, c_float, layout, M, N, Z, accumulate, tile):
    t = "bf16" if dtype == "bf16" else "f32"
    tc = "f32" if (c_float or dtype == "f32") else "bf16"
    return f"vu_gemm_kernel<{t},{tc},{kernel_forms(layout, exchanged(M, N, Z, accumulate))},{tile}>"


# ---- general tiled kernel (csrc/vu_gemm.h) ------------------------------------------------------------------------------------
# (route, (M, N, K), bf16 tile, fp32 tile for NT / NN, fp32 tile for the accumulating TT form)
# The half-row (32 x 64), eighth (32 x 32) and quarter (64 x 64 below 200 big tiles) routes exist for bf16 only: fp32 storage takes
# the tile named in the fourth / fifth column instead (launch_tiles falls through to 64 x 64, 128 x 64 or 128 x 128).
GENERAL = [
    ("ring64",     (32, 48, 520),     "64x64",   "64x64",   "64x64"),      # M <= 32: off the half-row route; K >= 512: PD = 4
    ("half256",    (64, 48, 512),     "32x64",   "64x64",   "64x64"),      # k-step 256
    ("half256sw",  (300, 64, 768),    "32x64",   "64x64",   "128x64"),     # the swapped 768 -> 64 layer, k-step 256
    ("half64",     (300, 64, 520),    "32x64",   "64x64",   "128x64"),     # k-step 64 with ring
    ("eighth256",  (200, 128, 1024),  "32x32",   "128x128", "128x128"),    # k-step 256
    ("eighth64",   (200, 128, 1032),  "32x32",   "128x128", "128x128"),    # k-step 64 with ring
    ("quarter64",  (1024, 512, 1024), "64x64",   "128x128", "128x128"),    # M N K = 2^29: below the big-tile threshold; 128 tiles of 64 x 64
    ("big128",     (2560, 2560, 24),  "128x128", "128x128", "128x128"),    # 400 tiles, K too short for the big-tile kernel
    ("tile12864",  (200, 130, 70),    "128x64",  "128x128", "128x128"),    # test_gemm_forms' shapes with integer operands
    ("tile12832",  (130, 24, 196),    "128x32",  "128x32",  "128x32"),
    ("tile12832k", (64, 16, 3072),    "128x32",  "128x32",  "128x32"),
    ("plain64",    (49, 49, 24),      "64x64",   "64x64",   "64x64"),      # K < 512: plain prefetch
]
# bf16 storage, fp32 accumulating output, TT, shapes neither the skinny (K < 1024 or N % 8) nor the big-tile kernel takes
GENERAL_F32ACC = [
    ("acc12864",   (200, 130, 70),    "128x64"),
    ("acc3264sk",  (200, 130, 1000),  "32x64"),      # few big tiles with a float output: 32 x 64, K split two ways (float atomics)
    ("acc12832",   (130, 24, 196),    "128x32"),
    ("acc64",      (49, 49, 24),      "64x64"),
]
# many small batched products with one k-step (the per-(sample, head) products): head-slice strides, ldc = 56
BATCHED = ("heads64", (98, 49, 49), 8, 8, 56, "64x64")

# ---- tall-skinny weight-gradient kernel (csrc/vu_tsgemm.hip): class pair -> ((M, N), tag tile) --------------------------------
# One entry per VU_TS(...) instantiation of vu_tsgemm_try (sixteen with the one-tile 'halves' form of 192 x 192).  An output with
# M > 192 AND N > 192 (the 768-class squares) is no further instantiation: it is VU_TS(192, 192, ...) again with tiles in both
# directions, taken only when the model executor has lent a slab (vu_gemm_set_scratch), which no stand-alone entry point does.  What
# stays covered by the whole-model tests only is therefore the slab path and tsgemm_reduce_kernel, not a kernel instantiation.
TS_CLASSES = [
    ((32, 64), (24, 56), "32x64"), ((64, 32), (56, 24), "64x32"), ((64, 64), (56, 40), "64x64"),
    ((128, 32), (120, 24), "128x32"), ((32, 128), (24, 120), "32x128"), ((128, 64), (120, 56), "128x64"),
    ((64, 128), (56, 120), "64x128"), ((128, 128), (104, 120), "128x128"), ((192, 32), (136, 24), "192x32"),
    ((32, 192), (24, 136), "32x192"), ((192, 64), (136, 56), "192x64"), ((64, 192), (56, 136), "64x192"),
    ((192, 128), (136, 120), "192x128"), ((128, 192), (120, 136), "128x192"),
    ((192, 192), (184, 192), "192x96"),              # one tile: two column halves per K slice
    ((192, 192), (384, 192), "192x192"), ((192, 192), (192, 384), "192x192"),      # several tiles
]
TS_K = (1031, 2048)      # odd (ragged last slice and last 32-step) and even


def ts_side_class(n):
    return 32 if n <= 32 else (64 if n <= 64 else (128 if n <= 128 else 192))


def _build():
    cases = []

    def add(name, dtype, c_float, layout, M, N, K, tag, Z1=1, Z2=1, alpha=1.0, bias=False, accumulate=0, ldc=None, scalar=False,
            ts_class=None, note=""):
        cases.append(Case(name + ("-scalar" if scalar else ""), dtype, c_float, layout, M, N, K, Z1, Z2, alpha, bias, accumulate,
                          ldc if ldc is not None else N + 8, tag, scalar, ts_class, note))

    for scalar in (False, True):
        for route, (M, N, K), tb, tf, tfa in GENERAL:
            # bf16 storage and output: NT with alpha and bias (the Linear forward), NN plain (data gradient), TT with bias
            add(f"{route}-bf16-NT", "bf16", 0, "NT", M, N, K, general_tag("bf16", 0, "NT", M, N, 1, 0, tb), alpha=0.5, bias=True, scalar=scalar)
            add(f"{route}-bf16-NN", "bf16", 0, "NN", M, N, K, general_tag("bf16", 0, "NN", M, N, 1, 0, tb), scalar=scalar)
            add(f"{route}-bf16-TT", "bf16", 0, "TT", M, N, K, general_tag("bf16", 0, "TT", M, N, 1, 0, tb), bias=True, scalar=scalar)
            # fp32 storage: the accumulating TT form as the weight gradients use it
            note = "" if tf == tb else f"fp32 storage has no {tb} route here: {tf} (NT / NN), {tfa} (TT accumulate)"
            add(f"{route}-f32-NT", "f32", 0, "NT", M, N, K, general_tag("f32", 0, "NT", M, N, 1, 0, tf), alpha=0.5, bias=True, scalar=scalar, note=note)
            add(f"{route}-f32-NN", "f32", 0, "NN", M, N, K, general_tag("f32", 0, "NN", M, N, 1, 0, tf), scalar=scalar, note=note)
            add(f"{route}-f32-TT", "f32", 1, "TT", M, N, K, general_tag("f32", 1, "TT", M, N, 1, 1, tfa), accumulate=1, scalar=scalar, note=note)
        for route, (M, N, K), tile in GENERAL_F32ACC:
            add(f"{route}-bf16-TT", "bf16", 1, "TT", M, N, K, general_tag("bf16", 1, "TT", M, N, 1, 1, tile), accumulate=1, scalar=scalar)
        route, (M, N, K), Z1, Z2, ldc, tile = BATCHED
        for dtype in ("bf16", "f32"):
            add(f"{route}-{dtype}-NT", dtype, 0, "NT", M, N, K, general_tag(dtype, 0, "NT", M, N, Z1 * Z2, 0, tile), Z1=Z1, Z2=Z2, alpha=0.5,
                ldc=ldc, scalar=scalar)
            add(f"{route}-{dtype}-NN", dtype, 0, "NN", M, N, K, general_tag(dtype, 0, "NN", M, N, Z1 * Z2, 0, tile), Z1=Z1, Z2=Z2, ldc=ldc,
                scalar=scalar)

    for cls, (M, N), tile in TS_CLASSES:
        for K in TS_K:
            add(f"ts{cls[0]}x{cls[1]}-{M}x{N}-K{K}", "bf16", 1, "TT", M, N, K, f"vu_tsgemm_kernel<{tile}>", accumulate=1, ts_class=cls)
    # a misaligned operand makes the skinny kernel decline: the same product on the general kernel (split K, float atomics)
    add("ts64x64-56x40-K1031", "bf16", 1, "TT", 56, 40, 1031, general_tag("bf16", 1, "TT", 56, 40, 1, 1, "64x64"), accumulate=1, scalar=True)

    # persistent small-weight kernel (csrc/vu_pgemm.hip); tag letter: T = the weight is n-contiguous (caller's NN)
    for M, N, K in ((1031, 32, 192), (1031, 192, 32)):
        add(f"persist-N{N}K{K}-NT", "bf16", 0, "NT", M, N, K, f"vu_pgemm_kernel<N,N{N},K{K}>", bias=True)
        add(f"persist-N{N}K{K}-NN", "bf16", 0, "NN", M, N, K, f"vu_pgemm_kernel<T,N{N},K{K}>", bias=True)
    add("persist-N32K192-NT", "bf16", 0, "NT", 1031, 32, 192, general_tag("bf16", 0, "NT", 1031, 32, 1, 0, "128x32"), bias=True, scalar=True)

    # big-tile kernel (csrc/vu_bgemm.hip); the tile is what its tile-count rule gives: fewer than 257 tiles of 112 x 192 -> 112 x 64
    add("bigtile-shortK-NT", "bf16", 0, "NT", 1000, 2104, 136, "bgemm_kernel<NN,bf16,112x64>", bias=True, note="99 half tiles: 112x64")
    add("bigtile-shortK-NN", "bf16", 0, "NN", 1000, 2104, 136, "bgemm_kernel<NT,bf16,112x64>", bias=True, note="99 half tiles: 112x64")
    add("bigtile-default-NT", "bf16", 0, "NT", 1000, 1048, 1032, "bgemm_kernel<NN,bf16,112x64>", note="54 half tiles: 112x64")
    add("bigtile-default-NN", "bf16", 0, "NN", 1000, 1048, 1032, "bgemm_kernel<NT,bf16,112x64>", note="54 half tiles: 112x64")
    add("bigtile-wgrad-TT", "bf16", 1, "TT", 2048, 2056, 520, "bgemm_kernel<TT,f32 acc,224x192>", accumulate=1,
        note="m-contiguous A: always 224x192")
    add("bigtile-shortK-NT", "bf16", 0, "NT", 1000, 2104, 136, general_tag("bf16", 0, "NT", 1000, 2104, 1, 0, "128x64"), bias=True, scalar=True)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}


# ---- operands and reference -----------------------------------------------------------------------------------------------------
def operands(case):
    """Logical operands (fp32 tensors holding small integers): a (Z1, Z2, M, K), b (Z1, Z2, K, N), base (Z1, Z2, M, N) or None,
    bias (N) or None.  Fixed seed per case."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    Z = (case.Z1, case.Z2)
    a = torch.randint(-OPERAND_MAX, OPERAND_MAX + 1, Z + (case.M, case.K), generator=g).float()
    b = torch.randint(-OPERAND_MAX, OPERAND_MAX + 1, Z + (case.K, case.N), generator=g).float()
    base = torch.randint(-BASE_MAX, BASE_MAX + 1, Z + (case.M, case.N), generator=g).float() if case.accumulate else None
    bias = torch.randint(-BIAS_MAX, BIAS_MAX + 1, (case.N,), generator=g).float() if case.bias else None
    return a, b, base, bias


def reference(case, a, b, base, bias):
    """alpha * a b (+ bias) (+ base) in float64 - exact for these integers - as (Z1, Z2, M, N) in the output type."""
    r = case.alpha * (a.double() @ b.double())
    if bias is not None:
        r = r + bias.double()
    if base is not None:
        r = r + base.double()
    return r.float().to(case.out_dtype)      # (double -> float is exact here; float -> bf16 is one round-to-nearest-even)


# ---- buffers with guard bands ---------------------------------------------------------------------------------------------------
def pack(logical, dtype, pad, fill, shift=0):
    """Lays (Z1, Z2, R, Cc) out as rows of a (Z1, R, Z2 * Cc + pad) matrix - batch z2 is a column slice, as the heads of a (B, N, D)
    activation - inside a flat buffer with GUARD (+ shift) elements of `fill` in front, GUARD behind and `fill` in the row padding.
    Returns (flat buffer, offset of the first element, row stride, stride of z1, stride of z2)."""
    Z1, Z2, R, Cc = logical.shape
    ld = Z2 * Cc + pad
    body = torch.full((Z1, R, ld), fill, dtype=dtype)
    body[:, :, :Z2 * Cc] = logical.permute(0, 2, 1, 3).reshape(Z1, R, Z2 * Cc).to(dtype)
    flat = torch.cat([torch.full((GUARD + shift,), fill, dtype=dtype), body.reshape(-1), torch.full((GUARD,), fill, dtype=dtype)])
    return flat, GUARD + shift, ld, R * ld, Cc


def gemm_buffers(case, a, b, base, bias):
    """Everything a vu_gemm call of the case needs, on the CPU: flat A / B / C / bias buffers (NaN around and between the operand
    rows, the sentinel around and between the output rows) and the element strides.  A and B rows are padded by 8 elements."""
    dt = case.tdtype
    nan = float("nan")
    sh = 1 if case.scalar else 0
    d = {}
    if case.layout == "TT":      # A stored (K, M)
        d["A"], d["offA"], d["sAk"], d["sA1"], d["sA2"] = pack(a.transpose(-1, -2), dt, 8, nan, sh)
        d["sAm"] = 1
    else:
        d["A"], d["offA"], d["sAm"], d["sA1"], d["sA2"] = pack(a, dt, 8, nan, sh)
        d["sAk"] = 1
    if case.layout == "NT":      # B stored (N, K)
        d["B"], d["offB"], d["sBn"], d["sB1"], d["sB2"] = pack(b.transpose(-1, -2), dt, 8, nan, sh)
        d["sBk"] = 1
    else:
        d["B"], d["offB"], d["sBk"], d["sB1"], d["sB2"] = pack(b, dt, 8, nan, sh)
        d["sBn"] = 1
    # C: (Z1, Z2, M, ldc) row-major, every batch its own rows
    sent = ACC_SENTINEL if case.accumulate else nan
    body = torch.full((case.Z1, case.Z2, case.M, case.ldc), sent, dtype=case.out_dtype)
    if base is not None:
        body[..., :case.N] = base.to(case.out_dtype)
    d["C"] = torch.cat([torch.full((GUARD + sh,), sent, dtype=case.out_dtype), body.reshape(-1), torch.full((GUARD,), sent, dtype=case.out_dtype)])
    d["offC"], d["sC1"], d["sC2"], d["sentinel"] = GUARD + sh, case.Z2 * case.M * case.ldc, case.M * case.ldc, sent
    if bias is not None:
        d["bias"] = torch.cat([torch.full((GUARD,), nan), bias, torch.full((GUARD,), nan)])
        d["offBias"] = GUARD
    return d


def bits(t):
    """The elements' bit patterns as integers."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])
