"""Whole-image restoration on the GPU (csrc/vu_tile.hip, vit_unet/torch/restore.py).

Per op, through the C ABI with NaN-filled outputs, against the numpy restatement of tests/test_restore_cpu.py:
  vu_tile_gather_u8 / _f32   byte / copy work: BIT-EXACT (the u8 form against the oracle's validation transform of the
                             numpy-cut windows)
  vu_tile_blend              |out - ref| <= 2e-6 max|v| against the float64 blend.  Derivation: at most 9 terms; each weight
                             carries 2 roundings and each product 1, the two running sums at most 8 each, one division:
                             about 22 units of 2^-24 = 1.3e-6 relative to sum(w |v|) / sum(w) <= max|v|.  out_u8 equals
                             clamp(floor(255 ref + 0.5)) wherever 255 ref is farther than 255 * 2e-6 * max|v| from a .5
                             boundary; closer pixels may differ by one level and are left out (at most 1 % of them).
End to end: TiledRestorer against the same composition done by hand (numpy plan, the product's own eval forward on the
same chunks, float64 blend) with the blend's bound - the window outputs are the same numbers - and, for the fp32 model,
against the CPU oracle's eval forward per window with the bound of tests/test_gpu_model.py::test_tiny_golden_fp32 (2e-4
of the output scale).  That file has no eval parity test against the oracle for bf16 storage, so none is made up here."""
import numpy as np
import pytest
import torch

import vit_unet_oracle as O
from test_restore_cpu import ref_axis, ref_blend, ref_windows_hwc
from vit_unet.torch import _lib, functions as F
from vit_unet.torch import model as M
from vit_unet.torch._lib import check, lib, ptr
from vit_unet.torch.restore import TiledRestorer, tile_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLEND_TOL = 2e-6

# (H, W, C, T, overlap): both axes larger than T with inward-shifted last windows whose origins (51, 89) are not
# multiples of 4; one axis smaller; both smaller; L == 1; L == T; W not a multiple of 4; T = 224
SHAPES = [(83, 121, 3, 32, 8), (20, 70, 3, 32, 5), (7, 9, 1, 32, 16), (1, 33, 3, 32, 0), (40, 1, 1, 32, 4), (32, 32, 3, 32, 16),
          (64, 96, 1, 32, 0), (100, 64, 3, 32, 16), (500, 300, 3, 224, 32), (100, 450, 1, 224, 112), (224, 224, 3, 224, 32)]


def st():
    return _lib.stream_ptr()


def nwin(H, W, T, ov):
    return len(ref_axis(H, T, ov)) * len(ref_axis(W, T, ov))


def image_u8(H, W, Cn, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, Cn), dtype=np.uint8)


def test_plan_has_the_unaligned_shifted_window():
    oy, ox = tile_plan(83, 121, 32, 8)
    assert oy[-1] == 51 and ox[-1] == 89 and oy[-1] % 4 and ox[-1] % 4


# ---------------------------------------------------------------- 3. gather
@pytest.mark.parametrize("H,W,Cn,T,ov", SHAPES)
def test_tile_gather_u8_bit_exact(H, W, Cn, T, ov):
    img = image_u8(H, W, Cn, seed=H + W)
    win = ref_windows_hwc(img, T, ov)                                   # (nt,T,T,C) crop / reflect by numpy indexing
    nt = win.shape[0]
    assert nt == nwin(H, W, T, ov)
    ref = O.denoise_prepare(win, win, T, None)[0]                       # the validation transform of every window
    d = torch.from_numpy(img).to(DEV)
    got = torch.full((nt, Cn, T, T), float("nan"), device=DEV)
    check(lib().vu_tile_gather_u8(ptr(d), ptr(got), H, W, Cn, T, ov, 0, nt, 0.456, 0.224, st()))
    assert torch.equal(got.cpu(), ref), (got.cpu() - ref).abs().max()
    if nt > 2:                                                          # a range inside the plan: windows [1, nt - 1)
        part = torch.full((nt - 2, Cn, T, T), float("nan"), device=DEV)
        check(lib().vu_tile_gather_u8(ptr(d), ptr(part), H, W, Cn, T, ov, 1, nt - 2, 0.456, 0.224, st()))
        assert torch.equal(part.cpu(), ref[1:nt - 1])
    # other normalisation constants, and an output that is not 16-byte aligned (scalar stores)
    ref2 = O.denoise_prepare(win, win, T, None, mean=0.3, std=0.5)[0]
    buf = torch.full((nt * Cn * T * T + 1,), float("nan"), device=DEV)
    off = buf[1:].view(nt, Cn, T, T)
    check(lib().vu_tile_gather_u8(ptr(d), ptr(off), H, W, Cn, T, ov, 0, nt, 0.3, 0.5, st()))
    assert torch.equal(off.cpu(), ref2) and torch.isnan(buf[0])


@pytest.mark.parametrize("T,Cn", [(32, 3), (32, 1), (224, 3)])
def test_tile_gather_u8_of_a_model_sized_image_is_the_validation_transform(T, Cn):
    from vit_unet.torch.dataset import DenoisingBatchTransform
    img = image_u8(T, T, Cn, seed=T)
    d = torch.from_numpy(img).to(DEV)
    got = torch.full((1, Cn, T, T), float("nan"), device=DEV)
    check(lib().vu_tile_gather_u8(ptr(d), ptr(got), T, T, Cn, T, 8, 0, 1, 0.456, 0.224, st()))
    want = DenoisingBatchTransform(T, train=False)(img[None], img[None])["x"]
    assert torch.equal(got, want)


@pytest.mark.parametrize("H,W,Cn,T,ov", SHAPES)
def test_tile_gather_f32_bit_exact(H, W, Cn, T, ov):
    rng = np.random.default_rng(H * W)
    img = rng.standard_normal((Cn, H, W)).astype(np.float32)
    ref = torch.from_numpy(np.ascontiguousarray(ref_windows_hwc(img.transpose(1, 2, 0), T, ov).transpose(0, 3, 1, 2)))
    nt = ref.shape[0]
    d = torch.from_numpy(img).to(DEV)
    got = torch.full((nt, Cn, T, T), float("nan"), device=DEV)
    check(lib().vu_tile_gather_f32(ptr(d), ptr(got), H, W, Cn, T, ov, 0, nt, st()))
    assert torch.equal(got.cpu(), ref)
    # an image that is not 16-byte aligned, and the last window alone
    buf = torch.zeros(img.size + 1, device=DEV)
    buf[1:].copy_(d.reshape(-1))
    got2 = torch.full((1, Cn, T, T), float("nan"), device=DEV)
    check(lib().vu_tile_gather_f32(ptr(buf[1:].view(Cn, H, W)), ptr(got2), H, W, Cn, T, ov, nt - 1, 1, st()))
    assert torch.equal(got2.cpu(), ref[nt - 1:])


# ---------------------------------------------------------------- 4. blend
def check_u8(got_u8, ref64, vmax, what=""):
    """got (H,W,C) uint8 against clamp(floor(255 ref + 0.5)) on every pixel whose 255 ref is farther than
    255 * 2e-6 * max|v| from a .5 boundary; the left-out share may not exceed 1 %."""
    s = 255.0 * ref64.transpose(1, 2, 0)
    want = np.clip(np.floor(s + 0.5), 0, 255)
    near = np.abs(s - np.floor(s) - 0.5) <= 255.0 * BLEND_TOL * vmax
    share = near.mean()
    print(f"{what} u8: left out {100 * share:.3f} % of {s.size} values")
    assert share <= 0.01, share
    g = got_u8.cpu().numpy().astype(np.float64)
    assert np.array_equal(g[~near], want[~near]), np.abs(g - want)[~near].max()
    assert np.abs(g - want).max() <= 1


@pytest.mark.parametrize("H,W,Cn,T,ov", SHAPES)
def test_tile_blend_against_float64(H, W, Cn, T, ov):
    nt = nwin(H, W, T, ov)
    tiles = np.random.default_rng(nt + H).uniform(0, 1, (nt, Cn, T, T)).astype(np.float32)
    ref = ref_blend(tiles, H, W, T, ov)
    vmax = float(np.abs(tiles).max())
    d = torch.from_numpy(tiles).to(DEV)
    out = torch.full((Cn, H, W), float("nan"), device=DEV)
    u8 = torch.full((H, W, Cn), 77, dtype=torch.uint8, device=DEV)
    check(lib().vu_tile_blend(ptr(d), ptr(out), ptr(u8), H, W, Cn, T, ov, st()))
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max()
    print(f"blend {H}x{W}x{Cn} T {T} overlap {ov}: max err {err:.3e} (bound {BLEND_TOL * vmax:.3e})")
    assert torch.isfinite(out).all() and err <= BLEND_TOL * vmax, err
    check_u8(u8, ref, vmax, f"blend {H}x{W}x{Cn}")
    # either output alone gives the same bits, and so does a second run (a gather: no atomics)
    out2 = torch.full((Cn, H, W), float("nan"), device=DEV)
    u82 = torch.zeros((H, W, Cn), dtype=torch.uint8, device=DEV)
    check(lib().vu_tile_blend(ptr(d), ptr(out2), None, H, W, Cn, T, ov, st()))
    check(lib().vu_tile_blend(ptr(d), None, ptr(u82), H, W, Cn, T, ov, st()))
    assert torch.equal(out, out2) and torch.equal(u8, u82)
    # signed values of another scale, outputs that are not 16-byte / 4-byte aligned
    tiles2 = (tiles * 60 - 30).astype(np.float32)
    d2 = torch.from_numpy(tiles2).to(DEV)
    fb = torch.full((Cn * H * W + 1,), float("nan"), device=DEV)
    ub = torch.zeros(H * W * Cn + 1, dtype=torch.uint8, device=DEV)
    check(lib().vu_tile_blend(ptr(d2), ptr(fb[1:].view(Cn, H, W)), ptr(ub[1:].view(H, W, Cn)), H, W, Cn, T, ov, st()))
    ref2 = ref_blend(tiles2, H, W, T, ov)
    assert np.abs(fb[1:].view(Cn, H, W).cpu().numpy().astype(np.float64) - ref2).max() <= BLEND_TOL * float(np.abs(tiles2).max())
    assert torch.isnan(fb[0]) and ub[0] == 0
    g = ub[1:].view(H, W, Cn).cpu().numpy()
    s = ref2.transpose(1, 2, 0)
    assert (g[s < -0.01] == 0).all() and (g[s > 1.01] == 255).all()      # clamped on both sides


@pytest.mark.parametrize("H,W,Cn,T", [(64, 96, 3, 32), (32, 32, 1, 32), (448, 224, 3, 224)])
def test_tile_blend_of_disjoint_windows_is_bit_exact(H, W, Cn, T):
    """overlap = 0 and H, W multiples of T: one covering window of weight 1 per pixel, so out = (0 + 1 v) / 1 = v."""
    img = np.random.default_rng(W).standard_normal((Cn, H, W)).astype(np.float32)
    d = torch.from_numpy(img).to(DEV)
    nt = (H // T) * (W // T)
    tiles = torch.full((nt, Cn, T, T), float("nan"), device=DEV)
    check(lib().vu_tile_gather_f32(ptr(d), ptr(tiles), H, W, Cn, T, 0, 0, nt, st()))
    out = torch.full((Cn, H, W), float("nan"), device=DEV)
    check(lib().vu_tile_blend(ptr(tiles), ptr(out), None, H, W, Cn, T, 0, st()))
    assert torch.equal(out, d)


def test_tile_argument_errors():
    L = lib()
    t = torch.zeros(4 * 3 * 32 * 32, device=DEV)
    o = torch.zeros(3 * 40 * 40, device=DEV)
    u = torch.zeros(40 * 40 * 3, dtype=torch.uint8, device=DEV)
    bad = [lambda: L.vu_tile_blend(ptr(t), ptr(o), None, 40, 40, 3, 32, 17, st()),                # overlap > T / 2
           lambda: L.vu_tile_blend(ptr(t), None, None, 40, 40, 3, 32, 8, st()),                   # no output
           lambda: L.vu_tile_blend(ptr(t), ptr(t), None, 40, 40, 3, 32, 8, st()),                 # output aliases the windows
           lambda: L.vu_tile_blend(ptr(t), ptr(t[100:]), None, 40, 40, 3, 32, 8, st()),
           lambda: L.vu_tile_blend(ptr(t), ptr(o), None, 40, 40, 5, 32, 8, st()),                 # channels
           lambda: L.vu_tile_blend(ptr(t), ptr(o), None, 40, 40, 3, 0, 0, st()),                  # T <= 0
           lambda: L.vu_tile_gather_u8(ptr(u), ptr(t), 40, 40, 3, 32, 8, 3, 2, 0.456, 0.224, st()),   # windows [3, 5) of 4
           lambda: L.vu_tile_gather_u8(ptr(u), ptr(t), 40, 40, 3, 32, 8, 0, 0, 0.456, 0.224, st()),   # no window
           lambda: L.vu_tile_gather_u8(ptr(u), ptr(t), 40, 40, 3, 32, 8, 0, 4, 0.456, 0.0, st()),     # std
           lambda: L.vu_tile_gather_u8(None, ptr(t), 40, 40, 3, 32, 8, 0, 4, 0.456, 0.224, st()),
           lambda: L.vu_tile_gather_f32(ptr(o), ptr(t), 40, 40, 3, 32, 8, -1, 2, st()),
           lambda: L.vu_tile_gather_f32(ptr(o), None, 40, 40, 3, 32, 8, 0, 4, st())]
    for i, call in enumerate(bad):
        assert call() < 0, i
        assert L.vu_last_error(), i
    assert L.vu_tile_blend(ptr(t), ptr(t), None, 40, 40, 3, 32, 8, st()) < 0 and "alias" in L.vu_last_error().decode()


# ---------------------------------------------------------------- 5. / 6. end to end
SMALL = dict(depth=1, depth_te=1, size_bottleneck=1, preprocessing="conv", im_size=32, patch_size=8, num_channels=3,
             hidden_dim=16, num_heads=2, attn_drop=0.2, proj_drop=0.2, linear_drop=0.0)


def small_model(dtype):
    cfg = O.Config(**SMALL)
    w = O.make_weights(cfg, seed=3)
    m = M.HViT_UNet(dtype=dtype, **SMALL)
    m.load_state_dict({k: v.clone() for k, v in w.items()})
    return m.to(DEV), cfg, w


def quantised(out_f32):
    """The uint8 image that belongs to a float image of the same call: both leave the kernel from one accumulator, so
    out_u8 is clamp(floor(255 out + 0.5)) of the float32 output exactly (float32 arithmetic, as the kernel's), whatever
    the scale of the model's outputs; the float image itself is held to the float64 blend."""
    o = out_f32.cpu()
    return torch.clamp(torch.floor(o * 255.0 + 0.5), 0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def by_hand(m, x_windows, batch):
    """The product's own eval forward on chunks of `batch` windows -> (nt,C,T,T) float32 numpy."""
    was = m.training
    m.eval()
    with torch.no_grad():
        outs = [m(x_windows[i:i + batch]).clone() for i in range(0, x_windows.shape[0], batch)]
    m.train(was)
    return torch.cat(outs).cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_restorer_small_model_against_hand_composition_and_oracle(dtype):
    m, cfg, w = small_model(dtype)
    T, ov, batch = 32, 8, 6
    H, W = 83, 121
    img = image_u8(H, W, 3, seed=11)
    nt = nwin(H, W, T, ov)
    assert nt == 20 and nt % batch
    r = TiledRestorer(m, overlap=ov, batch=batch)
    got_u8 = r(img)
    got = r(torch.from_numpy(img), output="f32")                       # a host torch tensor is taken as well
    assert got_u8.shape == (H, W, 3) and got_u8.dtype == torch.uint8 and got_u8.is_cuda
    assert got.shape == (3, H, W) and got.dtype == torch.float32 and got.is_cuda
    win = ref_windows_hwc(img, T, ov)
    x = O.denoise_prepare(win, win, T, None)[0]
    v = by_hand(m, x.to(DEV), batch)
    ref = ref_blend(v, H, W, T, ov)
    vmax = float(np.abs(v).max())
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max()
    print(f"small {dtype}: restorer vs hand composition {err:.3e} (bound {BLEND_TOL * vmax:.3e}, max|v| {vmax:.3f})")
    assert err <= BLEND_TOL * vmax
    assert torch.equal(got_u8.cpu(), quantised(got))
    # float input: windows cut unchanged, (C,H,W) float32 back
    chw = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (3, H, W)).astype(np.float32)).to(DEV)
    gf = r(chw)
    assert gf.shape == (3, H, W) and gf.dtype == torch.float32
    xw = np.ascontiguousarray(ref_windows_hwc(chw.cpu().numpy().transpose(1, 2, 0), T, ov).transpose(0, 3, 1, 2))
    vf = by_hand(m, torch.from_numpy(xw).to(DEV), batch)
    assert np.abs(gf.cpu().numpy().astype(np.float64) - ref_blend(vf, H, W, T, ov)).max() <= BLEND_TOL * float(np.abs(vf).max())
    # the convenience method: the same restorer, built once
    assert torch.equal(m.restore(img, overlap=ov, batch=batch), got_u8)
    assert len(m._restorers) == 1 and m.restore(img, overlap=ov, batch=batch) is not None and len(m._restorers) == 1
    assert [o.shape for o in r([img, img[:40, :50]])] == [(H, W, 3), (40, 50, 3)]
    if dtype == torch.float32:
        # the CPU oracle's eval forward per window, blended in float64.  A blend is a convex combination of window outputs,
        # so the forward's bound carries over unchanged: 2e-4 of the scale of the oracle's window outputs
        vo = O.forward(w, cfg, x, training=False).detach().numpy()
        eo = np.abs(got.cpu().numpy().astype(np.float64) - ref_blend(vo, H, W, T, ov)).max() / np.abs(vo).max()
        print(f"small fp32: restorer vs oracle windows {eo:.3e}")
        assert eo < 2e-4


def test_restorer_base_bf16_against_hand_composition():
    torch.manual_seed(0)
    m = M.get_vit_unet("base", dtype=torch.bfloat16).to(DEV)
    T, ov, batch = 224, 32, 5
    H, W = 500, 700
    img = image_u8(H, W, 3, seed=2)
    assert nwin(H, W, T, ov) == 12
    r = TiledRestorer(m, overlap=ov, batch=batch)
    got, got_u8 = r(img, output="f32"), r(img)
    win = ref_windows_hwc(img, T, ov)
    x = O.denoise_prepare(win, win, T, None)[0]
    v = by_hand(m, x.to(DEV), batch)
    ref = ref_blend(v, H, W, T, ov)
    vmax = float(np.abs(v).max())
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max()
    print(f"base bf16: restorer vs hand composition {err:.3e} (bound {BLEND_TOL * vmax:.3e}, max|v| {vmax:.3f})")
    assert np.isfinite(v).all() and err <= BLEND_TOL * vmax
    assert torch.equal(got_u8.cpu(), quantised(got))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_restorer_is_deterministic_and_leaves_the_model_alone(dtype):
    """Two calls give the same bits; the training flag, the BatchNorm running statistics and the batch counters are
    untouched; the chunk size does not change the image beyond the blend's bound (2e-6 of the output scale; if the eval
    forward is batch-invariant, as tests/test_gpu_model.py::test_size_independent_properties_base_bf16 finds for Base, the
    images are bit-identical).  Which of the two holds for this small model has not been observed on hardware yet: the test
    prints it per chunk size and asserts the bound only."""
    m, _, _ = small_model(dtype)
    m.train()
    img = image_u8(83, 121, 3, seed=4)
    m._ensure_flat()
    bn0 = m._bn.clone()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    a = TiledRestorer(m, overlap=8, batch=20)(img, output="f32")       # one big batch: all 20 windows
    b = TiledRestorer(m, overlap=8, batch=20)(img, output="f32")
    assert torch.equal(a, b)
    vmax = float(a.abs().max())          # |blend| <= max|v|, and the bound below only needs a scale that is not larger
    for batch in (7, 1):                 # 7 does not divide 20
        c = TiledRestorer(m, overlap=8, batch=batch)(img, output="f32")
        d = (c - a).abs().max().item()
        print(f"{dtype} batch {batch} vs one batch of 20: max diff {d:.3e} ({'bit-identical' if torch.equal(a, c) else 'differs'})")
        assert d <= BLEND_TOL * vmax, d
    assert m.training and all(mod.training for mod in m.modules())
    assert torch.equal(m._bn, bn0)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k


def test_tiled_metrics():
    m, _, _ = small_model(torch.float32)
    rng = np.random.default_rng(8)
    clean = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((50, 70, 3), (33, 40, 3))]
    noisy = [np.clip(c.astype(np.int32) + rng.integers(-20, 21, c.shape), 0, 255).astype(np.uint8) for c in clean]
    p = F.psnr_tiled(m, zip(noisy, clean), overlap=8)
    s = F.ssim_tiled(m, zip(noisy, clean), overlap=8)
    assert p.shape == (2,) and s.shape == (2,) and np.isfinite(p).all() and np.isfinite(s).all()
    r = TiledRestorer(m, overlap=8)
    for i in range(2):
        out = r(noisy[i], output="f32").cpu().numpy().astype(np.float64)
        mse = ((out - clean[i].transpose(2, 0, 1) / 255.0) ** 2).mean()
        assert abs(p[i] - 10 * np.log10(1.0 / mse)) < 1e-3
        y = torch.from_numpy(clean[i].transpose(2, 0, 1) / 255.0).float()[None]
        assert abs(s[i] - float(O.ssim(y, torch.from_numpy(out).float()[None]).reshape(-1)[0])) < 1e-4
