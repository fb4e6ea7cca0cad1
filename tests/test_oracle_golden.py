"""The CPU oracle against the golden vectors generated from the unmodified reference
(tests/golden/make_golden.py).  This is what pins parity."""
import json
import os

import numpy as np
import pytest
import torch

import vit_unet_oracle as O

TINY = ["tiny_a", "tiny_b", "tiny_c"]
TOL = 2e-5   # fp32 oracle vs fp32 reference: max |diff| / max |ref|


def close(got, ref, tol=TOL):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30)
    assert err < tol, f"scaled max error {err:.3e} >= {tol:.1e}"


def _load(golden_dir, name):
    with open(os.path.join(golden_dir, "manifest.json")) as f:
        man = json.load(f)
    g = {}
    for f in [name + ".npz"] + sorted(f for f in os.listdir(golden_dir) if f.startswith(name + "_part") and f.endswith(".npz")):
        g.update(np.load(os.path.join(golden_dir, f)))     # a fixture over 1 MB is stored in parts (make_golden.py)
    return man, g


@pytest.mark.parametrize("name", TINY)
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_tiny_model_forward_backward(golden_dir, name, mode):
    man, g = _load(golden_dir, name)
    case = man["cases"][name]
    cfg = O.Config(**case["config"])
    assert O.param_count(cfg) == case["params"]
    w = O.make_weights(cfg, seed=case["weights_seed"])
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    for k, _ in O.param_shapes(cfg):
        w[k].requires_grad_(True)
    out = O.forward(w, cfg, x, training=(mode == "train"))
    loss = O.mse_loss(out, y)
    loss.backward()
    close(out.detach().numpy(), g[f"{mode}.out"])
    np.testing.assert_allclose(loss.item(), g[f"{mode}.loss"], rtol=1e-5)
    for k in g:
        if k.startswith(f"{mode}.grad."):
            pname = k[len(f"{mode}.grad."):]
            if mode == "train" and pname.endswith("reatten_matrix.bias"):
                continue   # exactly 0 in exact arithmetic (train-mode BN removes the mean): noise
            ref = g[k]
            got = w[pname].grad.numpy()
            scale = np.abs(ref).max() + 1e-12
            assert np.abs(got - ref).max() / scale < 2e-3, pname   # fp32-vs-fp32 gradient noise
    gabs = np.array([float(w[k].grad.double().abs().sum()) for k, _ in O.param_shapes(cfg)])
    sel = np.array([not (mode == "train" and k.endswith("reatten_matrix.bias"))
                    for k, _ in O.param_shapes(cfg)])
    np.testing.assert_allclose(gabs[sel], g[f"{mode}.gradabs"][sel], rtol=1e-2)  # per-parameter L1 summary
    if mode == "train":
        for k in g:
            if k.startswith("train.buf."):
                np.testing.assert_allclose(w[k[len("train.buf."):]].numpy(), g[k], rtol=1e-4, atol=1e-9)


def test_retile_ops(golden_dir):
    _, g = _load(golden_dir, "ops")
    X = torch.from_numpy(g["patch.in"])
    t = O.patchify(X, 8)
    assert np.array_equal(t.numpy(), g["patch.out_s8"])          # permutations are bit-exact
    assert np.array_equal(O.unpatchify(t, 3).numpy(), g["unpatch.out"])
    assert np.array_equal(O.downsample(t, 3).numpy(), g["down.out"])
    assert np.array_equal(O.upsample(t, 3).numpy(), g["up.out"])
    assert np.array_equal(O.upsample(O.downsample(t, 3), 3).numpy(), t.numpy())


@pytest.mark.parametrize("tag,N,C,s,h,hid", [("n49", 49, 3, 8, 4, 16), ("d12", 16, 3, 4, 4, 8)])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_block_ops(golden_dir, tag, N, C, s, h, hid, mode):
    _, g = _load(golden_dir, "ops")
    training = mode == "train"
    cfg = O.Config(depth=0, depth_te=1, size_bottleneck=1, preprocessing="conv", im_size=int(N ** 0.5) * s,
                   patch_size=s, num_channels=C, hidden_dim=hid, num_heads=h)
    x, enc = torch.from_numpy(g[f"{tag}.x"]), torch.from_numpy(g[f"{tag}.enc"])

    def params(prefix):
        return {k[len(f"{tag}.{prefix}."):]: torch.from_numpy(v.copy()) for k, v in g.items()
                if k.startswith(f"{tag}.{prefix}.")}
    p = params("blk")
    y, amap = O.reattention(x, x, p, "ReAttn.", h, C, training=training, attn_drop=0., proj_drop=0.,
                            return_map=True)
    close(amap.numpy(), g[f"{tag}.{mode}.attn.map"])
    close(y.numpy(), g[f"{tag}.{mode}.attn.out"])
    p = params("blk")
    close(O.te_block(x, p, "", cfg, training=training).numpy(), g[f"{tag}.{mode}.block.out"])
    p = params("skp")
    close(O.skip_block(enc, x, p, "", cfg, training=training).numpy(), g[f"{tag}.{mode}.skip.out"])


@pytest.mark.parametrize("name", ["base", "large"])
def test_full_config_checksums(golden_dir, name):
    """Full-size eval forward: weights regenerated from the seed, compared with the reference's
    sampled outputs / checksums.  (lite and seg512 take ~5 s each on the reference; they are
    covered by the GPU tests against the same manifest.)"""
    man, _ = _load(golden_dir, "ops")
    ref = man["full"][name]
    kw = dict(O.PRESETS[name], attn_drop=0.0, proj_drop=0.0)
    cfg = O.Config(**kw)
    assert O.param_count(cfg) == ref["params"] == man["kat"]["packaged_counts"][name]
    w = O.make_weights(cfg, seed=0)
    x, _ = O.make_batch(cfg, B=ref["B"], seed=1234)
    with torch.no_grad():
        out = O.forward(w, cfg, x, training=False)
    flat = out.reshape(-1)
    got = flat[torch.tensor(ref["sample_idx"])].double().numpy()
    close(got, np.array(ref["sample"]), 1e-4)
    assert abs(float(out.double().mean()) - ref["mean"]) < 1e-4 * max(1.0, abs(ref["mean"]))
    assert abs(float(out.abs().max()) - ref["absmax"]) < 1e-3 * ref["absmax"]


def test_parameter_count_kats(golden_dir):
    """README.md:16,34,52 counts via the derivation of SURVEY §4 / App. B, and packaged counts."""
    man, _ = _load(golden_dir, "ops")
    for name in ("lite", "base", "large"):
        cfg = O.Config(**O.PRESETS[name])
        total = O.param_count(cfg)
        assert total == man["kat"]["packaged_counts"][name]
        n_te = 2 * cfg.depth * cfg.depth_te + cfg.size_bottleneck
        C = cfg.num_channels
        readme = total - n_te * 2 * cfg.P + (9 * C * C + C)
        assert readme == man["kat"]["readme_counts"][name]
    seg = O.Config(**dict(O.PRESETS["base"], im_size=512, num_channels=1))
    assert O.param_count(seg) == man["kat"]["packaged_counts"]["seg512"]


def test_keep_mask_statistics():
    m = O.keep_mask(1 << 20, 0.2, seed=123, stream=5)
    rate = m.float().mean().item()
    assert abs(rate - 0.8) < 2e-3
    m2 = O.keep_mask(1 << 20, 0.2, seed=123, stream=6)
    assert (m != m2).float().mean().item() > 0.25      # different streams decorrelate
    assert torch.equal(m, O.keep_mask(1 << 20, 0.2, seed=123, stream=5))
    # neighbouring pairs are not correlated
    a, b = m[0::2].float(), m[1::2].float()
    assert abs(((a - a.mean()) * (b - b.mean())).mean().item()) < 2e-3


def test_quad_mask_statistics():
    """The 8-bit-per-key dropout scheme of the non-materialising attention form (csrc/vu_flash.hip vu_quad_word +
    vu_quad_head: one word per (sample, row, key quad), a third round per head)."""
    N, H = 784, 8
    mall = O.keep_mask_quad(4, H, 400, N, 0.2, seed=123, stream=5).float()      # (4, 8, 400, 784): 10 M elements
    assert O.quad_threshold(0.2) == 51

    def corr(a, b):
        a, b = a - a.mean(), b - b.mean()
        return abs((a * b).mean().item() / (a.std().item() * b.std().item()))
    for h in range(H):
        m = mall[:, h].reshape(-1, N)
        assert abs(m.mean().item() - (1 - 51 / 256)) < 3e-3
        lanes = [m[:, r::4].reshape(-1) for r in range(4)]
        for a in lanes:
            assert abs(a.mean().item() - (1 - 51 / 256)) < 5e-3
        assert max(corr(lanes[i], lanes[j]) for i in range(4) for j in range(i)) < 1e-2     # byte lanes of one word
        assert max(corr(a[:-1], a[1:]) for a in lanes) < 1.5e-2                               # neighbouring words
        assert corr(m[:-1].reshape(-1), m[1:].reshape(-1)) < 1e-2                             # neighbouring map rows
        kept = m.sum(dim=1)
        assert 0.8 < kept.var().item() / (N * (51 / 256) * (1 - 51 / 256)) < 1.2            # binomial row counts
    # heads (they share the two-round word): masks and byte lanes of different heads are uncorrelated
    flat = [mall[:, h].reshape(-1) for h in range(H)]
    assert max(corr(flat[i], flat[j]) for i in range(H) for j in range(i)) < 5e-3
    q = [mall[:, h].reshape(-1, 4) for h in range(H)]
    assert max(corr(q[i][:, a], q[j][:, b]) for i in range(H) for j in range(i) for a in range(4) for b in range(4)) < 1e-2
    m2 = O.keep_mask_quad(4, H, 400, N, 0.2, seed=123, stream=6).float()
    assert corr(mall.reshape(-1), m2.reshape(-1)) < 5e-3                                      # streams decorrelate
    assert torch.equal(mall.bool(), O.keep_mask_quad(4, H, 400, N, 0.2, seed=123, stream=5))


def test_metric_oracles_hand_values():
    """PSNR / Dice / SSIM restatements against hand-computed values (the reference holds no fixtures
    for them: functions.py:7-19 defers to scikit-image, README.md:85-101 is prose)."""
    y = torch.full((2, 1, 9, 9), 0.5)
    x = y + 0.1
    assert torch.allclose(O.psnr(y, x), torch.full((2,), 20.0, dtype=torch.float64), atol=1e-5)   # 10 log10(1/0.01)
    # Dice, README snippet: 1 - (2*I + 1)/(S + T + 1)
    a, b = torch.tensor([1.0, 0.0, 1.0, 1.0]), torch.tensor([1.0, 1.0, 0.0, 1.0])
    assert abs(O.dice_loss(a, b).item() - (1 - 5.0 / 7.0)) < 1e-7
    # SSIM of constant images: variances vanish, S = (2ab + C1)/(a^2 + b^2 + C1)
    s = O.ssim(y.numpy(), x.numpy())
    c1 = 0.01 ** 2
    assert torch.allclose(s, torch.full((2,), (2 * 0.5 * 0.6 + c1) / (0.25 + 0.36 + c1), dtype=torch.float64), atol=1e-9)
    # brute-force windows on a small random pair
    g = torch.Generator().manual_seed(5)
    p, q = torch.rand(1, 2, 10, 12, generator=g).double().numpy(), torch.rand(1, 2, 10, 12, generator=g).double().numpy()
    win, tot = 7, 0.0
    for c in range(2):
        vals = []
        for i in range(10 - win + 1):
            for j in range(12 - win + 1):
                u, v = p[0, c, i:i + win, j:j + win].ravel(), q[0, c, i:i + win, j:j + win].ravel()
                cov = np.cov(u, v, ddof=1)
                vals.append(((2 * u.mean() * v.mean() + c1) * (2 * cov[0, 1] + 0.03 ** 2))
                            / ((u.mean() ** 2 + v.mean() ** 2 + c1) * (cov[0, 0] + cov[1, 1] + 0.03 ** 2)))
        tot += np.mean(vals)
    assert abs(O.ssim(p, q).item() - tot / 2) < 1e-10
    assert abs(O.ssim(p, p).item() - 1.0) < 1e-12


@pytest.mark.parametrize("name,dtype", [("base", torch.float64), ("lite", torch.float32)])
def test_full_config_train_golden(golden_dir, name, dtype):
    """Full-size TRAIN-mode step (BatchNorm batch statistics, dropout 0) of the oracle against the reference driven
    in float64 (tests/golden/full_train.npz: loss, sampled outputs, per-parameter gradient L1, sampled gradients,
    running statistics).  Base is ill-conditioned in float32 - the reference's own float32 run is 2e-2 / cosine 0.89
    away from its float64 run (manifest `ref32`) - so the oracle is run in float64 there and must agree to 1e-7: that
    pins the ALGORITHM at full size.  Lite is well conditioned (ref32 deviation 7e-6) and is checked in float32.
    (large runs the same code with more blocks; its float32 run is chaotic in the reference itself.)"""
    man, g = _load(golden_dir, "full_train")
    meta = man["full_train"][name]
    kw = dict(O.PRESETS[name], attn_drop=0.0, proj_drop=0.0)
    cfg = O.Config(**kw)
    w = O.make_weights(cfg, seed=meta["weights_seed"], dtype=dtype)
    x, y = O.make_batch(cfg, B=meta["B"], seed=meta["batch_seed"], dtype=dtype)
    for k, _ in O.param_shapes(cfg):
        w[k].requires_grad_(True)
    out = O.forward(w, cfg, x, training=True)
    loss = O.mse_loss(out, y)
    loss.backward()
    f64 = dtype == torch.float64
    np.testing.assert_allclose(loss.item(), float(g[f"{name}.loss"]), rtol=1e-9 if f64 else 2e-5)
    close(out.detach().reshape(-1)[torch.from_numpy(g[f"{name}.out_idx"])].numpy(), g[f"{name}.out_sample"],
          1e-7 if f64 else 2e-4)
    names = [k for k, _ in O.param_shapes(cfg)]
    gabs = np.array([float(w[k].grad.double().abs().sum()) for k in names])
    sel = np.array([not k.endswith("reatten_matrix.bias") for k in names])
    # (float32: the q/k conv weight gradients of the last decoder are sums of ~1e6 cancelling terms: absolute floor)
    np.testing.assert_allclose(gabs[sel], g[f"{name}.gradabs"][sel], rtol=1e-6 if f64 else 1e-2,
                               atol=0 if f64 else 2e-5 * g[f"{name}.gradabs"].max())
    for k in g:
        if k.startswith(f"{name}.grad."):
            pname = k[len(f"{name}.grad."):]
            if pname.endswith("reatten_matrix.bias"):
                continue
            got = w[pname].grad.reshape(-1)[torch.from_numpy(g[f"{name}.grad_idx.{pname}"])].double().numpy()
            scale = float(g[f"{name}.gradmax.{pname}"]) + 1e-30
            assert np.abs(got - g[k]).max() / scale < (1e-6 if f64 else 2e-3), pname
    for k in g:
        if k.startswith(f"{name}.buf."):
            np.testing.assert_allclose(w[k[len(f"{name}.buf."):]].double().numpy(), g[k], rtol=1e-7 if f64 else 1e-3, atol=1e-12)
    r32 = meta["ref32"]        # the conditioning statement the GPU tests lean on
    if name == "lite":
        assert r32["out_err"] < 1e-4 and r32["grad_cos_all"] > 0.9999


def test_round_e4m3_pinned_by_torch_float8_and_table_values():
    """The oracle's OCP e4m3 rounding (BASELINE config 5's fp8 attention operands) against torch's own
    float8_e4m3fn conversion on every bf16 bit pattern in range and on a million fp32 values, plus the
    format's table values: max 448, min normal 2^-6, min subnormal 2^-9, ties to even, saturation."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.bfloat16).float()
    r = O.round_e4m3(x)
    ok = (x.abs() <= 448) & ~torch.isnan(x)
    assert torch.equal(r[ok], x[ok].to(torch.float8_e4m3fn).float())
    big = (x.abs() > 448) & ~torch.isnan(x)
    assert torch.equal(r[big].abs().unique(), torch.tensor([448.0]))
    assert torch.isnan(r[torch.isnan(x)]).all()
    xf = torch.randn(1 << 20, generator=torch.Generator().manual_seed(3)) * 3
    assert torch.equal(O.round_e4m3(xf), xf.to(torch.float8_e4m3fn).float())
    t = torch.tensor([0.0, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -10, 2.0 ** -6, 0.3, 17.0, 19.0, 447.0, 464.0, 1e9, -1e9])
    e = torch.tensor([0.0, 2.0 ** -9, 0.0, 2.0 ** -9, 2.0 ** -6, 0.3125, 16.0, 20.0, 448.0, 448.0, 448.0, -448.0])
    assert torch.equal(O.round_e4m3(t), e)
    assert O.round_e4m3(t.to(torch.bfloat16)).dtype == torch.bfloat16
    # straight-through: identity gradient
    q = torch.randn(64, requires_grad=True)
    O._e4(q, "e4m3").sum().backward()
    assert torch.equal(q.grad, torch.ones(64))
