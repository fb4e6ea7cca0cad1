"""Native-resolution training patches and the self-ensemble on the GPU (csrc/vu_patch.hip, dataset.DenoisingPatchTransform,
restore.TiledRestorer(ensemble=), run_denoising(patch_train=)).

Per op, through the C ABI with NaN-filled outputs, against the numpy restatement of tests/test_patch_cpu.py:
  vu_patch_pairs_u8   byte work: BIT-EXACT against the oracle's validation transform (denoise_prepare without a resize or a
                      warp) of the patches numpy cuts and turns
  vu_dihedral_f32     a permutation, one float32 add and one float32 multiply, each rounded once: BIT-EXACT against numpy
End to end: the ensemble against the same composition done by hand (numpy windows and ops, the product's own eval forward on
the same chunks, float32 sum in op order, x 1/K, float64 blend) with the blend's bound of tests/test_gpu_restore.py,
|out - ref| <= 2e-6 max|v|: the averaged windows the kernels hand to the blend are the same float32 numbers as the hand-made
ones (sum and product are single IEEE operations in a fixed order), so the ensemble adds nothing to that bound."""
import numpy as np
import pytest
import torch

import vit_unet_oracle as O
from test_gpu_restore import BLEND_TOL, by_hand, image_u8, nwin, quantised, small_model
from test_patch_cpu import ref_dihedral, ref_patches
from test_restore_cpu import ref_blend, ref_windows_hwc
from vit_unet.torch import _lib, functions as F
from vit_unet.torch._lib import check, lib, ptr
from vit_unet.torch.dataset import DenoisingBatchTransform, DenoisingDataset, DenoisingPatchTransform, dihedral_inverse
from vit_unet.torch.engine import TrainStep
from vit_unet.torch.restore import TiledRestorer

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

# (H, W, C, T): several 32 x 32 tiles with partial ones; W - T = 1; T neither a multiple of 4 nor of the tile and H == T;
# a patch smaller than one tile with two channels; the product's 224 (7 x 7 whole tiles, 16-byte stores)
PATCH_SHAPES = [(83, 121, 3, 32), (40, 33, 1, 32), (33, 64, 3, 33), (50, 47, 2, 7), (237, 229, 3, 224)]


def st():
    return _lib.stream_ptr()


def crop_table(H, W, T, seed):
    """16 crops: every op twice; the two corners, an origin that is no multiple of 4 on either axis, the rest drawn."""
    rng = np.random.default_rng(seed)
    t = np.zeros((16, 3), dtype=np.int32)
    t[:, 0] = rng.integers(0, H - T + 1, 16)
    t[:, 1] = rng.integers(0, W - T + 1, 16)
    t[:, 2] = np.arange(16) % 8
    t[0, :2] = (0, 0)
    t[1, :2] = (H - T, W - T)
    t[9, :2] = (0, 0)                                # the corners under an odd k as well (ops 1 and 2 / 0 and 1 ...)
    t[10, :2] = (H - T, W - T)
    t[3, :2] = (min(1, H - T), min(3, W - T))
    t[5, :2] = (min(5, H - T), min(2, W - T))
    return t


def reference(noisy, clean, T, table, mean=0.456, std=0.224):
    """numpy cut and op, then the oracle's validation transform with im == T: no resize happens."""
    return O.denoise_prepare(ref_patches(noisy, T, table), ref_patches(clean, T, table), T, None, mean=mean, std=std)


def run_patch(noisy, clean, x, y, H, W, Cn, T, table, mean=0.456, std=0.224):
    d = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(DEV)
    check(lib().vu_patch_pairs_u8(ptr(noisy), ptr(clean), ptr(x), ptr(y), H, W, Cn, T, ptr(d), len(table), mean, std, st()),
          "vu_patch_pairs_u8")


# ---------------------------------------------------------------- vu_patch_pairs_u8
@pytest.mark.parametrize("H,W,Cn,T", PATCH_SHAPES)
def test_patch_pairs_bit_exact(H, W, Cn, T):
    noisy, clean = image_u8(H, W, Cn, seed=H), image_u8(H, W, Cn, seed=W + 1000)
    table = crop_table(H, W, T, seed=H * W)
    assert sorted(table[:, 2].tolist()) == sorted(list(range(8)) * 2)
    assert (table[:, 0] % 4 != 0).any() or H - T < 1
    assert (table[:, 1] % 4 != 0).any()
    rx, ry = reference(noisy, clean, T, table)
    dn, dc = torch.from_numpy(noisy).to(DEV), torch.from_numpy(clean).to(DEV)
    n = len(table)
    x, y = torch.full((n, Cn, T, T), NAN, device=DEV), torch.full((n, Cn, T, T), NAN, device=DEV)
    run_patch(dn, dc, x, y, H, W, Cn, T, table)
    assert torch.equal(x.cpu(), rx), (x.cpu() - rx).abs().max()
    assert torch.equal(y.cpu(), ry), (y.cpu() - ry).abs().max()
    # other normalisation constants, outputs offset by one float (not 16-byte aligned: scalar stores), the float before untouched
    rx2, ry2 = reference(noisy, clean, T, table, mean=0.3, std=0.5)
    bx, by = torch.full((n * Cn * T * T + 1,), NAN, device=DEV), torch.full((n * Cn * T * T + 1,), NAN, device=DEV)
    ox, oy = bx[1:].view(n, Cn, T, T), by[1:].view(n, Cn, T, T)
    run_patch(dn, dc, ox, oy, H, W, Cn, T, table, mean=0.3, std=0.5)
    assert torch.equal(ox.cpu(), rx2) and torch.equal(oy.cpu(), ry2)
    assert torch.isnan(bx[0]) and torch.isnan(by[0])
    # each pair omitted in turn: the other side carries the same bits
    x1, y1 = torch.full((n, Cn, T, T), NAN, device=DEV), torch.full((n, Cn, T, T), NAN, device=DEV)
    run_patch(dn, None, x1, None, H, W, Cn, T, table)
    run_patch(None, dc, None, y1, H, W, Cn, T, table)
    assert torch.equal(x1, x) and torch.equal(y1, y)
    # the documented clamp: (-5, W, 11) is read as (0, W - T, 3)
    x2, y2 = torch.full((2, Cn, T, T), NAN, device=DEV), torch.full((2, Cn, T, T), NAN, device=DEV)
    x3, y3 = torch.full((2, Cn, T, T), NAN, device=DEV), torch.full((2, Cn, T, T), NAN, device=DEV)
    run_patch(dn, dc, x2, y2, H, W, Cn, T, np.array([[-5, W, 11], [H, -1, 8 + 6]]))
    run_patch(dn, dc, x3, y3, H, W, Cn, T, np.array([[0, W - T, 3], [H - T, 0, 6]]))
    assert torch.equal(x2, x3) and torch.equal(y2, y3) and torch.isfinite(x2).all()
    r3 = reference(noisy, clean, T, [(0, W - T, 3), (H - T, 0, 6)])
    assert torch.equal(x3.cpu(), r3[0]) and torch.equal(y3.cpu(), r3[1])


@pytest.mark.parametrize("T,Cn", [(32, 3), (33, 1), (224, 3)])
def test_patch_of_a_patch_sized_image_is_the_validation_transform(T, Cn):
    noisy, clean = image_u8(T, T, Cn, seed=T), image_u8(T, T, Cn, seed=T + 1)
    x, y = torch.full((1, Cn, T, T), NAN, device=DEV), torch.full((1, Cn, T, T), NAN, device=DEV)
    run_patch(torch.from_numpy(noisy).to(DEV), torch.from_numpy(clean).to(DEV), x, y, T, T, Cn, T, np.array([[0, 0, 0]]))
    want = DenoisingBatchTransform(T, train=False)(noisy[None], clean[None])
    assert torch.equal(x, want["x"]) and torch.equal(y, want["y"])


# ---------------------------------------------------------------- vu_dihedral_f32
def dihedral_nchw(a, op):
    """ref_dihedral of every (T,T) plane of an (n,C,T,T) array."""
    return np.ascontiguousarray(ref_dihedral(a.transpose(2, 3, 0, 1), op).transpose(2, 3, 0, 1))


def run_dihedral(src, dst, op, accumulate=0, scale=1.0):
    n, Cn, T, _ = src.shape
    check(lib().vu_dihedral_f32(ptr(src), ptr(dst), n, Cn, T, op, accumulate, scale, st()), "vu_dihedral_f32")


@pytest.mark.parametrize("n,Cn,T", [(3, 3, 32), (2, 1, 33), (1, 4, 7), (2, 3, 224)])
def test_dihedral_bit_exact(n, Cn, T):
    rng = np.random.default_rng(n * T)
    a = rng.standard_normal((n, Cn, T, T)).astype(np.float32)
    d0 = rng.standard_normal((n, Cn, T, T)).astype(np.float32)
    src = torch.from_numpy(a).to(DEV)
    third = np.float32(1.0 / 3.0)
    for op in range(8):
        v = dihedral_nchw(a, op)
        got = torch.full((n, Cn, T, T), NAN, device=DEV)
        run_dihedral(src, got, op)
        assert torch.equal(got.cpu(), torch.from_numpy(v)), op
        again = torch.full((n, Cn, T, T), NAN, device=DEV)
        run_dihedral(src, again, op)
        assert torch.equal(again, got), op                                      # a second run gives the same bits
        acc = torch.from_numpy(d0).to(DEV)
        run_dihedral(src, acc, op, accumulate=1)
        assert torch.equal(acc.cpu(), torch.from_numpy(d0 + v)), op             # one float32 add
        sc = torch.full((n, Cn, T, T), NAN, device=DEV)
        run_dihedral(src, sc, op, scale=0.125)
        assert torch.equal(sc.cpu(), torch.from_numpy(v * np.float32(0.125))), op
        # accumulate and scale 1/3 into a destination offset by one float (scalar accesses), the float before untouched
        buf = torch.full((a.size + 1,), 77.0, device=DEV)
        off = buf[1:].view(n, Cn, T, T)
        off.copy_(torch.from_numpy(d0))
        run_dihedral(src, off, op, accumulate=1, scale=1.0 / 3.0)
        assert torch.equal(off.cpu(), torch.from_numpy((d0 + v) * third)), op
        assert buf[0] == 77.0
        # a source offset by one float
        sbuf = torch.zeros(a.size + 1, device=DEV)
        sbuf[1:].copy_(src.reshape(-1))
        got2 = torch.full((n, Cn, T, T), NAN, device=DEV)
        run_dihedral(sbuf[1:].view(n, Cn, T, T), got2, op, scale=float(third))
        assert torch.equal(got2.cpu(), torch.from_numpy(v * third)), op
    back = torch.full((n, Cn, T, T), NAN, device=DEV)                           # op, then its inverse: the identity
    for op in range(8):
        t = torch.full((n, Cn, T, T), NAN, device=DEV)
        run_dihedral(src, t, op)
        run_dihedral(t, back, dihedral_inverse(op))
        assert torch.equal(back, src), op


def test_dihedral_refuses_overlap_on_the_device():
    t = torch.zeros(2 * 3 * 8 * 8 + 16, device=DEV)
    a = t[:384].view(2, 3, 8, 8)
    L = lib()
    assert L.vu_dihedral_f32(ptr(a), ptr(a), 2, 3, 8, 1, 0, 1.0, st()) < 0 and "overlap" in L.vu_last_error().decode()
    assert L.vu_dihedral_f32(ptr(a), ptr(t[16:400]), 2, 3, 8, 1, 0, 1.0, st()) < 0
    assert (t == 0).all()


# ---------------------------------------------------------------- DenoisingPatchTransform
def test_patch_transform_list_of_two_sizes():
    T, P = 32, 3
    sizes = [(83, 121), (40, 50)]
    noisy = [image_u8(h, w, 3, seed=h) for h, w in sizes]
    clean = [image_u8(h, w, 3, seed=w) for h, w in sizes]
    table = np.array([[[0, 0, 1], [51, 89, 6], [7, 13, 3]], [[8, 18, 5], [3, 1, 0], [0, 17, 7]]])
    t = DenoisingPatchTransform(T, per_image=P, seed=0)
    got = t(noisy, clean, crops=table)
    assert got["x"].shape == (2 * P, 3, T, T) and got["y"].shape == (2 * P, 3, T, T)
    assert got["x"].dtype == torch.float32 and got["x"].is_cuda
    for b in range(2):                                                          # the patches of image 0 come first
        rx, ry = reference(noisy[b], clean[b], T, table[b])
        assert torch.equal(got["x"][b * P:(b + 1) * P].cpu(), rx) and torch.equal(got["y"][b * P:(b + 1) * P].cpu(), ry)
    # host torch and device torch inputs give the same bits as host numpy
    for conv in (torch.from_numpy, lambda a: torch.from_numpy(a).to(DEV)):
        g2 = t([conv(a) for a in noisy], [conv(a) for a in clean], crops=table)
        assert torch.equal(g2["x"], got["x"]) and torch.equal(g2["y"], got["y"])
    # a (B,H,W,C) batch, drawn crops: the same seed gives the same patches, and they are the reference of the drawn table
    nb, cb = np.stack([noisy[0], noisy[0][::-1]]), np.stack([clean[0], clean[0][::-1]])
    a = DenoisingPatchTransform(T, per_image=P, seed=5)(nb, cb)
    b = DenoisingPatchTransform(T, per_image=P, seed=5)(torch.from_numpy(nb).to(DEV), torch.from_numpy(cb))
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["y"], b["y"])
    drawn = DenoisingPatchTransform(T, per_image=P, seed=5).draw([(83, 121)] * 2)
    for k in range(2):
        rx, ry = reference(nb[k], cb[k], T, drawn[k])
        assert torch.equal(a["x"][k * P:(k + 1) * P].cpu(), rx) and torch.equal(a["y"][k * P:(k + 1) * P].cpu(), ry)
    # train=False: one centred crop per image, op 0
    v = DenoisingPatchTransform(T, per_image=P, train=False)(noisy, clean)
    assert v["x"].shape == (2, 3, T, T)
    for b, (h, w) in enumerate(sizes):
        rx, ry = reference(noisy[b], clean[b], T, [((h - T) // 2, (w - T) // 2, 0)])
        assert torch.equal(v["x"][b:b + 1].cpu(), rx) and torch.equal(v["y"][b:b + 1].cpu(), ry)


def test_patch_transform_refuses_before_any_launch():
    T, P = 32, 2
    t = DenoisingPatchTransform(T, per_image=P, seed=0)
    img = image_u8(40, 50, 3)
    ok = np.array([[[0, 0, 0], [8, 18, 7]]])
    assert t([img], [img], crops=ok)["x"].shape == (2, 3, T, T)
    for bad in ([[[9, 0, 0], [0, 0, 0]]], [[[0, 19, 0], [0, 0, 0]]], [[[0, 0, 8], [0, 0, 0]]], [[[-1, 0, 0], [0, 0, 0]]],
                [[[0, 0, -1], [0, 0, 0]]]):
        with pytest.raises((_lib.VuError, AssertionError)):
            t([img], [img], crops=np.array(bad))
    with pytest.raises((_lib.VuError, AssertionError)):
        t([img], [img], crops=np.zeros((1, 3, 3), np.int32))                    # table of another shape
    with pytest.raises((_lib.VuError, AssertionError)):
        t([img], [img[:, :49]])                                                 # mismatched pair
    with pytest.raises((_lib.VuError, AssertionError)):
        t([img[:31]], [img[:31]])                                               # smaller than a patch
    with pytest.raises((_lib.VuError, AssertionError)):
        t([img, img], [img])


def test_dataset_hands_all_items_to_a_patch_transform():
    imgs = {f"/{kind}/{name}.png": image_u8(h, w, 3, seed=s)
            for s, (kind, name, h, w) in enumerate([("n", "a", 40, 50), ("c", "a", 40, 50), ("n", "b", 64, 33), ("c", "b", 64, 33)])}
    ds = DenoisingDataset(["a", "b"], augments=DenoisingPatchTransform(32, per_image=2, seed=9), clean_folder="/c", noisy_folder="/n",
                          read=lambda path: imgs[path])
    got = ds.transform([ds[0], ds[1]])
    want = DenoisingPatchTransform(32, per_image=2, seed=9)([imgs["/n/a.png"], imgs["/n/b.png"]], [imgs["/c/a.png"], imgs["/c/b.png"]])
    assert got["x"].shape == (4, 3, 32, 32) and torch.equal(got["x"], want["x"]) and torch.equal(got["y"], want["y"])
    with pytest.raises(TypeError):
        DenoisingDataset(["a"], augments=object())


# ---------------------------------------------------------------- ensemble
def ensemble_by_hand(m, img, T, ov, batch, ops):
    """numpy windows -> ref_dihedral -> the product's own eval forward on the same chunks -> inverse ref_dihedral -> float32
    sum in op order -> x 1/K: the (nt,C,T,T) float32 windows the blend receives."""
    win = ref_windows_hwc(img, T, ov)
    x = O.denoise_prepare(win, win, T, None)[0].numpy()
    outs = []
    for t0 in range(0, x.shape[0], batch):
        chunk, acc = x[t0:t0 + batch], None
        for op in ops:
            v = by_hand(m, torch.from_numpy(dihedral_nchw(chunk, op)).to(DEV), batch)
            back = dihedral_nchw(v, dihedral_inverse(op))
            acc = back if acc is None else acc + back
            assert acc.dtype == np.float32
        outs.append(acc * np.float32(1.0 / len(ops)))
    return np.concatenate(outs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ensemble_against_hand_composition(dtype):
    m, _, _ = small_model(dtype)
    T, ov, batch, H, W = 32, 8, 6, 83, 121
    img = image_u8(H, W, 3, seed=11)
    assert nwin(H, W, T, ov) == 20
    m.train()
    m._ensure_flat()
    bn0 = m._bn.clone()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    plain = TiledRestorer(m, overlap=ov, batch=batch)
    one = TiledRestorer(m, overlap=ov, batch=batch, ensemble=1)
    assert torch.equal(one(img, output="f32"), plain(img, output="f32")) and torch.equal(one(img), plain(img))
    for K in (2, 8):
        r = TiledRestorer(m, overlap=ov, batch=batch, ensemble=K)
        got, got_u8 = r(img, output="f32"), r(img)
        assert got.shape == (3, H, W) and got_u8.shape == (H, W, 3) and got_u8.dtype == torch.uint8
        v = ensemble_by_hand(m, img, T, ov, batch, TiledRestorer.ENSEMBLE_OPS[K])
        ref = ref_blend(v, H, W, T, ov)
        vmax = float(np.abs(v).max())
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max()
        print(f"ensemble {K} {dtype}: restorer vs hand composition {err:.3e} (bound {BLEND_TOL * vmax:.3e}, max|v| {vmax:.3f})")
        assert np.isfinite(v).all() and torch.isfinite(got).all() and err <= BLEND_TOL * vmax
        assert torch.equal(got_u8.cpu(), quantised(got))
        assert not torch.equal(got, plain(img, output="f32"))                   # the ensemble is not the plain path
        assert torch.equal(r(img, output="f32"), got)                           # and gives the same bits again
        assert torch.equal(m.restore(img, overlap=ov, batch=batch, ensemble=K), got_u8)
    assert torch.equal(m.restore(img, overlap=ov, batch=batch), plain(img)) and len(m._restorers) == 3
    assert m.training and all(mod.training for mod in m.modules())
    assert torch.equal(m._bn, bn0)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k


def test_tiled_psnr_with_ensemble():
    m, _, _ = small_model(torch.float32)
    rng = np.random.default_rng(8)
    clean = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((50, 70, 3), (33, 40, 3))]
    noisy = [np.clip(c.astype(np.int32) + rng.integers(-20, 21, c.shape), 0, 255).astype(np.uint8) for c in clean]
    p = F.psnr_tiled(m, zip(noisy, clean), overlap=8, ensemble=8)
    s = F.ssim_tiled(m, zip(noisy, clean), overlap=8, ensemble=8)
    assert p.shape == (2,) and np.isfinite(p).all() and s.shape == (2,) and np.isfinite(s).all()
    r = TiledRestorer(m, overlap=8, ensemble=8)
    for i in range(2):
        out = r(noisy[i], output="f32").cpu().numpy().astype(np.float64)
        mse = ((out - clean[i].transpose(2, 0, 1) / 255.0) ** 2).mean()
        assert abs(p[i] - 10 * np.log10(1.0 / mse)) < 1e-3


# ---------------------------------------------------------------- training
def test_train_steps_on_patch_batches():
    m, _, _ = small_model(torch.float32)
    m.train()
    rng = np.random.default_rng(1)
    clean = rng.integers(0, 256, (4, 40, 48, 3), dtype=np.uint8)
    noisy = np.clip(clean.astype(np.int32) + rng.integers(-20, 21, clean.shape), 0, 255).astype(np.uint8)
    t = DenoisingPatchTransform(32, per_image=2, seed=4)
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    ts = TrainStep(m, lr=1e-3, seed=3)
    losses = []
    for _ in range(2):
        b = t(noisy, clean)
        assert b["x"].shape == (8, 3, 32, 32)
        losses.append(float(ts.step(b["x"], b["y"])))
    assert np.isfinite(losses).all(), losses
    changed = [k for k, v in m.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert len(changed) > len(before) // 2, changed
    assert all(torch.isfinite(v).all() for v in m.parameters())


def test_run_denoising_patch_train(tmp_path):
    from vit_unet.torch.run import run_denoising
    rng = np.random.default_rng(21)
    clean = rng.integers(0, 256, (6, 230, 240, 3), dtype=np.uint8)
    noisy = np.clip(clean.astype(np.int32) + rng.integers(-20, 21, clean.shape), 0, 255).astype(np.uint8)
    folder = tmp_path / "models"
    res = run_denoising(noisy, clean, n_epochs=1, folds=2, model_string="lite", batch_size=2, im_size=224, patch_train=True,
                        crops_per_image=1, ensemble=2, folder=str(folder))
    assert [len(p) for p in res["psnr"]] == [3, 3]
    assert all(np.isfinite(p).all() for p in res["psnr"]) and np.isfinite(res["psnr_mean"])
    assert (folder / "best-checkpoint.bin").exists() and (folder / "last-checkpoint.bin").exists()
    with pytest.raises(AssertionError):
        run_denoising(noisy, clean, batch_size=6, patch_train=True, crops_per_image=4)     # 4 does not divide 6
