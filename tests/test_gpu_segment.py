"""Whole-slice / volume segmentation on the GPU (csrc/vu_segtile.hip, vit_unet/torch/segment.py).

Per op, through the C ABI with NaN-filled outputs, against the numpy restatement of tests/test_segment_cpu.py:
  vu_tile_gather_i16   BIT-EXACT against the oracle's seg_prepare (same size, no warp: the intensity window only) of the
                       numpy-cut windows, int16 values over the full range, both clips
  vu_seg_blend         logits bit-equal to vu_tile_blend(out_f32, C = 1) slice by slice, and |logits - ref| <= 2e-6 max|v|
                       against the float64 blend (the derivation of tests/test_gpu_restore.py: at most 9 terms; each weight
                       carries 2 roundings and each product 1, the two running sums at most 8 each, one division: about 22
                       units of 2^-24 = 1.3e-6 relative to sum(w |v|) / sum(w) <= max|v|); mask == (logits >= zthr) exactly
                       with the call's own logits, and equal to the float64 mask on every pixel with |z_ref - zthr| >
                       2e-6 max|v| (the left-out share may not exceed 1 % per slice); counts equal to the numpy counts of
                       the call's own mask and the truth, exactly.
End to end: TiledSegmenter on the small model of tests/test_gpu_restore.py with num_channels = 1 (the constructor takes that
shape as it is), fp32 and bf16, against the same composition done by hand (numpy windows, the oracle's seg_prepare, the
product's own eval forward on the documented chunks, float64 blend) within the blend's bound and, fp32 only, against the CPU
oracle's eval forward per window within 2e-4 of the output scale, as the restorer test does."""
import numpy as np
import pytest
import torch

import vit_unet_oracle as O
from test_restore_cpu import ref_blend
from test_segment_cpu import ref_counts, ref_nt, ref_seg_blend, ref_volume_windows
from vit_unet.torch import _lib, functions as F
from vit_unet.torch import model as M
from vit_unet.torch._lib import check, lib, ptr
from vit_unet.torch.restore import TiledRestorer
from vit_unet.torch.segment import TiledSegmenter, dice_from_counts, iou_from_counts, logit_threshold

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLEND_TOL = 2e-6

# (D, H, W, overlap, T): inward-shifted windows at origins 51 and 89 with an odd W; one axis smaller than the window; both
# smaller; H = 1 without overlap; exactly one window; no overlap; odd W; the production window size; one window of the
# benchmark configuration's shape
VOLUMES = [(3, 83, 121, 8, 32), (2, 20, 70, 5, 32), (1, 7, 9, 16, 32), (2, 1, 33, 0, 32), (4, 32, 32, 16, 32), (2, 64, 96, 0, 32),
           (3, 37, 45, 8, 32), (2, 300, 250, 32, 224), (1, 512, 512, 32, 512)]
WINDOWS = [(-1024.0, 1024.0), (-1000.0, 2000.0)]


def st():
    return _lib.stream_ptr()


def volume_i16(D, H, W, seed=0):
    v = np.random.default_rng(seed).integers(-32768, 32768, (D, H, W)).astype(np.int16)
    v.reshape(-1)[:2] = (-32768, 32767)
    return v


# ---------------------------------------------------------------- 1. gather
@pytest.mark.parametrize("D,H,W,ov,T", VOLUMES)
def test_tile_gather_i16_bit_exact(D, H, W, ov, T):
    L = lib()
    vol = volume_i16(D, H, W, seed=H + W)
    win = ref_volume_windows(vol, T, ov)                                # (D nt,T,T) crop / reflect by numpy indexing
    nt = ref_nt(H, W, T, ov)
    N = D * nt
    assert win.shape[0] == N
    d = torch.from_numpy(vol).to(DEV)
    refs = []
    for lo, hi in WINDOWS:
        ref = O.seg_prepare(win, None, T, None, lo, hi)[0]              # same size, no warp: the window only
        refs.append(ref)
        assert ref.min() == 0.0 and ref.max() == 1.0                    # both clips occur
        got = torch.full((N, 1, T, T), float("nan"), device=DEV)
        check(L.vu_tile_gather_i16(ptr(d), ptr(got), D, H, W, T, ov, 0, N, lo, hi, st()))
        assert torch.equal(got.cpu(), ref), (got.cpu() - ref).abs().max()
    lo, hi = WINDOWS[0]
    ref = refs[0]
    if D > 1 and nt > 1:                                                # starts inside slice 0, ends inside slice 1
        g0, n = nt - 1, min(nt, 3)
        part = torch.full((n, 1, T, T), float("nan"), device=DEV)
        check(L.vu_tile_gather_i16(ptr(d), ptr(part), D, H, W, T, ov, g0, n, lo, hi, st()))
        assert torch.equal(part.cpu(), ref[g0:g0 + n])
    elif D > 1:                                                         # one window a slice: slices [0, 2)
        part = torch.full((2, 1, T, T), float("nan"), device=DEV)
        check(L.vu_tile_gather_i16(ptr(d), ptr(part), D, H, W, T, ov, 0, 2, lo, hi, st()))
        assert torch.equal(part.cpu(), ref[:2])
    # the last window alone, into an output offset by one float (scalar stores)
    buf = torch.full((T * T + 1,), float("nan"), device=DEV)
    check(L.vu_tile_gather_i16(ptr(d), ptr(buf[1:].view(1, 1, T, T)), D, H, W, T, ov, N - 1, 1, lo, hi, st()))
    assert torch.equal(buf[1:].view(1, 1, T, T).cpu(), ref[N - 1:]) and torch.isnan(buf[0])
    # an input offset by one int16 (2-byte aligned only)
    ib = torch.zeros(vol.size + 1, dtype=torch.int16, device=DEV)
    ib[1:].copy_(d.reshape(-1))
    got = torch.full((N, 1, T, T), float("nan"), device=DEV)
    check(L.vu_tile_gather_i16(ptr(ib[1:].view(D, H, W)), ptr(got), D, H, W, T, ov, 0, N, lo, hi, st()))
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("T", [32, 224])
def test_tile_gather_i16_of_a_model_sized_slice_is_the_validation_transform(T):
    from vit_unet.torch.dataset import SegmentationBatchTransform
    vol = volume_i16(1, T, T, seed=T)
    d = torch.from_numpy(vol).to(DEV)
    for lo, hi in WINDOWS:
        got = torch.full((1, 1, T, T), float("nan"), device=DEV)
        check(lib().vu_tile_gather_i16(ptr(d), ptr(got), 1, T, T, T, 8, 0, 1, lo, hi, st()))
        want = SegmentationBatchTransform(T, train=False, window=(lo, hi))(vol)["x"]
        assert torch.equal(got, want)


# ---------------------------------------------------------------- 2. blend
def seg_blend(tiles, truth, nz, H, W, T, ov, zthr, label, want=("logits", "mask", "counts"), off=0):
    """One vu_seg_blend call; every output that is wanted starts `off` elements into a pre-filled buffer."""
    L = lib()
    px = nz * H * W
    res, guard = {}, {}
    if "logits" in want:
        guard["logits"] = torch.full((px + off,), float("nan"), device=DEV)
        res["logits"] = guard["logits"][off:].view(nz, H, W)
    if "mask" in want:
        guard["mask"] = torch.full((px + off,), 77, dtype=torch.uint8, device=DEV)
        res["mask"] = guard["mask"][off:].view(nz, H, W)
    scratch, nbytes, tr = None, 0, None
    if "counts" in want:
        res["counts"] = torch.full((nz, 3), -1, dtype=torch.int64, device=DEV)
        nbytes = L.vu_seg_blend_scratch_bytes(nz, H, W)
        scratch = torch.full((nbytes // 4,), -1, dtype=torch.int32, device=DEV)
        tb = torch.zeros(px + off, dtype=torch.uint8, device=DEV)
        tb[off:].copy_(truth.reshape(-1))
        tr = tb[off:].view(nz, H, W)
    check(L.vu_seg_blend(ptr(tiles), ptr(tr), ptr(res.get("logits")), ptr(res.get("mask")), ptr(res.get("counts")), ptr(scratch),
                         nbytes, nz, H, W, T, ov, zthr, label, st()), "vu_seg_blend")
    for k, g in guard.items():                                          # nothing written in front of an offset output
        assert off == 0 or (torch.isnan(g[:off]).all() if k == "logits" else (g[:off] == 77).all())
    return res


@pytest.mark.parametrize("D,H,W,ov,T", VOLUMES)
def test_seg_blend(D, H, W, ov, T):
    L = lib()
    nt = ref_nt(H, W, T, ov)
    rng = np.random.default_rng(nt + H)
    tiles = rng.uniform(-1, 1, (D * nt, 1, T, T)).astype(np.float32)
    truth = rng.integers(0, 3, (D, H, W)).astype(np.uint8)
    vmax = float(np.abs(tiles).max())
    d, tr = torch.from_numpy(tiles).to(DEV), torch.from_numpy(truth).to(DEV)
    # the parent's blend, slice by slice
    tb = torch.full((D, H, W), float("nan"), device=DEV)
    for z in range(D):
        check(L.vu_tile_blend(ptr(d[z * nt:(z + 1) * nt]), ptr(tb[z]), None, H, W, 1, T, ov, st()))
    for thr in (0.5, 0.3):
        zthr = logit_threshold(thr)
        zref, mref = ref_seg_blend(tiles, D, H, W, T, ov, zthr)
        full = seg_blend(d, tr, D, H, W, T, ov, zthr, -1)
        lg, mk = full["logits"], full["mask"]
        assert torch.equal(lg, tb)                                       # bit for bit vu_tile_blend
        err = np.abs(lg.cpu().numpy().astype(np.float64) - zref).max()
        print(f"seg_blend {D}x{H}x{W} T {T} overlap {ov} thr {thr}: max err {err:.3e} (bound {BLEND_TOL * vmax:.3e})")
        assert err <= BLEND_TOL * vmax, err
        assert torch.equal(mk, (lg >= zthr).to(torch.uint8))
        near = np.abs(zref - zthr) <= BLEND_TOL * vmax
        share = near.reshape(D, -1).mean(1).max()
        print(f"  mask: left out at most {100 * share:.4f} % of a slice")
        assert share <= 0.01, share
        mkn = mk.cpu().numpy()
        assert np.array_equal(mkn[~near], mref[~near])
        assert torch.equal(full["counts"].cpu(), torch.from_numpy(ref_counts(mkn, truth, -1)))
        for label in (1, 2):
            c = seg_blend(d, tr, D, H, W, T, ov, zthr, label, want=("counts",))["counts"]
            assert torch.equal(c.cpu(), torch.from_numpy(ref_counts(mkn, truth, label))), label
        # optional outputs omitted one at a time, and a second run: the same bits
        for want in (("mask", "counts"), ("logits", "counts"), ("logits", "mask"), ("logits", "mask", "counts")):
            r = seg_blend(d, tr, D, H, W, T, ov, zthr, -1, want=want)
            for k in want:
                assert torch.equal(r[k], full[k]), (want, k)
        # logits, mask and truth buffers that are 4 / 1 byte aligned only
        for off in (1, 3):
            r = seg_blend(d, tr, D, H, W, T, ov, zthr, -1, off=off)
            for k in ("logits", "mask", "counts"):
                assert torch.equal(r[k], full[k]), (off, k)
        if D > 1:                                                        # nz smaller than D: slices [1, D)
            r = seg_blend(d[nt:], tr[1:], D - 1, H, W, T, ov, zthr, 2)
            assert torch.equal(r["logits"], lg[1:]) and torch.equal(r["mask"], mk[1:])
            assert torch.equal(r["counts"].cpu(), torch.from_numpy(ref_counts(mkn[1:], truth[1:], 2)))


def test_seg_blend_thresholds_at_the_extremes():
    """zthr = -inf sets every pixel and +inf none, whatever the logits, and the counts follow; label 0 counts truth == 0."""
    D, H, W, ov, T = 2, 37, 45, 8, 32
    nt = ref_nt(H, W, T, ov)
    d = torch.full((D * nt, 1, T, T), 0.25, device=DEV)
    tr = torch.ones(D, H, W, dtype=torch.uint8, device=DEV)
    r = seg_blend(d, tr, D, H, W, T, ov, float("-inf"), -1)
    assert (r["mask"] == 1).all() and r["counts"].cpu().tolist() == [[H * W] * 3] * D
    r = seg_blend(d, tr, D, H, W, T, ov, float("inf"), -1)
    assert (r["mask"] == 0).all() and r["counts"].cpu().tolist() == [[0, H * W, 0]] * D
    r = seg_blend(d, tr, D, H, W, T, ov, 0.0, 0)                         # label 0: no truth pixel among the ones
    assert torch.equal(r["mask"], (r["logits"] >= 0).to(torch.uint8)) and r["counts"][:, 1:].cpu().tolist() == [[0, 0]] * D


# ---------------------------------------------------------------- 3. end to end
SMALL = dict(depth=1, depth_te=1, size_bottleneck=1, preprocessing="conv", im_size=32, patch_size=8, num_channels=1,
             hidden_dim=16, num_heads=2, attn_drop=0.2, proj_drop=0.2, linear_drop=0.0)
VOL = (2, 83, 121)          # 20 windows a slice at overlap 8
_cache = {}


def small_model(dtype):
    cfg = O.Config(**SMALL)
    w = O.make_weights(cfg, seed=3)
    m = M.HViT_UNet(dtype=dtype, **SMALL)
    m.load_state_dict({k: v.clone() for k, v in w.items()})
    return m.to(DEV), cfg, w


def volume_and_windows():
    """The test volume (values around the window, so that the model sees more than the two clip levels) and its windows
    under the default intensity window, computed once."""
    if "vol" not in _cache:
        vol = np.random.default_rng(11).integers(-1500, 1500, VOL).astype(np.int16)
        win = ref_volume_windows(vol, 32, 8)
        _cache["vol"], _cache["x"] = vol, O.seg_prepare(win, None, 32, None, -1024.0, 1024.0)[0].contiguous()
    return _cache["vol"], _cache["x"]


def by_hand(m, x, D, nt, batch, ops=(0,)):
    """The documented execution order with the product's own eval forward: groups of G = max(1, batch // nt) slices, chunks
    of `batch` windows inside a group, the self-ensemble loop of TiledRestorer per chunk -> (D nt,1,T,T) float32 numpy."""
    L, T = lib(), x.shape[-1]
    was = m.training
    m.eval()
    G = max(1, batch // nt)
    outs = torch.empty_like(x)
    with torch.no_grad():
        for z0 in range(0, D, G):
            g0, nw = z0 * nt, min(G, D - z0) * nt
            for c0 in range(0, nw, batch):
                n = min(batch, nw - c0)
                xs, o = x[g0 + c0:g0 + c0 + n].contiguous(), outs[g0 + c0:g0 + c0 + n]
                if len(ops) == 1:
                    o.copy_(m(xs))
                    continue
                xt = torch.empty_like(xs)
                for k, op in enumerate(ops):
                    check(L.vu_dihedral_f32(ptr(xs), ptr(xt), n, 1, T, op, 0, 1.0, st()))
                    v = m(xt).clone()
                    check(L.vu_dihedral_f32(ptr(v), ptr(o), n, 1, T, L.vu_dihedral_inverse(op), int(k > 0),
                                            1.0 / len(ops) if k == len(ops) - 1 else 1.0, st()))
    m.train(was)
    return outs.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_segmenter_small_model_against_hand_composition_and_oracle(dtype):
    m, cfg, w = small_model(dtype)
    T, ov, batch = 32, 8, 6
    D, H, W = VOL
    vol, x = volume_and_windows()
    nt = ref_nt(H, W, T, ov)
    assert nt == 20 and nt % batch
    s = TiledSegmenter(m, overlap=ov, batch=batch)
    got = s(vol, output="logits")
    mask = s(torch.from_numpy(vol))                                     # a host torch tensor is taken as well
    assert got.shape == VOL and got.dtype == torch.float32 and got.is_cuda
    assert mask.shape == VOL and mask.dtype == torch.uint8 and mask.is_cuda
    v = by_hand(m, x.to(DEV), D, nt, batch)
    ref, _ = ref_seg_blend(v, D, H, W, T, ov, 0.0)
    vmax = float(np.abs(v).max())
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max()
    print(f"small {dtype}: segmenter vs hand composition {err:.3e} (bound {BLEND_TOL * vmax:.3e}, max|v| {vmax:.3f})")
    assert np.isfinite(v).all() and err <= BLEND_TOL * vmax
    assert torch.equal(mask, (got >= 0).to(torch.uint8))
    assert torch.equal(s(vol, output="prob"), torch.sigmoid(got))
    # a threshold inside the range of this model's logits, so that the mask is neither empty nor full
    thr = float(torch.sigmoid(got.median()))
    s2 = TiledSegmenter(m, overlap=ov, batch=batch, threshold=thr, label=2)
    truth = np.random.default_rng(5).integers(0, 3, VOL).astype(np.uint8)
    sc = s2.score(vol, truth)
    mk = sc["mask"].cpu().numpy()
    assert torch.equal(sc["mask"], (got >= s2.zthr).to(torch.uint8)) and 0 < mk.sum() < mk.size
    want = ref_counts(mk, truth, 2)
    assert sc["counts"].dtype == torch.int64 and not sc["counts"].is_cuda and np.array_equal(sc["counts"].numpy(), want)
    p, t, b = (int(c) for c in want.sum(0))
    assert sc["dice"] == 2 * b / (p + t) == dice_from_counts(p, t, b) and sc["iou"] == b / (p + t - b) == iou_from_counts(p, t, b)
    # dice_tiled / iou_tiled: one value per pair; a (H,W) slice and its truth as the second pair
    pairs = [(vol, truth), (vol[1], truth[1])]
    dt = F.dice_tiled(m, pairs, overlap=ov, batch=batch, threshold=thr, label=2)
    it = F.iou_tiled(m, pairs, overlap=ov, batch=batch, threshold=thr, label=2)
    assert dt.shape == (2,) and it.shape == (2,) and dt[0] == sc["dice"] and it[0] == sc["iou"]
    p1, t1, b1 = (int(c) for c in want[1])
    assert dt[1] == dice_from_counts(p1, t1, b1) and it[1] == iou_from_counts(p1, t1, b1)
    # (H,W) and list inputs; the convenience method builds its segmenter once
    one = s(vol[1], output="logits")
    assert one.shape == (H, W) and torch.equal(one, got[1])
    outs = s([vol, vol[0, :40, :50]])
    assert [tuple(o.shape) for o in outs] == [VOL, (40, 50)] and torch.equal(outs[0], mask)
    assert torch.equal(m.segment(vol, overlap=ov, batch=batch), mask)
    assert len(m._segmenters) == 1 and torch.equal(m.segment(vol, "logits", overlap=ov, batch=batch), got) and len(m._segmenters) == 1
    if dtype == torch.float32:
        # the CPU oracle's eval forward per window, blended in float64: a blend is a convex combination of window outputs,
        # so the forward's bound carries over unchanged: 2e-4 of the scale of the oracle's window outputs
        vo = O.forward(w, cfg, x, training=False).detach().numpy()
        eo = np.abs(got.cpu().numpy().astype(np.float64) - ref_seg_blend(vo, D, H, W, T, ov, 0.0)[0]).max() / np.abs(vo).max()
        print(f"small fp32: segmenter vs oracle windows {eo:.3e}")
        assert eo < 2e-4


@pytest.mark.parametrize("ensemble", [2, 8])
def test_segmenter_ensemble_against_hand_composition(ensemble):
    m, _, _ = small_model(torch.float32)
    T, ov, batch = 32, 8, 45                                            # G = 2: one chunk of 40 windows across both slices
    D, H, W = VOL
    vol, x = volume_and_windows()
    nt = ref_nt(H, W, T, ov)
    got = TiledSegmenter(m, overlap=ov, batch=batch, ensemble=ensemble)(vol, output="logits")
    v = by_hand(m, x.to(DEV), D, nt, batch, TiledRestorer.ENSEMBLE_OPS[ensemble])
    ref, _ = ref_seg_blend(v, D, H, W, T, ov, 0.0)
    vmax = float(np.abs(v).max())
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max()
    print(f"ensemble {ensemble}: segmenter vs hand composition {err:.3e} (bound {BLEND_TOL * vmax:.3e})")
    assert err <= BLEND_TOL * vmax
    plain = TiledSegmenter(m, overlap=ov, batch=batch)(vol, output="logits")
    assert not torch.equal(plain, got)                                  # the ensemble is not the single pass


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_segmenter_is_deterministic_and_leaves_the_model_alone(dtype):
    """Two calls give the same bits; the training flag, the BatchNorm running statistics and the batch counters are
    untouched; the chunk size does not change the logits beyond the blend's bound (2e-6 of the output scale)."""
    m, _, _ = small_model(dtype)
    m.train()
    vol, _ = volume_and_windows()
    m._ensure_flat()
    bn0 = m._bn.clone()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    a = TiledSegmenter(m, overlap=8, batch=20)(vol, output="logits")    # one slice a chunk
    b = TiledSegmenter(m, overlap=8, batch=20)(vol, output="logits")
    assert torch.equal(a, b)
    vmax = float(a.abs().max())          # |blend| <= max|v|, and the bound below only needs a scale that is not larger
    for batch in (45, 7):                # one chunk across both slices; 7 does not divide 20
        c = TiledSegmenter(m, overlap=8, batch=batch)(vol, output="logits")
        d = (c - a).abs().max().item()
        print(f"{dtype} batch {batch} vs batch 20: max diff {d:.3e} ({'bit-identical' if torch.equal(a, c) else 'differs'})")
        assert d <= BLEND_TOL * vmax, d
    assert m.training and all(mod.training for mod in m.modules())
    assert torch.equal(m._bn, bn0)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k
