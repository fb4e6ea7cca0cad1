"""Native-resolution patches and the self-ensemble, host side (no GPU): the numpy restatement of the eight dihedral ops
that tests/test_gpu_patch.py holds the HIP kernels of csrc/vu_patch.hip against, the crop tables `DenoisingPatchTransform`
draws, and every argument error the C entries report before any GPU call."""
import ctypes as C

import numpy as np
import pytest

from vit_unet.torch import _lib
from vit_unet.torch.dataset import DenoisingPatchTransform, dihedral_inverse
from vit_unet.torch.restore import TiledRestorer


# ---------------------------------------------------------------- numpy restatement (the definition of the header)
def ref_dihedral(p, op):
    """(T,T,...) patch -> D_op(p): op & 3 counter-clockwise quarter turns of the (left-right flipped when op & 4) patch."""
    return np.rot90(np.fliplr(p) if op & 4 else p, k=op & 3, axes=(0, 1))


def closed_form_inverse(op):
    return op if op & 4 else (4 - op) & 3


def ref_patches(img, T, crops):
    """(H,W,C) image, [(y0, x0, op)] -> (n,T,T,C) patches D_op(img[y0:y0+T, x0:x0+T])."""
    return np.stack([np.ascontiguousarray(ref_dihedral(img[y0:y0 + T, x0:x0 + T], op)) for y0, x0, op in crops])


# ---------------------------------------------------------------- 1. the eight ops
def test_eight_ops_are_distinct_and_invert():
    p = np.arange(6 * 6 * 2).reshape(6, 6, 2)
    outs = [ref_dihedral(p, op) for op in range(8)]
    for a in range(8):
        for b in range(a + 1, 8):
            assert not np.array_equal(outs[a], outs[b]), (a, b)
    for op in range(8):
        inv = dihedral_inverse(op)
        assert inv == closed_form_inverse(op) == _lib.lib().vu_dihedral_inverse(op)
        assert np.array_equal(ref_dihedral(ref_dihedral(p, op), inv), p), op
    assert [dihedral_inverse(op) for op in range(8)] == [0, 3, 2, 1, 4, 5, 6, 7]


def test_dihedral_inverse_outside_the_range():
    L = _lib.lib()
    for op in (-1, 8, 100, -8):
        assert L.vu_dihedral_inverse(op) < 0
        with pytest.raises(_lib.VuError):
            dihedral_inverse(op)


def test_index_formulas():
    T = 5
    p = np.arange(T * T).reshape(T, T)
    for op in range(8):
        m = p[:, ::-1] if op & 4 else p                     # m[a,b] = p[a, T-1-b]
        out = ref_dihedral(p, op)
        for i in range(T):
            for j in range(T):
                want = (m[i, j], m[j, T - 1 - i], m[T - 1 - i, T - 1 - j], m[T - 1 - j, i])[op & 3]
                assert out[i, j] == want, (op, i, j)


# ---------------------------------------------------------------- 2. the draws
def test_patch_transform_draws():
    sizes = [(83, 121), (40, 33), (224, 300), (32, 32)]
    T = 32
    a = DenoisingPatchTransform(T, per_image=5, seed=7).draw(sizes)
    b = DenoisingPatchTransform(T, per_image=5, seed=7).draw(sizes)
    c = DenoisingPatchTransform(T, per_image=5, seed=8).draw(sizes)
    assert a.shape == (4, 5, 3) and a.dtype == np.int32
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    t = DenoisingPatchTransform(T, per_image=64, seed=1)
    big = np.concatenate([t.draw(sizes) for _ in range(4)], axis=1)
    for k, (H, W) in enumerate(sizes):
        assert big[k, :, 0].min() >= 0 and big[k, :, 0].max() <= H - T
        assert big[k, :, 1].min() >= 0 and big[k, :, 1].max() <= W - T
        assert big[k, :, 2].min() >= 0 and big[k, :, 2].max() <= 7
    assert set(big[0, :, 2].tolist()) == set(range(8))          # 256 draws: every op turns up
    assert big[0, :, 0].max() > 40 and big[0, :, 1].max() > 70  # and the far corner region is reached
    assert (big[3, :, :2] == 0).all()                           # H == W == T: only the origin
    v = DenoisingPatchTransform(T, per_image=5, train=False)
    assert v.per_image == 1
    assert v.draw(sizes).tolist() == [[[25, 44, 0]], [[4, 0, 0]], [[96, 134, 0]], [[0, 0, 0]]]
    with pytest.raises(_lib.VuError):
        t.draw([(31, 100)])
    with pytest.raises(_lib.VuError):
        DenoisingPatchTransform(T, std=0.0)
    with pytest.raises(_lib.VuError):
        DenoisingPatchTransform(0)


def test_restorer_ensemble_argument():
    from vit_unet.torch import model as M
    m = M.HViT_UNet(1, 1, 1, "conv", 32, 8, 3, 16, 2, 0., 0., 0.)
    for bad in (3, 0, 16, -1, "8", None):
        with pytest.raises(_lib.VuError, match="ensemble"):
            TiledRestorer(m, overlap=8, ensemble=bad)
    for k, ops in ((1, (0,)), (2, (0, 4)), (4, (0, 1, 2, 3)), (8, tuple(range(8)))):
        r = TiledRestorer(m, overlap=8, ensemble=k)
        assert r.ensemble == k and TiledRestorer.ENSEMBLE_OPS[k] == ops
    assert TiledRestorer(m, overlap=8).ensemble == 1
    with pytest.raises(_lib.VuError, match="ensemble"):
        m.restore(np.zeros((40, 40, 3), np.uint8), overlap=8, ensemble=3)


# ---------------------------------------------------------------- 3. argument errors of the C entries (before any GPU call)
def test_patch_argument_errors():
    L = _lib.lib()
    # the checks return before any pointer is used: host buffers stand in for device memory
    u8 = (C.c_uint8 * 4096)()
    f = (C.c_float * 4096)()
    tab = (C.c_int * 12)()
    n_, c_, x_, y_, t_ = (C.cast(b, C.c_void_p) for b in (u8, u8, f, f, tab))

    def pp(noisy=n_, clean=c_, x=x_, y=y_, H=16, W=16, Cn=3, T=8, crops=t_, n=4, mean=0.456, std=0.224):
        return L.vu_patch_pairs_u8(noisy, clean, x, y, H, W, Cn, T, crops, n, mean, std, None)

    for call, word in ((lambda: pp(H=7), "smaller"), (lambda: pp(W=7), "smaller"), (lambda: pp(Cn=5), "channels"),
                       (lambda: pp(Cn=0), "channels"), (lambda: pp(std=0.0), "std"), (lambda: pp(n=0), "no crop"),
                       (lambda: pp(T=0), "patch size"), (lambda: pp(crops=None), "null"),
                       (lambda: pp(noisy=None, clean=None, x=None, y=None), "null"),
                       (lambda: pp(noisy=None), "null"), (lambda: pp(y=None), "null")):
        assert call() < 0
        assert word in L.vu_last_error().decode(), L.vu_last_error()


def test_dihedral_argument_errors():
    L = _lib.lib()
    f = (C.c_float * 4096)()
    base = C.addressof(f)
    src, dst = C.c_void_p(base), C.c_void_p(base + 4 * 2048)

    def dh(s=src, d=dst, n=2, Cn=3, T=8, op=0, acc=0, scale=1.0):
        return L.vu_dihedral_f32(s, d, n, Cn, T, op, acc, scale, None)

    for call, word in ((lambda: dh(op=8), "op"), (lambda: dh(op=-1), "op"), (lambda: dh(n=0), "empty"), (lambda: dh(T=0), "empty"),
                       (lambda: dh(Cn=0), "empty"), (lambda: dh(s=None), "null"), (lambda: dh(d=None), "null"),
                       (lambda: dh(d=src), "overlap"),                                       # in place
                       (lambda: dh(d=C.c_void_p(base + 4 * 383)), "overlap"),                # the last float of src
                       (lambda: dh(s=dst, d=C.c_void_p(base + 4 * 2048 - 4 * 383)), "overlap")):
        assert call() < 0
        assert word in L.vu_last_error().decode(), L.vu_last_error()
