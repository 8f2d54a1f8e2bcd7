"""The full radial kernels (csrc/rpgp_radial.hip: rpgp_radial_mvm / _dense / _bilinear_grad) through the C-ABI against the float64
family oracle with one component of group = d (tests/radial_reference.py): the entry bound and the max-abs gate of the dense
block, the row bound and the norm-wise gate of the product, the norm-wise gates of both forms of the derivative — at every tiling
edge (d = 1 ... 385 around the feature chunks of 4 and 32 and the 128-feature slices, rows and columns around the 64-wide tiles,
T = 1 / 11 / 16), for all four kinds, with one pair of exact duplicate rows and one pair at 1 + 1e-4 in every input."""
import numpy as np
import pytest
import torch

from tests import radial_reference as rr

pytestmark = pytest.mark.gpu

SCALE, NOISE = 0.7, 0.13


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("kind,d,N,M,T", rr.cases())
def test_radial_kernels_match_float64(gpu_device, kind, d, N, M, T):
    from rpgp_amd import ops
    rng = np.random.default_rng(1000 + d + N)
    Z, Z1 = rr.inputs(N, d, d + N), rr.inputs(M, d, d + N + 1)
    V = rng.standard_normal((N, T)).astype(np.float32)
    Zt, Z1t, Vt = _dev(Z, gpu_device), _dev(Z1, gpu_device), _dev(V, gpu_device)
    figures = {}
    # product: symmetric with noise, rectangular; bit-identical when repeated
    sym = ops.radial_mvm(kind, Zt, None, Vt, SCALE, NOISE)
    assert torch.equal(sym, ops.radial_mvm(kind, Zt, None, Vt, SCALE, NOISE))
    figures["sym"] = rr.check_product(sym.cpu().numpy(), Z, None, V, kind, SCALE, NOISE)
    rect = ops.radial_mvm(kind, Z1t, Zt, Vt, SCALE)
    assert torch.equal(rect, ops.radial_mvm(kind, Z1t, Zt, Vt, SCALE))
    figures["rect"] = rr.check_product(rect.cpu().numpy(), Z1, Z, V, kind, SCALE)
    # the symmetric form equals the rectangular form on the same Z (they differ in the forced diagonal only)
    same = ops.radial_mvm(kind, Zt, Zt.clone(), Vt, SCALE).cpu().numpy().astype(np.float64)
    assert np.abs(sym.cpu().numpy() - NOISE * V - same).max() <= 2.0 * rr.row_bound(Z, Z, V, kind, SCALE).max()
    # the diagonal contribution is exact: V = e_i gives out[i] == scale + noise
    eye = np.eye(N, dtype=np.float32)[:, :min(N, 16)]
    dg = ops.radial_mvm(kind, Zt, None, _dev(eye, gpu_device), SCALE, NOISE).cpu().numpy()
    assert all(dg[i, i] == np.float32(SCALE) + np.float32(NOISE) for i in range(eye.shape[1]))
    # dense block: rectangular, and the square block of one Z (exact diagonal)
    Kd = ops.radial_dense(kind, Z1t, Zt, 1.3)
    assert torch.equal(Kd, ops.radial_dense(kind, Z1t, Zt, 1.3))
    figures["dense"] = rr.check_dense(Kd.cpu().numpy(), Z1, Z, kind, 1.3)
    Ks = ops.radial_dense(kind, Zt, Zt, 1.3).cpu().numpy()
    rr.check_dense(Ks, Z, Z, kind, 1.3)
    assert (np.diag(Ks) == np.float32(1.3)).all()
    # derivative: factors and explicit S
    n = rr.grad_rows(d, N)
    Zg, Zgt = Z[:n], _dev(Z[:n], gpu_device)
    L, R = rng.standard_normal((n, T)).astype(np.float32), rng.standard_normal((n, T)).astype(np.float32)
    Lt, Rt = _dev(L, gpu_device), _dev(R, gpu_device)
    gZ, gs = ops.radial_bilinear_grad(kind, Zgt, Lt, Rt, 1.3)
    gZ2, gs2 = ops.radial_bilinear_grad(kind, Zgt, Lt, Rt, 1.3)
    assert torch.equal(gZ, gZ2) and torch.equal(gs, gs2)
    figures["grad"] = rr.check_grad(gZ.cpu().numpy(), float(gs), *rr.grad_factors(Zg, L, R, kind, 1.3))
    S = rng.standard_normal((n, n)).astype(np.float32)
    S = ((S + S.T) / 2).astype(np.float32)
    St = _dev(S, gpu_device)
    gZ, gs = ops.radial_bilinear_grad_dense(kind, Zgt, St, 1.3)
    gZ2, gs2 = ops.radial_bilinear_grad_dense(kind, Zgt, St, 1.3)
    assert torch.equal(gZ, gZ2) and torch.equal(gs, gs2)
    figures["gradS"] = rr.check_grad(gZ.cpu().numpy(), float(gs), *rr.grad_dense(Zg, S, kind, 1.3))
    print("radial %s d=%d N=%d M=%d T=%d: %s" % (kind, d, N, M, T, {k: tuple("%.2e" % x for x in v) for k, v in figures.items()}))


def test_radial_wide_blocks_go_through_in_pieces(gpu_device):
    """More than 16 columns: 16-column pieces of the product, summed pieces of the derivative."""
    from rpgp_amd import ops
    kind, d, N, T = "Matern", 21, 129, 19
    rng = np.random.default_rng(3)
    Z = rr.inputs(N, d, 3)
    V, L, R = (rng.standard_normal((N, T)).astype(np.float32) for _ in range(3))
    Zt = _dev(Z, gpu_device)
    rr.check_product(ops.radial_mvm(kind, Zt, None, _dev(V, gpu_device), SCALE, NOISE).cpu().numpy(), Z, None, V, kind, SCALE,
                     NOISE)
    gZ, gs = ops.radial_bilinear_grad(kind, Zt, _dev(L, gpu_device), _dev(R, gpu_device), 1.3)
    rr.check_grad(gZ.cpu().numpy(), float(gs), *rr.grad_factors(Z, L, R, kind, 1.3))


def test_radial_argument_errors(gpu_device):
    """RPGP_EINVAL for d = 0, d = 1025, T = 17 (and T = 0), a null or misaligned pointer, a short leading dimension; RPGP_EWORKSPACE
    for a short workspace."""
    from rpgp_amd import _lib
    lib = _lib.load()
    N = 40
    Z = torch.zeros(N, 1025, device=gpu_device)
    V = torch.zeros(N, 17, device=gpu_device)
    out = torch.empty(N, 17, device=gpu_device)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=gpu_device)
    st = torch.cuda.current_stream().cuda_stream

    def mvm(d=8, T=4, z=None, v=None, o=None, w=None, ld=1025, wsz=None, kind=0):
        return lib.rpgp_radial_mvm(kind, Z.data_ptr() if z is None else z, None, V.data_ptr() if v is None else v,
                                   out.data_ptr() if o is None else o, N, N, d, ld, ld, T, 1.0, 0.0,
                                   ws.data_ptr() if w is None else w, ws.numel() if wsz is None else wsz, st)
    assert mvm() == 0
    for bad in (dict(d=0), dict(d=1025), dict(T=17), dict(T=0), dict(kind=4), dict(kind=-1), dict(z=0), dict(v=0), dict(o=0),
                dict(w=0), dict(z=Z.data_ptr() + 2), dict(v=V.data_ptr() + 1), dict(w=ws.data_ptr() + 4), dict(d=8, ld=7)):
        assert mvm(**bad) == _lib.RPGP_EINVAL, bad
    assert mvm(wsz=16) == _lib.RPGP_EWORKSPACE
    assert lib.rpgp_radial_mvm(0, Z.data_ptr(), None, V.data_ptr(), out.data_ptr(), N, N + 1, 8, 1025, 1025, 4, 1.0, 0.0,
                               ws.data_ptr(), ws.numel(), st) == _lib.RPGP_EINVAL      # symmetric needs M == N
    K = torch.empty(N, N, device=gpu_device)
    g = torch.empty(N, 1025, device=gpu_device)
    gs = torch.empty(1, device=gpu_device)
    for d in (0, 1025):
        assert lib.rpgp_radial_dense(0, Z.data_ptr(), Z.data_ptr(), K.data_ptr(), N, N, d, 1025, 1025, N, 1.0, ws.data_ptr(),
                                     ws.numel(), st) == _lib.RPGP_EINVAL
        assert lib.rpgp_radial_bilinear_grad(0, Z.data_ptr(), V.data_ptr(), V.data_ptr(), None, g.data_ptr(), gs.data_ptr(), N,
                                             d, 1025, 1025, 4, 0, 1.0, ws.data_ptr(), ws.numel(), st) == _lib.RPGP_EINVAL
    assert lib.rpgp_radial_dense(0, Z.data_ptr(), Z.data_ptr(), K.data_ptr(), N, N, 8, 1025, 1025, N - 1, 1.0, ws.data_ptr(),
                                 ws.numel(), st) == _lib.RPGP_EINVAL
    for T in (0, 17):
        assert lib.rpgp_radial_bilinear_grad(0, Z.data_ptr(), V.data_ptr(), V.data_ptr(), None, g.data_ptr(), gs.data_ptr(), N,
                                             8, 1025, 1025, T, 0, 1.0, ws.data_ptr(), ws.numel(), st) == _lib.RPGP_EINVAL
    assert lib.rpgp_radial_bilinear_grad(0, Z.data_ptr(), None, None, K.data_ptr(), g.data_ptr(), gs.data_ptr(), N, 8, 1025,
                                         1025, 0, N - 1, 1.0, ws.data_ptr(), ws.numel(), st) == _lib.RPGP_EINVAL
    assert lib.rpgp_radial_workspace_bytes(0, 5, 1) == 0 and lib.rpgp_radial_workspace_bytes(5, 5, 17) == 0
    torch.cuda.synchronize()


def test_radial_large_n_symmetric_equals_rectangular_and_is_linear(gpu_device):
    """Size-independent properties at a size the dense oracle cannot reach (N = 20011, d = 33: two feature chunks, a ragged
    last tile): the symmetric product equals the rectangular one on the same Z, and the operator is linear."""
    from rpgp_amd import ops
    N, d = 20011, 33
    for kind in ("Matern", "RBF", "InverseMQ"):
        rng = np.random.default_rng(1)
        Z = rr.inputs(N, d, 1)
        V = rng.standard_normal((N, 2)).astype(np.float32)
        Zt, Vt = _dev(Z, gpu_device), _dev(V, gpu_device)
        a = ops.radial_mvm(kind, Zt, None, Vt, 0.5, 0.0)
        b = ops.radial_mvm(kind, Zt, Zt.clone(), Vt, 0.5)
        assert float((a - b).norm() / b.norm()) < 3e-6
        c = ops.radial_mvm(kind, Zt, None, 2.0 * Vt[:, :1] - 3.0 * Vt[:, 1:], 0.5, 0.0)
        assert float((c - (2.0 * a[:, :1] - 3.0 * a[:, 1:])).norm() / c.norm()) < 3e-6
