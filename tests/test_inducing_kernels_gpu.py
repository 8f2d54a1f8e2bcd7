"""The inducing-point sums (csrc/rpgp_inducing.hip: rpgp_inducing_gram / _grad) through ops against float64
(tests/sgpr_reference.py): the derived bounds of G and g, the norm-wise gate of the derivative for random well-scaled C and v —
all four kinds, d = 1 ... 385 around the feature chunks of 4 and 32, rows around the 64-row blocks, M around the 64-column tiles
up to the limit 1024, T = 0 / 1 / 2 / 16, with duplicate and near-duplicate rows among the inducing points.  Every case runs with
the default workspace and with the 64-row one, so that N = 257 and N = 1237 cross slab edges."""
import numpy as np
import pytest
import torch

from tests import sgpr_reference as sr

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("kind,d,N,M,T", sr.kernel_cases())
def test_inducing_sums_match_float64(gpu_device, kind, d, N, M, T):
    from rpgp_amd import ops
    Z, U, Y, C, v = sr.kernel_inputs(kind, d, N, M, T)
    Zt, Ut, Ct = _dev(Z, gpu_device), _dev(U, gpu_device), _dev(C, gpu_device)
    Yt, vt = (_dev(Y, gpu_device), _dev(v, gpu_device)) if T else (None, None)
    ref_grad = sr.sums_grad(Z, U, Y, C, v, kind)
    out, figures = {}, {}
    for rows in (None, 64):
        G, g = ops.inducing_gram(kind, Zt, Ut, Yt, rows=rows)
        G2, g2 = ops.inducing_gram(kind, Zt, Ut, Yt, rows=rows)
        assert torch.equal(G, G2) and torch.equal(g, g2)                       # repeated calls are bit-identical
        assert G.dtype == torch.float64 and tuple(G.shape) == (M, M) and tuple(g.shape) == (M, T)
        figures["sums", rows] = sr.check_sums(G.cpu().numpy(), g.cpu().numpy(), Z, U, Y, kind)
        gU, q = ops.inducing_grad(kind, Zt, Ut, Yt, Ct, vt, rows=rows)
        gU2, q2 = ops.inducing_grad(kind, Zt, Ut, Yt, Ct, vt, rows=rows)
        assert torch.equal(gU, gU2) and torch.equal(q, q2)
        assert gU.dtype == torch.float64 and tuple(gU.shape) == (M, d) and tuple(q.shape) == (d,)
        figures["grad", rows] = sr.check_grad(gU.cpu().numpy(), q.cpu().numpy(), *ref_grad)
        out[rows] = [t.cpu().numpy() for t in (G, g, gU, q)]
    print("inducing %s d=%d N=%d M=%d T=%d: %s" % (kind, d, N, M, T, {k: tuple("%.2e" % x for x in f) for k, f in figures.items()}))
    # the two slab lengths: the same sums in another order (float64)
    for a, b in zip(out[None], out[64]):
        scale = max(float(np.abs(a).max()), 1e-300) if a.size else 1.0
        assert a.size == 0 or float(np.abs(a - b).max()) <= 1e-12 * scale


def test_inducing_argument_errors(gpu_device):
    """RPGP_EINVAL for d = 0 / 1025, M = 0 / 1025, T = -1 / 17, an unknown kind, a null or misaligned pointer, a short leading
    dimension; RPGP_EWORKSPACE below the 64-row workspace; any size from there up is accepted."""
    from rpgp_amd import _lib
    lib = _lib.load()
    N, M, d, T = 40, 9, 8, 2
    Z = torch.zeros(N, 1025, device=gpu_device)
    U = torch.zeros(M, 1025, device=gpu_device)
    Y = torch.zeros(N, 16, device=gpu_device)
    G = torch.empty(1025 * 8, dtype=torch.float64, device=gpu_device)
    g = torch.empty(1025 * 2, dtype=torch.float64, device=gpu_device)
    Cm = torch.zeros(M, M, dtype=torch.float64, device=gpu_device)
    v = torch.zeros(M, T, dtype=torch.float64, device=gpu_device)
    gU = torch.empty(M, 1025, dtype=torch.float64, device=gpu_device)
    q = torch.empty(1025, dtype=torch.float64, device=gpu_device)
    ws = torch.empty(8 << 20, dtype=torch.uint8, device=gpu_device)
    st = torch.cuda.current_stream().cuda_stream
    floor = lib.rpgp_inducing_workspace_bytes(M, d, T, 64)
    assert 0 < floor <= ws.numel() and lib.rpgp_inducing_workspace_bytes(M, d, T, 1) == floor
    assert lib.rpgp_inducing_workspace_bytes(M, d, T, 65) > floor
    assert lib.rpgp_inducing_workspace_bytes(M, d, T, 64) == lib.rpgp_inducing_workspace_bytes(M, d, T, 64)
    for bad in ((0, d, T), (1025, d, T), (M, 0, T), (M, 1025, T), (M, d, -1), (M, d, 17)):
        assert lib.rpgp_inducing_workspace_bytes(*bad, 64) == 0, bad
    assert lib.rpgp_inducing_workspace_bytes(M, d, T, 0) == 0

    def gram(kind=0, z=None, u=None, y=None, G_=None, g_=None, n=N, m=M, d_=d, ldz=1025, ldu=1025, t=T, w=None, wsz=floor):
        return lib.rpgp_inducing_gram(kind, Z.data_ptr() if z is None else z, U.data_ptr() if u is None else u,
                                      Y.data_ptr() if y is None else y, G.data_ptr() if G_ is None else G_,
                                      g.data_ptr() if g_ is None else g_, n, m, d_, ldz, ldu, t,
                                      ws.data_ptr() if w is None else w, wsz, st)

    def grad(kind=0, z=None, c=None, v_=None, o=None, q_=None, m=M, d_=d, ldz=1025, t=T, w=None, wsz=floor):
        return lib.rpgp_inducing_grad(kind, Z.data_ptr() if z is None else z, U.data_ptr(), Y.data_ptr(),
                                      Cm.data_ptr() if c is None else c, v.data_ptr() if v_ is None else v_,
                                      gU.data_ptr() if o is None else o, q.data_ptr() if q_ is None else q_, N, m, d_, ldz, 1025,
                                      t, ws.data_ptr() if w is None else w, wsz, st)
    assert gram() == 0 and grad() == 0
    assert gram(wsz=ws.numel()) == 0 and grad(wsz=floor + 12345) == 0              # more bytes: longer slabs, any size
    assert gram(t=0, y=0, g_=0) == 0                                               # T = 0: no Y, no g
    for bad in (dict(d_=0), dict(d_=1025), dict(m=0), dict(m=1025), dict(t=17), dict(t=-1), dict(kind=4), dict(kind=-1),
                dict(z=0), dict(u=0), dict(y=0), dict(G_=0), dict(g_=0), dict(w=0), dict(n=0), dict(z=Z.data_ptr() + 2),
                dict(G_=G.data_ptr() + 4), dict(w=ws.data_ptr() + 4), dict(ldz=7), dict(ldu=7)):
        assert gram(**bad) == _lib.RPGP_EINVAL, bad
    for bad in (dict(d_=0), dict(d_=1025), dict(m=0), dict(m=1025), dict(t=17), dict(kind=4), dict(z=0), dict(c=0), dict(v_=0),
                dict(o=0), dict(q_=0), dict(w=0), dict(c=Cm.data_ptr() + 4), dict(ldz=7)):
        assert grad(**bad) == _lib.RPGP_EINVAL, bad
    assert gram(wsz=floor - 1) == _lib.RPGP_EWORKSPACE and grad(wsz=16) == _lib.RPGP_EWORKSPACE
    torch.cuda.synchronize()
