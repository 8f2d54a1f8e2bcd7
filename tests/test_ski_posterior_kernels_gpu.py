"""The two row kernels of the closed-form SKI posterior (csrc/rpgp_ski_post.hip) on the device, entry by entry against the numpy
restatement within the derived bounds of tests/ski_posterior_reference.py (no margin), at the smallest shapes where they can go
wrong: row counts around the 64- and 256-row pieces of the plan, one to twenty projections, strips and LDS chunks of every
height, T = 0 ... 16, a row stride above J, and coordinates that pile into one cell, sit on nodes, clip at both ends or leave most
cells empty."""
import numpy as np
import pytest
import torch

from oracle import ski as sko
from tests import ski_posterior_reference as R

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 5000]
GRIDS = [(1, 16), (3, 64), (3, 1024), (20, 64)]
COLUMNS = [0, 1, 2, 16]
COORDS = ["uniform", "identical", "nodes", "ends", "clusters", "per_projection", "weights"]


def coordinates(kind, N, J, G, seed):
    """(Z, grid block) as numpy float64."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        Z = rng.uniform(-2.0, 3.0, (N, J))
        return Z, R.block(*sko.grid_params(np.concatenate([Z, [[-2.0] * J, [3.0] * J]]), None, G), J)
    if kind == "weights":                                       # the weights flag and a kind: both parse, neither enters
        Z = rng.uniform(-2.0, 3.0, (N, J))
        g0, h = sko.grid_params(np.concatenate([Z, [[-2.0] * J, [3.0] * J]]), None, G)
        return Z, R.block(g0, h, J, weights=rng.uniform(0.5, 2.0, J), kind="Matern")
    if kind == "per_projection":                                # ranges 100 x apart between the projections
        Z = rng.uniform(-1.0, 1.0, (N, J)) * (100.0 ** (np.arange(J) / max(J - 1, 1)))[None, :]
        ext = np.concatenate([Z, -np.abs(Z).max(0, keepdims=True), np.abs(Z).max(0, keepdims=True) + 1e-3])
        return Z, R.block(*sko.grid_params_reference(ext, None, G), J)
    if kind == "clusters":                                      # three tight clusters: most cells stay empty
        Z = rng.choice([-1.7, 0.4, 2.9], (N, J)) + 1e-4 * rng.standard_normal((N, J))
        return Z, R.block(*sko.grid_params(np.array([[-2.0], [3.0]]), None, G), J)
    g0, h = -2.0, 2.0 ** -3                                     # a power-of-two spacing: the grid coordinate is exact on both sides
    if kind == "identical":                                     # one cell takes everything
        return np.tile(g0 + h * (np.arange(J) % (G - 4) + 1.37), (N, 1)), R.block(g0, h, J)
    if kind == "nodes":                                         # rows exactly on nodes, the first and the last served one included
        m = rng.integers(1, G - 1, (N, J))
        m[0::3, :] = 1
        m[1::3, :] = G - 2
        return g0 + h * m, R.block(g0, h, J)
    if kind == "ends":                                          # beyond both ends: the stencil clips at first tap 0 and G - 4
        u = rng.uniform(-3.0, G + 1.0, (N, J))
        u[0::4, :] = rng.uniform(-3.0, 1.0, u[0::4, :].shape)
        u[1::4, :] = rng.uniform(G - 2.0, G + 1.0, u[1::4, :].shape)
        return g0 + h * u, R.block(g0, h, J)
    raise ValueError(kind)


_ratios = {"A": 0.0, "g": 0.0, "rowsum": 0.0, "quadform": 0.0}


def _record(key, value):
    _ratios[key] = max(_ratios[key], value)
    print("worst %s error / bound so far: %.3g" % (key, _ratios[key]))


def _gram_case(dev, kind, N, J, G, T, seed, ldz=None):
    from rpgp_amd import ops
    Z, gp = coordinates(kind, N, J, G, seed)
    rng = np.random.default_rng(seed + 1)
    Y = rng.standard_normal((N, T)) if T else None
    Zd = torch.from_numpy(Z).to(dev)
    if ldz is not None:                                         # rows of a wider array: unit column stride, row stride ldz
        wide = torch.full((N, ldz), float("nan"), dtype=torch.float64, device=dev)
        wide[:, :J] = Zd
        Zd = wide[:, :J]
        assert Zd.stride(0) == ldz
    gpd = torch.from_numpy(gp).to(dev)
    Yd = None if Y is None else torch.from_numpy(Y).to(dev)
    A, g = ops.ski_gram(Zd, gpd, Yd, grid_size=G)
    A2, g2 = ops.ski_gram(Zd, gpd, Yd, grid_size=G)
    assert torch.equal(A, A.t()), "A is not bitwise symmetric"
    assert torch.equal(A, A2) and (g is None or torch.equal(g, g2)), "a second call is not bit-identical"
    assert (g is None) == (T == 0) and (g is None or tuple(g.shape) == (J * G, T))
    A, g = A.cpu().numpy(), None if g is None else g.cpu().numpy()
    A_ref, g_ref = R.gram(Z, gp, G, Y)
    bA, bg = R.gram_bound(Z, gp, G, Y)
    ra = R.worst_ratio(A, A_ref, bA)
    rg = 0.0 if Y is None else R.worst_ratio(g, g_ref, bg)
    rs = R.block_row_sums(A, Z, gp, G, bA)
    print("%s N=%d J=%d G=%d T=%d: A %.3g, g %.3g, row sums %.3g of the bound" % (kind, N, J, G, T, ra, rg, rs))
    _record("A", ra)
    _record("g", rg)
    _record("rowsum", rs)
    assert ra <= 1.0 and rg <= 1.0 and rs <= 1.0, (ra, rg, rs)


@pytest.mark.parametrize("J, G", GRIDS)
@pytest.mark.parametrize("N", SIZES)
def test_gram_sizes(gpu_device, N, J, G):
    T = COLUMNS[(SIZES.index(N) + GRIDS.index((J, G))) % 4]     # every T meets every grid and every row count class
    _gram_case(gpu_device, "uniform", N, J, G, T, seed=1000 * J + N)


@pytest.mark.parametrize("kind", COORDS[1:])
@pytest.mark.parametrize("J, G, N, T", [(3, 64, 257, 2), (1, 16, 65, 16), (20, 64, 257, 1), (3, 1024, 5000, 1)])
def test_gram_coordinates(gpu_device, kind, J, G, N, T):
    _gram_case(gpu_device, kind, N, J, G, T, seed=7 * J + G)


@pytest.mark.parametrize("T", COLUMNS)
def test_gram_columns_and_row_stride(gpu_device, T):
    _gram_case(gpu_device, "uniform", 257, 3, 64, T, seed=50 + T)
    _gram_case(gpu_device, "uniform", 65, 3, 64, T, seed=60 + T, ldz=5)


def _quadform_case(dev, kind, M, J, G, seed, ldz=None, identity=False):
    from rpgp_amd import ops
    Z, gp = coordinates(kind, M, J, G, seed)
    rng = np.random.default_rng(seed + 2)
    n = J * G
    C = np.eye(n) if identity else rng.standard_normal((n, n))  # (not symmetric: both triangles are read, nothing doubled)
    Zd = torch.from_numpy(Z).to(dev)
    if ldz is not None:
        wide = torch.full((M, ldz), float("nan"), dtype=torch.float64, device=dev)
        wide[:, :J] = Zd
        Zd = wide[:, :J]
    gpd, Cd = torch.from_numpy(gp).to(dev), torch.from_numpy(C).to(dev)
    out = ops.ski_quadform(Zd, gpd, Cd, grid_size=G)
    assert torch.equal(out, ops.ski_quadform(Zd, gpd, Cd, grid_size=G)), "a second call is not bit-identical"
    out = out.cpu().numpy()
    r = R.check_quadform(out, Z, gp, G, C)
    if identity:                                                # C = I gives sum w^2
        g0, h, _, _ = R.parse_block(gp, J)
        W = R.interp(Z, g0, h, G)
        w2 = np.asarray(W.multiply(W).sum(axis=1)).reshape(-1)
        r = max(r, R.worst_ratio(out, w2, R.quadform_bound(Z, gp, G, C)))
    print("%s M=%d J=%d G=%d: quadratic form %.3g of the bound" % (kind, M, J, G, r))
    _record("quadform", r)
    assert r <= 1.0, r


@pytest.mark.parametrize("J, G", GRIDS)
@pytest.mark.parametrize("M", SIZES)
def test_quadform_sizes(gpu_device, M, J, G):
    _quadform_case(gpu_device, "uniform", M, J, G, seed=2000 * J + M, identity=(M == 65))


@pytest.mark.parametrize("kind", COORDS[1:])
def test_quadform_coordinates_and_row_stride(gpu_device, kind):
    _quadform_case(gpu_device, kind, 257, 3, 64, seed=77)
    _quadform_case(gpu_device, kind, 63, 20, 64, seed=78, ldz=23)


def test_error_codes(gpu_device):
    from rpgp_amd import _lib, ops
    lib = _lib.load()
    dev = gpu_device
    N, J, G, T = 40, 3, 64, 2
    Z, gp = coordinates("uniform", N, J, G, 5)
    Zd, gpd = torch.from_numpy(Z).to(dev), torch.from_numpy(gp).to(dev)
    Y = torch.zeros((N, T), dtype=torch.float64, device=dev)
    A = torch.zeros((J * G, J * G), dtype=torch.float64, device=dev)
    g = torch.zeros((J * G, T), dtype=torch.float64, device=dev)
    out = torch.zeros(N, dtype=torch.float64, device=dev)
    need = lib.rpgp_ski_gram_f64_workspace_bytes(N, J, G, T)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream

    def gram(Z=p(Zd), gp=p(gpd), Y=p(Y), A=p(A), g=p(g), N=N, ldz=J, J=J, G=G, T=T, w=p(ws), wb=need):
        return lib.rpgp_ski_gram_f64(Z, gp, Y, A, g, N, ldz, J, G, T, w, wb, st)

    def quad(Z=p(Zd), gp=p(gpd), C=p(A), out=p(out), M=N, ldz=J, J=J, G=G, ldc=J * G):
        return lib.rpgp_ski_quadform_f64(Z, gp, C, out, M, ldz, J, G, ldc, st)

    assert gram() == 0 and quad() == 0
    assert gram(T=0, Y=None, g=None) == 0                       # Y and g may be NULL when T == 0
    E, W = _lib.RPGP_EINVAL, _lib.RPGP_EWORKSPACE
    for bad in (dict(J=0), dict(G=7), dict(G=8193), dict(T=-1), dict(T=17), dict(N=0), dict(ldz=J - 1), dict(Z=None), dict(gp=None),
                dict(A=None), dict(Y=None), dict(g=None), dict(Z=p(Zd) + 4), dict(A=p(A) + 4), dict(Y=p(Y) + 4), dict(g=p(g) + 4),
                dict(w=p(ws) + 8)):
        assert gram(**bad) == E, bad
    assert gram(wb=need - 1) == W and gram(w=None) == W
    for shape in ((0, J, G, T), (N, 0, G, T), (N, J, 7, T), (N, J, G, 17), (N, J, G, -1)):
        assert lib.rpgp_ski_gram_f64_workspace_bytes(*shape) == 0
    for bad in (dict(J=0), dict(G=7), dict(M=0), dict(ldz=J - 1), dict(ldc=J * G - 1), dict(Z=None), dict(gp=None), dict(C=None),
                dict(out=None), dict(Z=p(Zd) + 4), dict(C=p(A) + 4), dict(out=p(out) + 4)):
        assert quad(**bad) == E, bad
    torch.cuda.synchronize()
    # the Python layer: float64 on the device only, shapes checked before the call
    with pytest.raises(TypeError):
        ops.ski_gram(Zd.float(), gpd, None, grid_size=G)
    with pytest.raises(RuntimeError):
        ops.ski_gram(Zd.cpu(), gpd.cpu(), None, grid_size=G)
    with pytest.raises(TypeError):
        ops.ski_quadform(Zd, gpd, A[:, :-1], grid_size=G)
    with pytest.raises(ValueError):
        ops.ski_gram(Zd, gpd, torch.zeros((N, 17), dtype=torch.float64, device=dev), grid_size=G)
