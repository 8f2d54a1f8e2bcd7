"""References for the inducing-point (SGPR) path — test helpers.

1. `sums` / `sums_grad`: float64 numpy statements of what rpgp_inducing_gram / rpgp_inducing_grad compute, on the float32 inputs
   exactly as the kernels receive them, with the derived bounds
       |delta G_jk| <= sum_i (|dK_ij| |K_ik| + |K_ij| |dK_ik|) + N 2^-53 sum_i |K_ij K_ik|      (dK: radial_reference.entry_bound)
       |delta g_jt| <= sum_i |dK_ij| |Y_it| + N 2^-53 sum_i |K_ij Y_it|
   and the norm-wise gate radial_reference.GATE_GRAD_REL of the derivative.
2. `dense_objective`: the collapsed bound by the DENSE N x N form — s Q + sigma^2 I is built and factorised, independent of the
   Woodbury algebra of rpgp_amd/sgpr.py — in float64 torch, its gradients by autograd; `dense_prediction` likewise.
3. `Emulation`: the kernel path in numpy — Gram-form float32 kernel entries (radial_reference's), float64 everywhere else, S
   rounded to float32 once — with the mutation table DEFECTS.  tests/test_sgpr_host.py holds the clean emulation to every gate
   and shows that every defect misses at least one.

GPU_CASES holds the cases of tests/test_sgpr_gpu.py with the relative error of every gradient of the clean emulation there: the
gradient gate of a case is 4 x that figure, and tests/test_sgpr_host.py re-derives the figures on the host.
"""
import math

import numpy as np
import torch

from oracle import family as fmo
from tests import radial_reference as rr

# (N, d, M, lengthscale) -> relative error of every gradient of the clean emulation against float64 on `problem` at
# s = 1.3, sigma^2 = 0.2, c = 0.1, RBF (see the module docstring); cond(K_uu) = 2.8e3 and 2.4e3
GPU_CASES = {
    (1500, 8, 64, 2.5): {"U": 1.7e-6, "ls": 1.7e-7, "s": 7.5e-8, "noise": 1.9e-7, "c": 5.0e-5},
    (1237, 21, 301, 4.0): {"U": 4.2e-6, "ls": 1.2e-7, "s": 5.5e-8, "noise": 1.5e-7, "c": 2.0e-6},
}
GATE_BOUND_REL = 1e-4             # the parity gate of SURVEY 8(d): bound, predictive mean and variance
JITTER = 1e-6

KERNEL_KINDS = ("RBF", "Matern", "InverseMQ", "Cosine")
KERNEL_DIMS = (1, 4, 5, 21, 33, 90, 385)
KERNEL_SIZES = ((1, 1), (5, 3), (63, 64), (257, 65), (257, 129), (1237, 301), (257, 1024))      # (N, M)
KERNEL_WIDTHS = (0, 1, 2, 16)


def kernel_cases():
    """(kind, d, N, M, T): the cross product thinned so that every value of every axis meets every kind at least once."""
    out = []
    for k, kind in enumerate(KERNEL_KINDS):
        for j, d in enumerate(KERNEL_DIMS):
            N, M = KERNEL_SIZES[(j + k) % len(KERNEL_SIZES)]
            out.append((kind, d, N, M, KERNEL_WIDTHS[(j + 2 * k) % len(KERNEL_WIDTHS)]))
    return out


def kernel_inputs(kind, d, N, M, T):
    """Z from radial_reference.inputs (centred, one exact and one near duplicate pair); U = the first rows of Z for its first
    half and a perturbed copy of them for the second (rows of Z taken cyclically when M > N); Y, and well-scaled C (symmetric),
    v."""
    rng = np.random.default_rng(7000 + 13 * d + N + M)
    Z = rr.inputs(N, d, d + N)
    h = (M + 1) // 2
    first = Z[np.arange(h) % N]
    second = (Z[np.arange(M - h) % N] * np.float32(1.0 + 1e-3) +
              np.float32(0.05) * rng.standard_normal((M - h, d)).astype(np.float32) * np.float32(min(1.0, 2.0 / np.sqrt(d))))
    U = np.concatenate([first, second]).astype(np.float32)
    Y = rng.standard_normal((N, T)).astype(np.float32)
    C = rng.standard_normal((M, M)) / M
    C = 0.5 * (C + C.T)
    v = rng.standard_normal((M, T))
    return Z, U, Y, C, v


# ---- 1. the sums and their adjoint in float64 -----------------------------------------------------------------------------
def _dphi(kind, d2):
    return fmo._dphi(kind, d2, fmo._phi(kind, d2))


def sums(Z, U, Y, kind):
    K = rr.kernel(Z, U, kind)
    Y = np.asarray(Y, dtype=np.float64).reshape(K.shape[0], -1)
    return K.T @ K, K.T @ Y


def sums_bounds(Z, U, Y, kind):
    K = np.abs(rr.kernel(Z, U, kind))
    dK = rr.entry_bound(Z, U, kind)
    Y = np.abs(np.asarray(Y, dtype=np.float64)).reshape(K.shape[0], -1)
    n = K.shape[0]
    cross = dK.T @ K
    return cross + cross.T + n * 2.0 ** -53 * (K.T @ K), dK.T @ Y + n * 2.0 ** -53 * (K.T @ Y)


def sums_grad(Z, U, Y, C, v, kind):
    """(gU, q) of f = sum(C o G) + sum(v o g) by direct differences, feature by feature."""
    Z64, U64 = np.asarray(Z, dtype=np.float64), np.asarray(U, dtype=np.float64)
    K = rr.kernel(Z, U, kind)
    Y = np.asarray(Y, dtype=np.float64).reshape(K.shape[0], -1)
    S = (2.0 * K @ C + Y @ np.asarray(v, dtype=np.float64).reshape(U64.shape[0], -1).T) * _dphi(kind, rr.sqdist(Z, U))
    gU, q = np.zeros_like(U64), np.zeros(U64.shape[1])
    for m in range(U64.shape[1]):
        diff = U64[None, :, m] - Z64[:, None, m]
        gU[:, m] = 2.0 * (S * diff).sum(0)
        q[m] = (S * diff * diff).sum()
    return gU, q


def check_sums(G, g, Z, U, Y, kind):
    """The derived bounds; returns (largest error / bound of G, of g)."""
    rG, rg = sums(Z, U, Y, kind)
    bG, bg = sums_bounds(Z, U, Y, kind)
    G, g = np.asarray(G, dtype=np.float64), np.asarray(g, dtype=np.float64).reshape(rg.shape)
    assert np.isfinite(G).all() and np.isfinite(g).all(), "non-finite entries"
    ratio_G = float((np.abs(G - rG) / bG).max())
    ratio_g = float((np.abs(g - rg) / np.maximum(bg, 1e-300)).max()) if rg.size else 0.0
    assert ratio_G <= 1.0, "G: %.3g of the bound" % ratio_G
    assert ratio_g <= 1.0, "g: %.3g of the bound" % ratio_g
    return ratio_G, ratio_g


def check_grad(gU, q, ref_gU, ref_q):
    """radial_reference.GATE_GRAD_REL, norm-wise; returns (rel gU, rel q)."""
    gU, q = np.asarray(gU, dtype=np.float64), np.asarray(q, dtype=np.float64)
    assert np.isfinite(gU).all() and np.isfinite(q).all(), "non-finite entries"
    ru, rq = rr.rel(gU, ref_gU), rr.rel(q, ref_q)
    assert ru <= rr.GATE_GRAD_REL, "gU rel %.3g" % ru
    assert rq <= rr.GATE_GRAD_REL, "q rel %.3g" % rq
    return ru, rq


# ---- 2. the objective by the dense N x N form -----------------------------------------------------------------------------
def _phi_t(kind, d2):
    if kind == "RBF":
        return torch.exp(-0.5 * d2)
    if kind == "InverseMQ":
        return 1.0 / torch.sqrt(1.0 + d2)
    r = torch.sqrt(d2 + 1e-30)
    return (1.0 + math.sqrt(3.0) * r) * torch.exp(-math.sqrt(3.0) * r)


def _d2_t(A, B):
    return ((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * A @ B.t()).clamp_min(0.0)


def _kuu_t(kind, U, jitter):
    d2 = _d2_t(U, U) * (1.0 - torch.eye(U.shape[0], dtype=U.dtype))
    return _phi_t(kind, d2) + jitter * torch.eye(U.shape[0], dtype=U.dtype)


def dense_objective(kind, X, y, U_raw, mu, ls, s, noise, c, jitter=JITTER, trace_with_s=True):
    """log N(y | c, s Q + sigma^2 I) - (s / (2 sigma^2)) tr(K_ff - Q) in float64 torch from the N x N matrix s Q + sigma^2 I and
    its Cholesky factor; every argument may require grad."""
    Z, U = (X - mu) / ls, (U_raw - mu) / ls
    n = X.shape[0]
    Kfu = _phi_t(kind, _d2_t(Z, U))
    Q = Kfu @ torch.linalg.solve(_kuu_t(kind, U, jitter), Kfu.t())
    L = torch.linalg.cholesky(s * Q + noise * torch.eye(n, dtype=X.dtype))
    r = (y - c).reshape(-1, 1)
    w = torch.linalg.solve_triangular(L, r, upper=False)
    ll = -0.5 * (w * w).sum() - torch.log(L.diagonal()).sum() - 0.5 * n * math.log(2.0 * math.pi)
    tr = n - Q.diagonal().sum()
    return ll - 0.5 * (s if trace_with_s else 1.0) * tr / noise


def exact_marginal(kind, X, y, mu, ls, s, noise, c):
    """log N(y | c, s K_ff + sigma^2 I): what the bound stays below."""
    Z = (X - mu) / ls
    n = X.shape[0]
    K = _phi_t(kind, _d2_t(Z, Z) * (1.0 - torch.eye(n, dtype=X.dtype)))
    L = torch.linalg.cholesky(s * K + noise * torch.eye(n, dtype=X.dtype))
    w = torch.linalg.solve_triangular(L, (y - c).reshape(-1, 1), upper=False)
    return -0.5 * (w * w).sum() - torch.log(L.diagonal()).sum() - 0.5 * n * math.log(2.0 * math.pi)


def dense_prediction(kind, X, y, Xs, U_raw, mu, ls, s, noise, c, jitter=JITTER):
    """Titsias' predictive mean and covariance through N x N solves: with Khat = s Q_ff + sigma^2 I,
    mean = c + s Q_*f Khat^-1 r, cov = s (K_** - Q_**) + s Q_** - s^2 Q_*f Khat^-1 Q_f*."""
    Z, Zs, U = (X - mu) / ls, (Xs - mu) / ls, (U_raw - mu) / ls
    n = X.shape[0]
    Kuu = _kuu_t(kind, U, jitter)
    Kfu, Ksu = _phi_t(kind, _d2_t(Z, U)), _phi_t(kind, _d2_t(Zs, U))
    Khat = s * Kfu @ torch.linalg.solve(Kuu, Kfu.t()) + noise * torch.eye(n, dtype=X.dtype)
    Qsf = Ksu @ torch.linalg.solve(Kuu, Kfu.t())
    Kss = _phi_t(kind, _d2_t(Zs, Zs) * (1.0 - torch.eye(Xs.shape[0], dtype=X.dtype)))
    mean = c + s * Qsf @ torch.linalg.solve(Khat, (y - c).reshape(-1, 1)).reshape(-1)
    cov = s * Kss - s * s * Qsf @ torch.linalg.solve(Khat, Qsf.t())
    return mean, cov


def cond_kuu(kind, U_raw, mu, ls, jitter=JITTER):
    return float(torch.linalg.cond(_kuu_t(kind, (U_raw - mu) / ls, jitter)))


def problem(N, d, M, ls, seed=0):
    """Synthetic regression set of the probes: X ~ N(0, 1) float32, y = sum sin + 0.1 noise (standardised), inducing points the
    first M rows, one lengthscale `ls` on every dimension."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g)
    y = torch.sin(X).sum(1) + 0.1 * torch.randn(N, generator=g)
    y = (y - y.mean()) / y.std()
    return X, y, X[:M].clone(), torch.full((d,), float(ls))


# ---- 3. emulation of the kernel path --------------------------------------------------------------------------------------
class Emulation:
    """rpgp_inducing_gram / _grad and the host algebra of rpgp_amd/sgpr.py in numpy: float32 Gram-form kernel entries
    (radial_reference.Emulation's distance and phi), exact products, float64 sums over slabs of `slab` rows, S rounded to
    float32.  `defect` switches ONE defect of the mutation table on."""

    DEFECTS = ("G_float32_sum", "C_float32", "drop_slab", "drop_Yvt", "grad_factor_2", "lower_triangle_missing",
               "trace_without_s")

    def __init__(self, kind, defect=None, slab=256):
        assert defect is None or defect in self.DEFECTS
        self.kind, self.defect, self.slab = kind, defect, slab
        self._rad = rr.Emulation(kind)

    def _entries(self, Z, U):
        d2 = self._rad._d2(np.asarray(Z, dtype=np.float32), np.asarray(U, dtype=np.float32), False)
        return rr._phi32(self.kind, d2)

    def _slabs(self, n):
        starts = list(range(0, n, self.slab))
        if self.defect == "drop_slab" and len(starts) > 1:
            starts = starts[:1] + starts[2:]
        return starts

    def gram(self, Z, U, Y):
        K = self._entries(Z, U)[0]
        Y = np.asarray(Y, dtype=np.float32).reshape(K.shape[0], -1)
        M = K.shape[1]
        G, g = np.zeros((M, M)), np.zeros((M, Y.shape[1]))
        for r0 in self._slabs(K.shape[0]):
            Ks, Ys = K[r0:r0 + self.slab], Y[r0:r0 + self.slab]
            if self.defect == "G_float32_sum":
                G += (Ks.T @ Ks).astype(np.float64)                    # (float32 accumulation inside the slab)
            else:
                G += Ks.T.astype(np.float64) @ Ks.astype(np.float64)
            g += Ks.T.astype(np.float64) @ Ys.astype(np.float64)
        if self.defect == "lower_triangle_missing":
            G = np.triu(G)
        return G, g

    def grad(self, Z, U, Y, C, v):
        K, dK = self._entries(Z, U)
        Z64, U64 = np.asarray(Z, dtype=np.float32).astype(np.float64), np.asarray(U, dtype=np.float32).astype(np.float64)
        Y = np.asarray(Y, dtype=np.float32).reshape(K.shape[0], -1).astype(np.float64)
        C = np.asarray(C, dtype=np.float64)
        if self.defect == "C_float32":
            C = C.astype(np.float32).astype(np.float64)
        v = np.asarray(v, dtype=np.float64).reshape(U64.shape[0], -1)
        d = Z64.shape[1]
        P, Q2, cs = np.zeros((U64.shape[0], d)), np.zeros((U64.shape[0], d)), np.zeros(U64.shape[0])
        for r0 in self._slabs(K.shape[0]):
            sl = slice(r0, r0 + self.slab)
            W = (1.0 if self.defect == "grad_factor_2" else 2.0) * (K[sl].astype(np.float64) @ C)
            if self.defect != "drop_Yvt":
                W = W + Y[sl] @ v.T
            S = (W * dK[sl].astype(np.float64)).astype(np.float32).astype(np.float64)
            P += S.T @ Z64[sl]
            Q2 += S.T @ (Z64[sl] * Z64[sl])
            cs += S.sum(0)
        gU = 2.0 * (cs[:, None] * U64 - P)
        q = (Q2 - 2.0 * U64 * P + cs[:, None] * U64 * U64).sum(0)
        return gU, q

    def objective(self, X, y, U_raw, mu, ls, s, noise, c, jitter=JITTER):
        """(bound, {parameter: gradient}) as rpgp_amd/sgpr.py forms them: Z, U in float32, K_uu in float64 torch from the float32
        U, G and g from `gram`, C and v by autograd, dU and dl from `grad`."""
        X32, mu32, ls32 = (np.asarray(a, dtype=np.float32) for a in (X, mu, ls))
        Z = ((X32 - mu32) / ls32).astype(np.float32)
        U = ((np.asarray(U_raw, dtype=np.float32) - mu32) / ls32).astype(np.float32)
        y64 = np.asarray(y, dtype=np.float32).astype(np.float64)
        n = Z.shape[0]
        Y = np.stack([y64, np.ones(n)], axis=1).astype(np.float32)
        G, g = self.gram(Z, U, Y)
        Gt, gt = torch.from_numpy(G).requires_grad_(True), torch.from_numpy(g).requires_grad_(True)
        Ut = torch.from_numpy(U.astype(np.float64)).requires_grad_(True)
        st, nt, ct = (torch.tensor(float(a), dtype=torch.float64, requires_grad=True) for a in (s, noise, c))
        a = st / nt
        Gs = 0.5 * (Gt + Gt.t()) if self.defect != "lower_triangle_missing" else Gt
        Kuu = _kuu_t(self.kind, Ut, jitter)
        A = Kuu + a * Gs
        Lu, La = torch.linalg.cholesky(Kuu), torch.linalg.cholesky(A)
        g_r = gt[:, 0] - ct * gt[:, 1]
        rr_ = float((y64 * y64).sum()) - 2.0 * ct * float(y64.sum()) + n * ct * ct
        beta = torch.cholesky_solve(g_r.reshape(-1, 1), La).reshape(-1)
        logdet = n * torch.log(nt) - 2.0 * torch.log(Lu.diagonal()).sum() + 2.0 * torch.log(La.diagonal()).sum()
        inv_quad = (rr_ - a * (g_r * beta).sum()) / nt
        trace = (st if self.defect != "trace_without_s" else 1.0) * (n - torch.cholesky_solve(Gs, Lu).diagonal().sum())
        value = -0.5 * (inv_quad + logdet + n * math.log(2.0 * math.pi)) - 0.5 * trace / nt
        value.backward()
        Cm = 0.5 * (Gt.grad + Gt.grad.t()).numpy()
        gU, q = self.grad(Z, U, Y, Cm, gt.grad.numpy())
        gU_total = gU + Ut.grad.numpy()                                 # (the sums' share + K_uu's share)
        ls64 = ls32.astype(np.float64)
        grads = {
            "U": gU_total / ls64,
            # dl_m: through Z (-(2 q_m) + sum_j gU_jm u_jm) / l_m and through U: -sum_j gU_total_jm u_jm / l_m
            "ls": (-2.0 * q + (gU * U).sum(0) - (gU_total * U).sum(0)) / ls64,
            "s": float(st.grad), "noise": float(nt.grad), "c": float(ct.grad),
        }
        return float(value), grads


def reference_objective(kind, X, y, U_raw, mu, ls, s, noise, c, jitter=JITTER):
    """(bound, {parameter: gradient}) of dense_objective in float64 on the float32 parameters widened."""
    t = {k: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
         for k, a in (("U", U_raw), ("ls", ls), ("s", s), ("noise", noise), ("c", c))}
    X64, y64, mu64 = (torch.tensor(np.asarray(a, dtype=np.float64)) for a in (X, y, mu))
    val = dense_objective(kind, X64, y64, t["U"], mu64, t["ls"], t["s"], t["noise"], t["c"], jitter)
    val.backward()
    return float(val.detach()), {k: (a.grad.numpy() if a.grad.dim() else float(a.grad)) for k, a in t.items()}
