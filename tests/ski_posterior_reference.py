"""TEST INFRASTRUCTURE — numpy float64 restatement of the closed-form posterior of the grid-interpolation (SKI) models
(rpgp_amd/ski_posterior.py, csrc/rpgp_ski_post.hip), built on oracle.ski.interp_matrix / interp_sparse / toeplitz / dense_kernel.

Notation: w_i is the row of 4 J cubic-convolution weights of point i in a vector of J G entries, W (N x JG) their stack.
    gram       A = W^T W,  g = W^T Y
    quadform   out_i = w_i^T C w_i
    closed_form    the posterior through A, g and JG x JG algebra (the formulas of ski_posterior.py)
    dense          the posterior of the SAME one-grid kernel through oracle.ski.dense_kernel: Cholesky of K + sigma^2 I, mean,
                   covariance, MVN log-density

Entrywise bounds of the two device kernels against this restatement (derived, not tuned; EPS = 2^-53):

1.  One weight.  Both sides form d = fl(z - g0) (the same rounding), then the device multiplies by the stored fl(1 / h) and the
    restatement divides by h: u_dev = u (1 + e1)(1 + e2), u_ref = u (1 + e3), |e| <= EPS, so |u_dev - u_ref| <= 3 EPS |u| + O(EPS^2)
    <= 4 EPS G for |u| <= G (the clip to [1, G - 2] is 1-Lipschitz).  As a function of the grid coordinate the weight on a fixed
    node m is the Keys kernel phi(|u - m|), continuous with phi(2) = 0 — also across a cell boundary, where the stencil moves by a
    node — and |phi'| <= 25 / 18 (piece 1, (4.5 U - 5) U at U = 5 / 9; piece 2 stays within [-1/2, 1/6]).  The only
    discontinuity of the rule is AT the upper clip u = G - 2 (the first tap is clamped to G - 4 there); rows within the rounding
    of it are outside the bound, and the edge cases of the suites put rows there on grids with a power-of-two spacing, where both
    sides are exact.  The Horner evaluation itself (fr + 1, 1 - fr, 2 - fr, then three multiply-adds and an add on magnitudes
    <= 4, fused or not) differs by at most 64 EPS between the two sides.  Hence
        dw = (25 / 18) 4 EPS G + 64 EPS                                                    (weight_bound)
    and a weight can be non-zero on one side only on the nodes of the other side's stencil and one node either way (P': the
    dilated pattern).
2.  A sum of n products in float64, in any order, fused or not, is within gamma_(n+1) sum |terms| of the exact sum,
    gamma_n = n EPS / (1 - n EPS); both sides sum, so 2 gamma_(n+1).
    A[a][b]:   dw (|W|^T P' + P'^T |W|)[a][b] + dw^2 (P'^T P')[a][b] + 2 gamma_(n_ab + 1) (|W|^T |W|)[a][b],   n_ab = (P'^T P')[a][b]
    g[a][t]:   dw (P'^T |Y|)[a][t] + 2 gamma_(n_a + 1) (|W|^T |Y|)[a][t]
    out_i:     dw (p'^T |C| |w| + |w|^T |C| p') + dw^2 p'^T |C| p' + 2 gamma_(8 J + 8) |w|^T |C| |w|
               (the device sums 4 J terms per column, its columns and six butterfly steps; the restatement 4 J + 4 J)
`test_ski_posterior_host.py` checks dw against weights evaluated in numpy.longdouble."""
import math

import numpy as np

from oracle import ski as sko

EPS = 2.0 ** -53
SLOPE = 25.0 / 18.0
KINDS = ("RBF", "Matern", "InverseMQ", "Cosine")
EIG_FLOOR = 1e-14


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * EPS / (1.0 - n * EPS)


def weight_bound(G):
    return SLOPE * 4.0 * EPS * G + 64.0 * EPS


# ---- the grid block ---------------------------------------------------------------------------------------------------------
def block(g0, h, J, weights=None, kind="RBF"):
    """The float64 grid block: shared grid for scalar (g0, h), per-projection grids for arrays."""
    kflag = 4.0 * KINDS.index(kind)
    w = None if weights is None else [float(x) for x in np.asarray(weights).reshape(-1)]
    if np.ndim(g0) == 0:
        return np.array([float(g0), float(h), 1.0 / float(h), (0.0 if w is None else 1.0) + kflag] + (w or []))
    tail = [v for j in range(J) for v in (float(g0[j]), float(h[j]), 1.0 / float(h[j]))]
    return np.array([0.0, 1.0, 1.0, (2.0 if w is None else 3.0) + kflag] + (w or [1.0] * J) + tail)


def parse_block(gp, J):
    """(g0 [J], h [J], weights [J] or None, kind) of a float64 grid block."""
    gp = np.asarray(gp, dtype=np.float64)
    flags = int(gp[3])
    w = gp[4:4 + J].copy() if flags & 1 else None
    if flags & 2:
        arr = gp[4 + J:4 + 4 * J].reshape(J, 3)
        return arr[:, 0].copy(), arr[:, 1].copy(), w, KINDS[(flags >> 2) & 3]
    return np.full(J, gp[0]), np.full(J, gp[1]), w, KINDS[(flags >> 2) & 3]


# ---- W and its dilated pattern ------------------------------------------------------------------------------------------------
def interp(Z, g0, h, G):
    """W (N x JG, scipy CSR): oracle.ski.interp_sparse of every projection side by side."""
    import scipy.sparse as sp
    Z = np.asarray(Z, dtype=np.float64)
    return sp.hstack([sko.interp_sparse(Z[:, j], float(g0[j]), float(h[j]), G) for j in range(Z.shape[1])], format="csr")


def first_taps(Z, g0, h, G):
    Z = np.asarray(Z, dtype=np.float64)
    u = np.clip((Z - np.asarray(g0)[None, :]) / np.asarray(h)[None, :], 1.0, G - 2.0)
    return np.clip(np.floor(u).astype(np.int64) - 1, 0, G - 4)


def pattern(Z, g0, h, G):
    """P' (N x JG, 0 / 1): the nodes of every row's stencil and one node either way."""
    import scipy.sparse as sp
    idx0 = first_taps(Z, g0, h, G)
    N, J = idx0.shape
    rows, cols = [], []
    for j in range(J):
        for k in range(-1, 5):
            n = idx0[:, j] + k
            ok = (n >= 0) & (n < G)
            rows.append(np.nonzero(ok)[0])
            cols.append(j * G + n[ok])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(N, J * G))


def weights_longdouble(z, g0, h, G):
    """(first tap, 4 weights) of one projection with the grid coordinate and the cubic evaluated in numpy.longdouble."""
    ld = np.longdouble
    u = np.clip((np.asarray(z, dtype=ld) - ld(g0)) / ld(h), ld(1.0), ld(G - 2.0))
    fl = np.floor(u)
    fr = u - fl
    idx0 = np.clip(fl.astype(np.int64) - 1, 0, G - 4)

    def cubic(U):
        return np.where(U < 1, ((ld(1.5) * U - ld(2.5)) * U) * U + 1, ((ld(-0.5) * U + ld(2.5)) * U - 4) * U + 2)
    return idx0, np.stack([cubic(fr + 1), cubic(fr), cubic(1 - fr), cubic(2 - fr)], axis=1)


# ---- the two sums and their bounds --------------------------------------------------------------------------------------------
def gram(Z, gp, G, Y=None):
    """(A, g): A = W^T W (dense JG x JG), g = W^T Y (None without Y)."""
    Z = np.asarray(Z, dtype=np.float64)
    g0, h, _, _ = parse_block(gp, Z.shape[1])
    W = interp(Z, g0, h, G)
    A = np.asarray((W.T @ W).todense())
    g = None if Y is None else np.asarray(W.T @ np.asarray(Y, dtype=np.float64).reshape(Z.shape[0], -1))
    return A, g


def gram_bound(Z, gp, G, Y=None):
    """Entrywise bounds (no margin) of A and g."""
    Z = np.asarray(Z, dtype=np.float64)
    g0, h, _, _ = parse_block(gp, Z.shape[1])
    aW = abs(interp(Z, g0, h, G))
    P = pattern(Z, g0, h, G)
    dw = weight_bound(G)
    cross = np.asarray((aW.T @ P).todense())
    cnt = np.asarray((P.T @ P).todense())
    bA = dw * (cross + cross.T) + dw * dw * cnt + 2.0 * gamma(cnt + 1.0) * np.asarray((aW.T @ aW).todense())
    bg = None
    if Y is not None:
        aY = np.abs(np.asarray(Y, dtype=np.float64).reshape(Z.shape[0], -1))
        na = np.asarray(P.sum(axis=0)).reshape(-1, 1)
        bg = dw * np.asarray(P.T @ aY) + 2.0 * gamma(na + 1.0) * np.asarray(aW.T @ aY)
    return bA, bg


def quadform(Z, gp, G, C):
    Z = np.asarray(Z, dtype=np.float64)
    g0, h, _, _ = parse_block(gp, Z.shape[1])
    W = interp(Z, g0, h, G)
    return np.asarray(W.multiply(W @ np.asarray(C, dtype=np.float64)).sum(axis=1)).reshape(-1)


def quadform_bound(Z, gp, G, C):
    Z = np.asarray(Z, dtype=np.float64)
    J = Z.shape[1]
    g0, h, _, _ = parse_block(gp, J)
    aW = abs(interp(Z, g0, h, G))
    P = pattern(Z, g0, h, G)
    aC = np.abs(np.asarray(C, dtype=np.float64))
    dw = weight_bound(G)
    WC, PC = aW @ aC, P @ aC

    def rows(S, D):
        return np.asarray(S.multiply(D).sum(axis=1)).reshape(-1)
    return dw * (rows(P, WC) + rows(aW, PC)) + dw * dw * rows(P, PC) + 2.0 * float(gamma(8 * J + 8)) * rows(aW, WC)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound (inf where the bound is zero and the entries differ)."""
    diff = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0.0, diff / bound, np.where(diff > 0.0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


def check_gram(A, g, Z, gp, G, Y=None):
    """(worst ratio of A, worst ratio of g) against the restatement; within the bound iff <= 1."""
    A_ref, g_ref = gram(Z, gp, G, Y)
    bA, bg = gram_bound(Z, gp, G, Y)
    return worst_ratio(A, A_ref, bA), (0.0 if Y is None else worst_ratio(g, g_ref, bg))


def block_row_sums(A, Z, gp, G, bA):
    """Worst ratio of sum_b A[(j, a)][(j', b)] - sum_i w_ia over every row and G-wide block: cubic-convolution weights sum to one
    (four roundings, 8 EPS per row), so the block sums of a row equal its column sum of W.  Bound: the entry bounds bA summed over
    the block, gamma_G of this function's own G-term sum, and (8 EPS + gamma_(N+1)) sum_i |w_ia|."""
    Z = np.asarray(Z, dtype=np.float64)
    N, J = Z.shape
    g0, h, _, _ = parse_block(gp, J)
    W = interp(Z, g0, h, G)
    col = np.asarray(W.sum(axis=0)).reshape(-1)
    acol = np.asarray(abs(W).sum(axis=0)).reshape(-1)
    A = np.asarray(A, dtype=np.float64)
    worst = 0.0
    for jp in range(J):
        blk = slice(jp * G, (jp + 1) * G)
        bound = bA[:, blk].sum(axis=1) + float(gamma(G)) * np.abs(A[:, blk]).sum(axis=1) + (8.0 * EPS + float(gamma(N + 1))) * acol
        worst = max(worst, worst_ratio(A[:, blk].sum(axis=1), col, bound))
    return worst


def check_quadform(out, Z, gp, G, C):
    return worst_ratio(out, quadform(Z, gp, G, C), quadform_bound(Z, gp, G, C))


# ---- the posterior ------------------------------------------------------------------------------------------------------------
def _root(h, G, s, weights, kind, J):
    import scipy.linalg as sl
    blocks = []
    for j in range(J):
        wj = 1.0 if weights is None else float(weights[j])
        lam, U = np.linalg.eigh(wj * sko.toeplitz(float(h[j]), G, kind))
        keep = lam > EIG_FLOOR * lam.max()
        blocks.append(U[:, keep] * np.sqrt(s * lam[keep]))
    return sl.block_diag(*blocks)


def _mvn_log_density(mean, cov, y):
    L = np.linalg.cholesky(cov)
    z = np.linalg.solve(L, y - mean)
    return float(-0.5 * z @ z - np.log(np.diag(L)).sum() - 0.5 * y.size * math.log(2.0 * math.pi))


def closed_form(Z, y, Zs, ys, gp, G, s, noise, c):
    """The posterior at Zs and at Z through the Gram sums: dict(mean, var, cov, lp, mean_train, lp_train, alpha, F)."""
    import scipy.linalg as sl
    Z, Zs = np.asarray(Z, dtype=np.float64), np.asarray(Zs, dtype=np.float64)
    J = Z.shape[1]
    g0, h, weights, kind = parse_block(gp, J)
    W, Ws = interp(Z, g0, h, G), interp(Zs, g0, h, G)
    S = _root(h, G, s, weights, kind, J)
    F = S.shape[1]
    A = np.asarray((W.T @ W).todense())
    g = W.T @ (y - c)
    M = noise * np.eye(F) + S.T @ A @ S
    L = np.linalg.cholesky(M)
    m_u = S @ sl.cho_solve((L, True), S.T @ g)
    Q = math.sqrt(noise) * sl.solve_triangular(L, S.T, lower=True).T          # sigma S L^-T
    C = Q @ Q.T
    logdet_M = 2.0 * np.log(np.diag(L)).sum()

    def log_density(Wx, Ax, mean, target):
        d = target - mean
        Lp = np.linalg.cholesky(M + S.T @ Ax @ S)
        u = sl.solve_triangular(Lp, S.T @ (Wx.T @ d), lower=True)
        quad = (d @ d - u @ u) / noise
        logdet = d.size * math.log(noise) + 2.0 * np.log(np.diag(Lp)).sum() - logdet_M
        return float(-0.5 * (quad + logdet + d.size * math.log(2.0 * math.pi)))

    mean = Ws @ m_u + c
    WQ = Ws @ Q
    mean_train = W @ m_u + c
    return dict(mean=mean, var=np.asarray(Ws.multiply(Ws @ C).sum(axis=1)).reshape(-1), cov=WQ @ WQ.T,
                lp=log_density(Ws, np.asarray((Ws.T @ Ws).todense()), mean, ys), mean_train=mean_train,
                lp_train=log_density(W, A, mean_train, y), alpha=(y - mean_train) / noise, F=F)


def dense(Z, y, Zs, ys, gp, G, s, noise, c):
    """The same quantities from the dense N x N kernel on the one grid (oracle.ski.dense_kernel)."""
    import scipy.linalg as sl
    Z, Zs = np.asarray(Z, dtype=np.float64), np.asarray(Zs, dtype=np.float64)
    J = Z.shape[1]
    g0, h, weights, kind = parse_block(gp, J)
    grid = (g0, h)
    K = sko.dense_kernel(Z, Z, s, G, grid, weights, kind)
    Ks = sko.dense_kernel(Zs, Z, s, G, grid, weights, kind)
    Kss = sko.dense_kernel(Zs, Zs, s, G, grid, weights, kind)
    N = Z.shape[0]
    cf = sl.cho_factor(K + noise * np.eye(N), lower=True)
    alpha = sl.cho_solve(cf, y - c)
    mean = Ks @ alpha + c
    cov = Kss - Ks @ sl.cho_solve(cf, Ks.T)
    mean_train = K @ alpha + c
    cov_train = K - K @ sl.cho_solve(cf, K)
    return dict(mean=mean, var=np.diag(cov).copy(), cov=cov,
                lp=_mvn_log_density(mean, cov + noise * np.eye(Zs.shape[0]), ys), mean_train=mean_train,
                lp_train=_mvn_log_density(mean_train, cov_train + noise * np.eye(N), y), alpha=alpha,
                prior_diag_scale=s * (np.ones(J) if weights is None else weights).sum())


# ---- the six cases of the end-to-end suites -----------------------------------------------------------------------------------
#        N     M   J   G     kind         rule         weights          s    sigma^2
CASES = [(600, 80, 3, 64, "RBF", "shared", None, 1.0, 0.1),
         (600, 80, 3, 64, "RBF", "reference", (0.5, 1.5, 1.0), 2.0, 1e-3),
         (600, 80, 2, 64, "Matern", "shared", None, 1.0, 0.05),
         (600, 80, 2, 64, "InverseMQ", "shared", None, 1.0, 0.05),
         (600, 80, 2, 64, "Cosine", "shared", None, 1.0, 0.05),
         (1500, 100, 3, 1024, "RBF", "shared", None, 1.0, 0.01)]
TOL = 1e-8


def case_data(k):
    """Coordinates (float32 values widened; the test rows drawn 1.3 x wider), targets and the grid block over the union."""
    N, M, J, G, kind, rule, weights, s, noise = CASES[k]
    rng = np.random.default_rng(100 + k)
    Z = rng.standard_normal((N, J)).astype(np.float32).astype(np.float64)
    Zs = (1.3 * rng.standard_normal((M, J))).astype(np.float32).astype(np.float64)
    y = np.sin(Z).sum(axis=1) + 0.1 * rng.standard_normal(N)
    ys = np.sin(Zs).sum(axis=1) + 0.1 * rng.standard_normal(M)
    g0, h = sko.grid_params(Z, Zs, G) if rule == "shared" else sko.grid_params_reference(Z, Zs, G)
    return Z, y, Zs, ys, block(g0, h, J, weights, kind), G, s, noise, 0.2


def compare(got, ref):
    """The normalised differences the suites hold to TOL: mean relative to max(1, max |mean|), variances and covariance entries
    relative to s sum_j w_j, log-densities relative to max(1, |value|)."""
    ms = max(1.0, float(np.abs(ref["mean"]).max()))
    ps = ref["prior_diag_scale"]
    out = {"mean": float(np.abs(got["mean"] - ref["mean"]).max()) / ms,
           "mean_train": float(np.abs(got["mean_train"] - ref["mean_train"]).max()) / max(1.0, float(np.abs(ref["mean_train"]).max())),
           "var": float(np.abs(got["var"] - ref["var"]).max()) / ps,
           "lp": abs(got["lp"] - ref["lp"]) / max(1.0, abs(ref["lp"])),
           "lp_train": abs(got["lp_train"] - ref["lp_train"]) / max(1.0, abs(ref["lp_train"]))}
    if got.get("cov") is not None:
        out["cov"] = float(np.abs(got["cov"] - ref["cov"]).max()) / ps
    return out
