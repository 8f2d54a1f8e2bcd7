"""The explicit features of the Chebyshev low-rank kernel on the host (no GPU): rpgp_lowrank_post_select through ctypes against a
numpy restatement of the degree-128 selection, its bounds on a dense grid, monotone ranks and determinism; and the algebra of
lowrank_posterior.py (CPU test double, features restated in float64 torch) against the dense float64 oracle."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import dense_gp as orc

TOL = 1e-10


def _post_select(h, tol=TOL, p_max=64):
    from rpgp_amd import _lib
    lib = _lib.load()
    p, r, tail = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_double(-1.0)
    G = np.zeros((p_max, p_max), dtype=np.float64)
    _lib.check(lib.rpgp_lowrank_post_select(float(h), float(tol), p_max, ctypes.byref(p), ctypes.byref(r), ctypes.byref(tail),
                                            G.ctypes.data), "rpgp_lowrank_post_select")
    return p.value, r.value, tail.value, G


def _cheb2d(h, M=128):
    """Coefficients of the degree-(M-1) interpolant of exp2(-h^2 (x - y)^2) at the Chebyshev points of the first kind."""
    k = np.arange(M)
    xs = np.cos(np.pi * (k + 0.5) / M)
    cs = np.cos(np.pi * np.outer(k, k + 0.5) / M)          # cs[m, k] = cos(pi m (k + 1/2) / M)
    f = np.exp2(-h * h * (xs[:, None] - xs[None, :]) ** 2)
    w = np.full(M, 2.0 / M)
    w[0] = 1.0 / M
    return (w[:, None] * cs) @ f @ (w[:, None] * cs).T


def _select_np(h, tol, p_max=64, M=128):
    """(p, selection tail, C_p) of the selection: smallest p with sum_{max(m,n) >= p} |c_mn| + allowance <= tol."""
    c = _cheb2d(h, M)
    a = np.abs(c)
    shell = np.array([a[q, :q + 1].sum() + a[:q, q].sum() for q in range(M)])
    unresolved = shell[M - 8:].sum()
    assert unresolved <= 1e-11
    allowance = 1e-13 + unresolved
    t, p = 0.0, M
    for q in range(M - 1, 0, -1):
        if t + shell[q] + allowance > tol:
            break
        t += shell[q]
        p = q
    if p > p_max:
        return 0, 0.0, None
    return p, t + allowance, c[:p, :p]


def _cheb(x, p):
    T = np.empty((p, x.size))
    T[0] = 1.0
    if p > 1:
        T[1] = x
    for m in range(2, p):
        T[m] = 2.0 * x * T[m - 1] - T[m - 2]
    return T


@pytest.mark.parametrize("h", [0.0, 1.5, 4.6, 7.0])
def test_post_select_against_the_numpy_selection_and_its_bounds(h):
    p, r, tail, G = _post_select(h)
    p_np, sel_tail, C = _select_np(h, TOL)
    assert p == p_np and 1 <= r <= p, (p, p_np, r)
    G = G[:p, :r]
    dropped = tail - sel_tail                              # (the two selection tails agree to the transform's rounding)
    assert dropped >= -1e-13
    assert np.abs(G @ G.T - C).max() <= max(dropped, 0.0) + 1e-13, (np.abs(G @ G.T - C).max(), dropped)
    x = np.linspace(-1.0, 1.0, 257)
    F = _cheb(x, p).T @ G                                  # 257 x r
    err = np.abs(F @ F.T - np.exp2(-h * h * (x[:, None] - x[None, :]) ** 2)).max()
    assert err <= tail, (h, p, r, err, tail)
    if h == 4.6:
        print("h = 4.6: p = %d, r = %d, tail = %.3g" % (p, r, tail))


def test_post_select_ranks_are_monotone():
    ranks = [_post_select(h)[:2] for h in np.linspace(0.0, 8.0, 33)]
    served = [p > 0 for p, _ in ranks]
    assert all(served[:29]) and served == sorted(served, reverse=True), ranks      # served up to h ~ 7.3, then not
    ranks = [pr for pr, ok in zip(ranks, served) if ok]
    for (p0, r0), (p1, r1) in zip(ranks, ranks[1:]):
        assert p0 <= p1 and r0 <= r1, ranks
    for h in (1.5, 4.6, 7.0):
        by_tol = [_post_select(h, tol)[:2] for tol in (1e-8, 1e-9, 1e-10)]
        for (p0, r0), (p1, r1) in zip(by_tol, by_tol[1:]):
            assert p0 <= p1 and r0 <= r1, (h, by_tol)


def test_post_select_not_served_and_deterministic():
    assert _post_select(12.0)[:2] == (0, 0)
    assert _post_select(float("nan"))[:2] == (0, 0)
    a, b = _post_select(4.6), _post_select(4.6)
    assert a[:3] == b[:3] and a[3].tobytes() == b[3].tobytes()


# ---- the algebra of the feature posterior ----------------------------------------------------------------------------------
def _features_torch(Z, mid, inv_w, G, scale):
    """float64 torch restatement of rpgp_lowrank_features_f64."""
    G = torch.as_tensor(G, dtype=torch.float64)
    p, r = G.shape
    X = (Z.double() - torch.as_tensor(mid, dtype=torch.float64)) * inv_w       # N x J
    T = [torch.ones_like(X), X]
    for _ in range(2, p):
        T.append(2.0 * X * T[-1] - T[-2])
    T = torch.stack(T[:p], dim=-1)                                          # N x J x p
    return (math.sqrt(scale) * (T @ G)).reshape(Z.shape[0], -1)


def _model(N, d, J, noise, s, seed=0):
    from rpgp_amd.kernels import AdditiveStructureRBFKernel, ScaledProjectionKernel, ScaleKernel
    from rpgp_amd.likelihoods import GaussianLikelihood, SmoothedBoxPrior
    from rpgp_amd.models import ExactGPModel, ExactMarginalLogLikelihood
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g)
    P = torch.randn(d, J, generator=g)
    ls = torch.rand(d, generator=g) * 1.5 + 1.0
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
    Xs = torch.randn(41, d, generator=g) * 0.8
    ys = torch.sin(Xs).sum(1)
    lin = torch.nn.Linear(d, J, bias=False)
    lin.weight.data = P.t().contiguous()
    k = ScaledProjectionKernel(lin, AdditiveStructureRBFKernel(J), prescale=True, ard_num_dims=d)
    k.initialize(lengthscale=ls)
    sk = ScaleKernel(k)
    sk.outputscale = s
    lik = GaussianLikelihood(noise_prior=SmoothedBoxPrior(1e-4, 10, sigma=0.01))
    lik.noise = noise
    model = ExactGPModel(X, y, lik, sk)
    model.mean_module.constant.data.fill_(0.2)
    ref = orc.DenseExactGP(X.double().numpy(), y.double().numpy(), P.double().numpy(),
                           k.lengthscale.detach().double().numpy().reshape(-1), float(sk.outputscale.detach()), float(lik.noise.detach()),
                           mean=float(model.mean_module.constant.detach()))
    return model, lik, ExactMarginalLogLikelihood(lik, model), X, y, Xs, ys, ref


def _log_density(mean, cov, y):
    L = np.linalg.cholesky(cov)
    z = np.linalg.solve(L, y - mean)
    return -0.5 * z @ z - np.log(np.diag(L)).sum() - 0.5 * y.size * math.log(2.0 * math.pi)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def test_feature_posterior_algebra_against_the_dense_oracle(oracle_backend, monkeypatch):
    from rpgp_amd import ops, settings
    from rpgp_amd.lowrank_posterior import LowrankPredictive
    monkeypatch.setattr(oracle_backend, "lowrank_post_select", ops.lowrank_post_select, raising=False)
    monkeypatch.setattr(oracle_backend, "lowrank_features", _features_torch, raising=False)
    model, lik, mll, X, y, Xs, ys, ref = _model(N=300, d=4, J=5, noise=0.05, s=0.9)
    sigma2 = float(lik.noise)
    model.eval()
    with settings.lowrank_posterior(True), torch.no_grad():
        out = model(Xs)
        st = model.prediction_strategy
        assert st.lowrank is not None, st.lowrank_fallback_reason
        assert isinstance(out, LowrankPredictive) and not out.covariance_materialized
        mean_ref, cov_ref = ref.predict(Xs.double().numpy(), full_cov=True)
        assert _rel(out._mean64.numpy(), mean_ref) <= 1e-7
        assert _rel(out._var64.numpy(), np.diag(cov_ref)) <= 1e-7
        lp = float(lik(out).log_prob(ys.double()))
        assert not out.covariance_materialized
        lp_ref = _log_density(mean_ref, cov_ref + sigma2 * np.eye(Xs.shape[0]), ys.double().numpy())
        assert abs(lp - lp_ref) <= 1e-7 * abs(lp_ref), (lp, lp_ref)
        assert _rel(out.covariance.double().numpy(), cov_ref) <= 1e-6      # (float32 result: the dtype's rounding)
        assert _rel((sigma2 * (out._V.t() @ out._V)).numpy(), cov_ref) <= 1e-7
        # at the training inputs: the closed form of the noisy log-density
        tr = model(X)
        mtr_ref, ctr_ref = ref.predict(X.double().numpy(), full_cov=True)
        assert _rel(tr._mean64.numpy(), mtr_ref) <= 1e-7
        lp_tr = st.train_log_prob(y)
        lp_tr_ref = _log_density(mtr_ref, ctr_ref + sigma2 * np.eye(X.shape[0]), y.double().numpy())
        assert abs(lp_tr - lp_tr_ref) <= 1e-7 * abs(lp_tr_ref), (lp_tr, lp_tr_ref)
        nll = -mll(tr, y).item()
        assert abs(nll + (lp_tr_ref + lik.log_prior().item()) / X.shape[0]) <= 1e-6 * abs(nll)
        # the mean cache and the solve
        alpha_ref = ref.solve(ref.y - ref.c)
        assert _rel(st.alpha64.reshape(-1).numpy(), alpha_ref) <= 1e-7
        B = torch.randn(X.shape[0], 3, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        assert _rel(st.solve(B).numpy(), ref.solve(B.numpy())) <= 1e-7
