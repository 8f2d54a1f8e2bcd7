"""Chebyshev feature ranks above 64 in the closed-form paths (settings.lowrank_max_rank), on the host (no GPU): the selection
rpgp_lowrank_post_select at p_max = 128 (ranks, limits, the tail bound on a grid, determinism), the setting and the runner flag,
and a model whose half-width of about 10 needs p = 83 under the CPU test double (features restated in float64 torch): served
with the cap at 128 and checked against the dense float64 references, not served with the default cap."""
import math

import numpy as np
import pytest
import torch

from oracle import dense_gp as orc
from rpgp_amd import ops

KAPPA = 0.84932180028801907

# (p, r) of the degree-128 selection and the eigenvalue drop rule, restated in numpy (LAPACK's eigvalsh)
RANKS = {(8.0, 1e-10): (68, 49), (8.0, 1e-12): (76, 54), (10.0, 1e-10): (83, 60), (10.0, 1e-12): (92, 65),
         (14.0, 1e-10): (113, 81), (14.0, 1e-12): (128, 89)}


def _cheb(x, p):
    T = np.empty((p, x.size))
    T[0] = 1.0
    if p > 1:
        T[1] = x
    for m in range(2, p):
        T[m] = 2.0 * x * T[m - 1] - T[m - 2]
    return T


@pytest.mark.parametrize("h,tol", sorted(RANKS))
def test_selection_ranks_and_tail_bound(h, tol):
    """p is exact.  r is exact at tol 1e-10.  At tol 1e-12 the drop rule p * sum |dropped| <= tol compares eigenvalues of about
    1e-14 / p: they are at the rounding level eps |C| of any eigensolver, so the tridiagonal QL solver that serves p > 64 and
    LAPACK order and size these near-equal eigenvalues differently, and r may differ by one there (observed: 66 for 65 at
    h = 10, 90 for 89 at h = 14).  Whatever r, the reported tail must bound the error of the factorised kernel."""
    p, r, tail, G = ops.lowrank_post_select(h, tol, p_max=128)
    p_ref, r_ref = RANKS[(h, tol)]
    print("h = %g tol = %g: p = %d r = %d tail = %.3g" % (h, tol, p, r, tail))
    assert p == p_ref
    assert abs(r - r_ref) <= (0 if tol == 1e-10 else 1), (r, r_ref)
    assert G.shape == (p, r) and np.isfinite(G).all()
    x = np.linspace(-1.0, 1.0, 200)                        # ends included
    F = _cheb(x, p).T @ G
    err = np.abs(F @ F.T - np.exp2(-h * h * (x[:, None] - x[None, :]) ** 2)).max()
    print("  grid error %.3g" % err)
    assert 0.0 < tail <= 10.0 * tol
    assert err <= tail, (h, tol, err, tail)


def test_selection_limits():
    assert ops.lowrank_post_select(15.0, 1e-10, p_max=128)[:2] == (0, 0)       # not resolved by the degree-128 reference
    assert ops.lowrank_post_select(15.0, 1e-12, p_max=128)[:2] == (0, 0)
    assert ops.lowrank_post_select(8.0, 1e-10, p_max=64)[:2] == (0, 0)         # needs p = 68
    assert ops.lowrank_post_select(8.0, 1e-10)[:2] == (0, 0)                   # the default cap is 64


@pytest.mark.parametrize("h", [8.0, 14.0])
def test_selection_is_deterministic(h):
    a = ops.lowrank_post_select(h, 1e-10, p_max=128)
    b = ops.lowrank_post_select(h, 1e-10, p_max=128)
    assert a[:3] == b[:3] and a[3].tobytes() == b[3].tobytes()


def test_narrow_selection_does_not_depend_on_the_cap():
    for h in (1.5, 4.6, 7.0):
        a = ops.lowrank_post_select(h, 1e-10)
        b = ops.lowrank_post_select(h, 1e-10, p_max=128)
        assert a[:3] == b[:3] and a[3].tobytes() == b[3].tobytes()


# ---- the setting and the runner flag -----------------------------------------------------------------------------------------
def test_setting_default_and_range():
    from rpgp_amd import settings
    assert settings.lowrank_max_rank.value() == 64
    with settings.lowrank_max_rank(128):
        assert settings.lowrank_max_rank.value() == 128
        with settings.lowrank_max_rank(1):
            assert settings.lowrank_max_rank.value() == 1
        assert settings.lowrank_max_rank.value() == 128
    assert settings.lowrank_max_rank.value() == 64
    for bad in (0, -1, 129, 1000, 64.5):
        with pytest.raises(ValueError):
            settings.lowrank_max_rank(bad)
    assert settings.lowrank_max_rank.value() == 64


def test_runner_flag_reaches_the_setting(monkeypatch):
    from rpgp_amd import runner, settings
    base = ["-m", "x.json", "-d", "synthetic:tiny", "-o", "o.csv"]
    assert runner.build_parser().parse_args(base + ["--lowrank_max_rank", "128"]).lowrank_max_rank == 128
    assert runner.build_parser().parse_args(base).lowrank_max_rank == 64
    seen = []

    def fake_run(*a, **k):
        seen.append((settings.lowrank_mll.on(), settings.lowrank_max_rank.value()))
        raise KeyboardInterrupt

    monkeypatch.setattr(runner, "run_experiment", fake_run)
    try:
        runner.main(["-m", "additive_rp_J20_K1", "-d", "synthetic:tiny", "-o", "o.csv", "--no_cv", "--lowrank_mll",
                     "--lowrank_max_rank", "96"])
    except KeyboardInterrupt:
        pass
    assert seen == [(True, 96)] and settings.lowrank_max_rank.value() == 64
    with pytest.raises(ValueError):
        runner.main(["-m", "additive_rp_J20_K1", "-d", "synthetic:tiny", "-o", "o.csv", "--no_cv", "--lowrank_max_rank", "129"])


# ---- model level, CPU test double ----------------------------------------------------------------------------------------------
def _features_torch(Z, mid, inv_w, G, scale, out=None, max_rank=64):
    """float64 torch restatement of rpgp_lowrank_features_f64 (differentiable in Z), with the wrapper's rank check."""
    G = torch.as_tensor(G, dtype=torch.float64)
    p, r = G.shape
    assert p <= max_rank <= 128
    X = (Z.double() - torch.as_tensor(mid, dtype=torch.float64)) * inv_w
    T = [torch.ones_like(X), X]
    for _ in range(2, p):
        T.append(2.0 * X * T[-1] - T[-2])
    T = torch.stack(T[:p], dim=-1)
    return (math.sqrt(scale) * (T @ G)).reshape(Z.shape[0], -1)


def _features_grad_torch(Z, mid, inv_w, G, scale, Y, alpha, v, ca, cy, out=None, max_rank=64):
    """float64 torch restatement of rpgp_lowrank_features_grad_f64 (through ops.chebyshev_derivative)."""
    Gd = torch.from_numpy(ops.chebyshev_derivative(torch.as_tensor(G, dtype=torch.float64).numpy()))
    p, r = Gd.shape
    assert p <= max_rank <= 128
    N, J = Z.shape
    X = (Z.double() - torch.as_tensor(mid, dtype=torch.float64)) * inv_w
    T = [torch.ones_like(X), X]
    for _ in range(2, p):
        T.append(2.0 * X * T[-1] - T[-2])
    P = torch.stack(T[:p], dim=-1) @ Gd                                          # N x J x r
    W = ca * alpha.reshape(-1, 1) * v.reshape(1, -1) + cy * Y[:, :J * r]
    return math.sqrt(scale) * inv_w * (P * W.reshape(N, J, r)).sum(-1)


def _install(ob, monkeypatch, calls):
    def grad(*a, **k):
        calls.append(1)
        return _features_grad_torch(*a, **k)
    monkeypatch.setattr(ob, "lowrank_post_select", ops.lowrank_post_select, raising=False)
    monkeypatch.setattr(ob, "lowrank_features", _features_torch, raising=False)
    monkeypatch.setattr(ob, "lowrank_features_grad", grad, raising=False)


HALF_WIDTH = 10.0


def _model(dtype, N=400, d=6, J=5, noise=0.05, s=0.9, seed=0):
    """N = 400, d = 6, J = 5, the lengthscales scaled by one factor so that the widest projected column has a half-width of
    HALF_WIDTH in the units of exp2(-h^2 (x - y)^2)."""
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
    Z = (X.double() / ls.double()) @ P.double()
    ls = ls * (KAPPA * float((0.5 * (Z.max(0).values - Z.min(0).values)).max()) / HALF_WIDTH)
    lin = torch.nn.Linear(d, J, bias=False)
    lin.weight.data = P.t().contiguous()
    lin.weight.requires_grad_(False)
    k = ScaledProjectionKernel(lin, AdditiveStructureRBFKernel(J), prescale=True, ard_num_dims=d)
    k.initialize(lengthscale=ls)
    sk = ScaleKernel(k)
    sk.outputscale = s
    lik = GaussianLikelihood(noise_prior=SmoothedBoxPrior(1e-4, 10, sigma=0.01))
    lik.noise = noise
    X, y = X.to(dtype), y.to(dtype)
    model = ExactGPModel(X, y, lik, sk).to(dtype)
    model.mean_module.constant.data.fill_(0.2)
    return model, lik, ExactMarginalLogLikelihood(lik, model), X, y, Xs.to(dtype), ys.to(dtype), P


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _log_density(mean, cov, y):
    L = np.linalg.cholesky(cov)
    z = np.linalg.solve(L, y - mean)
    return -0.5 * z @ z - np.log(np.diag(L)).sum() - 0.5 * y.size * math.log(2.0 * math.pi)


def test_wide_posterior_against_the_dense_oracle(oracle_backend, monkeypatch):
    """The bounds of tests/test_lowrank_posterior_host.py's served case (1e-7), against the dense float64 GP of the exact
    kernel."""
    from rpgp_amd import settings
    from rpgp_amd.lowrank_posterior import LowrankPredictive
    _install(oracle_backend, monkeypatch, [])
    model, lik, mll, X, y, Xs, ys, P = _model(torch.float32)
    pk = model.covar_module.base_kernel
    ref = orc.DenseExactGP(X.double().numpy(), y.double().numpy(), P.double().numpy(),
                           pk.lengthscale.detach().double().numpy().reshape(-1), float(model.covar_module.outputscale.detach()),
                           float(lik.noise.detach()), mean=float(model.mean_module.constant.detach()))
    sigma2 = float(lik.noise.detach())
    model.eval()
    with settings.lowrank_posterior(True), torch.no_grad():
        model(Xs)                                                          # default cap: not served, the reason names it
        st = model.prediction_strategy
        assert st.lowrank is None and "rank above 64" in st.lowrank_fallback_reason, st.lowrank_fallback_reason
        model.prediction_strategy = None
        with settings.lowrank_max_rank(128):
            out = model(Xs)
            st = model.prediction_strategy
            assert st.lowrank is not None, st.lowrank_fallback_reason
            p, r, F = st.lowrank.ranks
            assert 64 < p <= 128 and r <= p and F == 5 * r, (p, r, F)
            assert abs(st.lowrank.form.h - HALF_WIDTH) <= 0.05 * HALF_WIDTH
            assert isinstance(out, LowrankPredictive)
            mean_ref, cov_ref = ref.predict(Xs.double().numpy(), full_cov=True)
            assert _rel(out._mean64.numpy(), mean_ref) <= 1e-7
            assert _rel(out._var64.numpy(), np.diag(cov_ref)) <= 1e-7
            lp = float(lik(out).log_prob(ys.double()))
            lp_ref = _log_density(mean_ref, cov_ref + sigma2 * np.eye(Xs.shape[0]), ys.double().numpy())
            assert abs(lp - lp_ref) <= 1e-7 * abs(lp_ref), (lp, lp_ref)
            assert _rel((sigma2 * (out._V.t() @ out._V)).numpy(), cov_ref) <= 1e-7
            assert _rel(st.alpha64.reshape(-1).numpy(), ref.solve(ref.y - ref.c)) <= 1e-7
            # test rows outside the training range: the rebuild on the union interval runs under the same cap
            far = Xs * 1.5
            out2 = model(far)
            assert isinstance(out2, LowrankPredictive) and st.lowrank.rebuilds == 1 and st.lowrank.form.p > p
            m2, c2 = ref.predict(far.double().numpy(), full_cov=True)
            assert _rel(out2._mean64.numpy(), m2) <= 1e-7 and _rel(out2._var64.numpy(), np.diag(c2)) <= 1e-7


def _params(model, lik):
    return [model.covar_module.base_kernel.raw_lengthscale, model.covar_module.raw_outputscale, lik.raw_noise,
            model.mean_module.constant]


def _mll_reference(model, lik, X, y, P):
    """float64 autograd of the mll per datum through the dense N x N matrix K = B B^T + sigma^2 I of the same truncated features
    (interval held fixed), selected under the cap 128: the reference of tests/test_lowrank_mll_host.py."""
    from rpgp_amd.likelihoods import LOG2PI
    from rpgp_amd.lowrank_posterior import LowrankPosterior, tail_tolerance
    bk = model.covar_module.base_kernel.base_kernel
    params = [t.detach().clone().requires_grad_(True) for t in _params(model, lik)]
    raw_ls, raw_os, raw_noise, c = params
    ls = torch.nn.functional.softplus(raw_ls).reshape(-1)
    s = torch.nn.functional.softplus(raw_os).reshape(())
    noise = (torch.nn.functional.softplus(raw_noise) + lik.MIN_NOISE).reshape(())
    weight, il = bk._constants()
    Z = (X.double() / ls.reshape(1, -1)) @ P.double() / il
    N, J = Z.shape
    mid, h = LowrankPosterior._interval(Z.detach().min(0).values, Z.detach().max(0).values)
    p, r, tail, G = ops.lowrank_post_select(h, tail_tolerance(N, float(s.detach()) * weight * J, float(noise.detach())), 128)
    assert p > 64
    B = _features_torch(Z, mid, KAPPA / h, G, 1.0, max_rank=128) * torch.sqrt(s * weight)
    K = B @ B.t() + noise * torch.eye(N, dtype=torch.float64)
    rr = (y.double() - c).reshape(-1, 1)
    L = torch.linalg.cholesky(K)
    iq = (rr * torch.cholesky_solve(rr, L)).sum()
    ld = 2.0 * torch.log(L.diagonal()).sum()
    val = (-0.5 * (iq + ld + N * LOG2PI) + lik.noise_prior.log_prob(noise)) / N
    val.backward()
    return float(val.detach()), [t.grad.detach().clone() for t in params], (p, r, J * r)


@pytest.mark.parametrize("fused", [True, False])
def test_wide_mll_against_float64_autograd(oracle_backend, monkeypatch, fused):
    """Value and gradients at the bounds of tests/test_lowrank_mll_host.py's served case (1e-10); with the default cap the same
    model is not served and the reason names the cap in force."""
    from rpgp_amd import settings
    calls = []
    _install(oracle_backend, monkeypatch, calls)
    model, lik, mll, X, y, _, _, P = _model(torch.float64)
    model.train()
    ref, gref, ranks = _mll_reference(model, lik, X, y, P)
    assert ranks[0] > 64 and ranks[2] < X.shape[0], ranks
    noise = float(lik.noise.detach())
    with settings.lowrank_mll(True), settings.fused_training(False):
        op = model(X).covariance
        assert op.lowrank_mll_form(noise) is None and "rank above 64" in op.lowrank_mll_reason, op.lowrank_mll_reason
        with settings.lowrank_max_rank(96):
            op = model(X).covariance
            assert op.lowrank_mll_form(noise) is not None and op.lowrank_mll_form().ranks == ranks
        with settings.lowrank_max_rank(80):
            op = model(X).covariance
            assert op.lowrank_mll_form(noise) is None and "rank above 80" in op.lowrank_mll_reason, op.lowrank_mll_reason
    assert not calls
    with settings.lowrank_mll(True), settings.lowrank_max_rank(128), settings.fused_training(fused):
        val = mll(model(X), y)
        val.backward()
    assert len(calls) == 1
    assert abs(float(val) - ref) <= 1e-10 * abs(ref), (float(val), ref)
    for name, p, g in zip(("raw_lengthscale", "raw_outputscale", "raw_noise", "mean"), _params(model, lik), gref):
        err = float((p.grad.double() - g).abs().max() / max(float(g.abs().max()), 1e-300))
        assert err <= 1e-10, (name, err)
