"""The closed-form marginal likelihood of the Chebyshev low-rank features on the host (no GPU): the derivative coefficients of
ops.chebyshev_derivative against the analytic derivative, the "features" mode of InvQuadLogDet (CPU test double, features and
their adjoint restated in float64 torch) against float64 autograd of the same objective, the serving decision and its reasons,
and the runner flag."""
import math

import numpy as np
import pytest
import torch

from rpgp_amd import ops


def _cheb(x, p):
    T = np.empty((p, x.size))
    T[0] = 1.0
    if p > 1:
        T[1] = x
    for m in range(2, p):
        T[m] = 2.0 * x * T[m - 1] - T[m - 2]
    return T


def _cheb_prime(x, p):
    """T'_m(x) = m U_{m-1}(x)."""
    U = np.empty((p, x.size))
    U[0] = 1.0
    if p > 1:
        U[1] = 2.0 * x
    for m in range(2, p):
        U[m] = 2.0 * x * U[m - 1] - U[m - 2]
    D = np.zeros((p, x.size))
    for m in range(1, p):
        D[m] = m * U[m - 1]
    return D


@pytest.mark.parametrize("h", [0.0, 1.5, 4.6, 7.0])
def test_chebyshev_derivative_against_the_analytic_derivative(h):
    p, r, tail, G = ops.lowrank_post_select(h, 1e-10)
    assert p >= 1
    Gd = ops.chebyshev_derivative(G)
    assert Gd.shape == G.shape and not Gd[p - 1].any()
    x = np.linspace(-1.0, 1.0, 2001)
    got = _cheb(x, p).T @ Gd
    ref = _cheb_prime(x, p).T @ G
    scale = max(np.abs(ref).max(), 1.0)
    assert np.abs(got - ref).max() <= 1e-12 * p * p * scale, (h, np.abs(got - ref).max())
    # and a central difference of the features themselves
    e = 1e-6
    xi = x[1:-1]
    fd = (_cheb(np.clip(xi + e, -1, 1), p).T @ G - _cheb(np.clip(xi - e, -1, 1), p).T @ G) / (2 * e)
    assert np.abs(fd - got[1:-1]).max() <= 1e-6 * scale * p * p


def test_chebyshev_derivative_of_single_polynomials():
    for m in range(0, 9):
        c = np.zeros((9, 1))
        c[m] = 1.0
        x = np.linspace(-1, 1, 33)
        got = _cheb(x, 9).T @ ops.chebyshev_derivative(c)
        assert np.allclose(got[:, 0], _cheb_prime(x, 9)[m], atol=1e-12, rtol=0), m


# ---- the features mode under the CPU test double ---------------------------------------------------------------------------
def _features_torch(Z, mid, inv_w, G, scale):
    """float64 torch restatement of rpgp_lowrank_features_f64 (differentiable in Z)."""
    G = torch.as_tensor(G, dtype=torch.float64)
    p, r = G.shape
    X = (Z.double() - torch.as_tensor(mid, dtype=torch.float64)) * inv_w
    T = [torch.ones_like(X), X]
    for _ in range(2, p):
        T.append(2.0 * X * T[-1] - T[-2])
    T = torch.stack(T[:p], dim=-1)
    return (math.sqrt(scale) * (T @ G)).reshape(Z.shape[0], -1)


def _features_grad_torch(Z, mid, inv_w, G, scale, Y, alpha, v, ca, cy, out=None):
    """float64 torch restatement of rpgp_lowrank_features_grad_f64 (through ops.chebyshev_derivative)."""
    Gd = torch.from_numpy(ops.chebyshev_derivative(torch.as_tensor(G, dtype=torch.float64).numpy()))
    p, r = Gd.shape
    N, J = Z.shape
    X = (Z.double() - torch.as_tensor(mid, dtype=torch.float64)) * inv_w
    T = [torch.ones_like(X), X]
    for _ in range(2, p):
        T.append(2.0 * X * T[-1] - T[-2])
    P = torch.stack(T[:p], dim=-1) @ Gd                                          # N x J x r
    W = ca * alpha.reshape(-1, 1) * v.reshape(1, -1) + cy * Y[:, :J * r]
    g = math.sqrt(scale) * inv_w * (P * W.reshape(N, J, r)).sum(-1)
    if out is not None:
        out.copy_(g)
        return out
    return g


def _install(ob, monkeypatch, calls=None):
    def grad(*a, **k):
        if calls is not None:
            calls.append(1)
        return _features_grad_torch(*a, **k)
    monkeypatch.setattr(ob, "lowrank_post_select", ops.lowrank_post_select, raising=False)
    monkeypatch.setattr(ob, "lowrank_features", _features_torch, raising=False)
    monkeypatch.setattr(ob, "lowrank_features_grad", grad, raising=False)


def _model(N=300, d=4, J=5, noise=0.05, s=0.9, ls_scale=1.0, seed=0, dtype=torch.float64):
    from rpgp_amd.kernels import AdditiveStructureRBFKernel, ScaledProjectionKernel, ScaleKernel
    from rpgp_amd.likelihoods import GaussianLikelihood, SmoothedBoxPrior
    from rpgp_amd.models import ExactGPModel, ExactMarginalLogLikelihood
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g)
    P = torch.randn(d, J, generator=g)
    ls = (torch.rand(d, generator=g) * 1.5 + 1.0) * ls_scale
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
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
    return model, lik, ExactMarginalLogLikelihood(lik, model), X, y


def _params(model, lik):
    return [model.covar_module.base_kernel.raw_lengthscale, model.covar_module.raw_outputscale, lik.raw_noise,
            model.mean_module.constant]


def _reference(model, lik, X, y):
    """float64 autograd of the mll per datum with K = B B^T (the same truncated features, interval held fixed)."""
    from rpgp_amd.lowrank_posterior import LowrankPosterior, tail_tolerance
    from rpgp_amd.likelihoods import LOG2PI
    pk = model.covar_module.base_kernel
    bk = pk.base_kernel
    params = [t.detach().clone().requires_grad_(True) for t in _params(model, lik)]
    raw_ls, raw_os, raw_noise, c = params
    ls = torch.nn.functional.softplus(raw_ls).reshape(-1)
    s = torch.nn.functional.softplus(raw_os).reshape(())
    noise = (torch.nn.functional.softplus(raw_noise) + lik.MIN_NOISE).reshape(())
    weight, il = bk._constants()
    Z = (X.double() / ls.reshape(1, -1)) @ pk.projection_module.weight.t().double() / il
    N, J = Z.shape
    scale = float(s.detach()) * weight
    mid, h = LowrankPosterior._interval(Z.detach().min(0).values, Z.detach().max(0).values)
    p, r, tail, G = ops.lowrank_post_select(h, tail_tolerance(N, scale * J, float(noise.detach())))
    assert p > 0
    inv_w = 0.84932180028801907 / h
    B = _features_torch(Z, mid, inv_w, G, 1.0) * torch.sqrt(s * weight)
    K = B @ B.t() + noise * torch.eye(N, dtype=torch.float64)
    rr = (y.double() - c).reshape(-1, 1)
    L = torch.linalg.cholesky(K)
    iq = (rr * torch.cholesky_solve(rr, L)).sum()
    ld = 2.0 * torch.log(L.diagonal()).sum()
    lp = lik.noise_prior.log_prob(noise) if lik.noise_prior is not None else 0.0
    mll = (-0.5 * (iq + ld + N * LOG2PI) + lp) / N
    mll.backward()
    return float(mll), [t.grad.detach().clone() for t in params], (p, r, J * r)


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


@pytest.mark.parametrize("fused", [True, False])
def test_features_mode_against_float64_autograd(oracle_backend, monkeypatch, fused):
    from rpgp_amd import settings
    calls = []
    _install(oracle_backend, monkeypatch, calls)
    model, lik, mll, X, y = _model()
    model.train()
    ref, gref, ranks = _reference(model, lik, X, y)
    assert ranks[2] < X.shape[0]
    with settings.lowrank_mll(True), settings.fused_training(fused):
        out = model(X)
        val = mll(out, y)
        val.backward()
        if not fused:
            op = out.covariance
            assert op.lowrank_mll_served and op.lowrank_mll_reason is None
            assert op.lowrank_mll_form().ranks == ranks
    assert len(calls) == 1
    assert abs(float(val) - ref) <= 1e-10 * abs(ref), (float(val), ref)
    for name, p, g in zip(("raw_lengthscale", "raw_outputscale", "raw_noise", "mean"), _params(model, lik), gref):
        assert _rel(p.grad, g) <= 1e-10, (name, p.grad, g)


def test_features_mode_skip_logdet_forward_and_identities(oracle_backend, monkeypatch):
    """The value's log-determinant is 0 under skip_logdet_forward (as in the CG mode); the gradient is unchanged."""
    from rpgp_amd import settings
    _install(oracle_backend, monkeypatch)
    model, lik, mll, X, y = _model(seed=2)
    model.train()
    ref, gref, _ = _reference(model, lik, X, y)
    with settings.lowrank_mll(True), settings.fused_training(False), settings.skip_logdet_forward(True):
        out = model(X)
        val = mll(out, y)
        val.backward()
        fm = out.covariance.lowrank_mll_form()
    N = X.shape[0]
    logdet = (N - fm.B.shape[1]) * math.log(fm.noise) + 2.0 * float(torch.log(fm.L.diagonal()).sum())
    assert abs((float(val) - 0.5 * logdet / N) - ref) <= 1e-10 * abs(ref)
    for p, g in zip(_params(model, lik), gref):
        assert _rel(p.grad, g) <= 1e-10
    # tr(Khat^-1) and tr(Khat^-1 K) from the F x F factor
    K = fm.B @ fm.B.t()
    Kh = K + fm.noise * torch.eye(N, dtype=torch.float64)
    Kinv = torch.linalg.inv(Kh)
    tr_minv = float(torch.cholesky_inverse(fm.L).diagonal().sum())
    F = fm.B.shape[1]
    assert abs(float(Kinv.diagonal().sum()) - ((N - F) / fm.noise + tr_minv)) <= 1e-10 * float(Kinv.diagonal().sum())
    assert abs(float((Kinv @ K).diagonal().sum()) - (F - fm.noise * tr_minv)) <= 1e-9 * F


def _op(Z, noise=0.1, s=1.0, shard=None):
    from rpgp_amd.operators import AdditiveRPOperator
    op = AdditiveRPOperator(Z, None, torch.tensor(s, dtype=Z.dtype), 1.0 / Z.shape[1], shard=shard)
    op._noise_host = noise
    return op


def test_serving_decision_and_reasons(oracle_backend, monkeypatch):
    from rpgp_amd import settings
    _install(oracle_backend, monkeypatch)
    g = torch.Generator().manual_seed(1)
    Z = torch.randn(400, 6, generator=g, dtype=torch.float64)
    # off: never taken
    op = _op(Z)
    assert op.lowrank_mll_form() is None and not op.lowrank_mll_served and "off" in op.lowrank_mll_reason
    with settings.lowrank_mll(True):
        op = _op(Z)
        assert op.lowrank_mll_form() is not None and op.lowrank_mll_served and op.lowrank_mll_reason is None
        p, r, F = op.lowrank_mll_form().ranks
        assert 1 <= r <= p <= 64 and F == 6 * r
        # F >= N
        op = _op(Z[:F])
        assert op.lowrank_mll_form() is None and "F >= N" in op.lowrank_mll_reason
        # J > 64
        op = _op(torch.randn(4000, 65, generator=g, dtype=torch.float64))
        assert op.lowrank_mll_form() is None and "J = 65" in op.lowrank_mll_reason
        # p > 64: a half-width beyond the largest rank
        op = _op(Z * 8.0)
        assert op.lowrank_mll_form() is None and "rank above 64" in op.lowrank_mll_reason
        # a sharded operator
        class _Shard:
            world_size, j0, j1 = 2, 0, 3
        op = _op(Z, shard=_Shard())
        assert op.lowrank_mll_form() is None and "sharded" in op.lowrank_mll_reason
        # the decision is taken once per operator
        op = _op(Z)
        fm = op.lowrank_mll_form()
        assert op.lowrank_mll_form(0.5) is fm


def test_not_served_step_is_unchanged_under_the_cpu_double(oracle_backend, monkeypatch):
    """With the setting on but p > 64 (short lengthscales), the step is the setting-off step, bit for bit."""
    from rpgp_amd import settings
    calls = []
    _install(oracle_backend, monkeypatch, calls)

    def step(on, fused):
        model, lik, mll, X, y = _model(N=260, ls_scale=0.05, dtype=torch.float32, seed=3)
        model.train()
        with settings.max_cholesky_size(0), settings.deterministic_probes(True), settings.min_preconditioning_size(100), \
                settings.lowrank_mll(on), settings.fused_training(fused):
            val = mll(model(X), y)
            val.backward()
        return val.detach().clone(), [p.grad.detach().clone() for p in _params(model, lik)]

    for fused in (True, False):
        v0, g0 = step(False, fused)
        v1, g1 = step(True, fused)
        assert torch.equal(v0, v1)
        for a, b in zip(g0, g1):
            assert torch.equal(a, b)
    assert not calls


def test_runner_flag_reaches_the_setting(monkeypatch):
    from rpgp_amd import runner, settings
    args = runner.build_parser().parse_args(["-m", "x.json", "-d", "synthetic:tiny", "-o", "o.csv", "--lowrank_mll"])
    assert args.lowrank_mll
    assert not runner.build_parser().parse_args(["-m", "x.json", "-d", "synthetic:tiny", "-o", "o.csv"]).lowrank_mll
    seen = []

    def fake_run(*a, **k):
        seen.append(settings.lowrank_mll.on())
        raise KeyboardInterrupt

    monkeypatch.setattr(runner, "run_experiment", fake_run)
    try:
        runner.main(["-m", "additive_rp_J20_K1", "-d", "synthetic:tiny", "-o", "o.csv", "--no_cv", "--lowrank_mll"])
    except KeyboardInterrupt:
        pass
    assert seen == [True] and settings.lowrank_mll.off()
