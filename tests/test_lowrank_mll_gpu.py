"""The closed-form marginal likelihood of the Chebyshev low-rank features on the MI355X (settings.lowrank_mll):
rpgp_lowrank_features_grad_f64 against float64 torch autograd of the features, one objective evaluation against the dense float64
oracle (fused and generic objective), the not-served step bit for bit as the setting-off step, an L-BFGS fit (bit-identical
repeats, and the same optimum as the fit driven by the dense float64 objective), the first step of an N = 200 000 fit, and the
runner with --lowrank_mll."""
import json
import math

import numpy as np
import pytest
import torch

from oracle import dense_gp as orc

pytestmark = pytest.mark.gpu

KAPPA = 0.84932180028801907
EPS = 2.0 ** -52


def _features_ref(Z, mid, inv_w, G, scale):
    X = (Z - mid) * inv_w
    p = G.shape[0]
    T = [torch.ones_like(X), X]
    for _ in range(2, p):
        T.append(2.0 * X * T[-1] - T[-2])
    T = torch.stack(T[:p], dim=-1)                        # N x J x p
    return (math.sqrt(scale) * (T @ G)).reshape(Z.shape[0], -1)


@pytest.mark.parametrize("h", [0.0, 1.5, 4.6, 7.0])
def test_features_grad_kernel_against_autograd(gpu_device, h):
    """gZ against autograd of sum(B * W) through the float64 torch features.  Bound: every product term is at most
    |Gd|_max |W|_max sqrt(s) inv_w, there are p r of them per entry and each carries O(p + r) roundings on either side, so
    |err| <= 8 eps (p + r) p r |Gd|_max |W|_max sqrt(s) inv_w (|Gd|_max <= p^2 |G|_max: Markov)."""
    from rpgp_amd import ops
    p, r, tail, G = ops.lowrank_post_select(h, 1e-10)
    assert p > 0
    Gt = torch.from_numpy(G).to(gpu_device)
    gd_max = float(np.abs(ops.chebyshev_derivative(G)).max())
    scale = 0.37
    for N in (1, 63, 20011):
        for J in (1, 7, 20, 64):
            g = torch.Generator().manual_seed(N * 100 + J)
            Z = (torch.randn(N, J, generator=g, dtype=torch.float64) * 1.3).to(gpu_device)
            zmin, zmax = Z.min(0).values, Z.max(0).values
            mid = 0.5 * (zmin + zmax)
            hw = float((0.5 * (zmax - zmin)).max())
            inv_w = 1.0 / hw if hw > 0 else 0.0
            F = J * r
            Y = torch.randn(N, F + 3, generator=g, dtype=torch.float64).to(gpu_device)      # ldy > F
            alpha = torch.randn(N, 1, generator=g, dtype=torch.float64).to(gpu_device)
            v = torch.randn(F, 1, generator=g, dtype=torch.float64).to(gpu_device)
            ca, cy = -0.7, 1.3
            big = torch.full((N, J + 5), float("nan"), dtype=torch.float64, device=gpu_device)
            out = ops.lowrank_features_grad(Z, mid, inv_w, G, scale, Y, alpha, v, ca, cy, out=big[:, :J])
            W = ca * alpha * v.reshape(1, -1) + cy * Y[:, :F]
            if p == 1:                                              # (constant features: nothing to differentiate)
                ref = torch.zeros_like(Z)
            else:
                Zr = Z.clone().requires_grad_(True)
                (_features_ref(Zr, mid, inv_w, Gt, scale) * W).sum().backward()
                ref = Zr.grad
            bound = 8 * EPS * (p + r) * p * r * gd_max * float(W.abs().max()) * math.sqrt(scale) * inv_w + 1e-300
            err = float((out - ref).abs().max())
            assert err <= bound, (h, N, J, err, bound)
            assert bool(torch.isnan(big[:, J:]).all())
            again = ops.lowrank_features_grad(Z, mid, inv_w, G, scale, Y, alpha, v, ca, cy)
            assert torch.equal(again, out)


def test_features_grad_kernel_limits(gpu_device):
    from rpgp_amd import ops
    f64 = dict(dtype=torch.float64, device=gpu_device)
    N = 8
    a = torch.zeros(N, 1, **f64)
    with pytest.raises(ValueError):                                  # J > 64
        ops.lowrank_features_grad(torch.zeros(N, 65, **f64), torch.zeros(65, **f64), 1.0, np.ones((3, 2)), 1.0,
                                  torch.zeros(N, 130, **f64), a, torch.zeros(130, **f64), 1.0, 1.0)
    with pytest.raises(ValueError):                                  # p > 64
        ops.lowrank_features_grad(torch.zeros(N, 2, **f64), torch.zeros(2, **f64), 1.0, np.ones((65, 2)), 1.0,
                                  torch.zeros(N, 4, **f64), a, torch.zeros(4, **f64), 1.0, 1.0)
    with pytest.raises(ValueError):                                  # r > p
        ops.lowrank_features_grad(torch.zeros(N, 2, **f64), torch.zeros(2, **f64), 1.0, np.ones((3, 4)), 1.0,
                                  torch.zeros(N, 8, **f64), a, torch.zeros(8, **f64), 1.0, 1.0)
    with pytest.raises(ValueError):                                  # Y narrower than J r
        ops.lowrank_features_grad(torch.zeros(N, 2, **f64), torch.zeros(2, **f64), 1.0, np.ones((3, 2)), 1.0,
                                  torch.zeros(N, 3, **f64), a, torch.zeros(4, **f64), 1.0, 1.0)


# ---- the objective --------------------------------------------------------------------------------------------------------
def _model(N, d, J, dev, noise=0.1, s=1.0, ls_factor=1.0, seed=0):
    from rpgp_amd.kernels import AdditiveStructureRBFKernel, ScaledProjectionKernel, ScaleKernel
    from rpgp_amd.likelihoods import GaussianLikelihood, SmoothedBoxPrior
    from rpgp_amd.models import ExactGPModel, ExactMarginalLogLikelihood
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g)
    P = torch.randn(d, J, generator=g)
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
    y = (y - y.mean()) / y.std()
    lin = torch.nn.Linear(d, J, bias=False)
    lin.weight.data = P.t().contiguous()
    lin.weight.requires_grad_(False)
    k = ScaledProjectionKernel(lin, AdditiveStructureRBFKernel(J), prescale=True, ard_num_dims=d)
    k.initialize(lengthscale=torch.full((d,), math.sqrt(d) * ls_factor))
    sk = ScaleKernel(k)
    sk.outputscale = s
    lik = GaussianLikelihood(noise_prior=SmoothedBoxPrior(1e-4, 10, sigma=0.01))
    lik.noise = noise
    model = ExactGPModel(X.to(dev), y.to(dev), lik, sk).to(dev)
    model.mean_module.constant.data.fill_(0.1)
    return model, lik, ExactMarginalLogLikelihood(lik, model), X.to(dev), y.to(dev)


def _params(model, lik):
    return [model.covar_module.base_kernel.raw_lengthscale, model.covar_module.raw_outputscale, lik.raw_noise,
            model.mean_module.constant]


def _dense_loss(model, lik, X, y, raw):
    """-mll per datum of the exact kernel in float64 torch on the device, as a function of the raw parameters.  Its value is
    the dense Cholesky's; its gradient comes from the surrogate 0.5 sum((Khat^-1 - alpha alpha^T) * Khat) + alpha^T r with
    Khat^-1 and alpha held fixed (the same first derivatives), so that autograd needs no N x N triangular solve (the library's
    solve runs out of workspace at these sizes)."""
    raw_ls, raw_os, raw_noise, c = raw
    pk = model.covar_module.base_kernel
    ls = torch.nn.functional.softplus(raw_ls).reshape(-1)
    s = torch.nn.functional.softplus(raw_os).reshape(())
    noise = (torch.nn.functional.softplus(raw_noise) + lik.MIN_NOISE).reshape(())
    P = pk.projection_module.weight.detach().t().double()
    Z = (X.double() / ls.reshape(1, -1)) @ P
    N, J = Z.shape
    K = torch.zeros(N, N, dtype=torch.float64, device=X.device)
    for j in range(J):
        K = K + torch.exp(-0.5 * (Z[:, j:j + 1] - Z[:, j:j + 1].t()) ** 2)
    Kh = (s / J) * K + noise * torch.eye(N, dtype=torch.float64, device=X.device)
    rr = (y.double() - c).reshape(-1, 1)
    with torch.no_grad():
        L = torch.linalg.cholesky(Kh)
        alpha = torch.cholesky_solve(rr, L)
        S = torch.cholesky_inverse(L) - alpha @ alpha.t()
        value = 0.5 * ((rr * alpha).sum() + 2.0 * torch.log(L.diagonal()).sum() + N * math.log(2 * math.pi))
    sur = 0.5 * (S * Kh).sum() + (alpha * rr).sum()
    lp = lik.noise_prior.log_prob(noise)
    return (value + (sur - sur.detach()) - lp) / N


class _Spy:
    """Counts the calls of the features mode's adjoint kernel (= objective evaluations in that mode)."""

    def __init__(self, monkeypatch):
        from rpgp_amd import backend, ops
        self.calls = 0
        inner = ops.lowrank_features_grad

        def counting(*a, **k):
            self.calls += 1
            return inner(*a, **k)
        monkeypatch.setattr(backend.HipBackend, "lowrank_features_grad", staticmethod(counting))


@pytest.mark.parametrize("fused", [True, False])
def test_objective_against_the_dense_oracle(gpu_device, monkeypatch, fused):
    from rpgp_amd import settings
    spy = _Spy(monkeypatch)
    N, d, J = 5000, 20, 20
    model, lik, mll, X, y = _model(N, d, J, gpu_device)
    model.train()
    with settings.lowrank_mll(True), settings.fused_training(fused):
        loss = mll.negative(model(X), y)
        loss.backward()
    assert spy.calls == 1
    pk = model.covar_module.base_kernel
    ref = orc.DenseExactGP(X.double().cpu().numpy(), y.double().cpu().numpy(),
                           pk.projection_module.weight.detach().t().double().cpu().numpy(),
                           pk.lengthscale.detach().double().cpu().numpy().reshape(-1),
                           float(model.covar_module.outputscale.detach()), float(lik.noise.detach()),
                           mean=float(model.mean_module.constant.detach()))
    mll_ref = ref.mll()
    assert abs(-float(loss) - mll_ref) <= 1e-6, (-float(loss), mll_ref)
    raw = [p.detach().double().clone().requires_grad_(True) for p in _params(model, lik)]
    _dense_loss(model, lik, X, y, raw).backward()
    # 1e-5 relative: float32 parameters and result; the truncation's own share is ~ N s tail / sigma^2 <= 1e-6.  The mean's
    # gradient -sum(alpha) / N is summed in float32 over N = 5 000 terms that cancel (measured 1.4e-5): it is held to 5e-5.
    for name, p, r in zip(("raw_lengthscale", "raw_outputscale", "raw_noise", "mean"), _params(model, lik), raw):
        err = float((p.grad.double() - r.grad).abs().max() / r.grad.abs().max())
        print("%s fused=%s: rel %.3g" % (name, fused, err))
        assert err <= (5e-5 if name == "mean" else 1e-5), (name, err)


def test_not_served_is_the_setting_off_step(gpu_device, monkeypatch):
    """Short lengthscales (half-width beyond rank 64): the step with the setting on is the setting-off step, bit for bit."""
    from rpgp_amd import settings
    spy = _Spy(monkeypatch)

    def step(on, fused):
        model, lik, mll, X, y = _model(4000, 20, 20, gpu_device, ls_factor=0.05)
        model.train()
        with settings.lowrank_mll(on), settings.fused_training(fused), settings.deterministic_probes(True):
            loss = mll.negative_and_backward(model(X), y)
        return loss.detach().clone(), [p.grad.detach().clone() for p in _params(model, lik)]

    for fused in (True, False):
        v0, g0 = step(False, fused)
        v1, g1 = step(True, fused)
        assert torch.equal(v0, v1), fused
        for a, b in zip(g0, g1):
            assert torch.equal(a, b), fused
    assert spy.calls == 0


def _lbfgs(params, closure, iters=20):
    opt = torch.optim.LBFGS(params, lr=1.0, max_iter=iters, line_search_fn="strong_wolfe")
    opt.step(closure)
    return opt.state[opt._params[0]]["n_iter"]


def test_lbfgs_fit(gpu_device, monkeypatch):
    """An L-BFGS fit (20 iterations, strong-Wolfe line search) on the features objective: two runs are bit-identical, and the
    hyper-parameters land within 2e-3 (relative) of the same fit driven by the dense float64 objective.  (A line search can try
    lengthscales short enough to need p > 64; those evaluations take the dense Cholesky of today's code, made the fallback
    here by max_cholesky_size, which is deterministic too.)"""
    from rpgp_amd import settings
    spy = _Spy(monkeypatch)

    def fit():
        model, lik, mll, X, y = _model(3000, 8, 20, gpu_device, seed=4)
        model.train()
        params = _params(model, lik)

        def closure():
            for p in params:
                p.grad = None
            loss = mll.negative(model(X), y)
            loss.backward()
            return loss

        with settings.lowrank_mll(True), settings.max_cholesky_size(4000):
            n_iter = _lbfgs(params, closure)
        return model, lik, X, y, [p.detach().clone() for p in params], n_iter

    model, lik, X, y, a, n_iter = fit()
    calls = spy.calls
    assert calls > 0
    _, _, _, _, b, _ = fit()
    assert spy.calls == 2 * calls
    for u, w in zip(a, b):
        assert torch.equal(u, w)
    # the same fit on the dense float64 objective, from the same start
    m0, l0, _, _ = _model(3000, 8, 20, gpu_device, seed=4)[:4]
    raw = [p.detach().double().clone().requires_grad_(True) for p in _params(m0, l0)]

    def closure64():
        for p in raw:
            p.grad = None
        loss = _dense_loss(m0, l0, X, y, raw)
        loss.backward()
        return loss

    _lbfgs(raw, closure64)
    sp = torch.nn.functional.softplus
    for name, u, w, f in zip(("lengthscale", "outputscale", "noise", "mean"), a, raw, (sp, sp, sp, lambda t: t)):
        fu, fw = f(u.double()), f(w.detach())
        err = float((fu - fw).abs().max() / fw.abs().max())
        print("lbfgs %s: rel %.3g (%d iterations, %d evaluations)" % (name, err, n_iter, calls))
        assert err <= 2e-3, (name, err)


def test_first_step_at_200k_against_the_lowrank_kernel_step(gpu_device, monkeypatch):
    """N = 200 000, J = 20, half-width 4.6: the first step is served; its value agrees with the lowrank_kernel step's (CG to
    0.01, 10 SLQ probes: their spread is ~1e-3 per datum) to 1e-2 per datum."""
    from rpgp_amd import settings
    spy = _Spy(monkeypatch)
    N, d, J = 200000, 20, 20
    model, lik, mll, X, y = _model(N, d, J, gpu_device, seed=5)
    pk = model.covar_module.base_kernel
    with torch.no_grad():
        Z = pk.project(X) * (pk.base_kernel.input_scale_factor() or 1.0)
        h0 = KAPPA * float(((Z.max(0).values - Z.min(0).values) * 0.5).max())
        pk.initialize(lengthscale=pk.lengthscale.detach().reshape(-1) * (h0 / 4.6))
    model.train()
    vals = {}
    for mode in ("mll", "kernel"):
        with settings.lowrank_mll(mode == "mll"), settings.lowrank_kernel(mode == "kernel"), \
                settings.deterministic_probes(True), settings.cg_tolerance(0.01), settings.max_cg_iterations(10000):
            loss = mll.negative(model(X), y)
            loss.backward()
        vals[mode] = float(loss)
        for p in _params(model, lik):
            p.grad = None
    assert spy.calls == 1
    print("200k first step: features %.8f, lowrank_kernel %.8f" % (vals["mll"], vals["kernel"]))
    assert abs(vals["mll"] - vals["kernel"]) <= 1e-2, vals


def test_runner_with_the_flag(gpu_device, tmp_path, monkeypatch):
    from rpgp_amd import runner, specs
    spy = _Spy(monkeypatch)
    spec = specs.get("additive_rp_prescale_J20.json")
    spec["train_kwargs"]["max_iter"] = 5
    spec["train_kwargs"]["init_iters"] = 1
    spec["model_kwargs"]["init_lengthscale_range"] = [3.0, 3.0]      # half-width ~4.5 on kin8nm: served from the first step
    sp = tmp_path / "spec.json"
    json.dump(spec, open(sp, "w"))
    torch.manual_seed(0)
    np.random.seed(0)
    df = runner.main(["-m", str(sp), "-d", "synthetic:kin8nm", "-o", str(tmp_path / "r.csv"), "--no_cv",
                      "--skip_random_restart", "--device", "cuda:0", "--lowrank_mll"])
    assert "error" not in df.columns, df
    row = df.iloc[0]
    assert np.isfinite(float(row["rmse"])) and np.isfinite(float(row["test_nll"]))
    print("runner --lowrank_mll: %d evaluations in the features mode" % spy.calls)
    assert spy.calls > 0
