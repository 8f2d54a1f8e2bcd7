"""Chebyshev feature ranks above 64 on the MI355X (settings.lowrank_max_rank): the padded-rank 72 ... 128 instantiations of
rpgp_lowrank_features_f64 and rpgp_lowrank_features_grad_f64 against float64 torch, B B^T of the selected G against the exact
kernel, narrow ranks under the wide cap bit for bit, the wrappers' limits, and one model at a half-width of about 10 end to end
(posterior and marginal likelihood against dense float64 references; the default cap leaves the step as it was)."""
import math

import numpy as np
import pytest
import torch

from oracle import dense_gp as orc
from tests.test_lowrank_mll_gpu import _Spy, _dense_loss, _params
from tests.test_lowrank_mll_gpu import _model as _mll_model
from tests.test_lowrank_posterior_gpu import _check_against_dense, _features_ref
from tests.test_lowrank_posterior_gpu import _model as _posterior_model

pytestmark = pytest.mark.gpu

KAPPA = 0.84932180028801907
EPS = 2.0 ** -52
HALF_WIDTH = 10.0
SHAPES = [(N, J) for N in (1, 63, 65, 257) for J in (1, 7, 64)]


def _problem(N, J, seed, dev):
    g = torch.Generator().manual_seed(seed)
    Z = (torch.randn(N, J, generator=g, dtype=torch.float64) * 1.3).to(dev)
    zmin, zmax = Z.min(0).values, Z.max(0).values
    hw = float((0.5 * (zmax - zmin)).max())
    return g, Z, 0.5 * (zmin + zmax), (1.0 / hw if hw > 0 else 0.0)


def _random_G(p, r, seed):
    return torch.randn(p, r, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).numpy()


@pytest.mark.parametrize("PB", [72, 80, 88, 96, 104, 112, 120, 128])
def test_wide_feature_kernel_against_torch(gpu_device, PB):
    """Every padded rank above 64 with p = PB - 3 (zero-padded rows) and r = 1, 17 (a partial second column tile) and p (r = p =
    125: eight column tiles, the largest LDS image), into a view of a wider NaN-filled buffer.  The bound has the form of
    tests/test_lowrank_posterior_gpu.py: 1e-13 p max|G| sqrt(scale)."""
    from rpgp_amd import ops
    p, scale, worst = PB - 3, 0.37, 0.0
    for r in (1, 17, p):
        G = _random_G(p, r, 1000 * PB + r)
        Gd = torch.from_numpy(G).to(gpu_device)
        bound = 1e-13 * p * float(np.abs(G).max()) * math.sqrt(scale)
        for N, J in SHAPES:
            _, Z, mid, inv_w = _problem(N, J, N * 100 + J, gpu_device)
            F = J * r
            big = torch.full((N, F + 5), float("nan"), dtype=torch.float64, device=gpu_device)
            out = ops.lowrank_features(Z, mid, inv_w, G, scale, out=big[:, :F], max_rank=128)
            err = float((out - _features_ref(Z, mid, inv_w, Gd, scale)).abs().max())
            worst = max(worst, err / bound)
            assert err <= bound, (PB, r, N, J, err, bound)
            assert bool(torch.isnan(big[:, F:]).all())
            assert torch.equal(ops.lowrank_features(Z, mid, inv_w, G, scale, max_rank=128), out)
    print("PB %d: largest error / bound = %.3g" % (PB, worst))


@pytest.mark.parametrize("PB", [72, 80, 88, 96, 104, 112, 120, 128])
def test_wide_features_grad_kernel_against_autograd(gpu_device, PB):
    """The same grid for the adjoint, against autograd of sum(B * W) through the float64 torch features, with the bound of
    tests/test_lowrank_mll_gpu.py: 8 eps (p + r) p r |Gd|_max |W|_max sqrt(s) inv_w."""
    from rpgp_amd import ops
    p, scale, worst = PB - 3, 0.37, 0.0
    ca, cy = -0.7, 1.3
    for r in (1, 17, p):
        G = _random_G(p, r, 2000 * PB + r)
        Gt = torch.from_numpy(G).to(gpu_device)
        gd_max = float(np.abs(ops.chebyshev_derivative(G)).max())
        for N, J in SHAPES:
            g, Z, mid, inv_w = _problem(N, J, N * 100 + J, gpu_device)
            F = J * r
            Y = torch.randn(N, F + 3, generator=g, dtype=torch.float64).to(gpu_device)      # ldy > F
            alpha = torch.randn(N, 1, generator=g, dtype=torch.float64).to(gpu_device)
            v = torch.randn(F, 1, generator=g, dtype=torch.float64).to(gpu_device)
            big = torch.full((N, J + 5), float("nan"), dtype=torch.float64, device=gpu_device)
            out = ops.lowrank_features_grad(Z, mid, inv_w, G, scale, Y, alpha, v, ca, cy, out=big[:, :J], max_rank=128)
            W = ca * alpha * v.reshape(1, -1) + cy * Y[:, :F]
            Zr = Z.clone().requires_grad_(True)
            (_features_ref(Zr, mid, inv_w, Gt, scale) * W).sum().backward()
            bound = 8 * EPS * (p + r) * p * r * gd_max * float(W.abs().max()) * math.sqrt(scale) * inv_w + 1e-300
            err = float((out - Zr.grad).abs().max())
            worst = max(worst, err / bound)
            assert err <= bound, (PB, r, N, J, err, bound)
            assert bool(torch.isnan(big[:, J:]).all())
            again = ops.lowrank_features_grad(Z, mid, inv_w, G, scale, Y, alpha, v, ca, cy, max_rank=128)
            assert torch.equal(again, out)
    print("PB %d: largest error / bound = %.3g" % (PB, worst))


@pytest.mark.parametrize("h", [8.0, 10.0, 14.0])
def test_wide_feature_gram_against_the_exact_kernel(gpu_device, h):
    """B B^T on 2 000 rows (d = 20, J = 20), the coordinates scaled to the half-width h, against the float64 kernel: within
    s tail + 1e-13, the shape of test_feature_gram_against_the_exact_kernel."""
    from rpgp_amd import ops
    d, J, s = 20, 20, 1.0
    X = torch.randn(2000, d, generator=torch.Generator().manual_seed(0)).double()
    P = torch.randn(d, J, generator=torch.Generator().manual_seed(1)).double()
    Z = (X / math.sqrt(d)) @ P
    Z = Z * (h / (KAPPA * float((0.5 * (Z.max(0).values - Z.min(0).values)).max()) * (1.0 + 2.0 ** -20)))
    zmin, zmax = Z.min(0).values, Z.max(0).values
    hh = KAPPA * float((0.5 * (zmax - zmin)).max()) * (1.0 + 2.0 ** -20)
    assert abs(hh - h) <= 1e-9 * h
    p, r, tail, G = ops.lowrank_post_select(hh, 1e-10, p_max=128)
    assert p > 64
    Zd = Z.to(gpu_device)
    B = ops.lowrank_features(Zd, (0.5 * (zmin + zmax)).to(gpu_device), KAPPA / hh, G, s / J, max_rank=128)
    K = torch.zeros(2000, 2000, dtype=torch.float64, device=gpu_device)
    for j in range(J):
        K += torch.exp(-0.5 * (Zd[:, j:j + 1] - Zd[:, j:j + 1].t()) ** 2)
    err = float((B @ B.t() - (s / J) * K).abs().max())
    print("h = %g: p = %d r = %d, |B B^T - K| = %.3g, s tail = %.3g" % (h, p, r, err, s * tail))
    assert err <= s * tail + 1e-13, (err, s * tail, p, r)


@pytest.mark.parametrize("h", [1.5, 4.6, 7.0])
def test_narrow_ranks_do_not_depend_on_the_cap(gpu_device, h):
    from rpgp_amd import ops
    p, r, tail, G = ops.lowrank_post_select(h, 1e-10)
    assert 0 < p <= 64
    g, Z, mid, inv_w = _problem(257, 7, 5, gpu_device)
    F = 7 * r
    Y = torch.randn(257, F, generator=g, dtype=torch.float64).to(gpu_device)
    alpha = torch.randn(257, 1, generator=g, dtype=torch.float64).to(gpu_device)
    v = torch.randn(F, 1, generator=g, dtype=torch.float64).to(gpu_device)
    assert torch.equal(ops.lowrank_features(Z, mid, inv_w, G, 0.37, max_rank=128), ops.lowrank_features(Z, mid, inv_w, G, 0.37))
    assert torch.equal(ops.lowrank_features_grad(Z, mid, inv_w, G, 0.37, Y, alpha, v, -0.7, 1.3, max_rank=128),
                       ops.lowrank_features_grad(Z, mid, inv_w, G, 0.37, Y, alpha, v, -0.7, 1.3))


@pytest.mark.parametrize("r", [1, 17])
def test_narrow_and_wide_staging_give_the_same_bits(gpu_device, r):
    """G with p = 61 (PB 64: static LDS, stride 80) and the same G with nine zero rows appended (p = 70, PB 72: dynamic LDS) give
    the same bits in the features and in the adjoint: the two further MFMA steps add exact zeros to the same accumulation chain,
    and the Chebyshev derivative of zero rows is zero rows.  N = 65: a second wave and a partial row block; r = 17: a partial
    second column tile; J = 7: more than one projection."""
    from rpgp_amd import ops
    G = _random_G(61, r, 3000 + r)
    Gz = np.concatenate([G, np.zeros((9, r))])
    for N in (1, 65):
        for J in (1, 7):
            g, Z, mid, inv_w = _problem(N, J, N * 100 + J, gpu_device)
            F = J * r
            Y = torch.randn(N, F, generator=g, dtype=torch.float64).to(gpu_device)
            alpha = torch.randn(N, 1, generator=g, dtype=torch.float64).to(gpu_device)
            v = torch.randn(F, 1, generator=g, dtype=torch.float64).to(gpu_device)
            assert torch.equal(ops.lowrank_features(Z, mid, inv_w, G, 0.37, max_rank=128),
                               ops.lowrank_features(Z, mid, inv_w, Gz, 0.37, max_rank=128)), (N, J)
            assert torch.equal(ops.lowrank_features_grad(Z, mid, inv_w, G, 0.37, Y, alpha, v, -0.7, 1.3, max_rank=128),
                               ops.lowrank_features_grad(Z, mid, inv_w, Gz, 0.37, Y, alpha, v, -0.7, 1.3, max_rank=128)), (N, J)


def test_wide_limits(gpu_device):
    from rpgp_amd import ops
    f64 = dict(dtype=torch.float64, device=gpu_device)
    N = 8
    Z, mid, a = torch.zeros(N, 2, **f64), torch.zeros(2, **f64), torch.zeros(N, 1, **f64)
    Y, v = torch.zeros(N, 4, **f64), torch.zeros(4, **f64)
    for G, kw in ((np.ones((129, 2)), {"max_rank": 128}), (np.ones((65, 2)), {}), (np.ones((3, 2)), {"max_rank": 129}),
                  (np.ones((97, 2)), {"max_rank": 96})):
        with pytest.raises(ValueError):
            ops.lowrank_features(Z, mid, 1.0, G, 1.0, **kw)
        with pytest.raises(ValueError):
            ops.lowrank_features_grad(Z, mid, 1.0, G, 1.0, Y, a, v, 1.0, 1.0, **kw)
    ops.lowrank_features(Z, mid, 1.0, np.ones((65, 2)), 1.0, max_rank=65)            # the cap itself is served
    ops.lowrank_features_grad(Z, mid, 1.0, np.ones((128, 2)), 1.0, Y, a, v, 1.0, 1.0, max_rank=128)


# ---- end to end: N = 1 500, d = 8, J = 20 at a half-width of about 10 ------------------------------------------------------------
N_E2E, D_E2E, J_E2E = 1500, 8, 20


def _lengthscale_factor(seed=0):
    """The factor on the lengthscale sqrt(d) that gives the widest projected column of both helper models (same seed, same
    draws of X and P) the half-width HALF_WIDTH."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N_E2E, D_E2E, generator=g)
    P = torch.randn(D_E2E, J_E2E, generator=g)
    Z = (X.double() / math.sqrt(D_E2E)) @ P.double()
    return KAPPA * float((0.5 * (Z.max(0).values - Z.min(0).values)).max()) / HALF_WIDTH


def test_wide_posterior_end_to_end(gpu_device):
    """Served with the cap at 128 (p above 64) and within the 1e-5 of the existing small-model posterior test of a dense float64
    solve; with the default cap the same model is not served and says why."""
    from rpgp_amd import settings
    ls = torch.full((D_E2E,), math.sqrt(D_E2E) * _lengthscale_factor())
    model, lik, mll, X, y, Xs, ys = _posterior_model(N_E2E, D_E2E, J_E2E, gpu_device, ls=ls)
    model.eval()
    with settings.lowrank_posterior(True), torch.no_grad():
        model(Xs)
        st = model.prediction_strategy
        assert st.lowrank is None and "rank above 64" in st.lowrank_fallback_reason, st.lowrank_fallback_reason
    model.prediction_strategy = None
    with settings.lowrank_max_rank(128):
        st = _check_against_dense(model, lik, X, y, Xs, ys, 1e-5)
    p, r, F = st.lowrank.ranks
    print("posterior: p = %d r = %d F = %d tail = %.3g h = %.4g" % (p, r, F, st.lowrank.form.tail, st.lowrank.form.h))
    assert 64 < p <= 128 and F == J_E2E * r and abs(st.lowrank.form.h - HALF_WIDTH) <= 0.02 * HALF_WIDTH


def test_wide_mll_end_to_end(gpu_device, monkeypatch):
    """One evaluation with lowrank_mll and the cap at 128 is served; value (1e-6 absolute) and gradients (1e-5 relative, the
    mean's 5e-5) against the dense float64 oracle: the bounds of the N = 5 000 test of tests/test_lowrank_mll_gpu.py."""
    from rpgp_amd import settings
    spy = _Spy(monkeypatch)
    model, lik, mll, X, y = _mll_model(N_E2E, D_E2E, J_E2E, gpu_device, ls_factor=_lengthscale_factor())
    model.train()
    with settings.lowrank_mll(True), settings.lowrank_max_rank(128):
        out = model(X)
        loss = mll.negative(out, y)
        loss.backward()
    assert spy.calls == 1
    pk = model.covar_module.base_kernel
    ref = orc.DenseExactGP(X.double().cpu().numpy(), y.double().cpu().numpy(),
                           pk.projection_module.weight.detach().t().double().cpu().numpy(),
                           pk.lengthscale.detach().double().cpu().numpy().reshape(-1),
                           float(model.covar_module.outputscale.detach()), float(lik.noise.detach()),
                           mean=float(model.mean_module.constant.detach()))
    mll_ref = ref.mll()
    print("mll: value error %.3g" % abs(-float(loss.detach()) - mll_ref))
    assert abs(-float(loss) - mll_ref) <= 1e-6, (-float(loss), mll_ref)
    raw = [p.detach().double().clone().requires_grad_(True) for p in _params(model, lik)]
    _dense_loss(model, lik, X, y, raw).backward()
    for name, p, r in zip(("raw_lengthscale", "raw_outputscale", "raw_noise", "mean"), _params(model, lik), raw):
        err = float((p.grad.double() - r.grad).abs().max() / r.grad.abs().max())
        print("mll: %s rel %.3g" % (name, err))
        assert err <= (5e-5 if name == "mean" else 1e-5), (name, err)


def test_default_cap_leaves_the_step_as_it_was(gpu_device, monkeypatch):
    """The same model under the default cap: the step with lowrank_mll on is the setting-off step, bit for bit, and the adjoint
    kernel is never called."""
    from rpgp_amd import settings
    spy = _Spy(monkeypatch)
    factor = _lengthscale_factor()

    def step(on):
        model, lik, mll, X, y = _mll_model(N_E2E, D_E2E, J_E2E, gpu_device, ls_factor=factor)
        model.train()
        with settings.lowrank_mll(on), settings.deterministic_probes(True):
            loss = mll.negative_and_backward(model(X), y)
        return loss.detach().clone(), [p.grad.detach().clone() for p in _params(model, lik)]

    v0, g0 = step(False)
    v1, g1 = step(True)
    assert torch.equal(v0, v1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    assert spy.calls == 0
