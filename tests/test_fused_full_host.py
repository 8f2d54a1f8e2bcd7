"""Host side of settings.fused_full (no GPU): `kind: full` models on operators.FullKernelOperator, with the radial entries of the
backend served by the float64 family oracle (one component of group = d) — the operator the kernel returns, the marginal
likelihood and its gradients against today's dense autograd path, the predictions against a dense float64 solve, what is not
served and why, and the runner's flag."""
import types

import numpy as np
import pytest
import torch

from oracle import family as fmo
from tests.oracle_backend import _np, _t


def _radial_entries(ob):
    """Extend the CPU test double with the radial entries, through oracle.family."""
    def radial_mvm(self, kind, Z1, Z2, V, scale, noise=0.0):
        squeeze = V.dim() == 1
        z1 = _np(Z1)
        z2 = z1 if Z2 is None else _np(Z2)
        v = _np(V).reshape(z2.shape[0], -1)
        r = _t(fmo.mvm(z1, z2, v, kind, z1.shape[1], [1.0], scale, noise if Z2 is None else 0.0), V)
        return r.squeeze(1) if squeeze else r

    def radial_dense(self, kind, Z1, Z2, scale):
        return _t(fmo.kernel_matrix(_np(Z1), _np(Z2), kind, Z1.shape[1], [1.0], scale), Z1)

    def radial_bilinear_grad(self, kind, Z, L, R, scale):
        g, gc = fmo.bilinear_grad(_np(Z), _np(L), _np(R), kind, Z.shape[1], [1.0], scale)
        return _t(g, Z), _t(np.array(gc[0]), Z)

    def radial_bilinear_grad_dense(self, kind, Z, S, scale):
        g, gc = fmo.bilinear_grad_dense(_np(Z), _np(S), kind, Z.shape[1], [1.0], scale)
        return _t(g, Z), _t(np.array(gc[0]), Z)

    for f in (radial_mvm, radial_dense, radial_bilinear_grad, radial_bilinear_grad_dense):
        setattr(ob, f.__name__, types.MethodType(f, ob))
    ob.radial_max_dims = 1024
    return ob


@pytest.fixture
def radial_backend(oracle_backend):
    return _radial_entries(oracle_backend)


def _problem(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g) + 2.0                     # (off-centre on purpose: the operator centres)
    y = torch.sin(X).sum(1) + 0.1 * torch.randn(n, generator=g)
    return X, (y - y.mean()) / y.std()


def _model(X, y, ard, kernel_type, seed=0):
    from rpgp_amd.training import create_exact_gp
    torch.manual_seed(seed)
    model, lik = create_exact_gp(X, y, "full", noise_prior=True, ard=ard, kernel_type=kernel_type)
    d = X.shape[1]
    # a lengthscale at which every kind is positive definite on these inputs (cos(pi r) only while r stays well below 1/2)
    ls = (40.0 if kernel_type == "Cosine" else 2.0) * (1.0 + 0.1 * torch.arange(d if ard else 1, dtype=torch.float32))
    model.covar_module.base_kernel.lengthscale = ls
    model.covar_module.outputscale = 1.3
    lik.noise = 0.2
    return model, lik


CONFIGS = [(True, "RBF"), (False, "RBF"), (True, "InverseMQ"), (False, "Matern"), (True, "Matern"), (False, "Cosine"),
           (False, "InverseMQ"), (True, "Cosine")]


def _mll_and_grads(X, y, ard, kernel_type, on):
    from rpgp_amd import settings
    from rpgp_amd.models import ExactMarginalLogLikelihood
    model, lik = _model(X, y, ard, kernel_type)
    mll = ExactMarginalLogLikelihood(lik, model)
    model.train()
    with settings.fused_full(on):
        out = model(model.train_inputs)
        cov = out.covariance
        val = mll(out, model.train_targets)
        val.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    return cov, float(val.detach()), grads, model


@pytest.mark.parametrize("ard,kernel_type", CONFIGS)
def test_full_kernel_operator_mll_matches_dense_autograd(radial_backend, ard, kernel_type):
    """Under settings.fused_full the `full` model is a FullKernelOperator, and its marginal likelihood and the gradients of the raw
    lengthscale(s), outputscale, noise and mean agree with the same model on today's dense autograd path to rtol 1e-4."""
    from rpgp_amd.dense_ops import DenseKernelOperator
    from rpgp_amd.operators import AdditiveRPOperator, FullKernelOperator
    X, y = _problem(90, 5, seed=3)
    cov_on, v_on, g_on, m_on = _mll_and_grads(X, y, ard, kernel_type, True)
    cov_off, v_off, g_off, m_off = _mll_and_grads(X, y, ard, kernel_type, False)
    assert type(cov_on) is FullKernelOperator and isinstance(cov_on, AdditiveRPOperator) and cov_on.kind == kernel_type
    assert m_on.covar_module.base_kernel.fused_full_reason is None
    assert type(cov_off) is DenseKernelOperator and "off" in m_off.covar_module.base_kernel.fused_full_reason
    assert len(cov_on.representation()) == 2 and cov_on.Z1.shape == (90, 5) and cov_on.Z1.requires_grad
    assert abs(float(cov_on.Z1.detach().mean())) < 1e-5                       # centred by the training inputs' column mean
    assert cov_on.lowrank_form(0.2) is None and cov_on.fused_pivoted_cholesky(5) is None and cov_on.native_sharding() is None
    assert abs(v_on - v_off) <= 1e-4 * abs(v_off)
    assert set(g_on) == set(g_off) and len(g_on) == 4
    for name in g_off:
        a, b = g_on[name].double().reshape(-1), g_off[name].double().reshape(-1)
        assert a.shape == b.shape and float((a - b).norm()) <= 1e-4 * float(b.norm()), (name, a, b)


def test_full_kernel_operator_protocol(radial_backend):
    """Product (with the fused noise), rows, dense form, constant diagonal, transpose and both derivative forms of the operator
    against the float64 oracle on its own Z."""
    from rpgp_amd.operators import AddedDiagOperator, FullKernelOperator
    g = torch.Generator().manual_seed(1)
    Z, Z2 = torch.randn(40, 7, generator=g) * 0.6, torch.randn(9, 7, generator=g) * 0.6
    V = torch.randn(40, 3, generator=g)
    s = torch.tensor(1.7)
    for kind in ("RBF", "Matern", "InverseMQ", "Cosine"):
        op = FullKernelOperator(Z, None, s, kind)
        K = fmo.kernel_matrix(Z.numpy(), Z.numpy(), kind, 7, [1.0], 1.7)
        assert np.allclose(op._matmul(V, noise=0.3).numpy(), K @ V.double().numpy() + 0.3 * V.numpy(), rtol=1e-5, atol=1e-5)
        assert np.allclose(AddedDiagOperator(op, 0.3)._matmul(V).numpy(), K @ V.double().numpy() + 0.3 * V.numpy(), rtol=1e-5,
                           atol=1e-5)
        assert np.allclose(op.to_dense().numpy(), K, atol=1e-6) and np.allclose(op._diagonal().numpy(), np.diag(K), atol=1e-6)
        idx = torch.tensor([3, 39, 3])
        assert np.allclose(op._get_rows(idx).numpy(), K[idx.numpy()], atol=1e-6)
        assert op.t() is op and tuple(op.shape) == (40, 40)
        opr = FullKernelOperator(Z2, Z, s, kind)
        Kr = fmo.kernel_matrix(Z2.numpy(), Z.numpy(), kind, 7, [1.0], 1.7)
        assert np.allclose(opr._matmul(V).numpy(), Kr @ V.double().numpy(), rtol=1e-5, atol=1e-5)
        W = torch.randn(9, 2, generator=g)
        assert np.allclose(opr.t()._matmul(W).numpy(), Kr.T @ W.double().numpy(), rtol=1e-5, atol=1e-5)
        assert len(opr.representation()) == 3
        with pytest.raises(ValueError):
            opr._matmul(V, noise=0.1)
        L, R = torch.randn(40, 4, generator=g), torch.randn(40, 4, generator=g)
        gZ, gs = op._bilinear_derivative(L, R)
        rZ, rc = fmo.bilinear_grad(Z.double().numpy(), L.numpy(), R.numpy(), kind, 7, [1.0], 1.7)
        assert np.allclose(gZ.numpy(), rZ, rtol=1e-4, atol=1e-5) and abs(float(gs) - rc[0]) < 1e-4 * max(1.0, abs(rc[0]))
        S = torch.randn(40, 40, generator=g)
        S = (S + S.t()) / 2
        gZ, gs = op.dense_weight_derivative(S)
        rZ, rc = fmo.bilinear_grad_dense(Z.double().numpy(), S.numpy(), kind, 7, [1.0], 1.7)
        assert np.allclose(gZ.numpy(), rZ, rtol=1e-4, atol=1e-5) and abs(float(gs) - rc[0]) < 1e-4 * max(1.0, abs(rc[0]))


@pytest.mark.parametrize("regime", ["chol", "cg"])
def test_full_kernel_cg_regime_and_predictions_match_dense(radial_backend, regime):
    """The CG / SLQ / pivoted-Cholesky route (no Cholesky of K) runs on the operator, and the eval-mode mean and covariance agree
    with the dense float64 solve at test_family_predictions_match_dense's tolerances — in both regimes."""
    from rpgp_amd import settings
    from rpgp_amd.models import ExactMarginalLogLikelihood
    from rpgp_amd.operators import FullKernelOperator
    X, y = _problem(60, 4, seed=4)
    Xs = torch.randn(9, 4, generator=torch.Generator().manual_seed(8)) + 2.0
    model, lik = _model(X, y, True, "InverseMQ")
    size = settings.max_cholesky_size(800 if regime == "chol" else 10)
    with settings.fused_full(True), size, settings.min_preconditioning_size(10), settings.cg_tolerance(1e-6), \
            settings.eval_cg_tolerance(1e-7), settings.max_cg_iterations(500), settings.num_trace_samples(40):
        model.train()
        mll = ExactMarginalLogLikelihood(lik, model)
        out = model(model.train_inputs)
        assert type(out.covariance) is FullKernelOperator
        val = mll(out, model.train_targets)
        val.backward()
        assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.requires_grad)
        model.eval(); lik.eval()
        with torch.no_grad():
            post = model(Xs)
            mean, cov = post.mean.numpy(), post.covariance.numpy()
        assert not model.prediction_strategy.dense_path or regime == "chol"
    k = model.covar_module.base_kernel
    ls = k.lengthscale.detach().double().reshape(-1)
    Z, Zs = (X.double() / ls).numpy(), (Xs.double() / ls).numpy()
    s, noise, c = float(model.covar_module.outputscale), float(lik.noise), float(model.mean_module.constant)
    K = fmo.kernel_matrix(Z, Z, "InverseMQ", 4, [1.0], s) + noise * np.eye(60)
    Ks = fmo.kernel_matrix(Zs, Z, "InverseMQ", 4, [1.0], s)
    Kss = fmo.kernel_matrix(Zs, Zs, "InverseMQ", 4, [1.0], s)
    r = y.double().numpy() - c
    ref_mean = Ks @ np.linalg.solve(K, r) + c
    ref_cov = Kss - Ks @ np.linalg.solve(K, Ks.T)
    assert np.allclose(mean, ref_mean, rtol=1e-4, atol=1e-5)
    assert np.allclose(cov, ref_cov, rtol=1e-3, atol=1e-5)
    ref_mll = (-0.5 * r @ np.linalg.solve(K, r) - 0.5 * np.linalg.slogdet(K)[1] - 0.5 * 60 * np.log(2 * np.pi)
               + float(lik.log_prior().detach())) / 60
    assert abs(float(val) - ref_mll) < (1e-4 if regime == "chol" else 5e-2) * max(1.0, abs(ref_mll))


def test_not_served_keeps_the_dense_operator_and_says_why(radial_backend, oracle_backend):
    from rpgp_amd import backend, settings
    from rpgp_amd.dense_ops import DenseKernelOperator
    from rpgp_amd.operators import FullKernelOperator
    from tests.oracle_backend import OracleBackend
    X, y = _problem(30, 3, seed=5)
    assert settings.fused_full.off()                                            # off by default
    model, _ = _model(X, y, True, "RBF")
    k = model.covar_module.base_kernel
    assert type(model.covar_module(X)) is DenseKernelOperator and "off" in k.fused_full_reason
    with settings.fused_full(True):
        assert type(model.covar_module(X)) is FullKernelOperator and k.fused_full_reason is None
        # a float64 model (--double)
        m64, _ = _model(X, y, True, "RBF")
        m64 = m64.double()
        assert type(m64.covar_module(X.double())) is DenseKernelOperator
        assert "float64" in m64.covar_module.base_kernel.fused_full_reason
        # more columns than the kernels take
        wide = torch.randn(4, 1025)
        kw, _ = _model(wide, torch.randn(4), False, "RBF")
        assert type(kw.covar_module(wide)) is DenseKernelOperator and "1025" in kw.covar_module.base_kernel.fused_full_reason
        # a backend without the radial entries
        prev = backend.set_backend(OracleBackend())
        try:
            assert type(model.covar_module(X)) is DenseKernelOperator and "radial" in k.fused_full_reason
        finally:
            backend.set_backend(prev)
        # host tensors with the HIP backend
        hip = backend.HipBackend()
        prev = backend.set_backend(hip)
        try:
            assert type(model.covar_module(X)) is DenseKernelOperator and "host" in k.fused_full_reason
        finally:
            backend.set_backend(prev)
    assert type(model.covar_module(X)) is DenseKernelOperator


def test_centre_is_the_training_mean_once_per_model(radial_backend):
    """mu is the column mean of the training inputs, detached, fixed at the model's first call: the same mu shifts the test inputs
    of a cross-covariance (translation invariance keeps K what it is)."""
    from rpgp_amd import settings
    X, y = _problem(30, 3, seed=6)
    Xs = torch.randn(5, 3, generator=torch.Generator().manual_seed(2)) - 4.0
    model, _ = _model(X, y, False, "Matern")
    with settings.fused_full(True):
        op = model.covar_module(X)
        mu = model.covar_module.base_kernel._center
        assert torch.allclose(mu, X.mean(0)) and not mu.requires_grad
        cross = model.covar_module(Xs, X)
        assert model.covar_module.base_kernel._center is mu
        ls = float(model.covar_module.base_kernel.lengthscale)
        assert torch.allclose(cross.Z1, (Xs - mu) / ls) and torch.allclose(cross.Z2, op.Z1)
        ref = fmo.kernel_matrix((Xs / ls).numpy(), (X / ls).numpy(), "Matern", 3, [1.0], float(model.covar_module.outputscale))
        assert np.allclose(cross.to_dense().numpy(), ref, atol=1e-5)


def test_runner_accepts_fused_full():
    from rpgp_amd import runner
    p = runner.build_parser()
    base = ["-m", "ARD_model_spec", "-d", "pol", "-o", "out.csv"]
    assert p.parse_args(base + ["--fused_full"]).fused_full is True
    assert p.parse_args(base).fused_full is False
