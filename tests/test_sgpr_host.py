"""Host side of `kind: sgpr` (no GPU): the model is served, the dense path equals the dense N x N float64 reference, the bound is a
bound, the native host logic on a CPU double of the two backend entries equals the dense path in value and in every gradient,
the prediction equals the N x N form, the runner serves the spec — and the emulation of the kernel path (tests/sgpr_reference.py)
stays within every gate the GPU tests apply while every defect of its mutation table misses one."""
import json
import types

import numpy as np
import pytest
import torch

from tests import radial_reference as rr
from tests import sgpr_reference as sr
from tests.oracle_backend import _np

S, NOISE, C = 1.3, 0.2, 0.1


def _inducing_entries(ob):
    """Extend the CPU test double with the two inducing-point entries, through the float64 statements of sgpr_reference."""
    def inducing_gram(self, kind, Z, U, Y=None, rows=None):
        y = np.zeros((Z.shape[0], 0)) if Y is None else _np(Y).reshape(Z.shape[0], -1)
        G, g = sr.sums(_np(Z), _np(U), y, kind)
        self.calls["inducing_gram"] = self.calls.get("inducing_gram", 0) + 1
        return torch.from_numpy(G), torch.from_numpy(g)

    def inducing_grad(self, kind, Z, U, Y, C, v, rows=None):
        y = np.zeros((Z.shape[0], 0)) if Y is None else _np(Y).reshape(Z.shape[0], -1)
        assert C.dtype == torch.float64 and torch.equal(C, C.t()) and (v is None or v.dtype == torch.float64)
        gU, q = sr.sums_grad(_np(Z), _np(U), y, _np(C), np.zeros((U.shape[0], 0)) if v is None else _np(v), kind)
        self.calls["inducing_grad"] = self.calls.get("inducing_grad", 0) + 1
        return torch.from_numpy(gU), torch.from_numpy(q)

    for f in (inducing_gram, inducing_grad):
        setattr(ob, f.__name__, types.MethodType(f, ob))
    ob.inducing_max_points = 1024
    ob.radial_max_dims = 1024
    return ob


@pytest.fixture
def inducing_backend(oracle_backend):
    return _inducing_entries(oracle_backend)


def _model(X, y, M, kernel_type="RBF", ard=True, ls=2.5, dtype=torch.float32):
    from rpgp_amd.training import create_exact_gp
    torch.manual_seed(0)
    model, lik = create_exact_gp(X, y, "sgpr", noise_prior=True, ard=ard, kernel_type=kernel_type, inducing_points=M)
    model.covar_module.base_kernel.base_kernel.lengthscale = ls
    model.covar_module.outputscale = S
    lik.noise = NOISE
    model.mean_module.constant.data.fill_(C)
    return model.to(dtype), lik


def _bound_and_grads(model, lik, native):
    """(bound, {name: gradient}) of the model's objective without priors and without the division by N."""
    from rpgp_amd import settings
    model.train()
    for p in model.parameters():
        p.grad = None
    with settings.sgpr_native(native):
        out = model(model.train_inputs)
        val = out.covariance.log_prob(lik.noise.reshape(()), model.train_targets, out.mean)
        val.backward()
    return out.covariance, float(val.detach()), {n: p.grad.detach().double().clone() for n, p in model.named_parameters()}


def _reference(model, lik, kind, X, y):
    """Value and gradients of the dense N x N form with respect to the model's RAW parameters (chain rule on the float64 side)."""
    k = model.covar_module.base_kernel
    raw = {n: p.detach().double().clone().requires_grad_(True) for n, p in model.named_parameters()}
    ls = torch.nn.functional.softplus(raw["covar_module.base_kernel.base_kernel.raw_lengthscale"]).reshape(-1)
    s = torch.nn.functional.softplus(raw["covar_module.raw_outputscale"])
    noise = torch.nn.functional.softplus(raw["likelihood.raw_noise"]).reshape(()) + 1e-4
    mu = X.double().mean(0) if getattr(k, "_center", None) is None else k._center.double()
    val = sr.dense_objective(kind, X.double(), y.double(), raw["covar_module.base_kernel.inducing_points"], mu, ls, s, noise,
                             raw["mean_module.constant"].reshape(()))
    val.backward()
    return float(val.detach()), {n: p.grad for n, p in raw.items()}


def test_sgpr_kind_is_served_and_says_which_path():
    """create_exact_gp(..., "sgpr") builds ScaleKernel(InducingPointKernel(base, X[:M], likelihood)) (it raised
    NotImplementedError before); on the host with the HIP backend the dense path serves and says why."""
    from rpgp_amd import backend, training
    from rpgp_amd.kernels import InducingPointKernel, RBFKernel, ScaleKernel
    from rpgp_amd.sgpr import InducingPointOperator
    X, y, _, _ = sr.problem(60, 3, 10, 2.5)
    model, lik = _model(X, y, 10, ard=False)
    assert "sgpr" in training.EXACT_GP_KINDS and "sgpr" not in training.REFERENCE_ONLY_KINDS
    sk = model.covar_module
    assert type(sk) is ScaleKernel and type(sk.base_kernel) is InducingPointKernel and type(sk.base_kernel.base_kernel) is RBFKernel
    ip = sk.base_kernel
    assert ip.likelihood is lik and torch.equal(ip.inducing_points.detach(), X[:10]) and ip.inducing_points.requires_grad
    assert sum(p.numel() for p in model.parameters()) == 10 * 3 + 1 + 1 + 1 + 1      # U, lengthscale, outputscale, noise, mean
    prev = backend.set_backend(backend.HipBackend())
    try:
        op = model(X).covariance
        assert type(op) is InducingPointOperator and not op.native and "host" in ip.sgpr_reason
    finally:
        backend.set_backend(prev)
    for kind in ("rp", "deep_rp_poly", "multi_full", "duvenaud_additive"):
        with pytest.raises(NotImplementedError):
            training.create_exact_gp(X, y, kind, noise_prior=True)


def test_value_errors_of_the_reference():
    from rpgp_amd.likelihoods import GaussianLikelihood
    from rpgp_amd.training import create_sgpr_kernel
    X = torch.randn(20, 3)
    with pytest.raises(ValueError, match="Unknown kernel type"):
        create_sgpr_kernel(3, kernel_type="Cosine", X=X, likelihood=GaussianLikelihood())
    with pytest.raises(ValueError, match="X is required"):
        create_sgpr_kernel(3, likelihood=GaussianLikelihood())
    with pytest.raises(ValueError, match="Likelihood is required"):
        create_sgpr_kernel(3, X=X)


@pytest.mark.parametrize("kernel_type,ard", [("RBF", True), ("Matern", False), ("InverseMQ", True)])
def test_dense_path_matches_the_dense_reference_in_float64(kernel_type, ard):
    """The dense torch path (--double, CPU) against the N x N form at N = 300: value and every gradient to 1e-9."""
    X, y, _, _ = sr.problem(300, 5, 40, 2.5, seed=1)
    model, lik = _model(X.double(), y.double(), 40, kernel_type, ard, dtype=torch.float64)
    op, val, grads = _bound_and_grads(model, lik, native=True)
    assert not op.native and "float64" in model.covar_module.base_kernel.sgpr_reason
    ref, rgrads = _reference(model, lik, kernel_type, X, y)
    assert abs(val - ref) <= 1e-9 * abs(ref)
    assert set(grads) == set(rgrads) and len(grads) == 5
    for n in grads:
        assert rr.rel(grads[n].numpy(), rgrads[n].numpy()) <= 1e-9, n


def test_bound_is_below_the_marginal_likelihood_and_tight_at_u_equal_x():
    X, y, _, ls = sr.problem(120, 4, 30, 2.5, seed=2)
    X64, y64, mu = X.double(), y.double(), X.double().mean(0)
    s, noise, c = (torch.tensor(v, dtype=torch.float64) for v in (S, NOISE, C))
    exact = float(sr.exact_marginal("RBF", X64, y64, mu, ls.double(), s, noise, c))
    for M in (5, 30, 90):
        model, lik = _model(X64, y64, M, dtype=torch.float64)
        _, val, _ = _bound_and_grads(model, lik, native=False)
        assert val <= exact + 1e-9 * abs(exact), (M, val, exact)
    # U = X: Q = K_ff up to the jitter (a relative perturbation of K_uu of 1e-6)
    model, lik = _model(X64, y64, 120, dtype=torch.float64)
    _, val, _ = _bound_and_grads(model, lik, native=False)
    assert val <= exact + 1e-9 * abs(exact) and abs(val - exact) <= 1e-3 * abs(exact), (val, exact)


@pytest.mark.parametrize("kernel_type,ard", [("RBF", True), ("Matern", True), ("InverseMQ", False)])
def test_native_host_logic_on_the_double_equals_the_dense_path(inducing_backend, kernel_type, ard):
    """One Gram call forward, one grad call backward, and the same value and gradients as the dense path (float32 model: the
    double computes the sums in float64 on the float32 coordinates, so the two differ by the rounding of Z and U alone)."""
    X, y, _, _ = sr.problem(150, 4, 20, 2.5, seed=3)
    model, lik = _model(X, y, 20, kernel_type, ard)
    op, val, grads = _bound_and_grads(model, lik, native=True)
    assert op.native and model.covar_module.base_kernel.sgpr_reason is None
    assert inducing_backend.calls["inducing_gram"] == 1 and inducing_backend.calls["inducing_grad"] == 1
    opd, vald, gradsd = _bound_and_grads(model, lik, native=False)
    assert not opd.native and "off" in model.covar_module.base_kernel.sgpr_reason
    assert inducing_backend.calls["inducing_gram"] == 1
    assert abs(val - vald) <= 2e-6 * abs(vald)
    assert set(grads) == set(gradsd) and len(grads) == 5
    for n in grads:
        assert rr.rel(grads[n].numpy(), gradsd[n].numpy()) <= 2e-4, (n, grads[n], gradsd[n])


def test_prediction_matches_the_n_by_n_form(inducing_backend):
    from rpgp_amd import settings
    from rpgp_amd.models import ExactMarginalLogLikelihood
    X, y, _, ls = sr.problem(140, 3, 25, 2.5, seed=4)
    Xs = torch.randn(17, 3, generator=torch.Generator().manual_seed(9))
    ys = torch.sin(Xs).sum(1)
    for native in (True, False):
        model, lik = _model(X, y, 25)
        model.eval(); lik.eval()
        with settings.sgpr_native(native), torch.no_grad():
            post = model(Xs)
            mean, var, cov = post.mean.double(), post.variance.double(), post.covariance.double()
            nll = -ExactMarginalLogLikelihood(lik, model)(post, ys)
            with settings.skip_posterior_variances(True):
                assert torch.allclose(model(Xs).mean, post.mean)
        k = model.covar_module.base_kernel
        rmean, rcov = sr.dense_prediction("RBF", X.double(), y.double(), Xs.double(), k.inducing_points.detach().double(),
                                          k._center.double(), k.base_kernel.lengthscale.detach().double().reshape(-1),
                                          float(model.covar_module.outputscale), float(lik.noise),
                                          float(model.mean_module.constant))
        assert rr.rel(mean.numpy(), rmean.numpy()) <= 1e-4 and rr.rel(cov.numpy(), rcov.numpy()) <= 1e-4
        assert rr.rel(var.numpy(), rcov.diagonal().numpy()) <= 1e-4 and torch.isfinite(nll)
        noisy = lik(post)
        assert torch.allclose(noisy.variance.double(), var + float(lik.noise), rtol=1e-5)


def test_more_inducing_points_than_rows_gives_n_points(inducing_backend):
    X, y, _, _ = sr.problem(30, 3, 10, 2.5, seed=5)
    model, lik = _model(X, y, 400)
    assert model.covar_module.base_kernel.inducing_points.shape == (30, 3)
    _, val, grads = _bound_and_grads(model, lik, native=True)
    assert np.isfinite(val) and all(torch.isfinite(g).all() for g in grads.values())


def test_more_than_one_rank_raises(monkeypatch):
    X, y, _, _ = sr.problem(30, 3, 10, 2.5, seed=5)
    model, _ = _model(X, y, 10)
    monkeypatch.setattr("rpgp_amd.distributed.is_distributed", lambda: True)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        model.covar_module(X)


def test_runner_end_to_end(tmp_path, monkeypatch, inducing_backend):
    """SGPR_ARD_model_spec through the CLI on a 277 x 6 synthetic set: every metric of train_exact_gp is there and finite."""
    from rpgp_amd import runner, specs
    monkeypatch.setitem(runner.SYNTHETIC_SHAPES, "sgpr277", (277, 6))
    spec = specs.get("SGPR_ARD_model_spec")
    assert spec["kind"] == "sgpr" and spec["model_kwargs"]["inducing_points"] == 400 and spec["model_kwargs"]["ard"] is True
    spec["model_kwargs"]["inducing_points"] = 40
    spec["train_kwargs"].update(max_iter=6, init_iters=1)
    sp = tmp_path / "spec.json"
    json.dump(spec, open(sp, "w"))
    df = runner.main(["-m", str(sp), "-d", "synthetic:sgpr277", "-o", str(tmp_path / "res.csv"), "--no_cv",
                      "--skip_random_restart"])
    row = df.iloc[0]
    assert "error" not in df.columns and row["n"] == 277 and row["d"] == 6
    for col in ("rmse", "prior_train_nmll", "train_mse", "train_nll", "test_nll", "test_pred_frac_in_cr"):
        assert np.isfinite(row[col]), col
    assert inducing_backend.calls["inducing_gram"] >= 6 and inducing_backend.calls["inducing_grad"] >= 6


# ---- the emulation of the kernel path: within every gate, and every defect outside one ------------------------------------
def _kernel_gates(emu, case):
    """The checks tests/test_inducing_kernels_gpu.py applies, on the emulation; returns the first gate missed or None."""
    kind, d, N, M, T = case
    Z, U, Y, Cm, v = sr.kernel_inputs(*case)
    try:
        G, g = emu.gram(Z, U, Y)
        sr.check_sums(G, g, Z, U, Y, kind)                    # (every entry of G: a triangle left unwritten misses it)
        sr.check_grad(*emu.grad(Z, U, Y, Cm, v), *sr.sums_grad(Z, U, Y, Cm, v, kind))
    except AssertionError as e:
        return str(e)
    return None


_HOST_KERNEL_CASES = [c for c in sr.kernel_cases() if c[1] * c[2] * c[3] <= 3e7]


@pytest.mark.parametrize("case", _HOST_KERNEL_CASES, ids=lambda c: "%s-d%d-N%d-M%d-T%d" % c)
def test_emulation_stays_within_the_kernel_gates(case):
    """Before the GPU test relies on the derived bounds of G and g and on GATE_GRAD_REL for the derivative: the float32 emulation
    stays within them at these inputs (near-duplicate rows against the inducing points included)."""
    assert _kernel_gates(sr.Emulation(case[0]), case) is None


def _objective_gates(kind, case, defect):
    """The gates tests/test_sgpr_gpu.py applies to a case, on the emulation: bound to 1e-4, every gradient to 4 x the recorded
    error of the clean emulation.  Returns (list of gates missed, the emulation's own relative errors)."""
    N, d, M, ls = case
    X, y, U, l = sr.problem(N, d, M, ls)
    args = (X.numpy(), y.numpy(), U.numpy(), X.mean(0).numpy(), l.numpy(), S, NOISE, C)
    ref, rgrads = sr.reference_objective(kind, *args)
    try:
        val, grads = sr.Emulation(kind, defect).objective(*args)
    except torch.linalg.LinAlgError:
        return ["A is not positive definite"], {}
    errs = {n: rr.rel(np.atleast_1d(grads[n]), np.atleast_1d(rgrads[n])) for n in rgrads}
    missed = ["bound"] if not abs(val - ref) <= sr.GATE_BOUND_REL * abs(ref) else []
    missed += [n for n, e in errs.items() if not e <= 4.0 * sr.GPU_CASES[case][n]]
    return missed, errs


@pytest.mark.parametrize("case", sorted(sr.GPU_CASES))
def test_clean_emulation_passes_the_objective_gates_and_reproduces_the_recorded_errors(case):
    """cond(K_uu) < 1e4 as the GPU test asserts; the clean emulation is inside every gate; its errors are the figures recorded
    next to the case in sgpr_reference.GPU_CASES (not above them, and not less than half of them: the record stays honest)."""
    N, d, M, ls = case
    X, _, U, l = sr.problem(N, d, M, ls)
    assert sr.cond_kuu("RBF", U.double(), X.double().mean(0), l.double()) < 1e4
    missed, errs = _objective_gates("RBF", case, None)
    assert missed == [], (missed, errs)
    for n, e in errs.items():
        assert 0.5 * sr.GPU_CASES[case][n] <= e <= sr.GPU_CASES[case][n], (n, e, sr.GPU_CASES[case][n])


@pytest.mark.parametrize("defect", sr.Emulation.DEFECTS)
def test_every_defect_misses_a_gate(defect):
    case = sorted(sr.GPU_CASES)[0]
    missed, errs = _objective_gates("RBF", case, defect)
    kernel_case = ("RBF", 5, 1237, 301, 2)
    kernel_missed = _kernel_gates(sr.Emulation("RBF", defect, slab=256), kernel_case)
    assert missed or kernel_missed, (defect, errs)
