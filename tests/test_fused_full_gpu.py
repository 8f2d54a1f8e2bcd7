"""settings.fused_full on the GPU: the native mBCG executor on an RPGP_OP_RADIAL descriptor against a dense float64 solve,
training and prediction of `kind: full` models on operators.FullKernelOperator against the same model on the dense torch path,
and one marginal-likelihood evaluation with its backward pass at a size where no N x N object may exist."""
import numpy as np
import pytest
import torch

from oracle import family as fmo
from tests import radial_reference as rr

pytestmark = pytest.mark.gpu


def test_native_executor_on_the_radial_operator(gpu_device):
    """rpgp_mbcg_solve on RPGP_OP_RADIAL with a rank-15 pivoted-Cholesky preconditioner (N = 2000, d = 21, T = 11) against
    np.linalg.solve on the float64 matrix, at the gates of test_native_and_torch_loops_match_fp64_oracle_solve."""
    from rpgp_amd import _lib, linear_cg as lcg
    from rpgp_amd.operators import AddedDiagOperator, FullKernelOperator
    from rpgp_amd.precond import WoodburyPreconditioner, pivoted_cholesky
    N, d, T, noise, s, tol = 2000, 21, 11, 0.3, 0.9, 1e-4
    Z = rr.inputs(N, d, 11)
    for kind in ("RBF", "Matern"):
        op = FullKernelOperator(torch.from_numpy(Z).to(gpu_device), None, torch.tensor(s, device=gpu_device), kind)
        khat = AddedDiagOperator(op, torch.tensor(noise, device=gpu_device))
        desc, _keep = khat.native_descriptor()
        assert desc.kind == _lib.RPGP_OP_RADIAL and desc.J == d and desc.N == N
        rhs = torch.randn(N, T, generator=torch.Generator().manual_seed(1)).to(gpu_device)
        pre = WoodburyPreconditioner(pivoted_cholesky(op._diagonal(), op._get_rows, 15), noise)
        before = lcg.stats.get("native_calls", 0)
        x = lcg.linear_cg(khat._matmul, rhs, operator=khat, tolerance=tol, max_iter=500, preconditioner=pre)
        assert lcg.stats.get("native_calls", 0) == before + 1, "native executor was not used"
        Kh = rr.kernel(Z, Z, kind, s) + noise * np.eye(N)
        b = rhs.double().cpu().numpy()
        xd, x_ref = x.double().cpu().numpy(), np.linalg.solve(Kh, b)
        res = np.linalg.norm(Kh @ xd - b, axis=0) / np.linalg.norm(b, axis=0)
        assert res.mean() < 2.0 * tol, (kind, res)
        assert np.linalg.norm(xd - x_ref) / np.linalg.norm(x_ref) < 100.0 * tol
        x2 = lcg.linear_cg(khat._matmul, rhs, operator=khat, tolerance=tol, max_iter=500, preconditioner=pre)
        assert torch.equal(x, x2)                                               # the product is bit-reproducible, so is the solve


def test_rbf_up_to_20_columns_is_routed_to_the_family_tile_kernel(gpu_device):
    """The measured crossover: the RBF with d <= 20 runs as one component of group d of the family tile kernels
    (zero-padded to the next instantiated group size), everything else on the radial kernels; both compute the same operator."""
    from rpgp_amd import _lib, ops
    from rpgp_amd.operators import AddedDiagOperator, FullKernelOperator
    N, T, s, noise = 1237, 11, 0.7, 0.13
    rng = np.random.default_rng(2)
    V = rng.standard_normal((N, T)).astype(np.float32)
    L, R = rng.standard_normal((N, T)).astype(np.float32), rng.standard_normal((N, T)).astype(np.float32)
    Vt, Lt, Rt = (torch.from_numpy(a).to(gpu_device) for a in (V, L, R))
    for kind, d, routed in (("RBF", 7, True), ("RBF", 20, True), ("RBF", 21, False), ("Matern", 7, False)):
        Z = rr.inputs(N, d, d)
        Zt = torch.from_numpy(Z).to(gpu_device)
        op = FullKernelOperator(Zt, None, torch.tensor(s, device=gpu_device), kind)
        assert (op._family_route() is not None) is routed
        desc, _keep = AddedDiagOperator(op, torch.tensor(noise, device=gpu_device)).native_descriptor()
        assert desc.kind == (_lib.RPGP_OP_FAMILY if routed else _lib.RPGP_OP_RADIAL)
        rr.check_product(op._matmul(Vt, noise=noise).cpu().numpy(), Z, None, V, kind, s, noise)
        rows = op._get_rows(torch.tensor([0, 5, N - 1], device=gpu_device)).cpu().numpy()
        rr.check_dense(rows, Z[[0, 5, N - 1]], Z, kind, s)
        assert all(rows[k, i] == np.float32(s) for k, i in enumerate((0, 5, N - 1)))       # the value _diagonal() claims, exactly
        gZ, gs = op._bilinear_derivative(Lt, Rt)
        assert gZ.shape == (N, d)
        rr.check_grad(gZ.cpu().numpy(), float(gs), *rr.grad_factors(Z, L, R, kind, s))
        if routed:
            direct = ops.radial_mvm(kind, Zt, None, Vt, s, noise)
            assert float((direct - op._matmul(Vt, noise=noise)).norm() / direct.norm()) < 2 * rr.GATE_PRODUCT_REL


def _problem(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n + 60, d, generator=g)
    y = torch.sin(X).sum(1) + 0.3 * X[:, 0] * X[:, 1] + 0.1 * torch.randn(n + 60, generator=g)
    y = (y - y.mean()) / y.std()
    return X[:n], y[:n], X[n:], y[n:]


@pytest.mark.parametrize("kernel_type,ard", [("RBF", True), ("InverseMQ", True)])
def test_full_model_trains_and_predicts_like_the_dense_path(gpu_device, kernel_type, ard):
    """train_exact_gp of kind "full" under settings.fused_full in the CG / SLQ regime (N = 1500, d = 8), then at the trained
    hyper-parameters: loss (5e-3 relative: the SLQ log-determinant carries probe noise), the deterministic mean gradient (1e-3),
    the direction of the whole gradient, and the predictive mean and variance (1e-4) against the flag-off dense path — the
    tolerances tests/test_gp_gpu.py holds CG to against Cholesky."""
    from rpgp_amd import linear_cg as lcg, settings
    from rpgp_amd.dense_ops import DenseKernelOperator
    from rpgp_amd.models import ExactMarginalLogLikelihood
    from rpgp_amd.operators import FullKernelOperator
    from rpgp_amd.training import train_exact_gp
    X, y, Xs, ys = _problem(1500, 8, 0)
    mk = dict(noise_prior=True, kernel_type=kernel_type, ard=ard, init_lengthscale_range=(2.5, 3.0))
    tk = {"verbose": False, "optimizer": "adam", "max_iter": 6, "lr": 0.1, "patience": 20, "smooth": True}
    torch.manual_seed(0)
    n_native = lcg.stats.get("native_calls", 0)
    with settings.fused_full(True), settings.max_cholesky_size(100):
        metrics, mean, model = train_exact_gp(X, y, Xs, ys, "full", mk, tk, devices=(str(gpu_device),), skip_random_restart=True)
    assert lcg.stats.get("native_calls", 0) > n_native                         # the training solves ran in the native executor
    assert np.isfinite(metrics["prior_train_nmll"]) and np.isfinite(metrics["test_nll"]) and torch.isfinite(mean).all()
    lik = model.likelihood
    mll = ExactMarginalLogLikelihood(lik, model)
    Xst = Xs.to(gpu_device)
    got = {}
    for on in (True, False):
        model.train(); lik.train()
        model.zero_grad(set_to_none=True)
        ctx = settings.max_cholesky_size(100) if on else settings.max_cholesky_size(4000)
        with settings.fused_full(on), ctx, settings.cg_tolerance(1e-6), settings.num_trace_samples(40), \
                settings.max_lanczos_quadrature_iterations(50), settings.deterministic_probes(True), \
                settings.eval_cg_tolerance(1e-7), settings.max_cg_iterations(2000):
            out = model(model.train_inputs)
            assert type(out.covariance) is (FullKernelOperator if on else DenseKernelOperator)
            val = mll(out, model.train_targets)
            val.backward()
            grads = {n: p.grad.detach().double().cpu().reshape(-1) for n, p in model.named_parameters() if p.requires_grad}
            model.eval(); lik.eval()
            with torch.no_grad():
                post = model(Xst)
                got[on] = (float(val.detach()), grads, post.mean.double().cpu().numpy(), post.variance.double().cpu().numpy())
            assert model.prediction_strategy.dense_path is (not on)
    (v1, g1, m1, s1), (v0, g0, m0, s0) = got[True], got[False]
    print("fused_full %s: loss %.6f vs %.6f, mean rel %.2e, var rel %.2e" %
          (kernel_type, v1, v0, np.linalg.norm(m1 - m0) / np.linalg.norm(m0), np.linalg.norm(s1 - s0) / np.linalg.norm(s0)))
    assert abs(v1 - v0) < 5e-3 * abs(v0)
    gm1, gm0 = float(g1["mean_module.constant"]), float(g0["mean_module.constant"])
    assert abs(gm1 - gm0) < 1e-3 * abs(gm0) + 1e-6
    a, b = torch.cat([g1[n] for n in sorted(g1)]), torch.cat([g0[n] for n in sorted(g0)])
    assert sorted(g1) == sorted(g0) and float(a @ b / (a.norm() * b.norm())) > 0.95
    assert np.linalg.norm(m1 - m0) / np.linalg.norm(m0) < 1e-4
    assert np.linalg.norm(s1 - s0) / np.linalg.norm(s0) < 1e-4


@pytest.mark.parametrize("kernel_type,d,routed", [("RBF", 20, True), ("InverseMQ", 21, False)])
def test_full_model_at_a_size_without_an_n_by_n_object(gpu_device, kernel_type, d, routed):
    """N = 30 000 under settings.fused_full, on the family tile route (ARD RBF, d = 20) and on the radial kernels (ARD InverseMQ,
    d = 21): one marginal-likelihood evaluation and its backward pass complete, and torch.cuda.max_memory_allocated stays below
    4 N^2 bytes — no N x N float32 object was ever built.  The grow-only kernel workspaces of earlier, larger tests are dropped
    first (with them the figure was 6.0 GB in a whole-suite run); what the process still holds then counts against the bound."""
    import gc
    from rpgp_amd import ops, settings
    from rpgp_amd.models import ExactMarginalLogLikelihood
    from rpgp_amd.operators import FullKernelOperator
    from rpgp_amd.training import create_exact_gp
    N = 30000
    g = torch.Generator().manual_seed(3)
    X = torch.randn(N, d, generator=g)
    y = torch.sin(X[:, :4]).sum(1) + 0.1 * torch.randn(N, generator=g)
    y = (y - y.mean()) / y.std()
    torch.manual_seed(0)
    model, lik = create_exact_gp(X, y, "full", noise_prior=True, ard=True, kernel_type=kernel_type,
                                 init_lengthscale_range=(4.0, 5.0))
    model, lik = model.to(gpu_device), lik.to(gpu_device)
    model.train_inputs, model.train_targets = X.to(gpu_device), y.to(gpu_device)
    mll = ExactMarginalLogLikelihood(lik, model)
    model.train()
    ops._workspaces.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(gpu_device)
    held = torch.cuda.memory_allocated(gpu_device)
    with settings.fused_full(True):
        out = model(model.train_inputs)
        assert type(out.covariance) is FullKernelOperator and (out.covariance._family_route() is not None) is routed
        val = mll(out, model.train_targets)
        val.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(gpu_device)
    print("fused_full %s d = %d N = %d: allocator peak %.3f GB, %.3f GB of it held before the evaluation (4 N^2 = %.3f GB)"
          % (kernel_type, d, N, peak / 1e9, held / 1e9, 4 * N * N / 1e9))
    assert torch.isfinite(val.detach()) and all(torch.isfinite(p.grad).all() for p in model.parameters() if p.requires_grad)
    assert float(model.covar_module.base_kernel.raw_lengthscale.grad.abs().max()) > 0.0
    assert peak < 4 * N * N, peak
