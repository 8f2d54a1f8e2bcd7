"""`kind: sgpr` on the device: the native path (one rpgp_inducing_gram forward, one rpgp_inducing_grad backward, float64 M x M
algebra) against the dense N x N float64 reference of tests/sgpr_reference.py at the two cases recorded there, a short Adam run
against the dense path in float64 on the device, and one evaluation at N = 200 000 without an N x M object."""
import gc

import numpy as np
import pytest
import torch

from tests import radial_reference as rr
from tests import sgpr_reference as sr

pytestmark = pytest.mark.gpu

S, NOISE, C = 1.3, 0.2, 0.1


def _model(X, y, M, ls, device, dtype=torch.float32):
    from rpgp_amd.training import create_exact_gp
    torch.manual_seed(0)
    model, lik = create_exact_gp(X, y, "sgpr", noise_prior=True, ard=True, kernel_type="RBF", inducing_points=M)
    model.covar_module.base_kernel.base_kernel.lengthscale = ls
    model.covar_module.outputscale = S
    lik.noise = NOISE
    model.mean_module.constant.data.fill_(C)
    model = model.to(device, dtype)
    model.train_inputs, model.train_targets = X.to(device, dtype), y.to(device, dtype)
    return model, lik


_NAMES = {"U": "covar_module.base_kernel.inducing_points", "ls": "covar_module.base_kernel.base_kernel.raw_lengthscale",
          "s": "covar_module.raw_outputscale", "noise": "likelihood.raw_noise", "c": "mean_module.constant"}


@pytest.mark.parametrize("case", sorted(sr.GPU_CASES))
def test_native_bound_gradients_and_prediction_match_float64(gpu_device, case):
    """Bound, predictive mean and variance to 1e-4 relative; every gradient to 4 x the error of the host emulation recorded in
    sgpr_reference.GPU_CASES (the margin covers summation order and the hardware transcendentals).  cond(K_uu) < 1e4 is a
    condition of the test."""
    N, d, M, ls = case
    X, y, U, l = sr.problem(N, d, M, ls)
    mu = X.mean(0)
    assert sr.cond_kuu("RBF", U.double(), mu.double(), l.double()) < 1e4
    model, lik = _model(X, y, M, ls, gpu_device)
    k = model.covar_module.base_kernel
    model.train()
    out = model(model.train_inputs)
    assert out.covariance.native and k.sgpr_reason is None
    val = out.covariance.log_prob(lik.noise.reshape(()), model.train_targets, out.mean)
    val.backward()
    # the reference at the parameters exactly as the model holds them (float32 values, widened), gradients with respect to
    # the natural parameters; the model's are with respect to the raw ones: softplus' = sigmoid, the same factor on both sides
    nat = dict(U_raw=k.inducing_points.detach().cpu().double().numpy(), mu=k._center.cpu().double().numpy(),
               ls=k.base_kernel.lengthscale.detach().cpu().double().reshape(-1).numpy(),
               s=float(model.covar_module.outputscale.detach()), noise=float(lik.noise.detach()),
               c=float(model.mean_module.constant.detach()))
    ref, rgrads = sr.reference_objective("RBF", X.numpy(), y.numpy(), **nat)
    chain = {"U": 1.0, "c": 1.0,
             "ls": torch.sigmoid(k.base_kernel.raw_lengthscale.detach().cpu().double()).reshape(-1).numpy(),
             "s": float(torch.sigmoid(model.covar_module.raw_outputscale.detach().double())),
             "noise": float(torch.sigmoid(lik.raw_noise.detach().double()))}
    params = dict(model.named_parameters())
    figures = {"bound": abs(float(val.detach()) - ref) / abs(ref)}
    for n, name in _NAMES.items():
        got = params[name].grad.detach().cpu().double().numpy().reshape(np.shape(rgrads[n]))
        figures[n] = rr.rel(np.atleast_1d(got), np.atleast_1d(rgrads[n] * chain[n]))
    # prediction
    Xs = torch.randn(200, d, generator=torch.Generator().manual_seed(11))
    model.eval(); lik.eval()
    with torch.no_grad():
        post = model(Xs.to(gpu_device))
        mean, var = post.mean.cpu().double().numpy(), post.variance.cpu().double().numpy()
    t = {a: torch.tensor(b, dtype=torch.float64) for a, b in nat.items()}
    rmean, rcov = sr.dense_prediction("RBF", X.double(), y.double(), Xs.double(), t["U_raw"], t["mu"], t["ls"], t["s"], t["noise"],
                                      t["c"])
    figures["mean"] = rr.rel(mean, rmean.numpy())
    figures["variance"] = rr.rel(var, rcov.diagonal().numpy())
    print("sgpr native N=%d d=%d M=%d ls=%g: %s" % (N, d, M, ls, {a: "%.2e" % b for a, b in figures.items()}))
    for n in ("bound", "mean", "variance"):
        assert figures[n] <= sr.GATE_BOUND_REL, (n, figures[n])
    for n in _NAMES:
        assert figures[n] <= 4.0 * sr.GPU_CASES[case][n], (n, figures[n], 4.0 * sr.GPU_CASES[case][n])


def test_six_adam_steps_lower_the_loss_and_match_the_dense_path_in_float64(gpu_device):
    from rpgp_amd import settings
    from rpgp_amd.models import ExactMarginalLogLikelihood
    from rpgp_amd.training import train_to_convergence
    N, d, M, ls = 1500, 8, 64, 2.5
    X, y, _, _ = sr.problem(N, d, M, ls)
    runs = {}
    for name, dtype, native in (("native", torch.float32, True), ("dense", torch.float64, False)):
        model, lik = _model(X, y, M, ls, gpu_device, dtype)
        losses = []
        with settings.sgpr_native(native):
            train_to_convergence(model, model.train_inputs, model.train_targets, optimizer=torch.optim.Adam, lr=0.05,
                                 objective=ExactMarginalLogLikelihood(lik, model), max_iter=6, check_conv=False,
                                 loss_log=losses)
            assert (model.covar_module.base_kernel.sgpr_reason is None) is native
        runs[name] = (losses, {n: p.detach().cpu().double() for n, p in model.named_parameters()})
    losses, params = runs["native"]
    print("sgpr adam: native %s dense %s" % (["%.6f" % v for v in losses], ["%.6f" % v for v in runs["dense"][0]]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert np.allclose(losses, runs["dense"][0], rtol=1e-4, atol=1e-6)
    for n, p in params.items():
        assert rr.rel(p.numpy(), runs["dense"][1][n].numpy()) <= 1e-3, n


def test_one_evaluation_at_a_size_without_an_n_by_m_object(gpu_device):
    """N = 200 000, M = 256, d = 8: one evaluation of the objective and its backward pass complete, and the allocator's peak rises
    by less than half of an N x M float32 block (0.5 * 4 N M bytes) over what was held before."""
    from rpgp_amd import ops
    from rpgp_amd.models import ExactMarginalLogLikelihood
    N, d, M = 200000, 8, 256
    X, y, _, _ = sr.problem(N, d, M, 2.5, seed=2)
    model, lik = _model(X, y, M, 2.5, gpu_device)
    mll = ExactMarginalLogLikelihood(lik, model)
    model.train()
    ops._workspaces.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(gpu_device)
    held = torch.cuda.memory_allocated(gpu_device)
    out = model(model.train_inputs)
    assert out.covariance.native
    val = mll(out, model.train_targets)
    val.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(gpu_device)
    print("sgpr N = %d M = %d: allocator peak %.1f MB over %.1f MB held (0.5 * 4 N M = %.1f MB)"
          % (N, M, (peak - held) / 1e6, held / 1e6, 0.5 * 4 * N * M / 1e6))
    assert torch.isfinite(val.detach()) and all(torch.isfinite(p.grad).all() for p in model.parameters())
    assert float(model.covar_module.base_kernel.inducing_points.grad.abs().max()) > 0.0
    assert peak - held < 0.5 * 4 * N * M, (peak, held)
