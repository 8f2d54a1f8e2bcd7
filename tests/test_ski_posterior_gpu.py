"""The closed-form posterior of the grid-interpolation models end to end on the device (settings.ski_posterior) against the dense
float64 posterior of the same one-grid kernel (tests/ski_posterior_reference.py: oracle.ski.dense_kernel, Cholesky of
K + sigma^2 I).  The reference takes the coordinates the device projected — float32 values widened — and the posterior's own grid
block, so no float32 error and no grid difference enters: what is compared is the float64 algebra and the two row kernels.

Tolerance 1e-8 (ski_posterior_reference.TOL): the mean relative to max(1, max |mean|), variances and covariance entries relative to
s sum_j w_j, the test and train log-density relative to max(1, |value|).  The numpy restatement of the same formulas is within
7.1e-11 of the dense posterior on every one of these quantities in all six cases (worst: the train log-density of the second case),
which leaves more than 100 x for the device's summation order."""
import numpy as np
import pytest
import torch

from tests import ski_posterior_reference as R

pytestmark = pytest.mark.gpu


def _model(k, dev):
    """The model of case k on the device: unit lengthscales and an identity projection, so the coordinates are the inputs."""
    from rpgp_amd.kernels import (AdditiveStructureRBFKernel, GeneralizedProjectionKernel, ScaledProjectionKernel, ScaleKernel,
                                  inv_softplus)
    from rpgp_amd.likelihoods import GaussianLikelihood, SmoothedBoxPrior
    from rpgp_amd.models import ExactGPModel
    N, M, J, G, kind, rule, weights, s, noise = R.CASES[k]
    Z, y, Zs, ys = R.case_data(k)[:4]
    X, Xs = torch.from_numpy(Z).float().to(dev), torch.from_numpy(Zs).float().to(dev)
    lin = torch.nn.Linear(J, J, bias=False)
    lin.weight.data = torch.eye(J)
    opts = {"grid_size": G, "num_dims": 1}
    if rule == "shared":
        base = ScaledProjectionKernel(lin, AdditiveStructureRBFKernel(J, weight=1.0, ski=True, ski_options=opts, kernel_type=kind),
                                      prescale=True, ard_num_dims=J)
        base.initialize(lengthscale=torch.ones(J))
    else:
        base = GeneralizedProjectionKernel([1] * J, J, kind, lin, weighted=True, ski=True, ski_options=opts)
        base.raw_lengthscales.data = inv_softplus(torch.ones(1, J)).float()
        base.raw_outputscales.data = inv_softplus(torch.tensor(weights)).float()
        assert base.grid_rule == "reference"
    sk = ScaleKernel(base)
    sk.outputscale = s
    lik = GaussianLikelihood(noise_prior=SmoothedBoxPrior(1e-4, 10, sigma=0.01))
    lik.noise = noise
    model = ExactGPModel(X, torch.from_numpy(y).float().to(dev), lik, sk).to(dev)
    model.mean_module.constant.data.fill_(0.2)
    return model, lik, Xs, torch.from_numpy(ys).to(dev)


@pytest.mark.parametrize("k", range(len(R.CASES)))
def test_posterior_against_the_dense_float64_posterior(gpu_device, k):
    from rpgp_amd import settings
    from rpgp_amd.ski_posterior import SKIPredictive
    N, M, J, G, kind, rule, weights, s, noise = R.CASES[k]
    model, lik, Xs, ys = _model(k, gpu_device)
    model.eval()
    with settings.ski_posterior(True), torch.no_grad():
        out = model(Xs)
        st = model.prediction_strategy
        post = st.ski_post
        assert post is not None, st.ski_posterior_reason
        assert isinstance(out, SKIPredictive) and not out.covariance_materialized
        assert post.rebuilds <= 1
        y64 = model.train_targets.double()
        ref = R.dense(post.Z.cpu().numpy(), y64.cpu().numpy(), post._test_coordinates(Xs).cpu().numpy(), ys.cpu().numpy(),
                      out._state.gp.cpu().numpy(), G, post.scale, post.noise, post.c)
        w_sum = float(J) if weights is None else float(model.covar_module.base_kernel.outputscales.double().sum())
        assert abs(ref["prior_diag_scale"] - post.scale * w_sum) <= 1e-12 * ref["prior_diag_scale"]
        lp = float(lik(out).log_prob(ys))
        assert not out.covariance_materialized
        tr = model(model.train_inputs)
        got = dict(mean=out._mean64.cpu().numpy(), var=out._var64.cpu().numpy(), cov=out.covariance64.cpu().numpy(), lp=lp,
                   mean_train=tr._mean64.cpu().numpy(), lp_train=float(lik(tr).log_prob(y64)))
        diffs = R.compare(got, ref)
        print("case %d %s: F = %d, rebuilds = %d, %s" % (k, R.CASES[k], post.features, post.rebuilds,
                                                          ", ".join("%s %.3g" % kv for kv in diffs.items())))
        assert max(diffs.values()) <= R.TOL, diffs
        assert abs(st.train_log_prob(model.train_targets) - ref["lp_train"]) <= R.TOL * max(1.0, abs(ref["lp_train"]))
        a_ref = ref["alpha"]
        assert np.abs(st.alpha64.reshape(-1).cpu().numpy() - a_ref).max() <= 1e-7 * max(1.0, np.abs(a_ref).max())
        # the float32 views of the same numbers
        assert np.abs(out.variance.double().cpu().numpy() - ref["var"]).max() <= 1e-6 * ref["prior_diag_scale"]
        assert np.abs(out.covariance.double().cpu().numpy() - ref["cov"]).max() <= 1e-6 * ref["prior_diag_scale"]


def test_rows_outside_the_block_rebuild_once(gpu_device):
    from rpgp_amd import settings
    model, lik, Xs, ys = _model(0, gpu_device)
    model.eval()
    with settings.ski_posterior(True), torch.no_grad():
        inside = model(0.5 * model.train_inputs[:50])
        post = model.prediction_strategy.ski_post
        assert post is not None and post.rebuilds == 0
        first = post.state
        wide = model(3.0 * Xs)                                   # beyond the training range in every column
        assert post.rebuilds == 1 and post.state is not first
        model(3.0 * Xs)
        model(Xs)
        assert post.rebuilds == 1
        assert torch.isfinite(wide._var64).all() and torch.isfinite(inside._var64).all()
        assert float(wide._var64.min()) >= -1e-9 and float(inside._var64.min()) >= -1e-9


def test_over_the_node_cap_falls_back_with_the_reason(gpu_device):
    from rpgp_amd import settings
    from rpgp_amd.ski_posterior import SKIPredictive
    model, lik, Xs, ys = _model(0, gpu_device)
    model.eval()
    with settings.ski_posterior(True), settings.ski_posterior_max_nodes(3 * 64 - 1), torch.no_grad():
        out = model(Xs)
    st = model.prediction_strategy
    assert st.ski_post is None and st.ski_posterior_reason == "J G = 192 nodes exceed 191"
    assert not isinstance(out, SKIPredictive) and torch.isfinite(out.mean).all() and hasattr(st, "dense_path")
    model.train()
    model.eval()
    with torch.no_grad():                                        # the setting off: no posterior object, no reason
        model(Xs)
    assert model.prediction_strategy.ski_post is None and model.prediction_strategy.ski_posterior_reason is None
