"""The closed-form posterior of the Chebyshev low-rank features (settings.lowrank_posterior) on the GPU: the feature kernel
rpgp_lowrank_features_f64 against a float64 torch restatement, B B^T against the exact kernel, the posterior against a dense
float64 solve of the exact GP, the C4 prediction against the setting-off path, the interval's rebuild and fallback, a large
test set without its covariance, and the runner end to end."""
import json
import math

import numpy as np
import pytest
import torch

from oracle import dense_gp as orc

pytestmark = pytest.mark.gpu

KAPPA = 0.84932180028801907


def _features_ref(Z, mid, inv_w, G, scale):
    X = (Z - mid) * inv_w
    p = G.shape[0]
    T = [torch.ones_like(X), X]
    for _ in range(2, p):
        T.append(2.0 * X * T[-1] - T[-2])
    T = torch.stack(T[:p], dim=-1)                        # N x J x p
    return (math.sqrt(scale) * (T @ G)).reshape(Z.shape[0], -1)


@pytest.mark.parametrize("h", [0.0, 1.5, 4.6, 7.0])
def test_feature_kernel_against_torch(gpu_device, h):
    from rpgp_amd import ops
    p, r, tail, G = ops.lowrank_post_select(h, 1e-10)
    assert p > 0
    Gd = torch.from_numpy(G).to(gpu_device)
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
            big = torch.full((N, F + 5), float("nan"), dtype=torch.float64, device=gpu_device)
            out = ops.lowrank_features(Z, mid, inv_w, G, scale, out=big[:, :F])
            ref = _features_ref(Z, mid, inv_w, Gd, scale)
            bound = 1e-13 * p * float(np.abs(G).max()) * math.sqrt(scale)
            err = float((out - ref).abs().max())
            assert err <= bound, (h, N, J, err, bound)
            assert bool(torch.isnan(big[:, F:]).all())
            again = ops.lowrank_features(Z, mid, inv_w, G, scale)
            assert torch.equal(again, out)


def test_feature_kernel_limits(gpu_device):
    from rpgp_amd import ops
    Z = torch.zeros(4, 65, dtype=torch.float64, device=gpu_device)
    G = np.ones((3, 2))
    with pytest.raises(ValueError):
        ops.lowrank_features(Z, torch.zeros(65, dtype=torch.float64), 1.0, G, 1.0)
    with pytest.raises(ValueError):
        ops.lowrank_features(Z[:, :4].contiguous(), torch.zeros(4, dtype=torch.float64), 1.0, np.ones((65, 2)), 1.0)


def test_feature_gram_against_the_exact_kernel(gpu_device):
    """B B^T on 2 000 rows of the C4 problem (d = 20, J = 20, lengthscale sqrt(d)) against the float64 kernel."""
    from rpgp_amd import ops
    d, J, s = 20, 20, 1.0
    X = torch.randn(50000, d, generator=torch.Generator().manual_seed(0))[:2000].double()
    P = torch.randn(d, J, generator=torch.Generator().manual_seed(1)).double()
    Z = (X / math.sqrt(d)) @ P
    zmin, zmax = Z.min(0).values, Z.max(0).values
    h = KAPPA * float((0.5 * (zmax - zmin)).max()) * (1.0 + 2.0 ** -20)
    p, r, tail, G = ops.lowrank_post_select(h, 1e-10)
    assert p > 0
    Zd = Z.to(gpu_device)
    B = ops.lowrank_features(Zd, (0.5 * (zmin + zmax)).to(gpu_device), KAPPA / h, G, s / J)
    K = torch.zeros(2000, 2000, dtype=torch.float64, device=gpu_device)
    for j in range(J):
        K += torch.exp(-0.5 * (Zd[:, j:j + 1] - Zd[:, j:j + 1].t()) ** 2)
    err = float((B @ B.t() - (s / J) * K).abs().max())
    assert err <= s * tail + 1e-13, (err, s * tail, p, r)


# ---- models ---------------------------------------------------------------------------------------------------------------
def _model(N, d, J, dev, noise=0.1, s=1.0, ls=None, seed=0, n_test=101):
    from rpgp_amd.kernels import AdditiveStructureRBFKernel, ScaledProjectionKernel, ScaleKernel
    from rpgp_amd.likelihoods import GaussianLikelihood, SmoothedBoxPrior
    from rpgp_amd.models import ExactGPModel, ExactMarginalLogLikelihood
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g)
    P = torch.randn(d, J, generator=g)
    ls = torch.full((d,), math.sqrt(d)) if ls is None else ls
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
    y = (y - y.mean()) / y.std()
    Xs = torch.randn(n_test, d, generator=g) * 0.7
    ys = (torch.sin(Xs).sum(1) - torch.sin(X).sum(1).mean()) / torch.sin(X).sum(1).std()
    lin = torch.nn.Linear(d, J, bias=False)
    lin.weight.data = P.t().contiguous()
    k = ScaledProjectionKernel(lin, AdditiveStructureRBFKernel(J), prescale=True, ard_num_dims=d)
    k.initialize(lengthscale=ls)
    sk = ScaleKernel(k)
    sk.outputscale = s
    lik = GaussianLikelihood(noise_prior=SmoothedBoxPrior(1e-4, 10, sigma=0.01))
    lik.noise = noise
    model = ExactGPModel(X.to(dev), y.to(dev), lik, sk).to(dev)
    model.mean_module.constant.data.fill_(0.1)
    return model, lik, ExactMarginalLogLikelihood(lik, model), X.to(dev), y.to(dev), Xs.to(dev), ys.to(dev)


class _DenseRef:
    """The exact GP in float64 on the device (the formulas of oracle.dense_gp.DenseExactGP), at the model's parameters."""

    def __init__(self, model, X, y):
        bk = model.covar_module.base_kernel
        self.Peff = bk.projection_module.weight.detach().t().double() / \
            bk.lengthscale.detach().double().reshape(-1, 1)
        self.scale = float(model.covar_module.outputscale.detach().double()) / self.Peff.shape[1]
        self.noise = float(model.likelihood.noise.detach().double())
        self.c = float(model.mean_module.constant.detach().double())
        self.Z = X.double() @ self.Peff
        self.y = y.double()
        Kh = self.K(self.Z, self.Z)
        Kh.diagonal().add_(self.noise)
        self.L = torch.linalg.cholesky(Kh)
        self.alpha = torch.cholesky_solve((self.y - self.c).reshape(-1, 1), self.L)

    def K(self, A, B):
        out = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float64, device=A.device)
        for j in range(A.shape[1]):
            out += torch.exp(-0.5 * (A[:, j:j + 1] - B[:, j:j + 1].t()) ** 2)
        return self.scale * out

    def predict(self, Xs):
        Zs = Xs.double() @ self.Peff
        Ksx = self.K(Zs, self.Z)
        mean = (Ksx @ self.alpha).reshape(-1) + self.c
        S = torch.empty_like(Ksx.t())
        for c0 in range(0, S.shape[1], 1024):              # (column panels: the library's solves run out of workspace)
            S[:, c0:c0 + 1024] = torch.cholesky_solve(Ksx[c0:c0 + 1024].t().contiguous(), self.L)
        return mean, self.K(Zs, Zs) - Ksx @ S

    def log_density(self, Xs, ys):
        mean, cov = self.predict(Xs)
        cov.diagonal().add_(self.noise)
        Lc = torch.linalg.cholesky(cov)
        z = torch.linalg.solve_triangular(Lc, (ys.double() - mean).reshape(-1, 1), upper=False)
        return float(-0.5 * (z * z).sum() - torch.log(Lc.diagonal()).sum() - 0.5 * ys.numel() * math.log(2 * math.pi))


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _check_against_dense(model, lik, X, y, Xs, ys, tol, ref=None):
    from rpgp_amd import settings
    ref = ref or _DenseRef(model, X, y)
    model.eval()
    with settings.lowrank_posterior(True), torch.no_grad():
        out = model(Xs)
        st = model.prediction_strategy
        assert st.lowrank is not None, st.lowrank_fallback_reason
        mean_ref, cov_ref = ref.predict(Xs)
        assert _rel(out.mean, mean_ref) <= tol
        assert _rel(out.variance, cov_ref.diagonal()) <= tol
        lp = float(lik(out).log_prob(ys.double()))
        lp_ref = ref.log_density(Xs, ys)
        assert abs(lp - lp_ref) <= tol * abs(lp_ref), (lp, lp_ref)
        cov = out.covariance.double()
        assert float((cov - cov_ref).norm() / cov_ref.norm()) <= tol
        lp_tr = st.train_log_prob(y)
        lp_tr_ref = ref.log_density(X, y)
        assert abs(lp_tr - lp_tr_ref) <= tol * abs(lp_tr_ref), (lp_tr, lp_tr_ref)
    return st


@pytest.mark.parametrize("N", [1800, 2600])
def test_posterior_against_the_dense_oracle(gpu_device, N):
    model, lik, mll, X, y, Xs, ys = _model(N, 6, 8, gpu_device, noise=0.05, seed=N)
    ref = _DenseRef(model, X, y)
    if N == 1800:                                   # the device reference is the oracle's
        bk = model.covar_module.base_kernel
        orc_gp = orc.DenseExactGP(X.double().cpu().numpy(), y.double().cpu().numpy(),
                                  bk.projection_module.weight.detach().t().double().cpu().numpy(),
                                  bk.lengthscale.detach().double().cpu().numpy().reshape(-1), float(model.covar_module.outputscale.detach()),
                                  float(lik.noise), mean=float(model.mean_module.constant))
        m_orc, _ = orc_gp.predict(Xs.double().cpu().numpy())
        assert np.abs(ref.predict(Xs)[0].cpu().numpy() - m_orc).max() <= 1e-10 * np.abs(m_orc).max()
    _check_against_dense(model, lik, X, y, Xs, ys, 1e-5, ref)


def test_posterior_c2_against_the_dense_oracle(gpu_device):
    model, lik, mll, X, y, Xs, ys = _model(7372, 8, 20, gpu_device, noise=0.05)
    st = _check_against_dense(model, lik, X, y, Xs, ys, 1e-5)
    # evaluate-on-train through the marginal likelihood: the closed form (no N x N covariance)
    with torch.no_grad():
        tr = model(X)
        nll = -mll(tr, y).item()
        assert not tr.covariance_materialized
        assert abs(nll + (st.train_log_prob(y) + lik.log_prior().item()) / X.shape[0]) <= 1e-6 * abs(nll)   # (float32 value)
    print("C2 ranks (p, r, F):", st.lowrank.ranks)


def test_c4_against_the_setting_off_path(gpu_device):
    from rpgp_amd import settings
    model, lik, mll, X, y, Xs, ys = _model(50000, 20, 20, gpu_device, noise=0.1, n_test=2000)
    model.eval()
    out = {}
    for on in (True, False):
        model.prediction_strategy = None
        # (the off side at the runner's eval_cg_tolerance 0.01 and one refinement round stops ~1e-4 from the exact mean: a
        #  tighter solve and more rounds, so that the comparison measures the feature posterior)
        with settings.lowrank_posterior(on), settings.eval_cg_tolerance(1e-4), settings.solve_refinement(4), torch.no_grad():
            o = model(Xs)
            out[on] = (o.mean.double(), o.variance.double())
            assert (model.prediction_strategy.lowrank is not None) == on
        model.prediction_strategy = None
        torch.cuda.empty_cache()
    assert _rel(out[True][0], out[False][0]) <= 1e-5
    # the off side's variances carry its float32 cross-covariance rows (3.9e-5 from the feature posterior, measured): the
    # variances are held to a float64 dense solve of the exact GP instead
    print("C4 variances, on against off: %.3g" % _rel(out[True][1], out[False][1]))
    ref = _DenseRef(model, model.train_inputs, model.train_targets)
    mean_ref, cov_ref = ref.predict(Xs)
    del ref
    print("C4 against float64 dense: mean %.3g (off %.3g), variances %.3g (off %.3g)" % (
        _rel(out[True][0], mean_ref), _rel(out[False][0], mean_ref), _rel(out[True][1], cov_ref.diagonal()),
        _rel(out[False][1], cov_ref.diagonal())))
    assert _rel(out[True][0], mean_ref) <= 1e-5
    assert _rel(out[True][1], cov_ref.diagonal()) <= 2e-5


def test_interval_rebuild_and_fallback(gpu_device):
    from rpgp_amd import settings
    model, lik, mll, X, y, Xs, ys = _model(1800, 6, 8, gpu_device, noise=0.05, seed=3)
    ref = _DenseRef(model, X, y)
    model.eval()
    with settings.lowrank_posterior(True), torch.no_grad():
        # a test row 30 % past the training range (the row with the widest coordinate, scaled): one rebuild on the union
        Zx = X.double() @ ref.Peff
        i = int((Zx - 0.5 * (Zx.max(0).values + Zx.min(0).values)).abs().max(1).values.argmax())
        Xw = Xs.clone()
        Xw[0] = X[i] * 1.3
        out = model(Xw)
        st = model.prediction_strategy
        assert st.lowrank is not None and st.lowrank.rebuilds == 1, st.lowrank_fallback_reason
        mean_ref, cov_ref = ref.predict(Xw)
        assert _rel(out.mean, mean_ref) <= 1e-5 and _rel(out.variance, cov_ref.diagonal()) <= 1e-5
        out = model(Xw)                                    # the wider interval is kept
        assert st.lowrank.rebuilds == 1
        # rows so far out that the union needs p > 64: this call takes the exact path
        Xf = Xs.clone()
        Xf[:5] = Xs[:5] * 12.0
        out = model(Xf)
        assert st.lowrank_fallback_reason and "64" in st.lowrank_fallback_reason, st.lowrank_fallback_reason
        mean_ref, cov_ref = ref.predict(Xf)
        assert _rel(out.mean, mean_ref) <= 1e-4 and _rel(out.variance, cov_ref.diagonal()) <= 1e-4


def test_setting_off_leaves_the_strategy_alone(gpu_device, monkeypatch):
    from rpgp_amd import backend, settings
    be = backend.get_backend()
    calls = []
    orig = be.lowrank_features
    monkeypatch.setattr(be, "lowrank_features", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    model, lik, mll, X, y, Xs, ys = _model(1800, 6, 8, gpu_device, noise=0.05)
    model.eval()
    with settings.lowrank_posterior(False), torch.no_grad():
        model(Xs)
    assert model.prediction_strategy.lowrank is None and not calls


def test_large_test_set_without_its_covariance(gpu_device):
    from rpgp_amd import settings
    model, lik, mll, X, y, Xs, ys = _model(20000, 10, 20, gpu_device, noise=0.1, n_test=30000)
    model.eval()
    with settings.lowrank_posterior(True), torch.no_grad():
        out = model(Xs)
        noisy = lik(out)
        lp = float(noisy.log_prob(ys))
        var = out.variance
        assert math.isfinite(lp) and bool((var > 0).all())
        assert not out.covariance_materialized and not noisy.covariance_materialized
        # at 3 000 rows the closed form equals the log-density of the explicit covariance
        small = lik(model(Xs[:3000]))
        lp_small = float(small.log_prob(ys[:3000].double()))
        C = small._post.noise * (small._V.t() @ small._V)
        C.diagonal().add_(small._post.noise)
        Lc = torch.linalg.cholesky(C)
        z = torch.linalg.solve_triangular(Lc, (ys[:3000].double() - small._mean64).reshape(-1, 1), upper=False)
        lp_exp = float(-0.5 * (z * z).sum() - torch.log(Lc.diagonal()).sum() - 1500.0 * math.log(2 * math.pi))
        assert abs(lp_small - lp_exp) <= 1e-8 * abs(lp_exp), (lp_small, lp_exp)


def test_runner_with_and_without_the_flag(gpu_device, tmp_path):
    from rpgp_amd import runner, specs
    spec = specs.get("additive_rp_prescale_J20.json")
    spec["train_kwargs"]["max_iter"] = 5
    spec["train_kwargs"]["init_iters"] = 1
    sp = tmp_path / "spec.json"
    json.dump(spec, open(sp, "w"))
    rows = {}
    for flag in ([], ["--lowrank_posterior"]):
        torch.manual_seed(0)                                # the same initialisation and probes for both fits
        np.random.seed(0)
        df = runner.main(["-m", str(sp), "-d", "synthetic:kin8nm", "-o", str(tmp_path / ("r%d.csv" % len(flag))), "--no_cv",
                          "--skip_random_restart", "--device", "cuda:0"] + flag)
        assert "error" not in df.columns, df
        rows[bool(flag)] = df.iloc[0]
    for key in ("rmse", "test_nll", "train_nll"):
        a, b = float(rows[True][key]), float(rows[False][key])
        assert abs(a - b) <= 1e-4 * abs(b), (key, a, b)
