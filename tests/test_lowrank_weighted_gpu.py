"""The closed-form low-rank likelihood and prediction for the weighted kinds on the MI355X: the two column-list feature kernels
(rpgp_lowrank_features_cols_f64 / rpgp_lowrank_features_grad_cols_f64) against their float64 torch restatement and, on the
identity column list, bit for bit against the existing pair; their limits; the Gram matrix of four column forms against the
float64 kernel; a weighted rp_poly model's objective, gradients and posterior against the dense float64 oracle; the not-served
step; and the runner with both flags."""
import json
import math

import numpy as np
import pytest
import torch

from oracle import family as fmo

pytestmark = pytest.mark.gpu

KAPPA = 0.84932180028801907
EPS = 2.0 ** -52
FORMS = [(0.0, 64), (1.5, 64), (4.6, 64), (10.0, 128)]          # (half-width, rank cap); h = 10: PB 88, dynamic LDS
COLS9 = ([4], [5, 0, 8], [6, 1, 3, 0, 8, 2, 7])                 # lists into ldz = 9 columns


def _cheb_stack(X, p):
    T = [torch.ones_like(X), X]
    for _ in range(2, p):
        T.append(2.0 * X * T[-1] - T[-2])
    return torch.stack(T[:p], dim=-1)


def _features_ref(Z, cols, mid, inv_w, G, col_scale):
    X = (Z[:, cols] - mid) * inv_w
    return ((_cheb_stack(X, G.shape[0]) @ G) * col_scale.reshape(1, -1, 1)).reshape(Z.shape[0], -1)


def _grad_ref(Z, cols, mid, inv_w, Gd, col_scale, W):
    N, nc = Z.shape[0], len(cols)
    X = (Z[:, cols] - mid) * inv_w
    P = _cheb_stack(X, Gd.shape[0]) @ Gd
    return col_scale.reshape(1, -1) * inv_w * (P * W.reshape(N, nc, -1)).sum(-1)


def _select(h, cap):
    from rpgp_amd import ops
    p, r, tail, G = ops.lowrank_post_select(h, 1e-10, cap)
    assert p > 0
    return p, r, G


def _case(N, ldz, cols, r, seed, dev):
    """Z inside the interval of every listed column (half-width 1.3 around a random midpoint), factors in [0.1, 2]."""
    g = torch.Generator().manual_seed(seed)
    nc, hw = len(cols), 1.3
    mid_all = torch.randn(ldz, generator=g, dtype=torch.float64)
    Z = mid_all + (torch.rand(N, ldz, generator=g, dtype=torch.float64) * 2.0 - 1.0) * hw
    cs = torch.rand(nc, generator=g, dtype=torch.float64) * 1.9 + 0.1
    Y = torch.randn(N, nc * r + 3, generator=g, dtype=torch.float64)
    alpha = torch.randn(N, 1, generator=g, dtype=torch.float64)
    v = torch.randn(nc * r, generator=g, dtype=torch.float64)
    return [t.to(dev) for t in (Z, mid_all[cols], cs, Y, alpha, v)] + [1.0 / hw]


def _check_kernels(p, G, cap, N, ldz, cols, r, dev):
    from rpgp_amd import ops
    Gr = np.ascontiguousarray(G[:, :r])
    Gt = torch.from_numpy(Gr).to(dev)
    Gd = ops.chebyshev_derivative(Gr)
    Gdt = torch.from_numpy(Gd).to(dev)
    Z, mid, cs, Y, alpha, v, inv_w = _case(N, ldz, cols, r, 1000 * N + 10 * len(cols) + r, dev)
    nc, F = len(cols), len(cols) * r
    kw = {"max_rank": cap}
    tag = (p, r, N, cols if nc <= 7 else "perm64")
    # features
    big = torch.full((N, F + 5), float("nan"), dtype=torch.float64, device=dev)
    out = ops.lowrank_features_cols(Z, cols, mid, inv_w, Gr, cs, out=big[:, :F], **kw)
    err = float((out - _features_ref(Z, cols, mid, inv_w, Gt, cs)).abs().max())
    bound = 1e-13 * p * float(np.abs(Gr).max()) * float(cs.max())
    assert err <= bound, ("features", tag, err, bound)
    assert bool(torch.isnan(big[:, F:]).all()) and not bool(torch.isnan(out).any())
    assert torch.equal(ops.lowrank_features_cols(Z, cols, mid, inv_w, Gr, cs, **kw), out)
    # adjoint
    ca, cy = -0.7, 1.3
    W = ca * alpha * v.reshape(1, -1) + cy * Y[:, :F]
    gbig = torch.full((N, ldz + 3), float("nan"), dtype=torch.float64, device=dev)
    gz = ops.lowrank_features_grad_cols(Z, cols, mid, inv_w, Gr, cs, Y, alpha, v, ca, cy, out=gbig[:, :ldz], **kw)
    ref = _grad_ref(Z, cols, mid, inv_w, Gdt, cs, W)
    bound = 8 * EPS * (p + r) * p * r * float(np.abs(Gd).max()) * float(W.abs().max()) * float(cs.max()) * inv_w + 1e-300
    err = float((gz[:, cols] - ref).abs().max())
    assert err <= bound, ("adjoint", tag, err, bound)
    rest = [j for j in range(ldz + 3) if j not in cols]
    assert bool(torch.isnan(gbig[:, rest]).all()) and not bool(torch.isnan(gz[:, cols]).any())
    again = torch.full((N, ldz), float("nan"), dtype=torch.float64, device=dev)
    ops.lowrank_features_grad_cols(Z, cols, mid, inv_w, Gr, cs, Y, alpha, v, ca, cy, out=again, **kw)
    assert torch.equal(again[:, cols], gz[:, cols])


@pytest.mark.parametrize("h, cap", FORMS)
def test_column_kernels_against_torch(gpu_device, h, cap):
    p, r_sel, G = _select(h, cap)
    if h == 10.0:
        assert 80 < p <= 88                                            # padded rank 88: the dynamic-LDS body
    # r in {1, 17, p}: G's columns truncated, or repeated (halved each time) where the selection kept fewer than p
    reps = -(-p // r_sel)
    Gp = np.ascontiguousarray(np.concatenate([G * 0.5 ** k for k in range(reps)], axis=1)[:, :p])
    ranks = sorted({1, min(17, p), p})
    for r in ranks:
        for N in (1, 63, 65, 257):
            for cols in COLS9:
                _check_kernels(p, Gp, cap, N, 9, cols, r, gpu_device)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(7)).tolist()
    _check_kernels(p, Gp, cap, 65, 64, perm, min(17, p), gpu_device)


@pytest.mark.parametrize("h, cap", FORMS[1:])
def test_identity_list_is_bit_equal_to_the_existing_kernels(gpu_device, h, cap):
    from rpgp_amd import ops
    p, r, G = _select(h, cap)
    scale = 0.37
    for N, J in ((65, 7), (257, 20)):
        cols = list(range(J))
        Z, mid, _, Y, alpha, v, inv_w = _case(N, J, cols, r, N + J, gpu_device)
        cs = torch.full((J,), math.sqrt(scale), dtype=torch.float64, device=gpu_device)
        a = ops.lowrank_features(Z, mid, inv_w, G, scale, max_rank=cap)
        b = ops.lowrank_features_cols(Z, cols, mid, inv_w, G, cs, max_rank=cap)
        assert torch.equal(a, b), (h, N, J)
        ga = ops.lowrank_features_grad(Z, mid, inv_w, G, scale, Y, alpha, v, -0.7, 1.3, max_rank=cap)
        gb = ops.lowrank_features_grad_cols(Z, cols, mid, inv_w, G, cs, Y, alpha, v, -0.7, 1.3, max_rank=cap)
        assert torch.equal(ga, gb), (h, N, J)


def test_limits(gpu_device):
    from rpgp_amd import ops
    f64 = dict(dtype=torch.float64, device=gpu_device)
    N = 8
    G = np.ones((3, 2))

    def both(Z, cols, G, **kw):
        nc, r = len(cols), G.shape[1]
        mid, cs = torch.zeros(nc, **f64), torch.ones(nc, **f64)
        with pytest.raises(ValueError):
            ops.lowrank_features_cols(Z, cols, mid, 1.0, G, cs, **kw)
        with pytest.raises(ValueError):
            ops.lowrank_features_grad_cols(Z, cols, mid, 1.0, G, cs, torch.zeros(N, nc * r, **f64), torch.zeros(N, **f64),
                                           torch.zeros(nc * r, **f64), 1.0, 1.0, **kw)
    both(torch.zeros(N, 70, **f64), list(range(65)), G)                # nc = 65
    both(torch.zeros(N, 9, **f64), [3, 5, 3], G)                       # a repeated column
    both(torch.zeros(N, 9, **f64), [0, 9], G)                          # a column >= ldz
    both(torch.zeros(N, 9, **f64), [0, -1], G)
    both(torch.zeros(N, 9, **f64), [0, 1], np.ones((129, 2)), max_rank=128)    # p = 129
    both(torch.zeros(N, 9, **f64), [0, 1], np.ones((65, 2)))           # p above the default cap
    both(torch.zeros(N, 9, **f64), [0, 1], np.ones((3, 4)))            # r > p
    # the C entry itself refuses what it can see
    from rpgp_amd import _lib
    lib = _lib.load()
    Z, B = torch.zeros(N, 9, **f64), torch.zeros(N, 200, **f64)
    ci = torch.zeros(70, dtype=torch.int32, device=gpu_device)
    d = torch.zeros(70, **f64)
    Gt = torch.ones(129, 2, **f64)
    for nc, ldz, p, r, ldb in ((65, 70, 3, 2, 200), (2, 9, 129, 2, 200), (2, 9, 3, 4, 200), (2, 9, 3, 2, 3), (3, 2, 3, 2, 200)):
        rc = lib.rpgp_lowrank_features_cols_f64(Z.data_ptr(), N, nc, ldz, ci.data_ptr(), d.data_ptr(), 1.0, Gt.data_ptr(), p, r,
                                                d.data_ptr(), B.data_ptr(), ldb, None)
        assert rc == _lib.RPGP_EINVAL, (nc, ldz, p, r, ldb, rc)


# ---- the Gram matrix of four column forms --------------------------------------------------------------------------------
def _problem(dev, N=1500, d=8, J=20, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g, dtype=torch.float64)
    P = torch.randn(d, J, generator=g, dtype=torch.float64) / math.sqrt(d)
    ls = torch.tensor([0.5 * 2.0 ** (3.0 * j / 19.0) for j in range(J)], dtype=torch.float64)
    w = torch.rand(J, generator=g, dtype=torch.float64) + 0.5
    return X, P, ls, w / w.sum()


def test_gram_of_four_column_forms(gpu_device):
    from rpgp_amd import backend, ops
    from rpgp_amd.lowrank_posterior import column_forms, tail_tolerance
    X, P, ls, w = _problem(gpu_device)
    s, noise = 0.9, 0.05
    Z = ((X @ P) / ls).to(gpu_device)
    N, J = Z.shape
    zmin, zmax = Z.min(0).values, Z.max(0).values
    forms, why = column_forms(backend.get_backend(), Z, zmin, zmax, w, s, noise)
    assert forms is not None, why
    print("classes (p, r, columns):", forms.class_ranks, "F =", forms.F)
    assert forms.class_ranks == [(44, 31, 8), (26, 18, 6), (18, 12, 5), (13, 8, 1)] and forms.F == 424
    B = forms.features(backend.get_backend(), Z)
    K = torch.zeros(N, N, dtype=torch.float64, device=gpu_device)
    for j in range(J):
        K += float(w[j]) * torch.exp(-0.5 * (Z[:, j:j + 1] - Z[:, j:j + 1].t()) ** 2)
    err = float((B @ B.t() - s * K).abs().max())
    bound = s * sum(float(w[c.cols].sum()) * c.tail for c in forms.classes)
    print("max |B B^T - K| = %.3g, bound %.3g" % (err, bound))
    assert err <= bound + 1e-13, (err, bound)
    h = KAPPA * float((0.5 * (zmax - zmin)).max()) * (1.0 + 2.0 ** -20)
    p1, r1, _, _ = ops.lowrank_post_select(h, tail_tolerance(N, s * float(w.sum()), noise))
    assert p1 > 0 and forms.F < J * r1, (forms.F, J * r1)
    assert (forms.p, forms.r) == (p1, r1)                              # the widest class has the single form's ranks


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _model(dev, kernel_type="RBF", noise=0.05, s=0.9):
    from rpgp_amd.kernels import PolynomialProjectionKernel, ScaleKernel, inv_softplus
    from rpgp_amd.likelihoods import GaussianLikelihood, SmoothedBoxPrior
    from rpgp_amd.models import ExactGPModel, ExactMarginalLogLikelihood
    X, P, ls, w = _problem(dev)
    X, P = X.float(), P.float()
    N, d = X.shape
    J = P.shape[1]
    g = torch.Generator().manual_seed(11)
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
    y = (y - y.mean()) / y.std()
    Xs = torch.randn(101, d, generator=g) * 0.7
    ys = (torch.sin(Xs).sum(1) - torch.sin(X).sum(1).mean()) / torch.sin(X).sum(1).std()
    kern = PolynomialProjectionKernel(J, 1, d, kernel_type, [P[:, j:j + 1].clone() for j in range(J)], weighted=True)
    kern.raw_lengthscales.data = inv_softplus(ls).reshape(1, -1).float()
    kern.raw_outputscales.data = inv_softplus(w).float()
    sk = ScaleKernel(kern)
    sk.outputscale = s
    lik = GaussianLikelihood(noise_prior=SmoothedBoxPrior(1e-4, 10, sigma=0.01))
    lik.noise = noise
    model = ExactGPModel(X.to(dev), y.to(dev), lik, sk).to(dev)
    # The mean's gradient is -sum(alpha) / N (alpha = Khat^-1 (y - c)), which a float32 model sums from float32 terms.  y is
    # centred, so with c near 0 the terms cancel: at c = 0.1 sum |alpha| / |sum alpha| = 4e4 on this problem and rounding the
    # terms to float32 alone moves the sum by 2^-24 (sum alpha^2 / 3)^1/2 / |sum alpha| = 5e-5, the whole bound of the check
    # below, whatever the code computes.  At c = 1 the condition number is 3e3 and that rounding 3e-6, an order below the bound.
    model.mean_module.constant.data.fill_(1.0)
    return model, lik, ExactMarginalLogLikelihood(lik, model), X.to(dev), y.to(dev), Xs.to(dev), ys.to(dev)


def _params(model, lik):
    kern = model.covar_module.base_kernel
    return [kern.raw_lengthscales, model.covar_module.raw_outputscale, kern.raw_outputscales, lik.raw_noise,
            model.mean_module.constant]


NAMES = ("raw_lengthscales", "raw_outputscale", "raw_outputscales", "raw_noise", "mean")


class _Dense:
    """The exact weighted GP in float64 torch on the device, as a function of the raw parameters."""

    def __init__(self, model, lik, X, y, raw=None):
        sp = torch.nn.functional.softplus
        self.raw = raw or [p.detach().double().clone().requires_grad_(True) for p in _params(model, lik)]
        raw_ls, raw_os, raw_w, raw_noise, c = self.raw
        self.Wp = model.covar_module.base_kernel.projection_module.weight.detach().double().t()
        self.ls, self.s, self.w = sp(raw_ls).reshape(1, -1), sp(raw_os).reshape(()), sp(raw_w).reshape(-1)
        self.noise = (sp(raw_noise) + lik.MIN_NOISE).reshape(())
        self.c, self.lik = c, lik
        self.Z = self.coords(X)
        self.y = y.double()

    def coords(self, X):
        return (X.double() @ self.Wp) / self.ls

    def K(self, A, B):
        out = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float64, device=A.device)
        for j in range(A.shape[1]):
            out = out + self.w[j] * torch.exp(-0.5 * (A[:, j:j + 1] - B[:, j:j + 1].t()) ** 2)
        return self.s * out

    def loss(self):
        """-mll per datum: the dense Cholesky's value; the gradient through the surrogate with Khat^-1, alpha held fixed."""
        N = self.Z.shape[0]
        Kh = self.K(self.Z, self.Z) + self.noise * torch.eye(N, dtype=torch.float64, device=self.Z.device)
        rr = (self.y - self.c).reshape(-1, 1)
        with torch.no_grad():
            L = torch.linalg.cholesky(Kh)
            alpha = torch.cholesky_solve(rr, L)
            S = torch.cholesky_inverse(L) - alpha @ alpha.t()
            value = 0.5 * ((rr * alpha).sum() + 2.0 * torch.log(L.diagonal()).sum() + N * math.log(2 * math.pi))
        sur = 0.5 * (S * Kh).sum() + (alpha * rr).sum()
        return (value + (sur - sur.detach()) - self.lik.noise_prior.log_prob(self.noise)) / N

    def predict(self, Xs):
        with torch.no_grad():
            N = self.Z.shape[0]
            Kh = self.K(self.Z, self.Z) + self.noise * torch.eye(N, dtype=torch.float64, device=self.Z.device)
            L = torch.linalg.cholesky(Kh)
            Zs = self.coords(Xs)
            Ksx = self.K(Zs, self.Z)
            mean = (Ksx @ torch.cholesky_solve((self.y - self.c).reshape(-1, 1), L)).reshape(-1) + self.c
            return mean, self.K(Zs, Zs) - Ksx @ torch.cholesky_solve(Ksx.t().contiguous(), L)


def test_objective_and_posterior_against_the_dense_oracle(gpu_device):
    """The float32 weighted rp_poly model (N = 1 500, J = 20, lengthscales spread 8 x: four classes).  Bounds: those of the
    unweighted model's tests (1e-6 on the value, 1e-5 relative on the gradients, 5e-5 on the mean's; 1e-5 on the posterior),
    the component weights' gradient held to the outputscale's."""
    from rpgp_amd import settings
    model, lik, mll, X, y, Xs, ys = _model(gpu_device)
    model.train()
    with settings.lowrank_mll(True):
        out = model(X)
        loss = mll.negative(out, y)
        loss.backward()
    op = out.covariance
    assert op.lowrank_mll_served, op.lowrank_mll_reason
    fm = op.lowrank_mll_form()
    print("classes (p, r, columns):", fm.class_ranks, "F =", fm.ranks[2], "tail %.3g" % fm.tail)
    assert len(fm.class_ranks) >= 2 and sum(nc for _, _, nc in fm.class_ranks) == 20
    dense = _Dense(model, lik, X, y)
    ref = dense.loss()
    ref.backward()
    # the device reference's kernel is the oracle's
    Zn = dense.Z.detach().cpu().numpy()[:200]
    Ko = fmo.kernel_matrix(Zn, Zn, "RBF", 1, dense.w.detach().cpu().numpy(), float(dense.s.detach()))
    assert np.abs(dense.K(dense.Z[:200], dense.Z[:200]).detach().cpu().numpy() - Ko).max() <= 1e-14
    print("value %.10f, dense %.10f" % (float(loss.detach()), float(ref.detach())))
    errs = {}
    for name, p, r in zip(NAMES, _params(model, lik), dense.raw):
        assert p.grad is not None and p.grad.shape == r.grad.shape
        errs[name] = float((p.grad.double() - r.grad).abs().max() / r.grad.abs().max())
        print("%s: rel %.3g" % (name, errs[name]))
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-6, (float(loss.detach()), float(ref.detach()))
    for name in NAMES:
        assert errs[name] <= (5e-5 if name == "mean" else 1e-5), (name, errs[name])
    # the posterior
    model.eval()
    with settings.lowrank_posterior(True), torch.no_grad():
        pred = model(Xs)
        st = model.prediction_strategy
        assert st.lowrank is not None, st.lowrank_fallback_reason
        assert len(st.lowrank.class_ranks) >= 2
        mean_ref, cov_ref = dense.predict(Xs)
        em = float((pred.mean.double() - mean_ref).abs().max() / mean_ref.abs().max())
        ev = float((pred.variance.double() - cov_ref.diagonal()).abs().max() / cov_ref.diagonal().abs().max())
        print("posterior mean rel %.3g, variance rel %.3g" % (em, ev))
        assert em <= 1e-5 and ev <= 1e-5, (em, ev)


def test_not_served_is_todays_step(gpu_device):
    """A Matern rp_poly model with both settings on: the loss and the gradients of the settings-off step, bit for bit."""
    from rpgp_amd import settings

    def step(on):
        model, lik, mll, X, y, _, _ = _model(gpu_device, kernel_type="Matern")
        model.train()
        with settings.lowrank_mll(on), settings.lowrank_posterior(on), settings.deterministic_probes(True):
            out = model(X)
            loss = mll.negative(out, y)
            loss.backward()
        assert not out.covariance.lowrank_mll_served
        return loss.detach().clone(), [p.grad.detach().clone() for p in _params(model, lik)]

    v0, g0 = step(False)
    v1, g1 = step(True)
    assert torch.equal(v0, v1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


def test_runner_with_both_flags(gpu_device, tmp_path, monkeypatch):
    """additive_rp_J20_K1 (weighted rp_poly, J = 20, k = 1) on 1 500 training rows, against the exact flag-off run (dense
    Cholesky: --use_chol on both sides, so that neither fit carries the noise of stochastic trace probes)."""
    from rpgp_amd import runner, specs
    monkeypatch.setitem(runner.SYNTHETIC_SHAPES, "w1500", (1667, 8))
    spec = specs.get("additive_rp_J20_K1.json")
    spec["train_kwargs"]["max_iter"] = 5
    spec["train_kwargs"]["init_iters"] = 1
    spec["model_kwargs"]["init_lengthscale_range"] = [3.0, 3.0]      # half-widths 1.1 ... 4.1 here: served from the first step
    sp = tmp_path / "spec.json"
    json.dump(spec, open(sp, "w"))
    rows = {}
    for flag in ([], ["--lowrank_mll", "--lowrank_posterior"]):
        torch.manual_seed(0)
        np.random.seed(0)
        df = runner.main(["-m", str(sp), "-d", "synthetic:w1500", "-o", str(tmp_path / ("r%d.csv" % len(flag))), "--no_cv",
                          "--skip_random_restart", "--device", "cuda:0", "--use_chol"] + flag)
        assert "error" not in df.columns, df
        rows[bool(flag)] = df.iloc[0]
    on, off = rows[True], rows[False]
    print("served share %.2f, posterior served %d, test NLL %.8f against %.8f"
          % (on["lowrank_mll_share"], on["lowrank_posterior_served"], float(on["test_nll"]), float(off["test_nll"])))
    assert int(on["trained_epochs"]) >= 1 and np.isfinite(float(on["rmse"]))
    assert float(on["lowrank_mll_share"]) == 1.0 and int(on["lowrank_posterior_served"]) == 1
    assert "lowrank_mll_share" not in off.index or not np.isfinite(float(off["lowrank_mll_share"]))
    a, b = float(on["test_nll"]), float(off["test_nll"])
    assert abs(a - b) <= 1e-4 * abs(b), (a, b)
