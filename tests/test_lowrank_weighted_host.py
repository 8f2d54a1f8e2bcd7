"""The closed-form low-rank likelihood and prediction for the weighted kinds on the host (no GPU): the class rule of the column
forms, the serving decision with its reasons, the "features" mode of InvQuadLogDet on a weighted rp_poly model (CPU test double,
the two column-list feature kernels restated in float64 torch) against float64 autograd of the same feature objective and
against the dense float64 kernel, and the feature posterior against a dense float64 solve."""
import math

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from oracle import family as fmo
from rpgp_amd import ops

KAPPA = 0.84932180028801907


def _cheb_stack(X, p):
    T = [torch.ones_like(X), X]
    for _ in range(2, p):
        T.append(2.0 * X * T[-1] - T[-2])
    return torch.stack(T[:p], dim=-1)


def _features_cols_torch(Z, cols, mid, inv_w, G, col_scale, out=None, max_rank=64):
    """float64 torch restatement of rpgp_lowrank_features_cols_f64 (differentiable in Z and col_scale)."""
    G = torch.as_tensor(G, dtype=torch.float64)
    cols = [int(c) for c in cols]
    X = (Z.double()[:, cols] - torch.as_tensor(mid, dtype=torch.float64)) * inv_w
    cs = torch.as_tensor(col_scale, dtype=torch.float64).reshape(1, -1, 1)
    B = ((_cheb_stack(X, G.shape[0]) @ G) * cs).reshape(Z.shape[0], -1)
    if out is not None:
        out.copy_(B)
        return out
    return B


def _features_grad_cols_torch(Z, cols, mid, inv_w, G, col_scale, Y, alpha, v, ca, cy, out=None, max_rank=64):
    """float64 torch restatement of rpgp_lowrank_features_grad_cols_f64 (through ops.chebyshev_derivative)."""
    Gd = torch.from_numpy(ops.chebyshev_derivative(torch.as_tensor(G, dtype=torch.float64).numpy()))
    p, r = Gd.shape
    cols = [int(c) for c in cols]
    N, nc = Z.shape[0], len(cols)
    X = (Z.double()[:, cols] - torch.as_tensor(mid, dtype=torch.float64)) * inv_w
    P = _cheb_stack(X, p) @ Gd                                                    # N x nc x r
    W = ca * alpha.reshape(-1, 1) * v.reshape(1, -1) + cy * Y[:, :nc * r]
    g = torch.as_tensor(col_scale, dtype=torch.float64).reshape(1, -1) * inv_w * (P * W.reshape(N, nc, r)).sum(-1)
    if out is None:
        out = torch.full((N, Z.shape[1]), float("nan"), dtype=torch.float64)
    out[:, cols] = g
    return out


def _install(ob, monkeypatch, calls=None):
    def feat(*a, **k):
        if calls is not None:
            calls.append("features")
        return _features_cols_torch(*a, **k)

    def grad(*a, **k):
        if calls is not None:
            calls.append("grad")
        return _features_grad_cols_torch(*a, **k)
    monkeypatch.setattr(ob, "lowrank_post_select", ops.lowrank_post_select, raising=False)
    monkeypatch.setattr(ob, "lowrank_features_cols", feat, raising=False)
    monkeypatch.setattr(ob, "lowrank_features_grad_cols", grad, raising=False)


def _spread(J, spread, base=0.5):
    """Lengthscales base * spread^(j / (J - 1)): the last projection's is `spread` times the first's."""
    return torch.tensor([base * spread ** (j / max(J - 1, 1)) for j in range(J)], dtype=torch.float64)


def _model(N=300, d=4, J=5, spread=8.0, noise=0.05, s=0.9, seed=0, dtype=torch.float64, kernel_type="RBF", k=1,
           lengthscales=None, weights=None, degrees=None):
    """A weighted rp_poly model (general_rp_poly with `degrees`) with per-projection lengthscales spread `spread` times."""
    from rpgp_amd.kernels import GeneralizedProjectionKernel, PolynomialProjectionKernel, ScaleKernel, inv_softplus
    from rpgp_amd.likelihoods import GaussianLikelihood, SmoothedBoxPrior
    from rpgp_amd.models import ExactGPModel, ExactMarginalLogLikelihood
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g)
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
    if degrees is None:
        Ws = [torch.randn(d, k, generator=g) / math.sqrt(d) for _ in range(J)]
        kern = PolynomialProjectionKernel(J, k, d, kernel_type, Ws, weighted=True)
    else:
        lin = torch.nn.Linear(d, sum(degrees), bias=False)
        lin.weight.data = torch.randn(sum(degrees), d, generator=g) / math.sqrt(d)
        kern = GeneralizedProjectionKernel(degrees, d, kernel_type, lin, weighted=True)
        J = len(degrees)
    ncol = kern.raw_lengthscales.numel()
    ls = _spread(ncol, spread) if lengthscales is None else torch.as_tensor(lengthscales, dtype=torch.float64)
    w = torch.rand(J, generator=g).double() + 0.5 if weights is None else torch.as_tensor(weights, dtype=torch.float64)
    w = w / w.sum()
    kern.raw_lengthscales.data = inv_softplus(ls).reshape(1, -1).to(kern.raw_lengthscales)
    kern.raw_outputscales.data = inv_softplus(w).to(kern.raw_outputscales)
    sk = ScaleKernel(kern)
    sk.outputscale = s
    lik = GaussianLikelihood(noise_prior=SmoothedBoxPrior(1e-4, 10, sigma=0.01))
    lik.noise = noise
    X, y = X.to(dtype), y.to(dtype)
    model = ExactGPModel(X, y, lik, sk).to(dtype)
    model.mean_module.constant.data.fill_(0.2)
    return model, lik, ExactMarginalLogLikelihood(lik, model), X, y


def _params(model, lik):
    kern = model.covar_module.base_kernel
    return [kern.raw_lengthscales, model.covar_module.raw_outputscale, kern.raw_outputscales, lik.raw_noise,
            model.mean_module.constant]


NAMES = ("raw_lengthscales", "raw_outputscale", "raw_outputscales", "raw_noise", "mean")


def _leaves(model, lik, X):
    """float64 leaves of the model's parameters and (Z, s, w, noise, c) built from them."""
    kern = model.covar_module.base_kernel
    leaves = [t.detach().double().clone().requires_grad_(True) for t in _params(model, lik)]
    raw_ls, raw_os, raw_w, raw_noise, c = leaves
    Z = (X.double() @ kern.projection_module.weight.detach().double().t()) / F.softplus(raw_ls).reshape(1, -1)
    s = F.softplus(raw_os).reshape(())
    w = F.softplus(raw_w).reshape(-1)
    noise = (F.softplus(raw_noise) + lik.MIN_NOISE).reshape(())
    return leaves, Z, s, w, noise, c


def _mll(K, noise, c, y, lik, N):
    from rpgp_amd.likelihoods import LOG2PI
    Kh = K + noise * torch.eye(N, dtype=torch.float64)
    rr = (y.double() - c).reshape(-1, 1)
    L = torch.linalg.cholesky(Kh)
    iq = (rr * torch.cholesky_solve(rr, L)).sum()
    ld = 2.0 * torch.log(L.diagonal()).sum()
    return (-0.5 * (iq + ld + N * LOG2PI) + lik.noise_prior.log_prob(noise)) / N


def _feature_reference(model, lik, X, y, be):
    """float64 autograd of the mll per datum with K = B B^T: the same column forms, held fixed."""
    from rpgp_amd.lowrank_posterior import column_forms
    leaves, Z, s, w, noise, c = _leaves(model, lik, X)
    N = Z.shape[0]
    Zd = Z.detach()
    forms, why = column_forms(be, Zd, Zd.min(0).values, Zd.max(0).values, w.detach(), float(s.detach()), float(noise.detach()))
    assert forms is not None, why
    cs = torch.sqrt(s * w)
    B = torch.cat([_features_cols_torch(Z, cl.cols, cl.mid, cl.inv_w, cl.G, cs[cl.cols]) for cl in forms.classes], dim=1)
    val = _mll(B @ B.t(), noise, c, y, lik, N)
    val.backward()
    return float(val.detach()), [t.grad.detach().clone() for t in leaves], forms


def _dense_kernel(Z, s, w):
    """s sum_c w_c exp(-(z_c - z'_c)^2 / 2) in float64 torch."""
    D = Z.unsqueeze(1) - Z.unsqueeze(0)                                           # N x N x J
    return s * (torch.exp(-0.5 * D * D) * w.reshape(1, 1, -1)).sum(-1)


def _dense_reference(model, lik, X, y):
    leaves, Z, s, w, noise, c = _leaves(model, lik, X)
    K = _dense_kernel(Z, s, w)
    ref = fmo.kernel_matrix(Z.detach().numpy(), Z.detach().numpy(), "RBF", 1, w.detach().numpy(), float(s.detach()))
    assert np.abs(K.detach().numpy() - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max())
    val = _mll(K, noise, c, y, lik, Z.shape[0])
    val.backward()
    return float(val.detach()), [t.grad.detach().clone() for t in leaves]


def _rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


# ---- the class rule --------------------------------------------------------------------------------------------------------
def test_class_rule():
    from rpgp_amd.lowrank_posterior import MAX_FORMS, MAX_J, column_classes
    assert MAX_FORMS == 4 and MAX_J == 64
    assert column_classes([4.6, 2.4, 2.2, 1.1, 0.5, 0.2, 0.0]) == [0, 0, 1, 2, 3, 3, 3]
    assert column_classes([1.3] * 6) == [0] * 6
    assert column_classes([0.0, 0.0]) == [0, 0]
    assert column_classes([0.0, 2.0, 0.9]) == [1, 0, 1]                            # a zero width joins the last non-empty class
    assert column_classes([1.0, 2.0, 4.0]) == [2, 1, 0]                            # exact powers of two: floor(log2) itself


def test_column_forms_partition_the_features():
    from rpgp_amd.lowrank_posterior import column_forms

    class _Be:
        lowrank_post_select = staticmethod(ops.lowrank_post_select)
    half = torch.tensor([4.6, 2.4, 2.2, 1.1, 0.5, 0.2, 0.0], dtype=torch.float64) / KAPPA
    J = half.numel()
    g = torch.Generator().manual_seed(0)
    Z = (torch.rand(500, J, generator=g, dtype=torch.float64) * 2.0 - 1.0) * half
    w = torch.rand(J, generator=g, dtype=torch.float64) + 0.1
    forms, why = column_forms(_Be, Z, -half, half, w, 0.9, 0.05)
    assert forms is not None, why
    assert forms.cls == [0, 0, 1, 2, 3, 3, 3]
    assert [c.cols for c in forms.classes] == [[0, 1], [2], [3], [4, 5, 6]]
    assert forms.F == sum(len(c.cols) * c.r for c in forms.classes) == forms.comp.numel()
    f0 = 0
    for c in forms.classes:                                                        # class-major, dense, in column order
        assert c.f0 == f0 and c.f1 == f0 + len(c.cols) * c.r
        assert forms.comp[c.f0:c.f1].tolist() == [j for j in c.cols for _ in range(c.r)]
        assert abs(c.h - max(float(KAPPA * half[j]) for j in c.cols) * (1.0 + 2.0 ** -20)) <= 1e-15 * c.h
        f0 = c.f1
    counts = torch.bincount(forms.comp, minlength=J)
    assert counts.tolist() == [forms.classes[g_].r for g_ in forms.cls]             # a partition: every column r_g features
    ranks = [(c.p, c.r) for c in forms.classes]
    assert ranks == sorted(ranks, reverse=True) and ranks[0] > ranks[-1]            # narrower classes need fewer terms
    assert (forms.p, forms.r) == ranks[0]
    tail = sum(float(w[c.cols].sum()) * c.tail for c in forms.classes) / float(w.sum())
    assert abs(forms.tail - tail) <= 1e-15 * tail
    assert torch.equal(forms.col_scale, (0.9 * w).sqrt())
    # all-equal half-widths: one class, F = J r
    one, _ = column_forms(_Be, Z, -half[:1].expand(J), half[:1].expand(J), w, 0.9, 0.05)
    assert len(one.classes) == 1 and one.F == J * one.classes[0].r and one.classes[0].cols == list(range(J))
    assert forms.F < one.F


# ---- served ----------------------------------------------------------------------------------------------------------------
def _step(model, lik, mll, X, y, on, posterior=False):
    from rpgp_amd import settings
    for p in _params(model, lik):
        p.grad = None
    model.train()
    with settings.lowrank_mll(on):
        out = model(X)
        val = mll(out, y)
        val.backward()
    return val.detach().clone(), [p.grad.detach().clone() for p in _params(model, lik)], out.covariance


def test_weighted_model_is_served(oracle_backend, monkeypatch):
    """Fails without the feature: a FamilyAdditiveOperator is then never served."""
    model, lik, mll, X, y = _model()
    v_bare, g_bare, _ = _step(model, lik, mll, X, y, False)                       # a backend without the feature kernels
    calls = []
    _install(oracle_backend, monkeypatch, calls)
    v_off, g_off, op = _step(model, lik, mll, X, y, False)
    assert not calls and not op.lowrank_mll_served                                # (never asked: the setting is off)
    assert torch.equal(v_off, v_bare) and all(torch.equal(a, b) for a, b in zip(g_off, g_bare))
    v_on, g_on, op = _step(model, lik, mll, X, y, True)
    assert op.lowrank_mll_served and op.lowrank_mll_reason is None
    fm = op.lowrank_mll_form()
    assert len(fm.class_ranks) >= 2 and sum(nc for _, _, nc in fm.class_ranks) == 5
    assert fm.ranks == (max(p for p, _, _ in fm.class_ranks), max(r for _, r, _ in fm.class_ranks),
                        sum(r * nc for _, r, nc in fm.class_ranks))
    assert calls.count("features") == len(fm.class_ranks) == calls.count("grad")   # one launch per class each way
    # the forward ran in the features mode
    from rpgp_amd.inv_quad_logdet import InvQuadLogDet

    class _Ctx:
        needs_input_grad = (False,) * 6
    ctx = _Ctx()
    from rpgp_amd import settings
    with settings.lowrank_mll(True), torch.no_grad():
        InvQuadLogDet.forward(ctx, op.Z1, op.outputscale, lik.noise.reshape(()), y - 0.2, op, op.comp_weights)
    assert ctx.mode == "features"
    assert abs(float(v_on) - float(v_off)) <= 1e-6 * abs(float(v_off))


# ---- value and gradients ---------------------------------------------------------------------------------------------------
def test_value_and_gradients_against_float64_autograd_and_the_dense_kernel(oracle_backend, monkeypatch):
    _install(oracle_backend, monkeypatch)
    model, lik, mll, X, y = _model()
    ref, gref, forms = _feature_reference(model, lik, X, y, oracle_backend)
    assert len(forms.classes) >= 2 and forms.F < X.shape[0]
    val, grads, op = _step(model, lik, mll, X, y, True)
    assert op.lowrank_mll_served and op.lowrank_mll_form().ranks[2] == forms.F
    print("value rel %.3g" % (abs(float(val) - ref) / abs(ref)))
    for name, g, gr in zip(NAMES, grads, gref):
        print("%s rel %.3g" % (name, _rel(g, gr)))
    assert abs(float(val) - ref) <= 1e-9 * abs(ref), (float(val), ref)
    for name, g, gr in zip(NAMES, grads, gref):
        assert g.shape == gr.shape and _rel(g, gr) <= 1e-9, (name, g, gr)
    assert grads[2].numel() == 5                                                   # every component weight
    # the dense float64 kernel: a per-entry tail eps = tail_tolerance(N, s sum w, sigma^2) moves Khat by at most
    # N s sum_c w_c eps <= 1e-6 sigma^2 in the 2-norm (lowrank_posterior.REL_ACCURACY), i.e. the value by 1e-6 relative; the
    # gradients are held to 1e-5 relative (the bounds of the unweighted model's comparison with the dense oracle)
    dref, dgref = _dense_reference(model, lik, X, y)
    assert abs(float(val) - dref) <= 1e-6 * abs(dref), (float(val), dref)
    for name, g, gr in zip(NAMES, grads, dgref):
        print("dense %s rel %.3g" % (name, _rel(g, gr)))
        assert _rel(g, gr) <= 1e-5, (name, g, gr)


# ---- reasons ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case, kwargs, reason", [
    ("zero weight", dict(), "a component weight is not positive"),
    ("Matern", dict(kernel_type="Matern"), "not a plain symmetric additive-RP RBF operator"),
    ("group 2", dict(k=2, J=3), "not a plain symmetric additive-RP RBF operator"),
    ("mixed groups", dict(degrees=[1, 2, 1]), "not a plain symmetric additive-RP RBF operator"),
    ("rank above the cap", dict(lengthscales=[0.02, 1.0, 1.5, 2.0, 4.0]), "needs a Chebyshev rank above 64"),
])
def test_reasons_and_todays_step(oracle_backend, monkeypatch, case, kwargs, reason):
    from rpgp_amd.operators import FamilyAdditiveOperator, MixedGroupOperator
    calls = []
    _install(oracle_backend, monkeypatch, calls)
    model, lik, mll, X, y = _model(**kwargs)
    if case == "zero weight":
        model.covar_module.base_kernel.raw_outputscales.data[1] = -800.0           # softplus(-800) is exactly 0 in float64
        assert float(model.covar_module.base_kernel.outputscales[1].detach()) == 0.0
    v_off, g_off, _ = _step(model, lik, mll, X, y, False)
    v_on, g_on, op = _step(model, lik, mll, X, y, True)
    assert isinstance(op, MixedGroupOperator if case == "mixed groups" else FamilyAdditiveOperator)
    assert not op.lowrank_mll_served and reason in op.lowrank_mll_reason, op.lowrank_mll_reason
    if case == "rank above the cap":
        hmax = KAPPA * 0.5 * float((op.Z1.max(0).values - op.Z1.min(0).values).max())
        assert hmax > 7.3 and ("%.3g" % (hmax * (1.0 + 2.0 ** -20))) in op.lowrank_mll_reason
    assert "grad" not in calls and (case == "rank above the cap" or not calls)
    assert torch.equal(v_on, v_off)
    for a, b in zip(g_on, g_off):
        assert torch.equal(a, b)


def test_size_reasons(oracle_backend, monkeypatch):
    from rpgp_amd import lowrank_posterior, settings
    from rpgp_amd.operators import FamilyAdditiveOperator
    _install(oracle_backend, monkeypatch)
    g = torch.Generator().manual_seed(1)
    Z = torch.randn(400, 6, generator=g, dtype=torch.float64) / _spread(6, 8.0)
    w = torch.full((6,), 1.0 / 6, dtype=torch.float64)

    def op_of(Z, w=w):
        op = FamilyAdditiveOperator(Z, None, torch.tensor(1.0, dtype=torch.float64), w, "RBF", 1)
        op._noise_host = 0.1
        return op
    with settings.lowrank_mll(True):
        op = op_of(Z)
        fm = op.lowrank_mll_form()
        assert fm is not None and op.lowrank_mll_form(0.5) is fm                   # decided once per operator
        F_ = fm.ranks[2]
        op = op_of(Z[:24])                                                         # 6 columns of >= 4 features each
        assert op.lowrank_mll_form() is None and "F >= N" in op.lowrank_mll_reason, op.lowrank_mll_reason
        monkeypatch.setattr(lowrank_posterior, "MAX_FEATURES", F_ - 1)
        op = op_of(Z)
        assert op.lowrank_mll_form() is None and "features exceed %d" % (F_ - 1) in op.lowrank_mll_reason
        monkeypatch.undo()
        _install(oracle_backend, monkeypatch)
        op = op_of(torch.randn(3000, 65, generator=g, dtype=torch.float64), torch.full((65,), 1.0 / 65, dtype=torch.float64))
        assert op.lowrank_mll_form() is None and "J = 65" in op.lowrank_mll_reason
        op = FamilyAdditiveOperator(Z, Z[:50], torch.tensor(1.0, dtype=torch.float64), w, "RBF", 1)
        op._noise_host = 0.1
        assert op.lowrank_mll_form() is None and "rectangular" in op.lowrank_mll_reason


# ---- the posterior ---------------------------------------------------------------------------------------------------------
def _log_density(mean, cov, y):
    L = np.linalg.cholesky(cov)
    z = np.linalg.solve(L, y - mean)
    return -0.5 * z @ z - np.log(np.diag(L)).sum() - 0.5 * y.size * math.log(2.0 * math.pi)


def _nrel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def test_posterior_against_a_dense_float64_solve(oracle_backend, monkeypatch):
    from rpgp_amd import settings
    from rpgp_amd.lowrank_posterior import ColumnForms, LowrankPredictive
    calls = []
    _install(oracle_backend, monkeypatch, calls)
    model, lik, mll, X, y = _model()
    N = X.shape[0]
    g = torch.Generator().manual_seed(5)
    mix = torch.rand(41, N, generator=g, dtype=torch.float64)
    Xs = (mix / mix.sum(1, keepdim=True)) @ X                                      # convex combinations: inside every range
    ys = torch.sin(Xs).sum(1)
    _, Z, s, w, noise, c = _leaves(model, lik, X)
    _, Zs, _, _, _, _ = _leaves(model, lik, Xs)
    Z, Zs, s, w, sigma2, c = Z.detach(), Zs.detach(), float(s), w.detach().numpy(), float(noise), float(c)
    Zall = np.concatenate([Z.numpy(), Zs.numpy()])
    Kall = fmo.kernel_matrix(Zall, Zall, "RBF", 1, w, s)
    Khat = Kall[:N, :N] + sigma2 * np.eye(N)
    r = y.numpy() - c

    def dense(lo, hi):
        Kx = Kall[lo:hi, :N]
        sol = np.linalg.solve(Khat, Kx.T)
        return Kx @ np.linalg.solve(Khat, r) + c, Kall[lo:hi, lo:hi] - Kx @ sol
    model.eval()
    with settings.lowrank_posterior(True), torch.no_grad():
        out = model(Xs)
        st = model.prediction_strategy
        assert st.lowrank is not None, st.lowrank_fallback_reason
        post = st.lowrank
        assert isinstance(post.form, ColumnForms) and len(post.class_ranks) >= 2 and post.rebuilds == 0
        assert post.ranks[2] == sum(r_ * nc for _, r_, nc in post.class_ranks)
        assert isinstance(out, LowrankPredictive) and not out.covariance_materialized
        mean_ref, cov_ref = dense(N, N + 41)
        assert _nrel(out._mean64.numpy(), mean_ref) <= 1e-7
        assert _nrel(out._var64.numpy(), np.diag(cov_ref)) <= 1e-7
        lp = float(lik(out).log_prob(ys))
        lp_ref = _log_density(mean_ref, cov_ref + sigma2 * np.eye(41), ys.numpy())
        assert abs(lp - lp_ref) <= 1e-7 * abs(lp_ref), (lp, lp_ref)
        assert _nrel(out.covariance.double().numpy(), cov_ref) <= 1e-7
        tr = model(X)
        mtr_ref, ctr_ref = dense(0, N)
        assert _nrel(tr._mean64.numpy(), mtr_ref) <= 1e-7
        lp_tr = st.train_log_prob(y)
        lp_tr_ref = _log_density(mtr_ref, ctr_ref + sigma2 * np.eye(N), y.numpy())
        assert abs(lp_tr - lp_tr_ref) <= 1e-7 * abs(lp_tr_ref), (lp_tr, lp_tr_ref)
        Bm = torch.randn(N, 3, dtype=torch.float64, generator=g)
        assert _nrel(st.solve(Bm).numpy(), np.linalg.solve(Khat, Bm.numpy())) <= 1e-7
        # a test point outside one column's range: exactly one rebuild, on the union of the ranges
        assert post.rebuilds == 0
        i = int(Z[:, 0].abs().argmax())
        xo = torch.cat([Xs[:3], 1.5 * X[i:i + 1]])
        assert abs(float(1.5 * Z[i, 0])) > float(Z[:, 0].abs().max())
        out2 = model(xo)
        assert post.rebuilds == 1 and isinstance(out2, LowrankPredictive)
        Zo = np.concatenate([Z.numpy(), Zs[:3].numpy(), 1.5 * Z[i:i + 1].numpy()])
        Ko = fmo.kernel_matrix(Zo, Zo, "RBF", 1, w, s)
        mo = Ko[N:, :N] @ np.linalg.solve(Khat, r) + c
        vo = np.diag(Ko[N:, N:] - Ko[N:, :N] @ np.linalg.solve(Khat, Ko[N:, :N].T))
        assert _nrel(out2._mean64.numpy(), mo) <= 1e-7 and _nrel(out2._var64.numpy(), vo) <= 1e-7
        model(xo)
        model(Xs)
        assert post.rebuilds == 1                                                  # the wider interval now covers both


def test_refinement_keeps_to_the_plain_operator(oracle_backend):
    """The float64 twin of the weighted kernel is handed to the closed-form posterior only."""
    from rpgp_amd.operators import FamilyAdditiveOperator
    model, lik, mll, X, y = _model(dtype=torch.float32)
    sk = model.covar_module
    assert sk.float64_operator(X) is None
    op = sk.float64_operator(X, weighted=True)
    assert type(op) is FamilyAdditiveOperator and op.Z1.dtype == torch.float64 and op.comp_weights.dtype == torch.float64
    assert torch.equal(op.comp_weights, sk.base_kernel.outputscales.detach().double())
    for kw in (dict(kernel_type="Matern"), dict(k=2, J=3)):
        m2 = _model(dtype=torch.float32, **kw)[0]
        assert m2.covar_module.float64_operator(X, weighted=True) is None
