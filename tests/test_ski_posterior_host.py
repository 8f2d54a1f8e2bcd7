"""The closed-form posterior of the grid-interpolation models on the host (no GPU): the algebra against the dense posterior of
the same one-grid kernel, the derived bounds of the two row kernels with a mutation self-test of both checkers, and the host stack
(settings.ski_posterior, PredictionStrategy, the runner) through a CPU test double."""
import json

import numpy as np
import pytest
import torch

from tests import ski_posterior_reference as R
from tests.oracle_backend import OracleBackend


@pytest.mark.parametrize("k", range(len(R.CASES)))
def test_closed_form_equals_the_dense_posterior(k):
    data = R.case_data(k)
    diffs = R.compare(R.closed_form(*data), R.dense(*data))
    print(R.CASES[k], diffs)
    assert max(diffs.values()) <= R.TOL, diffs


# ---- the bounds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G, g0, h", [(16, -1.3, 0.21), (64, -3.0, 0.1), (1024, -5.01, 0.00987), (1024, 1000.0, 3.3e-4)])
def test_weight_bound_against_longdouble(G, g0, h):
    from oracle import ski as sko
    rng = np.random.default_rng(G)
    z = g0 + h * rng.uniform(-1.0, G + 1.0, 4000)                 # beyond both ends as well: |u| <= G + 1
    z = np.concatenate([z, g0 + h * np.arange(1, G - 2)])        # rows on the nodes (as close as float64 puts them)
    idx0, w = R.weights_longdouble(z, g0, h, G)
    W_ld = np.zeros((z.size, G), dtype=np.longdouble)
    for q in range(4):
        W_ld[np.arange(z.size), idx0 + q] += w[:, q]
    u = (z.astype(np.longdouble) - np.longdouble(g0)) / np.longdouble(h)
    away = np.abs(u - (G - 2)) > 1e-9                            # (the rule's one discontinuity: module docstring)
    err = np.abs(sko.interp_matrix(z, g0, h, G).astype(np.longdouble) - W_ld)[away].max()
    print("G = %d: worst weight error %.3g, bound %.3g" % (G, float(err), R.weight_bound(G)))
    assert float(err) <= R.weight_bound(G)


def _small_problem(seed=0, N=300, J=3, G=16, T=2):
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-1.0, 1.0, (N, J))
    h = 2.0 / (G - 5)
    Z[:7, 0] = 1.0 + h * rng.uniform(0.2, 0.8, 7)                # rows inside the last cell of projection 0 (first tap G - 4)
    gp = R.block(-1.0 - 2.0 * h, h, J)
    Y = rng.standard_normal((N, T))
    C = rng.standard_normal((J * G, J * G))
    return Z, gp, G, Y, C


def test_checkers_accept_the_restatement_and_reject_mutations():
    from oracle import ski as sko
    Z, gp, G, Y, C = _small_problem()
    N, J = Z.shape
    A, g = R.gram(Z, gp, G, Y)
    q = R.quadform(Z, gp, G, C)
    assert R.check_gram(A, g, Z, gp, G, Y) == (0.0, 0.0) and R.check_quadform(q, Z, gp, G, C) == 0.0
    # (a perturbation of a few ulps of every weight stays inside)
    g0, h, _, _ = R.parse_block(gp, J)
    W = R.interp(Z, g0, h, G).toarray() * (1.0 + 4.0 * R.EPS)
    ra, rg = R.check_gram(W.T @ W, W.T @ Y, Z, gp, G, Y)
    assert ra <= 1.0 and rg <= 1.0, (ra, rg)
    assert R.check_quadform(((W @ C) * W).sum(1), Z, gp, G, C) <= 1.0
    W = R.interp(Z, g0, h, G).toarray()

    # a tap dropped in the last cell
    Wm = W.copy()
    last = np.nonzero(R.first_taps(Z, g0, h, G)[:, 0] == R.first_taps(Z, g0, h, G)[:, 0].max())[0]
    Wm[last, R.first_taps(Z, g0, h, G)[last, 0] + 2] = 0.0
    ra, rg = R.check_gram(Wm.T @ Wm, Wm.T @ Y, Z, gp, G, Y)
    assert ra > 1.0 and rg > 1.0, (ra, rg)
    assert R.check_quadform(((Wm @ C) * Wm).sum(1), Z, gp, G, C) > 1.0
    # one row skipped
    ra, rg = R.check_gram(W[1:].T @ W[1:], W[1:].T @ Y[1:], Z, gp, G, Y)
    assert ra > 1.0 and rg > 1.0, (ra, rg)
    qm = q.copy()
    qm[N // 2] = 0.0
    assert R.check_quadform(qm, Z, gp, G, C) > 1.0
    # the lower triangle not mirrored
    Am = A.copy()
    Am[G:, :G] = 0.0
    assert R.check_gram(Am, g, Z, gp, G, Y)[0] > 1.0
    # C read from one triangle without doubling
    assert R.check_quadform(((W @ np.triu(C)) * W).sum(1), Z, gp, G, C) > 1.0
    # ... while one triangle doubled is the same sum for a symmetric C
    Cs = C + C.T
    q_tri = ((W @ (2.0 * np.triu(Cs, 1) + np.diag(np.diag(Cs)))) * W).sum(1)
    assert R.check_quadform(q_tri, Z, gp, G, Cs) <= 1.0


# ---- the host stack through a test double ---------------------------------------------------------------------------------------
class SkiSumsBackend(OracleBackend):
    """The oracle backend plus the two row passes, from the reference module."""
    name = "oracle-cpu with SKI Gram sums (tests only)"

    def ski_gram(self, Z, gp, Y=None, grid_size=1024):
        A, g = R.gram(Z.double().numpy(), gp.double().numpy(), grid_size, None if Y is None else Y.double().numpy())
        return torch.from_numpy(A), (None if g is None else torch.from_numpy(g))

    def ski_quadform(self, Z, gp, C, grid_size=1024):
        return torch.from_numpy(R.quadform(Z.double().numpy(), gp.double().numpy(), grid_size, C.double().numpy()))


@pytest.fixture
def ski_backend():
    from rpgp_amd import backend
    be = SkiSumsBackend()
    prev = backend.set_backend(be)
    yield be
    backend.set_backend(prev)


def _model(N=300, M=40, d=4, J=3, G=64, noise=0.05, s=1.3, seed=0, kind="additive_rp", **extra):
    from rpgp_amd.models import ExactMarginalLogLikelihood
    from rpgp_amd.training import create_exact_gp
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g)
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
    Xs = 1.3 * torch.randn(M, d, generator=g)
    ys = torch.sin(Xs).sum(1)
    kw = dict(J=J, ski=True, ski_options={"grid_size": G, "num_dims": 1}, noise_prior=True)
    kw.update({"prescale": True} if kind == "additive_rp" else {"k": 1})
    kw.update(extra)
    model, lik = create_exact_gp(X, y, kind, **kw)
    lik.noise = noise
    model.covar_module.outputscale = s
    model.mean_module.constant.data.fill_(0.2)
    return model, lik, ExactMarginalLogLikelihood(lik, model), X, y, Xs, ys


def _dense_reference(post, y, Xs, ys):
    st = post.state
    return R.dense(post.Z.numpy(), y.double().numpy(), post._test_coordinates(Xs).numpy(), ys.double().numpy(), st.gp.numpy(),
                   post.G, post.scale, post.noise, post.c)


@pytest.mark.parametrize("kind, extra", [("additive_rp", {}), ("additive_rp", {"kernel_type": "Matern"}),
                                         ("rp_poly", {"weighted": True, "init_mixin_range": (0.5, 1.5)})])
def test_host_stack_serves_the_closed_form(ski_backend, kind, extra):
    from rpgp_amd import settings
    from rpgp_amd.ski_posterior import SKIPredictive
    model, lik, mll, X, y, Xs, ys = _model(kind=kind, **extra)
    model.eval()
    with settings.ski_posterior(True), torch.no_grad():
        out = model(Xs)
        st = model.prediction_strategy
        post = st.ski_post
        assert post is not None, st.ski_posterior_reason
        assert isinstance(out, SKIPredictive) and not out.covariance_materialized
        before = post.rebuilds                                     # (1 when the test rows reach beyond the training range)
        ref = _dense_reference(post, y, Xs, ys)
        lp = float(lik(out).log_prob(ys.double()))
        assert not out.covariance_materialized
        tr = model(X)
        got = dict(mean=out._mean64.numpy(), var=out._var64.numpy(), lp=lp, mean_train=tr._mean64.numpy(),
                   lp_train=st.train_log_prob(y), cov=None)
        diffs = R.compare(got, ref)
        assert max(diffs.values()) <= R.TOL, diffs
        nll = -mll(out, ys.double()).item()
        assert abs(nll + (ref["lp"] + lik.log_prior().item()) / Xs.shape[0]) <= 1e-6 * max(1.0, abs(nll))
        nll_tr = -mll(tr, y.double()).item()
        assert abs(nll_tr + (ref["lp_train"] + lik.log_prior().item()) / X.shape[0]) <= 1e-6 * max(1.0, abs(nll_tr))
        assert np.abs(out.covariance.double().numpy() - ref["cov"]).max() <= 1e-5 * ref["prior_diag_scale"]       # (float32 result)
        assert np.abs(st.alpha64.reshape(-1).numpy() - ref["alpha"]).max() <= 1e-7 * np.abs(ref["alpha"]).max()
        with settings.skip_posterior_variances(True):
            m_only = model(Xs)
            assert float(m_only.variance.abs().max()) == 0.0
            assert np.abs(m_only.mean.double().numpy() - ref["mean"]).max() <= 1e-5 * max(1.0, np.abs(ref["mean"]).max())
        # a prediction inside the block does not rebuild; one whose rows fall outside it rebuilds once, on the union
        model(0.5 * Xs)
        assert post.rebuilds == before
        wide = model(4.0 * Xs)
        assert post.rebuilds == before + 1 and post.state is not out._state and torch.isfinite(wide._var64).all()
        model(4.0 * Xs)
        model(Xs)
        assert post.rebuilds == before + 1


def test_setting_off_takes_todays_branch(ski_backend):
    from rpgp_amd import settings
    from rpgp_amd.ski_posterior import SKIPredictive
    model, lik, mll, X, y, Xs, ys = _model()
    model.eval()
    with torch.no_grad():
        out = model(Xs)
    st = model.prediction_strategy
    assert st.ski_post is None and st.ski_posterior_reason is None and hasattr(st, "dense_path")
    assert not isinstance(out, SKIPredictive)
    assert not settings.ski_posterior.on() and settings.ski_posterior_max_nodes.value() == 24576


def test_not_served_reasons(ski_backend, monkeypatch):
    from rpgp_amd import backend, settings, ski_posterior
    from rpgp_amd.models import PredictionStrategy
    from rpgp_amd.ski_posterior import SKIPosterior

    def strategy(**kw):
        model = _model(**kw)[0]
        model.eval()
        with settings.ski_posterior(True):
            return PredictionStrategy(model)

    # over the node cap: the strategy falls back to today's state and still predicts
    model, lik, mll, X, y, Xs, ys = _model()
    model.eval()
    with settings.ski_posterior(True), settings.ski_posterior_max_nodes(100), torch.no_grad():
        out = model(Xs)
    st = model.prediction_strategy
    assert st.ski_post is None and "nodes exceed 100" in st.ski_posterior_reason and hasattr(st, "dense_path")
    assert torch.isfinite(out.mean).all()
    # as many kept eigenpairs as rows (Matern: full rank, 2 x 64 against 100 rows)
    st = strategy(N=100, J=2, kernel_type="Matern")
    assert st.ski_post is None and "features for 100 rows" in st.ski_posterior_reason
    # more than MAX_FEATURES
    monkeypatch.setattr(ski_posterior, "MAX_FEATURES", 10)
    st = strategy()
    assert st.ski_post is None and "features exceed 10" in st.ski_posterior_reason
    monkeypatch.undo()
    # the remaining conditions on a strategy that is served
    st = strategy()
    assert st.ski_post is not None
    st.op.row_shard = object()
    assert SKIPosterior.build(st) == (None, "sharded model")
    st.op.row_shard = None
    st.model.covar_module.shard = type("S", (), {"world_size": 2})()
    assert SKIPosterior.build(st) == (None, "sharded model")
    st.model.covar_module.shard = None
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2)
    assert SKIPosterior.build(st) == (None, "a world larger than 1")
    monkeypatch.undo()
    st.op.comp_weights = torch.tensor([1.0, -0.5, 1.0])
    assert SKIPosterior.build(st) == (None, "a component weight is negative")
    st.op.comp_weights = None
    noise = st.noise
    st.noise = torch.tensor(-1e6)
    assert SKIPosterior.build(st) == (None, "sigma^2 I + S^T A S is not positive definite")
    st.noise = noise
    # host tensors with the HIP backend (refused before any device call), and a backend without the two calls
    hip = type("HostHip", (backend.HipBackend,), {})()
    backend.set_backend(hip)
    assert SKIPosterior.build(st) == (None, "host tensors")
    backend.set_backend(OracleBackend())
    assert SKIPosterior.build(st) == (None, "the backend has no SKI Gram sums")
    backend.set_backend(ski_backend)
    assert SKIPosterior.build(st)[0] is not None


def test_runner_flag_and_metric(ski_backend, tmp_path, monkeypatch):
    from rpgp_amd import runner, specs
    monkeypatch.setitem(runner.SYNTHETIC_SHAPES, "ski400", (400, 3))
    spec = specs.get("additive_spread_prescale_Jd_ski.json")
    spec["train_kwargs"]["max_iter"] = 2
    spec["train_kwargs"]["init_iters"] = 1
    spec["model_kwargs"]["ski_options"]["grid_size"] = 64
    spec["model_kwargs"]["space_proj"] = False
    sp = tmp_path / "spec.json"
    json.dump(spec, open(sp, "w"))
    rows = {}
    for flags in ([], ["--ski_posterior"], ["--ski_posterior", "--ski_posterior_max_nodes", "100"]):
        torch.manual_seed(0)
        np.random.seed(0)
        df = runner.main(["-m", str(sp), "-d", "synthetic:ski400", "-o", str(tmp_path / ("r%d.csv" % len(flags))), "--no_cv",
                          "--skip_random_restart"] + flags)
        assert "error" not in df.columns, df
        rows[len(flags)] = df.iloc[0]
    assert "ski_posterior_served" not in rows[0].index
    assert int(rows[1]["ski_posterior_served"]) == 1 and int(rows[3]["ski_posterior_served"]) == 0
    for r in rows.values():
        assert np.isfinite(float(r["test_nll"])) and np.isfinite(float(r["rmse"]))
    # one grid in closed form against three grids: the same model, close but not equal
    assert abs(float(rows[1]["rmse"]) - float(rows[0]["rmse"])) <= 0.05 * float(rows[0]["rmse"]) + 1e-3
