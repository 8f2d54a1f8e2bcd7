"""Training and solving the exact additive-RP GP through the Chebyshev low-rank form (settings.lowrank_kernel):
RPGP_OP_LOWRANK in the native mBCG executor against a float64 dense solve; a C2-shaped fit with the switch on against the
same fit with it off (the sweep) and against the float64 oracle; the switch back to the sweep when the derivative rank
leaves the served range; and the first step of an N = 200 000 exact fit on against off."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _record_forms(monkeypatch):
    """Every decision of AdditiveRPOperator.lowrank_form: (served, (p, q) or None)."""
    from rpgp_amd import operators
    seen = []
    orig = operators.AdditiveRPOperator.lowrank_form

    def rec(self, noise=None):
        undecided = self._lowrank is None
        r = orig(self, noise)
        if undecided:
            seen.append((r is not None, (r.p, r.q) if r is not None else None))
        return r
    monkeypatch.setattr(operators.AdditiveRPOperator, "lowrank_form", rec)
    return seen


def test_lowrank_operator_in_the_native_executor(gpu_device):
    from rpgp_amd import settings, linear_cg as lcg
    from rpgp_amd.operators import AdditiveRPOperator, AddedDiagOperator
    from rpgp_amd.precond import pivoted_cholesky, WoodburyPreconditioner
    N, J, T, noise, s, tol = 4613, 7, 11, 0.3, 0.8, 1e-4
    g = torch.Generator().manual_seed(4)
    Z = (torch.randn(N, J, generator=g) * 1.5).to(gpu_device)
    rhs = torch.randn(N, T, generator=g).to(gpu_device)
    out, its = {}, {}
    for on in (False, True):
        op = AdditiveRPOperator(Z, outputscale=torch.tensor(s, device=gpu_device))
        khat = AddedDiagOperator(op, torch.tensor(noise, device=gpu_device), noise_value=noise)
        pre = WoodburyPreconditioner(pivoted_cholesky(op._diagonal(), op._get_rows, 15), noise)
        with settings.lowrank_kernel(on):
            before = lcg.stats.get("native_calls", 0)
            out[on] = lcg.linear_cg(khat._matmul, rhs, operator=khat, tolerance=tol, max_iter=500, preconditioner=pre)
            assert lcg.stats.get("native_calls", 0) == before + 1
            its[on] = lcg.stats["last_iterations"]
        assert op.lowrank_served == on
    Zd = Z.double().cpu().numpy()
    K = np.zeros((N, N))
    for j in range(J):
        d = Zd[:, j:j + 1] - Zd[:, j:j + 1].T
        K += np.exp(-0.5 * d * d)
    Kh = s * K + noise * np.eye(N)
    b = rhs.double().cpu().numpy()
    x_ref = np.linalg.solve(Kh, b)
    xd = out[True].double().cpu().numpy()
    res = np.linalg.norm(Kh @ xd - b, axis=0) / np.linalg.norm(b, axis=0)
    assert res.mean() < 2.0 * tol, res
    assert np.linalg.norm(xd - x_ref) / np.linalg.norm(x_ref) < 100.0 * tol
    assert abs(its[True] - its[False]) <= max(2, int(0.1 * its[False])), its


def _model(N, d, J, dev, seed=0, ls=None, h=None):
    from rpgp_amd.training import create_exact_gp
    from rpgp_amd.models import ExactMarginalLogLikelihood
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g)
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
    y = (y - y.mean()) / y.std()
    torch.manual_seed(seed)
    np.random.seed(seed)
    model, lik = create_exact_gp(X.to(dev), y.to(dev), "additive_rp", J=J, noise_prior=True, kernel_type="RBF",
                                 learn_proj=False, prescale=True, space_proj=False)
    model = model.to(dev)
    if ls is not None:
        model.covar_module.base_kernel.initialize(lengthscale=ls)
    if h is not None:
        _set_half_width(model, X.to(dev), h)
    return model, lik, ExactMarginalLogLikelihood(lik, model), X.to(dev), y.to(dev)


KAPPA = 0.8493218002880191


def _set_half_width(model, X, h):
    """Scale every lengthscale by one factor so that the widest projected column spans [mid - h / kappa, mid + h / kappa]:
    the half-width of the low-rank plan of the first step is h."""
    pk = model.covar_module.base_kernel
    with torch.no_grad():
        Z = pk.project(X) * (pk.base_kernel.input_scale_factor() or 1.0)
        h0 = KAPPA * float(((Z.max(0).values - Z.min(0).values) * 0.5).max())
        pk.initialize(lengthscale=pk.lengthscale.detach().reshape(-1) * (h0 / h))


def _grad_rel(a, b):
    """Relative 2-norm distance of two gradients (all raw parameters as one vector)."""
    a = torch.cat([t.reshape(-1) for t in a]).double()
    b = torch.cat([t.reshape(-1) for t in b]).double()
    return float((a - b).norm() / b.norm())


def _params(model, lik):
    return [p for p in model.parameters() if p.requires_grad]


def _step(model, lik, mll, X, y, on, opt=None):
    from rpgp_amd import settings
    with settings.lowrank_kernel(on):
        model.train()
        if opt is not None:
            opt.zero_grad()
        else:
            for p in _params(model, lik):
                p.grad = None
        loss = mll.negative(model(X), y)
        loss.backward()
        grads = [p.grad.detach().clone() for p in _params(model, lik)]
        if opt is not None:
            opt.step()
    return loss.item(), grads


def _settings():
    from rpgp_amd import settings
    return [settings.deterministic_probes(True), settings.cg_tolerance(1e-3), settings.max_cg_iterations(2000)]


class _Ctx:
    def __init__(self, cms):
        self.cms = cms

    def __enter__(self):
        for c in self.cms:
            c.__enter__()

    def __exit__(self, *a):
        for c in reversed(self.cms):
            c.__exit__(*a)


def test_c2_fit_on_against_off_and_the_oracle(gpu_device, monkeypatch):
    from oracle import dense_gp as orc
    from rpgp_amd.training import make_optimizer
    seen = _record_forms(monkeypatch)
    N, d, J = 7372, 8, 20
    losses = {}
    with _Ctx(_settings()):
        for on in (False, True):
            model, lik, mll, X, y = _model(N, d, J, gpu_device, h=3.0)
            if on:
                # first step: value and raw-parameter gradients against the float64 oracle (the CG-regime gates)
                seen.clear()
                v, grads = _step(model, lik, mll, X, y, True)
                assert seen and seen[0][0], seen
                bk = model.covar_module.base_kernel
                W = bk.projection_module.weight.detach().double().cpu().numpy()
                ref = orc.DenseExactGP(X.double().cpu().numpy(), y.double().cpu().numpy(), W.T,
                                       bk.lengthscale.detach().double().cpu().numpy().reshape(-1),
                                       float(model.covar_module.outputscale), float(lik.noise),
                                       mean=float(model.mean_module.constant))
                assert abs(-v - ref.mll()) <= 1e-2 * abs(ref.mll()), (v, ref.mll())
                v_off, g_off = _step(model, lik, mll, X, y, False)
                assert abs(v - v_off) <= 1e-4 * abs(v_off)
                assert _grad_rel(grads, g_off) <= 1e-3, (grads, g_off)
                model, lik, mll, X, y = _model(N, d, J, gpu_device, h=3.0)
            opt = make_optimizer(torch.optim.Adam, _params(model, lik), 0.02)
            seen.clear()
            losses[on] = [_step(model, lik, mll, X, y, on, opt)[0] for _ in range(20)]
            if on:
                assert len(seen) == 20 and all(s for s, _ in seen), seen
                print("C2 ranks per step:", [pq for _, pq in seen])
    for a, b in zip(losses[True], losses[False]):
        assert abs(a - b) <= 1e-4 * abs(b), (losses[True], losses[False])


def test_switches_to_the_sweep_once_when_q_leaves_the_served_range(gpu_device, monkeypatch):
    seen = _record_forms(monkeypatch)
    N, d, J = 3000, 4, 8
    served, pairs = [], []
    with _Ctx(_settings()):
        model, lik, mll, X, y = _model(N, d, J, gpu_device, seed=2)
        h = 2.0
        for k in range(12):                      # lengthscales driven down: the coordinate range widens every step
            _set_half_width(model, X, h)
            seen.clear()
            v_on, _ = _step(model, lik, mll, X, y, True)
            served.append(seen[0][0])
            v_off, _ = _step(model, lik, mll, X, y, False)
            pairs.append((v_on, v_off))
            h /= 0.75
    switches = sum(1 for a, b in zip(served, served[1:]) if a != b)
    assert served[0] and not served[-1] and switches == 1, served
    k = served.index(False)
    for v_on, v_off in (pairs[k - 1], pairs[k]):          # both sides of the switch
        assert abs(v_on - v_off) <= 1e-4 * abs(v_off), pairs


def test_first_step_at_200k_on_against_off(gpu_device, monkeypatch):
    from rpgp_amd import settings
    seen = _record_forms(monkeypatch)
    N, d, J = 200000, 20, 20
    out = {}
    with _Ctx(_settings() + [settings.cache_kernel(False)]):
        for on in (True, False):
            model, lik, mll, X, y = _model(N, d, J, gpu_device, seed=1, h=3.0)
            seen.clear()
            out[on] = _step(model, lik, mll, X, y, on)
            if on:
                assert seen and seen[0][0], seen
                print("N = 200 000 ranks:", seen[0][1])
            del model, lik, mll
    (v1, g1), (v0, g0) = out[True], out[False]
    assert abs(v1 - v0) <= 1e-4 * abs(v0), (v1, v0)
    assert _grad_rel(g1, g0) <= 1e-3, (g1, g0)
