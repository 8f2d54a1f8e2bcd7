"""The weighted rp_poly kinds through the Chebyshev low-rank product kernels (settings.lowrank_kernel on a
FamilyAdditiveOperator, RBF, k = 1): rpgp_mvm_sym_lowrank_weighted and rpgp_bilinear_grad_lowrank_weighted against the float64
oracle (oracle.family) and the family sweep over ragged sizes and product / derivative ranks that are small, mid-range and at
the edge of the served range; w = 1 bit for bit against the unweighted entries; a zero and a negative weight; j-ranges; run-to-run
bit identity; a plan without a derivative rank; RPGP_OP_LOWRANK_FAMILY in the native mBCG executor against a float64 dense
solve; a C2-sized fit with the setting on against off; and the switch back to the sweep when one projection's range leaves the
served ranks."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import family as fmo

pytestmark = pytest.mark.gpu

KAPPA = 0.8493218002880191        # the coordinate scale of rpgp_prepare: a = (z - mid) kappa
TAIL = 2.0 ** -26
SCALE = 0.7


def _product_rank(h):
    from rpgp_amd import _lib
    p = ctypes.c_int(0)
    _lib.load().rpgp_lowrank_select(float(h) * (1.0 + 2.0 ** -20), 64, ctypes.byref(p), None, None)
    return p.value


_HW = {}


def _half_width(kind, lo, hi):
    """A half-width h whose product rank (kind "p") or derivative rank (kind "q", the product rank served as well) lies in
    [lo, hi]."""
    from rpgp_amd import ops
    if (kind, lo, hi) not in _HW:
        for h in np.arange(0.2, 12.0, 0.01):
            p = _product_rank(h)
            r = p if kind == "p" else ops.lowrank_grad_select(h, 64)[0]
            if p > 0 and lo <= r <= hi:
                _HW[(kind, lo, hi)] = float(h)
                break
        else:
            raise AssertionError("no half-width with %s in [%d, %d]" % (kind, lo, hi))
    return _HW[(kind, lo, hi)]


def _inputs(N, J, T, h, dev, seed):
    """Z with every column spanning [-w, w] (w = h / kappa: the plan's half-width is h, rows 0 and 1 at +-w), L and R standard
    normal (L doubles as the product's V)."""
    g = torch.Generator().manual_seed(seed)
    w = h / KAPPA
    Z = (torch.rand(N, J, generator=g) * 2.0 - 1.0) * w
    Z[0] = w
    if N > 1:
        Z[1] = -w
    L = torch.randn(N, T, generator=g)
    R = torch.randn(N, T, generator=g)
    return Z.to(dev), L.to(dev), R.to(dev)


def _weights(J, dev):
    """Positive and spread 16 x: w_j = 0.05 + 2^(-4 j / max(J - 1, 1))."""
    return torch.tensor([0.05 + 2.0 ** (-4.0 * j / max(J - 1, 1)) for j in range(J)], dtype=torch.float32, device=dev)


def _plan(Z, tol=TAIL):
    from rpgp_amd import ops
    prep = ops.Prepared(Z)
    assert prep.fast_ok
    return prep, ops.LowrankTrainPlan(prep, tol)


def _np(t):
    return t.double().cpu().numpy()


def _rel(a, ref):
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


# ---- the product ------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (63, 5, 7), (2049, 16, 64), (4613, 11, 7), (2048, 11, 20)]
P_RANGES = [(1, 12), (30, 45), (63, 64)]
# (one point is a constant kernel, rank 1 whatever the half-width asked for: it runs once)
PRODUCT_CASES = [(N, T, J, pr) for (N, T, J) in SHAPES for pr in P_RANGES if N > 1 or pr == P_RANGES[0]]


@pytest.mark.parametrize("N,T,J,pr", PRODUCT_CASES)
def test_product_matches_the_float64_oracle_and_the_sweep(gpu_device, N, T, J, pr):
    from rpgp_amd import ops
    h = _half_width("p", *pr)
    Z, V, _ = _inputs(N, J, T, h, gpu_device, seed=N + 7 * T + J)
    w = _weights(J, gpu_device)
    prep, plan = _plan(Z)
    if N == 1:
        assert plan.p == 1
    else:
        assert pr[0] <= plan.p <= pr[1], plan.p
    fam = ops.Family("RBF", 1, w)
    kv = fmo.mvm(_np(Z), _np(Z), _np(V), "RBF", 1, _np(w), SCALE)
    for noise in (0.0, 0.3):
        ref = kv + noise * _np(V)
        out = ops.mvm_sym_lowrank_weighted(plan, prep, w, V, SCALE, noise)
        sweep = ops.family_mvm_sym(fam, Z, V, SCALE, noise)
        e_lr, e_sw, e_x = _rel(_np(out), ref), _rel(_np(sweep), ref), _rel(_np(out), _np(sweep))
        print("N %d T %d J %d p %d noise %.1f: oracle %.2e (sweep %.2e), against the sweep %.2e"
              % (N, T, J, plan.p, noise, e_lr, e_sw, e_x))
        assert e_lr <= 5e-7, (e_lr, plan.p)
        assert e_x <= 2e-6, (e_x, plan.p)
        if N > 1:                    # (one point: both paths add the same J products, nothing tells them apart)
            assert not torch.equal(out, sweep)               # really the other path


# ---- the derivative ---------------------------------------------------------------------------------------------------------
GRAD_CASES = [  # (N, T, J, q range): tests/test_lowrank_grad_gpu.py::CASES
    (1, 1, 1, (1, 12)),
    (63, 5, 7, (1, 12)),
    (2048, 11, 20, (30, 45)),
    (2048, 16, 64, (1, 12)),
    (4613, 11, 7, (30, 45)),
    (2048, 11, 20, (63, 64)),
    (4613, 1, 7, (63, 64)),
]


@pytest.mark.parametrize("N,T,J,qr", GRAD_CASES)
def test_derivative_matches_the_float64_oracle_and_the_sweep(gpu_device, N, T, J, qr):
    from rpgp_amd import ops
    h = _half_width("q", *qr)
    Z, L, R = _inputs(N, J, T, h, gpu_device, seed=N + 7 * T + J)
    w = _weights(J, gpu_device)
    prep, plan = _plan(Z)
    gZ_ref, gc_ref = fmo.bilinear_grad(_np(Z), _np(L), _np(R), "RBF", 1, _np(w), SCALE)
    if N == 1:                       # one point: a constant kernel (h = 0, p = q = 1), the derivative is exactly zero
        assert plan.served and plan.p == 1 and plan.q == 1
        gZ, gc = ops.bilinear_grad_lowrank_weighted(plan, w, L, R, SCALE)
        assert float(gZ.abs().max()) == 0.0
        assert _rel(_np(gc), gc_ref) <= 1e-6
        return
    assert plan.served and qr[0] <= plan.q <= qr[1], (plan.p, plan.q)
    gZ, gc = ops.bilinear_grad_lowrank_weighted(plan, w, L, R, SCALE)
    g = _np(gZ)
    rel = _rel(g, gZ_ref)
    rows = float(np.linalg.norm(g - gZ_ref, axis=1).max() / np.linalg.norm(gZ_ref, axis=1).max())
    rel_c = _rel(_np(gc), gc_ref)
    sZ, sc = ops.family_bilinear_grad(ops.Family("RBF", 1, w), Z, L, R, SCALE)
    rel_sweep, rel_c_sweep = _rel(_np(sZ), gZ_ref), _rel(_np(sc), gc_ref)
    print("N %d T %d J %d p %d q %d: gZ %.2e (sweep %.2e) rows %.2e gcomp %.2e (sweep %.2e)"
          % (N, T, J, plan.p, plan.q, rel, rel_sweep, rows, rel_c, rel_c_sweep))
    assert rel <= 2e-6, (rel, plan.p, plan.q)
    assert rows <= 1e-5, (rows, plan.p, plan.q)
    if plan.q < 63:
        assert rel_c <= 1e-6, (rel_c, plan.p, plan.q)
    else:                            # the edge of the served range: the bounds of tests/test_lowrank_grad_gpu.py there
        assert rel <= 1.25 * rel_sweep + 1e-8, (rel, rel_sweep)
        assert rel_c <= 4e-6, (rel_c, rel_c_sweep)


# ---- w = 1: the bits of the unweighted entries ------------------------------------------------------------------------------
def _raw_unweighted_product(plan, prep, V, scale, noise):
    from rpgp_amd import _lib, ops
    lib = _lib.load()
    N, J, T = plan.N, plan.J, V.shape[1]
    out = torch.empty_like(V)
    ws = torch.empty(max(int(lib.rpgp_mvm_sym_lowrank_workspace_bytes(plan.handle, N, T)), 1), dtype=torch.uint8,
                     device=V.device)
    rc = lib.rpgp_mvm_sym_lowrank_range(plan.handle, prep.buf.data_ptr(), V.data_ptr(), out.data_ptr(), N, J, T, 0, J, 1, 0,
                                        float(scale), float(noise), ws.data_ptr(), ws.numel(), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    return out


@pytest.mark.parametrize("N,J", [(65, 7), (2049, 20)])
@pytest.mark.parametrize("T", [1, 11])
def test_unit_weights_are_bit_equal_to_the_unweighted_entries(gpu_device, N, J, T):
    from rpgp_amd import ops
    Z, L, R = _inputs(N, J, T, _half_width("q", 30, 45), gpu_device, seed=N + T)
    prep, plan = _plan(Z)
    ones = torch.ones(J, device=gpu_device)
    for noise in (0.0, 0.3):
        assert torch.equal(ops.mvm_sym_lowrank_weighted(plan, prep, ones, L, SCALE, noise),
                           _raw_unweighted_product(plan, prep, L, SCALE, noise))
    assert prep.rank == plan.p
    assert torch.equal(ops.mvm_sym_lowrank_weighted(plan, prep, ones, L, SCALE, 0.3),
                       ops.mvm_sym_prepared(prep, L, SCALE, 0.3))
    gZ, gc = ops.bilinear_grad_lowrank_weighted(plan, ones, L, R, SCALE)
    uZ, gs = ops.bilinear_grad_lowrank(plan, L, R, SCALE)
    assert torch.equal(gZ, uZ)
    assert abs(float(gc.double().sum()) - gs.item()) <= 1e-6 * abs(gs.item())


# ---- weights of any sign ----------------------------------------------------------------------------------------------------
def test_a_zero_and_a_negative_weight(gpu_device):
    from rpgp_amd import ops
    N, J, T = 777, 20, 11
    Z, L, R = _inputs(N, J, T, _half_width("q", 30, 45), gpu_device, seed=21)
    w = _weights(J, gpu_device)
    w[3], w[5] = 0.0, -0.2
    prep, plan = _plan(Z)
    Zh, Lh, Rh, wh = _np(Z), _np(L), _np(R), _np(w)
    ref = fmo.mvm(Zh, Zh, Lh, "RBF", 1, wh, SCALE, 0.3)
    ref_abs = fmo.mvm(Zh, Zh, Lh, "RBF", 1, np.abs(wh), SCALE, 0.3)
    out = _np(ops.mvm_sym_lowrank_weighted(plan, prep, w, L, SCALE, 0.3))
    gZ_ref, gc_ref = fmo.bilinear_grad(Zh, Lh, Rh, "RBF", 1, wh, SCALE)
    gZ_abs, _ = fmo.bilinear_grad(Zh, Lh, Rh, "RBF", 1, np.abs(wh), SCALE)
    gZ, gc = ops.bilinear_grad_lowrank_weighted(plan, w, L, R, SCALE)
    e_p = float(np.linalg.norm(out - ref) / np.linalg.norm(ref_abs))
    e_g = float(np.linalg.norm(_np(gZ) - gZ_ref) / np.linalg.norm(gZ_abs))
    print("zero / negative weight: product %.2e, gZ %.2e, gcomp %.2e (relative to the result for |w|)"
          % (e_p, e_g, _rel(_np(gc), gc_ref)))
    assert e_p <= 5e-7 and e_g <= 2e-6, (e_p, e_g)
    assert float(gZ[:, 3].abs().max()) == 0.0
    assert float(gZ[:, 5].abs().max()) > 0.0
    # the component sums do not carry the weights: entry 3 is there, within the whole vector's gate
    assert _rel(_np(gc), gc_ref) <= 1e-6
    assert gc[3].item() != 0.0 and abs(gc[3].item() - gc_ref[3]) <= 1e-6 * np.linalg.norm(gc_ref)


# ---- j-ranges ---------------------------------------------------------------------------------------------------------------
def _raw_grad(plan, w, L, R, gZ, gc, j0, j1, scale):
    from rpgp_amd import _lib, ops
    lib = _lib.load()
    N, J, T = plan.N, plan.J, L.shape[1]
    nbytes = lib.rpgp_bilinear_grad_lowrank_workspace_bytes(plan.handle, N, T)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=L.device)
    rc = lib.rpgp_bilinear_grad_lowrank_weighted(plan.handle, w.data_ptr(), L.data_ptr(), R.data_ptr(), gZ.data_ptr(),
                                                 gc.data_ptr(), N, J, T, j0, j1, float(scale), ws.data_ptr(), ws.numel(),
                                                 ops._stream())
    torch.cuda.synchronize()
    return rc


def test_j_ranges_leave_the_rest_untouched_and_sum_to_the_whole(gpu_device):
    from rpgp_amd import ops
    N, J, T = 777, 20, 11
    Z, L, R = _inputs(N, J, T, _half_width("q", 30, 45), gpu_device, seed=3)
    w = _weights(J, gpu_device)
    prep, plan = _plan(Z)
    full, gc_full = ops.bilinear_grad_lowrank_weighted(plan, w, L, R, 1.3)
    whole = ops.mvm_sym_lowrank_weighted(plan, prep, w, L, 1.3, 0.0)
    parts = torch.zeros_like(whole, dtype=torch.float64)
    for j0, j1 in ((0, 5), (5, 6), (6, 20)):
        gZ = torch.full((N, J), float("nan"), device=gpu_device)
        gc = torch.full((J,), float("nan"), device=gpu_device)
        assert _raw_grad(plan, w, L, R, gZ, gc, j0, j1, 1.3) == 0
        assert torch.isnan(gZ[:, :j0]).all() and torch.isnan(gZ[:, j1:]).all()
        assert torch.isnan(gc[:j0]).all() and torch.isnan(gc[j1:]).all()
        assert torch.equal(gZ[:, j0:j1], full[:, j0:j1]) and torch.equal(gc[j0:j1], gc_full[j0:j1])
        # the ops entry zeroes what the range leaves out
        oZ, oc = ops.bilinear_grad_lowrank_weighted(plan, w, L, R, 1.3, j0=j0, j1=j1)
        assert torch.equal(oZ[:, j0:j1], full[:, j0:j1]) and float(oZ[:, :j0].abs().sum() + oZ[:, j1:].abs().sum()) == 0.0
        assert float(oc[:j0].abs().sum() + oc[j1:].abs().sum()) == 0.0
        parts += ops.mvm_sym_lowrank_weighted(plan, prep, w, L, 1.3, 0.0, j0=j0, j1=j1).double()
    assert _rel(_np(parts), _np(whole)) <= 2e-6


def test_repeated_calls_are_bit_identical(gpu_device):
    from rpgp_amd import ops
    Z, L, R = _inputs(5000, 20, 11, _half_width("q", 30, 45), gpu_device, seed=11)
    w = _weights(20, gpu_device)
    prep, plan = _plan(Z)
    a = ops.mvm_sym_lowrank_weighted(plan, prep, w, L, 0.9, 0.1)
    b = ops.mvm_sym_lowrank_weighted(plan, prep, w, L, 0.9, 0.1)
    assert torch.equal(a, b)
    c = ops.bilinear_grad_lowrank_weighted(plan, w, L, R, 0.9)
    d = ops.bilinear_grad_lowrank_weighted(plan, w, L, R, 0.9)
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])


def test_weights_are_checked_before_any_launch(gpu_device):
    from rpgp_amd import ops
    Z, L, R = _inputs(300, 4, 3, 2.0, gpu_device, seed=5)
    prep, plan = _plan(Z)
    good = _weights(4, gpu_device)
    for bad in (good[:3], torch.cat([good, good]), good.double(), good.cpu(), [1.0, 1.0, 1.0, 1.0]):
        with pytest.raises(ValueError):
            ops.mvm_sym_lowrank_weighted(plan, prep, bad, L, 1.0)
        with pytest.raises(ValueError):
            ops.bilinear_grad_lowrank_weighted(plan, bad, L, R, 1.0)


def test_plan_without_a_derivative_rank_answers_the_error_code(gpu_device):
    from rpgp_amd import _lib, ops, settings
    from rpgp_amd.operators import FamilyAdditiveOperator
    h = next(float(h) for h in np.arange(7.0, 12.0, 0.02)
             if ops.lowrank_grad_select(h, 64)[0] == 0 and _product_rank(h) > 0)
    Z, L, R = _inputs(300, 4, 3, h, gpu_device, seed=5)
    w = _weights(4, gpu_device)
    prep, plan = _plan(Z)
    assert plan.p > 0 and plan.q == 0 and not plan.served
    gZ = torch.zeros(300, 4, device=gpu_device)
    gc = torch.zeros(4, device=gpu_device)
    assert _raw_grad(plan, w, L, R, gZ, gc, 0, 4, 1.0) == _lib.RPGP_EINVAL
    assert float(gZ.abs().max()) == 0.0 and float(gc.abs().max()) == 0.0
    with pytest.raises(ValueError):
        ops.bilinear_grad_lowrank_weighted(plan, w, L, R, 1.0)
    with settings.lowrank_kernel(True):
        op = FamilyAdditiveOperator(Z, outputscale=torch.tensor(1.0, device=gpu_device), comp_weights=w)
        assert op.lowrank_form(1.0) is None and not op.lowrank_served and op.lowrank_ranks is None
        desc, _keep = op.native_descriptor(1.0)
        assert desc.kind == _lib.RPGP_OP_FAMILY


# ---- the native executor ----------------------------------------------------------------------------------------------------
def test_lowrank_family_operator_in_the_native_executor(gpu_device):
    from rpgp_amd import settings, linear_cg as lcg
    from rpgp_amd.operators import FamilyAdditiveOperator, AddedDiagOperator
    from rpgp_amd.precond import pivoted_cholesky, WoodburyPreconditioner
    N, J, T, noise, s, tol = 4613, 7, 11, 0.3, 0.8, 1e-4
    g = torch.Generator().manual_seed(4)
    Z = (torch.randn(N, J, generator=g) * 1.5).to(gpu_device)
    rhs = torch.randn(N, T, generator=g).to(gpu_device)
    w = _weights(J, gpu_device)
    out, its = {}, {}
    for on in (False, True):
        op = FamilyAdditiveOperator(Z, outputscale=torch.tensor(s, device=gpu_device), comp_weights=w)
        khat = AddedDiagOperator(op, torch.tensor(noise, device=gpu_device), noise_value=noise)
        pre = WoodburyPreconditioner(pivoted_cholesky(op._diagonal(), op._get_rows, 15), noise)
        with settings.lowrank_kernel(on):
            before = lcg.stats.get("native_calls", 0)
            out[on] = lcg.linear_cg(khat._matmul, rhs, operator=khat, tolerance=tol, max_iter=500, preconditioner=pre)
            assert lcg.stats.get("native_calls", 0) == before + 1
            its[on] = lcg.stats["last_iterations"]
        assert op.lowrank_served == on
        if on:
            print("executor: ranks", op.lowrank_ranks, "iterations on / off", its[True], its[False])
    Zd = _np(Z)
    Kh = fmo.kernel_matrix(Zd, Zd, "RBF", 1, _np(w), s) + noise * np.eye(N)
    b = _np(rhs)
    x_ref = np.linalg.solve(Kh, b)
    xd = _np(out[True])
    res = np.linalg.norm(Kh @ xd - b, axis=0) / np.linalg.norm(b, axis=0)
    assert res.mean() < 2.0 * tol, res
    assert np.linalg.norm(xd - x_ref) / np.linalg.norm(x_ref) < 100.0 * tol
    assert abs(its[True] - its[False]) <= max(2, int(0.1 * its[False])), its


# ---- fits -------------------------------------------------------------------------------------------------------------------
def _record_forms(monkeypatch):
    """Every decision of FamilyAdditiveOperator.lowrank_form: (served, (p, q) or None)."""
    from rpgp_amd import operators
    seen = []
    orig = operators.FamilyAdditiveOperator.lowrank_form

    def rec(self, noise=None):
        undecided = self._lowrank is None
        r = orig(self, noise)
        if undecided:
            seen.append((r is not None, (r.p, r.q) if r is not None else None))
        return r
    monkeypatch.setattr(operators.FamilyAdditiveOperator, "lowrank_form", rec)
    return seen


def _model(dev, N, d=8, J=20, kernel_type="RBF", h=3.0, noise=0.05, s=0.9, seed=0):
    """The weighted rp_poly model (k = 1) as tests/test_lowrank_weighted_gpu.py::_model builds it: lengthscales spread 8 x over
    the projections, scaled by one factor so that the widest projected column has the half-width h (plan units)."""
    import math
    from rpgp_amd.kernels import PolynomialProjectionKernel, ScaleKernel, inv_softplus
    from rpgp_amd.likelihoods import GaussianLikelihood, SmoothedBoxPrior
    from rpgp_amd.models import ExactGPModel, ExactMarginalLogLikelihood
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g, dtype=torch.float64)
    P = torch.randn(d, J, generator=g, dtype=torch.float64) / math.sqrt(d)
    ls = torch.tensor([0.5 * 2.0 ** (3.0 * j / max(J - 1, 1)) for j in range(J)], dtype=torch.float64)
    w = torch.rand(J, generator=g, dtype=torch.float64) + 0.5
    w = w / w.sum()
    Zc = (X @ P) / ls
    h0 = KAPPA * float(((Zc.max(0).values - Zc.min(0).values) * 0.5).max())
    ls = ls * (h0 / h)
    X, P = X.float(), P.float()
    g = torch.Generator().manual_seed(11)
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
    y = (y - y.mean()) / y.std()
    kern = PolynomialProjectionKernel(J, 1, d, kernel_type, [P[:, j:j + 1].clone() for j in range(J)], weighted=True)
    kern.raw_lengthscales.data = inv_softplus(ls).reshape(1, -1).float()
    kern.raw_outputscales.data = inv_softplus(w).float()
    sk = ScaleKernel(kern)
    sk.outputscale = s
    lik = GaussianLikelihood(noise_prior=SmoothedBoxPrior(1e-4, 10, sigma=0.01))
    lik.noise = noise
    model = ExactGPModel(X.to(dev), y.to(dev), lik, sk).to(dev)
    return model, lik, ExactMarginalLogLikelihood(lik, model), X.to(dev), y.to(dev)


NAMES = ("raw_lengthscales", "raw_outputscale", "raw_outputscales", "raw_noise", "mean")


def _params(model, lik):
    kern = model.covar_module.base_kernel
    return [kern.raw_lengthscales, model.covar_module.raw_outputscale, kern.raw_outputscales, lik.raw_noise,
            model.mean_module.constant]


def _grad_rel(a, b):
    """Relative 2-norm distance of two gradients (all raw parameters as one vector)."""
    a = torch.cat([t.reshape(-1) for t in a]).double()
    b = torch.cat([t.reshape(-1) for t in b]).double()
    return float((a - b).norm() / b.norm())


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


class _Settings:
    def __init__(self):
        from rpgp_amd import settings
        self.cms = [settings.deterministic_probes(True), settings.cg_tolerance(1e-3), settings.max_cg_iterations(2000)]

    def __enter__(self):
        for c in self.cms:
            c.__enter__()

    def __exit__(self, *a):
        for c in reversed(self.cms):
            c.__exit__(*a)


def test_c2_sized_fit_on_against_off(gpu_device, monkeypatch):
    from rpgp_amd.training import make_optimizer
    seen = _record_forms(monkeypatch)
    N = 7372
    losses = {}
    with _Settings():
        model, lik, mll, X, y = _model(gpu_device, N)
        seen.clear()
        v, grads = _step(model, lik, mll, X, y, True)
        assert seen and seen[0][0], seen
        v_off, g_off = _step(model, lik, mll, X, y, False)
        print("first step: value on %.8f off %.8f" % (v, v_off))
        assert abs(v - v_off) <= 1e-4 * abs(v_off), (v, v_off)
        # The gate is tests/test_lowrank_train_gpu.py's: the relative 2-norm distance of the two gradients with all raw parameters
        # as one vector.  Parameter by parameter (printed for the record) the two steps are as far apart as the solver's own
        # tolerance allows: at cg_tolerance 1e-3 the solves stop after 28 (on) and 29 (off) iterations and the lengthscales' /
        # outputscale's / weights' / mean's gradients differ by 1.0e-3 / 4.6e-4 / 1.5e-3 / 4.9e-3 (the mean's is a cancelling sum
        # of size 6e-5 beside the noise's 0.73); at 1e-5 both stop after 48 and they differ by 3.1e-5 / 5.3e-5 / 9.8e-5 / 1.1e-4.
        for name, a, b in zip(NAMES, grads, g_off):
            print("first step: gradient of %s on against off %.2e"
                  % (name, float((a.double() - b.double()).norm() / b.double().norm())))
        rel = _grad_rel(grads, g_off)
        print("first step: all raw parameters as one vector %.2e" % rel)
        assert rel <= 1e-3, rel
        for on in (False, True):
            model, lik, mll, X, y = _model(gpu_device, N)
            opt = make_optimizer(torch.optim.Adam, _params(model, lik), 0.02)
            seen.clear()
            losses[on] = [_step(model, lik, mll, X, y, on, opt)[0] for _ in range(20)]
            if on:
                assert len(seen) == 20 and all(s for s, _ in seen), seen
                print("ranks per step:", [pq for _, pq in seen])
            else:
                assert not any(s for s, _ in seen), seen
    for a, b in zip(losses[True], losses[False]):
        assert abs(a - b) <= 1e-4 * abs(b), (losses[True], losses[False])


def test_matern_model_is_the_settings_off_step_bit_for_bit(gpu_device):
    def step(on):
        model, lik, mll, X, y = _model(gpu_device, 1500, kernel_type="Matern")
        with _Settings():
            return _step(model, lik, mll, X, y, on)

    v0, g0 = step(False)
    v1, g1 = step(True)
    assert v0 == v1
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


def test_switches_to_the_sweep_once_when_a_rank_leaves_the_served_range(gpu_device, monkeypatch):
    """The lengthscale of ONE projection driven down: its column sets the shared half-width, and when p or q passes 64 the
    operator is the family sweep again."""
    from rpgp_amd.kernels import inv_softplus
    seen = _record_forms(monkeypatch)
    served, pairs = [], []
    with _Settings():
        model, lik, mll, X, y = _model(gpu_device, 3000, d=4, J=8, h=2.0, seed=2)
        kern = model.covar_module.base_kernel
        with torch.no_grad():
            Z = (X.double() @ kern.projection_module.weight.double().t())[:, 0]
            half0 = KAPPA * float((Z.max() - Z.min()) * 0.5)              # projection 0's half-width at lengthscale 1
        h = 2.0
        for k in range(12):
            with torch.no_grad():
                ls = torch.nn.functional.softplus(kern.raw_lengthscales.detach().double()).reshape(-1)
                ls[0] = half0 / h
                kern.raw_lengthscales.data = inv_softplus(ls).reshape(1, -1).float()
            seen.clear()
            v_on, _ = _step(model, lik, mll, X, y, True)
            served.append(seen[0][0])
            ranks = seen[0][1]
            v_off, _ = _step(model, lik, mll, X, y, False)
            pairs.append((v_on, v_off))
            print("half-width %.2f: served %s ranks %s, value on %.8f off %.8f" % (h, served[-1], ranks, v_on, v_off))
            h /= 0.75
    switches = sum(1 for a, b in zip(served, served[1:]) if a != b)
    assert served[0] and not served[-1] and switches == 1, served
    k = served.index(False)
    for v_on, v_off in (pairs[k - 1], pairs[k]):          # both sides of the switch
        assert abs(v_on - v_off) <= 1e-4 * abs(v_off), pairs
