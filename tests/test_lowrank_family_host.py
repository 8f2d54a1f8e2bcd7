"""Host side of settings.lowrank_kernel for the weighted kinds (no GPU): under the CPU test double, which has no weighted
low-rank entries, the switch leaves a weighted model's step exactly as it is; with a stub backend that records its calls, a
FamilyAdditiveOperator decides its form once, describes itself as RPGP_OP_LOWRANK_FAMILY, sends the product and the derivative
to the weighted entries with its family's weights, asks for the tolerance of the kernel's diagonal mass scale * sum |w|, and
keeps today's calls under every condition that is not served."""
import pytest
import torch

from rpgp_amd import _lib, ops
from tests.oracle_backend import OracleBackend
from tests.test_lowrank_weighted_host import _model, _params


def test_weighted_step_is_unchanged_under_the_cpu_double(oracle_backend):
    """The test double has no weighted low-rank entry points: with the switch on, the step is the family sweep's, bit for bit."""
    from rpgp_amd import settings
    from rpgp_amd.operators import FamilyAdditiveOperator

    def step(on):
        model, lik, mll, X, y = _model(N=260, dtype=torch.float32)
        model.train()
        with settings.max_cholesky_size(0), settings.deterministic_probes(True), settings.min_preconditioning_size(100), \
                settings.lowrank_kernel(on):
            out = model(X)
            val = mll(out, y)
            val.backward()
        op = out.covariance
        assert type(op) is FamilyAdditiveOperator and not op.lowrank_served and op.lowrank_ranks is None
        return val.detach().clone(), [p.grad.detach().clone() for p in _params(model, lik)]

    v0, g0 = step(False)
    v1, g1 = step(True)
    assert torch.equal(v0, v1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    assert settings.lowrank_kernel.off()


# ---- a stub backend with the weighted entries ------------------------------------------------------------------------------
class _Prep:
    def __init__(self, Z):
        self.N, self.J = Z.shape
        self.fast_ok, self.buf = True, None


class _Plan:
    p, q, served, handle = 31, 33, True, 1234


class _Stub(OracleBackend):
    """The CPU double plus prepare / lowrank_train_plan / the weighted entries (answered by the family sweep of the double),
    every call recorded."""

    def __init__(self, plan=_Plan()):
        super().__init__()
        self.calls, self.plan = [], plan

    def count(self, name):
        return sum(1 for c in self.calls if c[0] == name)

    def make_family(self, kind, group, weights, product=False):
        fam = super().make_family(kind, group, weights, product)
        fam.weights = weights
        fam.generic = weights.dtype == torch.float64
        return fam

    def prepare(self, Z):
        self.calls.append(("prepare",))
        return _Prep(Z)

    def lowrank_train_plan(self, prep, scale, noise, mass=None):
        self.calls.append(("plan", scale, noise, mass))
        return self.plan

    def mvm_sym_lowrank_weighted(self, plan, prep, weights, V, scale, noise=0.0, j0=0, j1=None, out=None):
        self.calls.append(("mvm_weighted", plan, prep, weights, scale, noise))
        return OracleBackend.family_mvm_sym(self, self._fam(weights), self.Z, V, scale, noise)

    def bilinear_grad_lowrank_weighted(self, plan, weights, L, R, scale, j0=0, j1=None):
        self.calls.append(("grad_weighted", plan, weights, scale))
        return OracleBackend.family_bilinear_grad(self, self._fam(weights), self.Z, L, R, scale)

    def _fam(self, weights):
        return OracleBackend.make_family(self, "RBF", 1, weights)

    def family_mvm_sym(self, fam, Z, V, scale, noise=0.0):
        self.calls.append(("family_mvm_sym",))
        return super().family_mvm_sym(fam, Z, V, scale, noise)

    def family_bilinear_grad(self, fam, Z, L, R, scale):
        self.calls.append(("family_bilinear_grad",))
        return super().family_bilinear_grad(fam, Z, L, R, scale)

    def mbcg_solve(self, *a, **k):
        raise AssertionError("not called here")

    def make_operator_desc(self, kind, N, J, scale, noise, **kw):
        return dict(kw, kind=kind, N=N, J=J, scale=scale, noise=noise), None


@pytest.fixture
def stub():
    from rpgp_amd import backend
    st = _Stub()
    prev = backend.set_backend(st)
    yield st
    backend.set_backend(prev)


def _operator(st, N=40, J=5, dtype=torch.float32, seed=0, **kw):
    from rpgp_amd.operators import FamilyAdditiveOperator
    g = torch.Generator().manual_seed(seed)
    cols = J * kw.get("group", 1)
    Z = torch.randn(N, cols, generator=g).to(dtype)
    w = (torch.rand(J, generator=g) + 0.25).to(dtype)
    w[1] = -w[1]                                              # weights of any sign
    st.Z = Z
    op = FamilyAdditiveOperator(Z, outputscale=torch.tensor(0.8, dtype=dtype), comp_weights=w, **kw)
    V = torch.randn(N, 3, generator=g).to(dtype)
    return op, Z, w, V


def test_served_operator_goes_to_the_weighted_entries(stub):
    from rpgp_amd import settings
    op, Z, w, V = _operator(stub)
    noise = 0.3
    with settings.lowrank_kernel(False):
        op_off, _, _, _ = _operator(stub)
        assert op_off.lowrank_form(noise) is None and not op_off.lowrank_served
        ref = op_off._matmul(V, noise)
        gref = op_off._bilinear_derivative(V, V.flip(1))
        assert op_off.native_descriptor(noise)[0]["kind"] == _lib.RPGP_OP_FAMILY
        assert not stub.count("prepare") and not stub.count("plan") and not stub.count("mvm_weighted")
    stub.calls.clear()
    with settings.lowrank_kernel(True):
        assert not op.lowrank_served and op.lowrank_ranks is None                  # undecided
        plan = op.lowrank_form(noise)
        assert plan is stub.plan and op.lowrank_served and op.lowrank_ranks == (31, 33)
        out = op._matmul(V, noise)
        desc, _keep = op.native_descriptor(noise)
        gZ, gs, gw = op._bilinear_derivative(V, V.flip(1))
        assert op.lowrank_form() is plan and op.lowrank_form(0.7) is plan
    # decided once per instance, at the tolerance of the diagonal mass scale * sum |w|
    assert stub.count("prepare") == 1 and stub.count("plan") == 1
    _, scale, nz, mass = next(c for c in stub.calls if c[0] == "plan")
    assert scale == pytest.approx(0.8) and nz == noise
    assert mass == pytest.approx(0.8 * float(w.abs().sum()), rel=1e-6) and mass > 0.8 * abs(float(w.sum())) * 1.1
    # the product and the derivative: the weighted entries, with the family's weights, never the sweep
    assert not stub.count("family_mvm_sym") and not stub.count("family_bilinear_grad")
    m = next(c for c in stub.calls if c[0] == "mvm_weighted")
    assert m[1] is plan and m[2] is op._prep and m[3] is op.fam.weights and m[4] == pytest.approx(0.8) and m[5] == noise
    d = next(c for c in stub.calls if c[0] == "grad_weighted")
    assert d[1] is plan and d[2] is op.fam.weights and d[3] == pytest.approx(0.8)
    assert torch.equal(out, ref)
    # the descriptor: RPGP_OP_LOWRANK_FAMILY with the family and the plan attached
    assert _lib.RPGP_OP_LOWRANK_FAMILY == 8
    assert desc["kind"] == _lib.RPGP_OP_LOWRANK_FAMILY and desc["family"] is op.fam and desc["lowrank"] is plan
    assert (desc["N"], desc["J"], desc["noise"]) == (40, 5, noise)
    # _finish_grads: (gZ, gcomp) -> d/dZ, d/d outputscale = sum_c w_c gcomp_c, d/d w_c = scale gcomp_c
    gZ_raw, gcomp = OracleBackend.family_bilinear_grad(stub, stub._fam(w), Z, V, V.flip(1), op._scale)
    assert torch.equal(gZ, gZ_raw) and torch.equal(gZ, gref[0])
    assert torch.allclose(gs, (w * gcomp).sum()) and torch.allclose(gw, op._scale * gcomp)
    assert torch.equal(gs, gref[1]) and torch.equal(gw, gref[2])
    # once decided under the setting, the operator keeps its form
    stub.calls.clear()
    assert torch.equal(op._matmul(V, noise), ref) and stub.count("mvm_weighted") == 1 and not stub.count("family_mvm_sym")


@pytest.mark.parametrize("case", ["float64", "group 2", "Matern", "product form", "J = 65", "no noise", "zero noise",
                                  "plan not served", "no weighted entries"])
def test_not_served_keeps_todays_calls(stub, monkeypatch, case):
    from rpgp_amd import settings
    kw, noise = {}, 0.3
    if case == "float64":
        kw = dict(dtype=torch.float64)
    elif case == "group 2":
        kw = dict(group=2)
    elif case == "Matern":
        kw = dict(kind="Matern")
    elif case == "product form":
        kw = dict(kind="Matern", group=2, product=True)
    elif case == "J = 65":
        kw = dict(J=65)
    elif case == "no noise":
        noise = None
    elif case == "zero noise":
        noise = 0.0
    elif case == "plan not served":
        stub.plan = None
    elif case == "no weighted entries":
        monkeypatch.delattr(_Stub, "bilinear_grad_lowrank_weighted")
    op, Z, w, V = _operator(stub, **kw)
    if case == "product form":
        assert op.product
    with settings.lowrank_kernel(True):
        assert op.lowrank_form(noise) is None and not op.lowrank_served and op.lowrank_ranks is None
        nz = noise or 0.0
        op._matmul(V, nz)
        desc = op.native_descriptor(nz)
        op._bilinear_derivative(V, V.flip(1))
    assert stub.count("plan") == (1 if case == "plan not served" else 0)
    assert not stub.count("mvm_weighted") and not stub.count("grad_weighted")
    assert stub.count("family_mvm_sym") == 1 and stub.count("family_bilinear_grad") == 1
    if case == "float64":
        assert desc is None                                    # (the runtime-(kind, group) kernels: the Python path, as today)
    else:
        assert desc[0]["kind"] == _lib.RPGP_OP_FAMILY and desc[0]["family"] is op.fam


def test_the_plan_tolerance_follows_the_diagonal_mass(monkeypatch):
    """ops.lowrank_train_plan(prep, scale, noise, mass=scale * sum |w|) builds its plan at lowrank_train_tol(N, 1, mass, noise)."""
    made = []

    class _FakePlan:
        served = True

        def __init__(self, prep, tol):
            self.tol = float(tol)
            made.append(self.tol)

    class _P:
        N, J, fast_ok = 200000, 20, True

    monkeypatch.setattr(ops, "LowrankTrainPlan", _FakePlan)
    monkeypatch.delenv("RPGP_LOWRANK", raising=False)
    monkeypatch.delenv("RPGP_FACT_ASM", raising=False)
    scale, noise, wabs = 0.9, 0.02, 3.7
    a = ops.lowrank_train_plan(_P(), scale, noise, mass=scale * wabs)
    assert a.tol == ops.lowrank_train_tol(200000, 1, scale * wabs, noise) == pytest.approx(1e-3 * noise / (scale * wabs * 200000))
    b = ops.lowrank_train_plan(_P(), scale, noise)
    assert b.tol == ops.lowrank_train_tol(200000, 20, scale, noise) and b.tol != a.tol
    assert made == [a.tol, b.tol]
    assert ops.lowrank_train_plan(_P(), scale, 0.0, mass=scale * wabs) is None     # no noise: no tolerance, not served
