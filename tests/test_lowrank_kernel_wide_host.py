"""Host side of settings.lowrank_kernel with a rank cap above 64 (no GPU): the cap entries' argument checks and sizes
(rpgp_lowrank_plan_bytes_cap, rpgp_lowrank_create_cap, rpgp_lowrank_grad_bytes); lowrank_form passes no max_rank at the default
cap and passes the cap above it (a CPU double defined here, next to a double with today's four-argument lowrank_train_plan); the
plan cached on a Prepared is keyed on (tolerance, cap); a non-finite max_abs is never served; and the ranks the degree-128
selection gives at half-widths 8, 10, 12 and 13 at the product's and at a training tolerance."""
import ctypes

import pytest
import torch

from rpgp_amd import _lib, ops
from tests.oracle_backend import OracleBackend


# ---- the C ABI: sizes and argument checks (none of these reaches the device) --------------------------------------------------
def test_plan_bytes_by_cap():
    lib = _lib.load()
    N, J = 1000, 7
    base = lib.rpgp_lowrank_plan_bytes(N, J)
    assert base == (64 * 64 + N * J) * 4
    for cap in (1, 8, 63, 64):                               # up to 64: the existing creators' layout
        assert lib.rpgp_lowrank_plan_bytes_cap(N, J, cap) == base
    for cap, ld in ((65, 72), (72, 72), (73, 80), (100, 104), (121, 128), (128, 128)):
        assert lib.rpgp_lowrank_plan_bytes_cap(N, J, cap) == (ld * ld + N * J) * 4
    for cap in (0, -1, 129, 1 << 20):
        assert lib.rpgp_lowrank_plan_bytes_cap(N, J, cap) == 0
    assert lib.rpgp_lowrank_plan_bytes_cap(0, J, 128) == 0
    assert lib.rpgp_lowrank_plan_bytes_cap(N, 0, 128) == 0
    assert lib.rpgp_lowrank_plan_bytes_cap(N, 65, 128) == 0


def test_create_cap_checks_its_arguments_before_the_device():
    lib = _lib.load()
    p, h = ctypes.c_int(-7), ctypes.c_void_p(None)
    buf = (ctypes.c_char * 64)()
    addr = ctypes.addressof(buf)
    for cap in (0, -3, 129, 4096):
        rc = lib.rpgp_lowrank_create_cap(addr, 100, 4, 1.0, 1e-8, cap, addr, 1 << 30, ctypes.byref(p), ctypes.byref(h), None)
        assert rc == _lib.RPGP_EINVAL and p.value == -7 and h.value is None
    for tol in (0.0, -1.0, float("nan")):
        rc = lib.rpgp_lowrank_create_cap(addr, 100, 4, 1.0, tol, 128, addr, 1 << 30, ctypes.byref(p), ctypes.byref(h), None)
        assert rc == _lib.RPGP_EINVAL and h.value is None
    # a plan buffer sized for rank 64 is too small for the cap 128; null pointers and sizes outside the limits
    small = lib.rpgp_lowrank_plan_bytes(100, 4)
    assert lib.rpgp_lowrank_create_cap(addr, 100, 4, 1.0, 1e-8, 128, addr, small, ctypes.byref(p), ctypes.byref(h),
                                       None) == _lib.RPGP_EWORKSPACE
    assert lib.rpgp_lowrank_create_cap(None, 100, 4, 1.0, 1e-8, 128, addr, 1 << 30, ctypes.byref(p), ctypes.byref(h),
                                       None) == _lib.RPGP_EINVAL
    assert lib.rpgp_lowrank_create_cap(addr, 100, 65, 1.0, 1e-8, 128, addr, 1 << 30, ctypes.byref(p), ctypes.byref(h),
                                       None) == _lib.RPGP_EINVAL
    assert h.value is None


def test_grad_bytes_of_no_handle_and_the_version():
    lib = _lib.load()
    assert lib.rpgp_lowrank_grad_bytes(None) == 0
    assert _lib.RPGP_LOWRANK_GRAD_BYTES == 65536 == 2 * 64 * 64 * 8
    assert lib.rpgp_version() == 4 == _lib.RPGP_ABI_VERSION


# ---- the ranks of the degree-128 selection above the old cap ------------------------------------------------------------------
TAIL = 2.0 ** -26
TRAIN_TOL = 1e-3 * 0.05 / (1.0 * 50000)                     # lowrank_train_tol at N = 50 000, scale J = 1, noise 0.05: 1e-9


def _p(h, tol, cap=128):
    """The plan's rank: rpgp_lowrank_create_cap selects at h (1 + 2^-20) and min(tol, 2^-26)."""
    lib = _lib.load()
    if tol >= TAIL:
        p = ctypes.c_int(0)
        assert lib.rpgp_lowrank_select(h * (1.0 + 2.0 ** -20), cap, ctypes.byref(p), None, None) == 0
        return p.value
    return ops.lowrank_post_select(h * (1.0 + 2.0 ** -20), tol, p_max=cap)[0]


def _q(h, tol, cap=128):
    return ops.lowrank_grad_select(h * (1.0 + 2.0 ** -20), cap, tol)[0]


# (p, q) at the product's tolerance 2^-26 and at TRAIN_TOL, from a numpy restatement of the selection (the DCT-II coefficients of
# the function at the 128 x 128 Chebyshev points, the antisymmetric part for the derivative, the shell sums and the smallest
# rank whose tail plus the allowance is within the tolerance)
RANKS = {8.0: ((59, 62), (64, 67)), 10.0: ((73, 76), (78, 82)), 12.0: ((86, 90), (93, 97)), 13.0: ((93, 98), (100, 105))}


@pytest.mark.parametrize("h", sorted(RANKS))
def test_ranks_above_the_old_cap(h):
    got = ((_p(h, TAIL), _q(h, TAIL)), (_p(h, TRAIN_TOL), _q(h, TRAIN_TOL)))
    print("h = %g: (p, q) at 2^-26 %s, at %.1e %s" % (h, got[0], TRAIN_TOL, got[1]))
    assert got == RANKS[h]
    # the cap is a cap: one below the rank is not served, the rank itself is, and the old cap serves no rank above 64
    for tol, (p, q) in zip((TAIL, TRAIN_TOL), got):
        assert _p(h, tol, p) == p and _q(h, tol, q) == q
        assert _p(h, tol, p - 1) == 0 and _q(h, tol, q - 1) == 0
        assert _q(h, tol, 64) == (q if q <= 64 else 0) and _p(h, tol, 64) == (p if p <= 64 else 0)


def test_selection_limits():
    # the degree-128 reference resolves the product's function up to h = 14 and the derivative's (one more factor x - y) up
    # to h = 13: a training step, which needs both, is served up to a half-width of about 13
    assert _p(14.0, TAIL) > 0 and _q(13.0, TAIL) > 0 and _q(14.0, TAIL) == 0
    assert _p(15.0, TAIL) == 0 and _q(15.0, TAIL) == 0
    for bad in (float("nan"), float("inf"), -1.0):
        assert _p(bad, TAIL) == 0 and _q(bad, TAIL) == 0


# ---- ops.lowrank_train_plan: the cap, the cache key, what is served -----------------------------------------------------------
class _Prep:
    def __init__(self, fast_ok=True, max_abs=3.0, buf=object()):
        self.N, self.J, self.fast_ok, self.max_abs, self.buf, self.device = 5000, 8, fast_ok, max_abs, buf, "cpu"


@pytest.fixture
def fake_plans(monkeypatch):
    made = []

    class _FakePlan:
        served = True

        def __init__(self, prep, tol, *rest):
            self.tol = float(tol)
            self.max_rank = rest[0] if rest else 64
            made.append((self.tol,) + tuple(rest))

    monkeypatch.setattr(ops, "LowrankTrainPlan", _FakePlan)
    monkeypatch.delenv("RPGP_LOWRANK", raising=False)
    monkeypatch.delenv("RPGP_FACT_ASM", raising=False)
    return made


def test_the_cached_plan_is_keyed_on_tolerance_and_cap(fake_plans):
    prep = _Prep()
    tol = ops.lowrank_train_tol(5000, 8, 0.9, 0.05)
    a = ops.lowrank_train_plan(prep, 0.9, 0.05)
    assert fake_plans == [(tol,)]                            # the default: today's two-argument construction
    assert ops.lowrank_train_plan(prep, 0.9, 0.05) is a and ops.lowrank_train_plan(prep, 0.9, 0.05, max_rank=64) is a
    b = ops.lowrank_train_plan(prep, 0.9, 0.05, max_rank=128)
    assert b is not a and fake_plans == [(tol,), (tol, 128)]
    assert ops.lowrank_train_plan(prep, 0.9, 0.05, max_rank=128) is b and len(fake_plans) == 2
    c = ops.lowrank_train_plan(prep, 0.9, 0.05, max_rank=96)
    assert c is not b and fake_plans[-1] == (tol, 96)
    d = ops.lowrank_train_plan(prep, 0.9, 0.01, max_rank=96)
    assert d is not c and fake_plans[-1] == (ops.lowrank_train_tol(5000, 8, 0.9, 0.01), 96)
    e = ops.lowrank_train_plan(prep, 0.9, 0.01)
    assert e is not d and fake_plans[-1] == (ops.lowrank_train_tol(5000, 8, 0.9, 0.01),) and len(fake_plans) == 5
    tm = ops.lowrank_train_tol(5000, 1, 2.5, 0.05)
    assert ops.lowrank_train_plan(prep, 0.9, 0.05, mass=2.5, max_rank=128).tol == tm and fake_plans[-1] == (tm, 128)


def test_what_is_served_beyond_fast_ok(fake_plans):
    wide = _Prep(fast_ok=False, max_abs=12.0)
    assert ops.lowrank_train_plan(wide, 0.9, 0.05) is None                     # the default cap keeps the sweep's guard
    assert ops.lowrank_train_plan(wide, 0.9, 0.05, max_rank=64) is None and not fake_plans
    assert ops.lowrank_train_plan(wide, 0.9, 0.05, max_rank=128) is not None and len(fake_plans) == 1
    # a non-finite max_abs (a Z with a NaN or an Inf) and a Z without prepared coordinates (J > 64) are never served
    for bad in (float("nan"), float("inf"), -float("inf")):
        for ok in (False, True):
            assert ops.lowrank_train_plan(_Prep(fast_ok=ok, max_abs=bad), 0.9, 0.05, max_rank=128) is None
    assert ops.lowrank_train_plan(_Prep(fast_ok=False, buf=None), 0.9, 0.05, max_rank=128) is None
    assert ops.lowrank_train_plan(wide, 0.9, 0.0, max_rank=128) is None        # no noise: no tolerance
    assert len(fake_plans) == 1


def test_the_switches_win_over_the_cap(fake_plans, monkeypatch):
    monkeypatch.setenv("RPGP_LOWRANK", "0")
    assert ops.lowrank_train_plan(_Prep(), 0.9, 0.05, max_rank=128) is None and not fake_plans


def test_the_plan_class_takes_a_cap_and_checks_it():
    """Without the feature LowrankTrainPlan(prep, tol, max_rank=...) is a TypeError.  A non-finite max_abs returns before any
    device call: p = q = 0, no handle."""
    for bad in (0, 129, -5):
        with pytest.raises(ValueError):
            ops.LowrankTrainPlan(_Prep(), 1e-9, max_rank=bad)
    for mx in (float("nan"), float("inf")):
        plan = ops.LowrankTrainPlan(_Prep(fast_ok=False, max_abs=mx), 1e-9, max_rank=128)
        assert (plan.p, plan.q, plan.handle, plan.max_rank) == (0, 0, None, 128) and not plan.served
    plan = ops.LowrankTrainPlan(_Prep(fast_ok=False, buf=None), 1e-9, max_rank=100)
    assert not plan.served and plan.handle is None


# ---- lowrank_form: no max_rank at the default cap, the cap above it -------------------------------------------------------------
class _StubPrep:
    def __init__(self, Z, fast_ok):
        self.N, self.J = Z.shape
        self.fast_ok, self.buf, self.max_abs = fast_ok, None, 11.0


class _Plan:
    p, q, served, handle = 90, 93, True, 4321


class _TodaysStub(OracleBackend):
    """A double with today's signature, lowrank_train_plan(prep, scale, noise, mass=None): a max_rank passed at the default cap
    would be a TypeError here."""
    fast_ok = True

    def __init__(self):
        super().__init__()
        self.calls = []

    def make_family(self, kind, group, weights, product=False):
        fam = super().make_family(kind, group, weights, product)
        fam.weights = weights
        fam.generic = weights.dtype == torch.float64
        return fam

    def prepare(self, Z):
        return _StubPrep(Z, self.fast_ok)

    def lowrank_train_plan(self, prep, scale, noise, mass=None):
        self.calls.append({"mass": mass})
        return _Plan()

    def mvm_sym_lowrank_weighted(self, *a, **k):
        raise AssertionError("not called here")

    def bilinear_grad_lowrank_weighted(self, *a, **k):
        raise AssertionError("not called here")


class _CapStub(_TodaysStub):
    """The same double with the new keyword."""

    def lowrank_train_plan(self, prep, scale, noise, mass=None, **kw):
        self.calls.append(dict(kw, mass=mass))
        return _Plan()


def _operators(seed=0):
    from rpgp_amd.operators import AdditiveRPOperator, FamilyAdditiveOperator
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(30, 4, generator=g)
    w = torch.rand(4, generator=g) + 0.25
    s = torch.tensor(0.8)
    return AdditiveRPOperator(Z, None, s, 1.0), FamilyAdditiveOperator(Z, outputscale=s, comp_weights=w)


def _with_backend(st):
    from rpgp_amd import backend

    class _Ctx:
        def __enter__(self):
            self.prev = backend.set_backend(st)
            return st

        def __exit__(self, *a):
            backend.set_backend(self.prev)
    return _Ctx()


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "weighted"])
def test_lowrank_form_carries_the_cap_only_above_the_default(which):
    from rpgp_amd import settings
    with _with_backend(_TodaysStub()) as st, settings.lowrank_kernel(True):
        op = _operators()[which]
        assert op.lowrank_form(0.3) is not None and op.lowrank_ranks == (90, 93)
        assert len(st.calls) == 1 and set(st.calls[0]) == {"mass"}
        with settings.lowrank_max_rank(48):                   # at or below 64: nothing is passed either
            op = _operators()[which]
            assert op.lowrank_form(0.3) is not None and len(st.calls) == 2
    with _with_backend(_CapStub()) as st, settings.lowrank_kernel(True):
        op = _operators()[which]
        assert op.lowrank_form(0.3) is not None and st.calls == [{"mass": st.calls[0]["mass"]}]
        for cap in (65, 96, 128):
            with settings.lowrank_max_rank(cap):
                op = _operators()[which]
                assert op.lowrank_form(0.3) is not None and op.lowrank_served
                assert st.calls[-1]["max_rank"] == cap
                assert op.lowrank_form() is op.lowrank_form(0.9) and len(st.calls) == 1 + (65, 96, 128).index(cap) + 1
    assert settings.lowrank_max_rank.value() == 64 and settings.lowrank_kernel.off()


def test_weighted_form_beyond_fast_ok_asks_the_plan_only_above_the_default():
    """A Z that is not fast_ok: at the default cap the weighted operator does not ask for a plan at all (today's behaviour); above
    it the plan decides."""
    from rpgp_amd import settings
    st = _CapStub()
    st.fast_ok = False
    with _with_backend(st), settings.lowrank_kernel(True):
        op = _operators()[1]
        assert op.lowrank_form(0.3) is None and not st.calls
        with settings.lowrank_max_rank(128):
            op = _operators()[1]
            assert op.lowrank_form(0.3) is not None and st.calls[-1]["max_rank"] == 128


def test_runner_help_names_the_kernel_mode():
    from rpgp_amd import runner
    text = runner.build_parser().format_help()
    assert "--lowrank_max_rank" in text and "--lowrank_kernel /" in " ".join(text.split())
