"""Host side of the panel plans of the low-rank product kernels (no GPU): rpgp_lowrank_panels_select's panel count, ranks and
bounds at half-widths 7 ... 45; its four coefficient blocks evaluated in numpy against the float64 functions, panel edges
included, and the whole panelled kernel against the exact one on [-h, h]; and the operators' use of settings.lowrank_panels:
off, the backend's lowrank_train_plan is called without the keyword, as it is for a backend that does not take it."""
import numpy as np
import pytest
import torch

from rpgp_amd import ops
from tests.oracle_backend import OracleBackend

KAPPA = 0.8493218002880191        # the coordinate scale of rpgp_prepare: a = (z - mid) kappa
HALF_WIDTHS = (7.0, 13.5, 20.0, 45.0)
TOLS = (2.0 ** -26, 1e-12)
ROUND = 1e-14                     # rounding of the numpy evaluation itself (sums of <= 64 x 64 terms of size <= 1)


def _cheb(x, n):
    return np.cos(np.outer(np.arange(n), np.arccos(np.clip(x, -1.0, 1.0))))


def _f(d):
    return np.exp2(-d * d)


def _g(d):
    """-(z - z') e(z, z') in z units for the prepared difference d = a - a'."""
    return -(d / KAPPA) * np.exp2(-d * d)


@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("h", HALF_WIDTHS)
def test_selection_is_minimal_and_within_tolerance(h, tol):
    sel = ops.lowrank_panels_select(h, tol)
    assert sel is not None
    P, hp = sel["P"], sel["h_p"]
    print("h %.1f tol %.1e: P %d h_p %.3f p %d q %d bounds %s dbounds %s" % (h, tol, P, hp, sel["p"], sel["q"], sel["bounds"],
                                                                             sel["dbounds"]))
    assert P >= 2 and hp == pytest.approx(h / P, rel=1e-15)
    assert 1 <= sel["p"] <= 64 and 1 <= sel["q"] <= 64
    assert sel["C0"].shape == sel["C1"].shape == (sel["p"],) * 2 and sel["D0"].shape == sel["D1"].shape == (sel["q"],) * 2
    assert (sel["bounds"] <= tol).all() and (sel["dbounds"] <= tol).all() and (sel["bounds"] >= 0).all()
    for fewer in range(2, P):                                  # no smaller count is served
        assert ops.lowrank_panels_select(h, tol, panels=fewer) is None, fewer
    again = ops.lowrank_panels_select(h, tol, panels=P)        # the count alone gives the same forms
    assert again["p"] == sel["p"] and again["q"] == sel["q"] and np.array_equal(again["C1"], sel["C1"])


@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("h", HALF_WIDTHS)
def test_forms_against_the_float64_functions(h, tol):
    sel = ops.lowrank_panels_select(h, tol)
    hp, p, q = sel["h_p"], sel["p"], sel["q"]
    x = np.unique(np.concatenate([np.linspace(-1.0, 1.0, 65), np.cos(np.pi * (np.arange(97) + 0.5) / 97), [-1.0, 1.0]]))
    Tp, Tq = _cheb(x, p), _cheb(x, q)
    d0 = hp * (x[:, None] - x[None, :])
    d1 = d0 - 2.0 * hp                                         # x in the lower panel, y in the upper
    e = [np.abs(Tp.T @ sel["C0"] @ Tp - _f(d0)).max(), np.abs(Tp.T @ sel["C1"] @ Tp - _f(d1)).max(),
         np.abs(Tq.T @ sel["D0"] @ Tq - _g(d0)).max(), np.abs(Tq.T @ sel["D1"] @ Tq - _g(d1)).max()]
    print("h %.1f tol %.1e: errors C0 %.2e C1 %.2e D0 %.2e D1 %.2e, tails %s %s" % (h, tol, *e, sel["bounds"][:2], sel["dbounds"][:2]))
    assert e[0] <= sel["bounds"][0] + ROUND and e[1] <= sel["bounds"][1] + ROUND
    assert e[2] <= sel["dbounds"][0] + ROUND and e[3] <= sel["dbounds"][1] + ROUND
    # the opposite order of a neighbouring pair: C1^T and -D1^T
    assert np.abs(Tp.T @ sel["C1"].T @ Tp - _f(d1).T).max() <= sel["bounds"][1] + ROUND
    assert np.abs(Tq.T @ (-sel["D1"].T) @ Tq - _g(-d1.T)).max() <= sel["dbounds"][1] + ROUND
    assert np.abs(sel["D0"] + sel["D0"].T).max() == 0.0        # D0 exactly antisymmetric, as rpgp_lowrank_grad_select's


@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("h", HALF_WIDTHS)
def test_panelled_kernel_on_the_whole_interval(h, tol):
    """Every entry of the kernel belongs to one case: same panel, neighbouring panels (either order) or dropped.  On a grid of
    [-h, h] with both ends and every inner panel edge, the panelled form is within the largest of the three bounds."""
    sel = ops.lowrank_panels_select(h, tol)
    P, hp, p, q = sel["P"], sel["h_p"], sel["p"], sel["q"]
    edges = -h + 2.0 * hp * np.arange(P + 1)
    a = np.unique(np.concatenate([np.linspace(-h, h, 301), edges, edges[1:-1] - 1e-9, [h]]))
    k = np.clip(np.floor((a + h) / (2.0 * hp)), 0, P - 1).astype(int)       # +h: the last panel; an inner edge: the upper panel
    assert k[-1] == P - 1 and all(k[np.searchsorted(a, e)] == i + 1 for i, e in enumerate(edges[1:-1]))
    x = (a - (-h + (2 * k + 1) * hp)) / hp
    assert np.abs(x).max() <= 1.0 + 1e-12
    Tp, Tq = _cheb(x, p), _cheb(x, q)
    dk = k[:, None] - k[None, :]
    d = a[:, None] - a[None, :]

    def assemble(T, same, nb, sign):
        s, lo, up = T.T @ same @ T, T.T @ nb @ T, T.T @ (sign * nb.T) @ T
        return np.where(dk == 0, s, np.where(dk == -1, lo, np.where(dk == 1, up, 0.0)))

    ek = np.abs(assemble(Tp, sel["C0"], sel["C1"], 1.0) - _f(d))
    eg = np.abs(assemble(Tq, sel["D0"], sel["D1"], -1.0) - _g(d))
    far = np.abs(dk) >= 2
    print("h %.1f tol %.1e P %d: kernel %.2e (dropped %.2e), derivative %.2e (dropped %.2e)"
          % (h, tol, P, ek.max(), ek[far].max() if far.any() else 0.0, eg.max(), eg[far].max() if far.any() else 0.0))
    if far.any():
        assert _f(d[far]).max() <= sel["bounds"][2] and np.abs(_g(d[far])).max() <= sel["dbounds"][2]
    else:
        assert P == 2 and sel["bounds"][2] == 0.0 and sel["dbounds"][2] == 0.0
    assert ek.max() <= sel["bounds"].max() + ROUND and eg.max() <= sel["dbounds"].max() + ROUND
    assert ek.max() <= tol and eg.max() <= tol


def test_limits_of_the_selection():
    from rpgp_amd import _lib
    lib = _lib.load()
    assert lib.rpgp_lowrank_panels_max() == 16
    assert ops.lowrank_panels_select(100.0, 1e-12)["P"] == 16              # the stated maximum: half-width about 100
    assert ops.lowrank_panels_select(150.0, 1e-12) is None and ops.lowrank_panels_select(150.0) is None
    assert ops.lowrank_panels_select(float("nan")) is None and ops.lowrank_panels_select(float("inf")) is None
    assert ops.lowrank_panels_select(0.0) is None
    assert ops.lowrank_panels_select(20.0, 1e-12, panels=2) is None       # h_p = 10: ranks above 64
    assert ops.lowrank_panels_select(20.0, 1e-12, panels=16) is None      # h_p = 1.25: the dropped values are above 1e-12
    for bad in (1, -1, 17):
        with pytest.raises(Exception):
            ops.lowrank_panels_select(20.0, 1e-12, panels=bad)
    # a count for every half-width from the end of the rank-64 single interval on
    for h in np.arange(6.4, 100.0, 0.37):
        assert ops.lowrank_panels_select(float(h), 1e-12) is not None, h
    assert lib.rpgp_lowrank_panels_plan_bytes(0, 3) == 0 and lib.rpgp_lowrank_panels_plan_bytes(10, 65) == 0
    # N rows, 2 x 64 x 64 fp32 coefficients, coordinates, panel indices and N / 2048 + 16 blocks of sorted slots per column
    assert lib.rpgp_lowrank_panels_plan_bytes(5000, 3) >= 2 * 64 * 64 * 4 + 5000 * 3 * 5 + 3 * (2 + 16) * 2048 * 8


# ---- the operators ------------------------------------------------------------------------------------------------------------
class _Prep:
    def __init__(self, Z):
        self.N, self.J = Z.shape
        self.fast_ok, self.buf = True, None


class _Recorder(OracleBackend):
    """The CPU double plus prepare and a lowrank_train_plan that records its keywords and serves nothing."""

    def __init__(self):
        super().__init__()
        self.kw = []

    def prepare(self, Z):
        return _Prep(Z)

    def make_family(self, kind, group, weights, product=False):
        fam = super().make_family(kind, group, weights, product)
        fam.weights, fam.generic = weights, False
        return fam

    def mvm_sym_lowrank_weighted(self, *a, **k):              # (the weighted operator asks whether the backend has them)
        raise AssertionError("not called here")

    bilinear_grad_lowrank_weighted = mvm_sym_lowrank_weighted


class _WithPanels(_Recorder):
    def lowrank_train_plan(self, prep, scale, noise, mass=None, max_rank=64, panels=False):
        self.kw.append({"mass": mass, "max_rank": max_rank, "panels": panels})
        return None


class _WithoutPanels(_Recorder):
    def lowrank_train_plan(self, prep, scale, noise, mass=None, max_rank=64):
        self.kw.append({"mass": mass, "max_rank": max_rank, "panels": "not taken"})
        return None


def _ops(weighted):
    from rpgp_amd.operators import AdditiveRPOperator, FamilyAdditiveOperator
    g = torch.Generator().manual_seed(0)
    Z = torch.randn(30, 4, generator=g)
    if weighted:
        return FamilyAdditiveOperator(Z, outputscale=torch.tensor(0.8), comp_weights=torch.rand(4, generator=g) + 0.25)
    return AdditiveRPOperator(Z, outputscale=torch.tensor(0.8))


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_the_keyword_is_passed_only_with_the_setting_on(weighted):
    from rpgp_amd import backend, settings

    def decide(be, panels):
        prev = backend.set_backend(be)
        try:
            op = _ops(weighted)
            with settings.lowrank_kernel(True), settings.lowrank_panels(panels):
                assert op.lowrank_form(0.3) is None and op.lowrank_panels is None
        finally:
            backend.set_backend(prev)
        assert len(be.kw) == 1
        return be.kw[0]

    assert settings.lowrank_panels.off()                       # off by default
    assert decide(_WithPanels(), False)["panels"] is False     # off: called without the keyword (the default shows)
    assert decide(_WithPanels(), True)["panels"] is True
    assert decide(_WithoutPanels(), True)["panels"] == "not taken"          # a backend without the capability: no panels
    assert decide(_WithoutPanels(), False)["panels"] == "not taken"


def test_setting_off_leaves_the_call_of_the_test_double_as_it_is(monkeypatch):
    """ops.lowrank_train_plan with the setting off: positional (prep, scale, noise) and no keyword at the default cap."""
    from rpgp_amd import backend, settings
    seen = []

    class _Exact(_Recorder):
        def lowrank_train_plan(self, *a, **k):
            seen.append((len(a), dict(k)))
            return None

    be = _Exact()
    prev = backend.set_backend(be)
    try:
        with settings.lowrank_kernel(True):
            assert _ops(False).lowrank_form(0.3) is None
        with settings.lowrank_kernel(True), settings.lowrank_panels(True):
            assert _ops(False).lowrank_form(0.3) is None
    finally:
        backend.set_backend(prev)
    assert seen == [(3, {}), (3, {"panels": True})]
