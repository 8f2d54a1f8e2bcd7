"""Host side of the low-rank bilinear derivative (csrc/rpgp_lowrank.hip through ctypes, no GPU): the derivative rank q of
rpgp_lowrank_grad_select covers the analytic derivative factor within its claimed tail, D is antisymmetric, q grows with the
half-width and is "not served" above the largest rank; the training tolerance of ops.lowrank_train_tol; and the switch
settings.lowrank_kernel leaves a fused-MLL step under the CPU test double exactly as it is."""
import math

import numpy as np
import pytest
import torch

from tests.test_host_stack import _build_model, _problem

KAPPA = (2.0 * math.log(2.0)) ** -0.5


def _cheb(x, q):
    T = np.empty((q, x.size))
    T[0] = 1.0
    if q > 1:
        T[1] = x
    for m in range(2, q):
        T[m] = 2.0 * x * T[m - 1] - T[m - 2]
    return T


@pytest.mark.parametrize("h", [0.5, 2.0, 5.0, 8.0, 9.4])
def test_expansion_matches_the_analytic_derivative_within_its_tail(h):
    from rpgp_amd import ops
    q, tail, D = ops.lowrank_grad_select(h, 64)
    if q == 0:
        assert ops.lowrank_grad_select(h, 128)[0] > 64       # only "not served" because it needs more than 64
        return
    assert 0.0 < tail <= 2.0 ** -26
    assert np.abs(D + D.T).max() <= 1e-15
    x = np.linspace(-1.0, 1.0, 200)
    T = _cheb(x, q)
    approx = T.T @ D @ T
    d = x[:, None] - x[None, :]
    # (kappa / h) * d/dx exp2(-h^2 (x - y)^2) = -(z - z') e(z, z') in z units
    exact = -2.0 * math.log(2.0) * KAPPA * h * d * np.exp2(-h * h * d * d)
    assert np.abs(approx - exact).max() <= tail


def test_rank_is_monotone_and_not_served_above_the_largest_rank():
    from rpgp_amd import ops
    hs = np.linspace(0.25, 9.5, 38)
    qs = [ops.lowrank_grad_select(h, 64)[0] for h in hs]
    served = [q for q in qs if q > 0]
    assert served and all(a <= b for a, b in zip(served, served[1:])), qs
    # once a half-width is not served, no wider one is
    first_off = next((i for i, q in enumerate(qs) if q == 0), len(qs))
    assert all(q == 0 for q in qs[first_off:]) and first_off < len(qs)
    assert ops.lowrank_grad_select(12.0, 64)[0] == 0
    assert ops.lowrank_grad_select(float("nan"), 64)[0] == 0
    # a tighter tolerance needs at least the rank of a looser one
    assert ops.lowrank_grad_select(4.0, 64, 1e-12)[0] >= ops.lowrank_grad_select(4.0, 64)[0]


def test_training_tolerance():
    from rpgp_amd import ops
    base = ops.lowrank_train_tol(50000, 20, 1.0, 0.01)
    assert 0.0 < base <= 2.0 ** -26
    assert ops.lowrank_train_tol(391386, 20, 1.0, 0.01) < base                 # tightens with N
    assert ops.lowrank_train_tol(50000, 20, 1.0, 0.1) > base                   # loosens with sigma^2
    assert ops.lowrank_train_tol(100, 20, 1.0, 1.0) == 2.0 ** -26              # never above the product's own bound
    n, j, s, nz = 391386, 20, 0.8, 0.02
    assert s * j * n * ops.lowrank_train_tol(n, j, s, nz) <= 1e-3 * nz * (1 + 1e-12)
    assert ops.lowrank_train_tol(1000, 20, 1.0, 0.0) == 0.0                    # no noise: no tolerance, not served


def test_fused_step_is_unchanged_under_the_cpu_double(oracle_backend):
    """The test double has no low-rank entry points: with the switch on, the step is the sweep's, bit for bit."""
    from rpgp_amd import settings

    def step(on):
        X, y, P, ls, noise, s = _problem(N=260, seed=3, noise=0.2)
        model, lik, mll = _build_model(X, y, P, ls, noise, s)
        model.train()
        with settings.max_cholesky_size(0), settings.deterministic_probes(True), settings.min_preconditioning_size(100), \
                settings.lowrank_kernel(on):
            val = mll(model(X), y)
            val.backward()
        grads = [p.grad.detach().clone() for p in (model.covar_module.base_kernel.raw_lengthscale,
                                                   model.covar_module.raw_outputscale, lik.raw_noise,
                                                   model.mean_module.constant)]
        return val.detach().clone(), grads

    v0, g0 = step(False)
    v1, g1 = step(True)
    assert torch.equal(v0, v1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    assert settings.lowrank_kernel.off()
