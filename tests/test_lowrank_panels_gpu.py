"""Panel plans of the low-rank product kernels (rpgp_lowrank_create_panels; settings.lowrank_kernel with
settings.lowrank_panels): the product and the bilinear derivative, plain and weighted, at half-widths 7 ... 45 (2 ... 8 panels)
against the float64 oracles and the exact sweeps; shapes at which the sorted projection blocks, the per-panel combine and the
64-row output blocks can go wrong; panel edges, empty panels, a single occupied panel, segments of exactly one projection block
and of a block plus one row; j-ranges, row slices, aliasing, guard zones, run-to-run bit identity and the bits of null against
all-ones weights; symmetry; both operator kinds in the native mBCG executor at half-width 20; a first step and a fit at
half-width 20; and what is not served.

Accuracy conditions (each printed with the panel count and (p, q) before it is asserted): those of
tests/test_lowrank_kernel_wide_gpu.py.  Both paths read the same float32 prepared coordinates, whose absolute error of about
ulp(h) grows with the half-width, so each result is held to the float64 oracle by the existing gate or, where that is not met,
by 1.25 x the error of the exact direct sweep on the same inputs + 1e-8:
  product: 5e-7 in relative 2-norm;  gZ: 2e-6 overall and 1e-5 on the worst row;  gscale / gcomp: 4e-6."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cmvm, dense_gp, family as fmo

pytestmark = pytest.mark.gpu

KAPPA = 0.8493218002880191        # the coordinate scale of rpgp_prepare: a = (z - mid) kappa
TOL = 1e-12                       # the tolerance of the test plans: the rank-64 single interval ends below half-width 6.5
SCALE = 0.7
HALF_WIDTHS = (7.0, 13.5, 20.0, 45.0)


def _inputs(N, J, T, h, dev, seed):
    """Z with every column spanning [-w, w] (w = h / kappa: the plan's half-width is h, rows 0 and 1 at +-w), L and R standard
    normal (L doubles as the product's V): tests/test_lowrank_kernel_wide_gpu.py::_inputs."""
    g = torch.Generator().manual_seed(seed)
    w = h / KAPPA
    Z = (torch.rand(N, J, generator=g) * 2.0 - 1.0) * w
    Z[0] = w
    if N > 1:
        Z[1] = -w
    L = torch.randn(N, T, generator=g)
    R = torch.randn(N, T, generator=g)
    return Z.to(dev), L.to(dev), R.to(dev)


def _weights(J, dev, signed=True):
    """tests/test_lowrank_family_gpu.py::_weights (positive, spread 16 x), with a zero and a negative weight from J = 3 on."""
    w = torch.tensor([0.05 + 2.0 ** (-4.0 * j / max(J - 1, 1)) for j in range(J)], dtype=torch.float32, device=dev)
    if signed and J >= 3:
        w[1], w[2] = 0.0, -0.2
    return w


def _panel_plan(Z, tol=TOL):
    from rpgp_amd import ops
    prep = ops.Prepared(Z)
    plan = ops.LowrankTrainPlan(prep, tol, panels=True)
    assert plan.served and plan.panels >= 2 and 0 < plan.p <= 64 and 0 < plan.q <= 64, (plan.panels, plan.p, plan.q)
    assert abs(plan.h_p * plan.panels - prep.max_abs) <= 1e-5 * prep.max_abs
    return prep, plan


def _np(t):
    return t.double().cpu().numpy()


def _rel(a, ref):
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def _rows(a, ref):
    return float(np.linalg.norm(a - ref, axis=1).max() / np.linalg.norm(ref, axis=1).max())


def _held(err, gate, sweep_err):
    """The accuracy condition of this file: the existing gate, or 1.25 x the exact sweep's error + 1e-8."""
    return err <= gate or err <= 1.25 * sweep_err + 1e-8


GUARD = 257


def _guarded(N, T, dev):
    """An N x T output inside a NaN-filled wider buffer: (buffer, view)."""
    buf = torch.full((N * T + 2 * GUARD,), float("nan"), device=dev)
    return buf, buf[GUARD:GUARD + N * T].view(N, T)


def _guards_untouched(buf, N, T):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + N * T:]).all())


def _raw_product(plan, prep, V, scale, noise, j0=0, j1=None, world=1, rank=0, w=None, out=None):
    """rpgp_mvm_sym_lowrank_range (w None) / rpgp_mvm_sym_lowrank_weighted into a guarded buffer (or `out`)."""
    from rpgp_amd import _lib, ops
    lib = _lib.load()
    N, J, T = plan.N, plan.J, V.shape[1]
    j1 = J if j1 is None else j1
    buf = None
    if out is None:
        buf, out = _guarded(N, T, V.device)
    ws = torch.empty(max(int(lib.rpgp_mvm_sym_lowrank_workspace_bytes(plan.handle, N, T)), 1), dtype=torch.uint8,
                     device=V.device)
    if w is None:
        rc = lib.rpgp_mvm_sym_lowrank_range(plan.handle, prep.buf.data_ptr(), V.data_ptr(), out.data_ptr(), N, J, T, j0, j1,
                                            world, rank, float(scale), float(noise), ws.data_ptr(), ws.numel(), ops._stream())
    else:
        rc = lib.rpgp_mvm_sym_lowrank_weighted(plan.handle, prep.buf.data_ptr(), w.data_ptr(), V.data_ptr(), out.data_ptr(), N,
                                               J, T, j0, j1, float(scale), float(noise), ws.data_ptr(), ws.numel(),
                                               ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    if buf is not None:
        assert _guards_untouched(buf, N, T)
    return out


def _raw_grad(plan, L, R, gZ, gout, j0, j1, scale, w=None, ws_bytes=None):
    from rpgp_amd import _lib, ops
    lib = _lib.load()
    N, J, T = plan.N, plan.J, L.shape[1]
    nbytes = lib.rpgp_bilinear_grad_lowrank_workspace_bytes(plan.handle, N, T) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=L.device)
    if w is None:
        rc = lib.rpgp_bilinear_grad_lowrank(plan.handle, L.data_ptr(), R.data_ptr(), gZ.data_ptr(), gout.data_ptr(), N, J, T,
                                            j0, j1, float(scale), ws.data_ptr(), int(nbytes), ops._stream())
    else:
        rc = lib.rpgp_bilinear_grad_lowrank_weighted(plan.handle, w.data_ptr(), L.data_ptr(), R.data_ptr(), gZ.data_ptr(),
                                                     gout.data_ptr(), N, J, T, j0, j1, float(scale), ws.data_ptr(), int(nbytes),
                                                     ops._stream())
    torch.cuda.synchronize()
    return rc


# ---- 1. the product and the derivative against the oracles ----------------------------------------------------------------------
def _check_product(dev, Z, V, tag):
    from rpgp_amd import ops
    N, J = Z.shape
    T = V.shape[1]
    prep, plan = _panel_plan(Z)
    w = _weights(J, dev)
    fam = ops.Family("RBF", 1, w)
    Zh, Vh = _np(Z), _np(V)
    kv = cmvm.mvm(Zh, Zh, Vh, SCALE)
    kw = fmo.mvm(Zh, Zh, Vh, "RBF", 1, _np(w), SCALE)
    ones = torch.ones(J, device=dev)
    for noise in (0.0, 0.3):
        out = _raw_product(plan, prep, V, SCALE, noise)
        sweep = ops.mvm_sym(Z, V, SCALE, noise)
        ref = kv + noise * Vh
        e, es = _rel(_np(out), ref), _rel(_np(sweep), ref)
        outw = _raw_product(plan, prep, V, SCALE, noise, w=w)
        sweepw = ops.family_mvm_sym(fam, Z, V, SCALE, noise)
        refw = kw + noise * Vh
        ew, esw = _rel(_np(outw), refw), _rel(_np(sweepw), refw)
        print("product %s N %d J %d T %d P %d h_p %.3f p %d q %d noise %.1f: plain %.2e (sweep %.2e), weighted %.2e (sweep %.2e)"
              % (tag, N, J, T, plan.panels, plan.h_p, plan.p, plan.q, noise, e, es, ew, esw))
        assert _held(e, 5e-7, es), (e, es, plan.panels)
        assert _held(ew, 5e-7, esw), (ew, esw, plan.panels)
        # repeated calls are bit-identical; null weights and weights of 1 give the same bits
        assert torch.equal(_raw_product(plan, prep, V, SCALE, noise), out)
        assert torch.equal(_raw_product(plan, prep, V, SCALE, noise, w=w), outw)
        assert torch.equal(_raw_product(plan, prep, V, SCALE, noise, w=ones), out)
        if N > 2:
            assert not torch.equal(out, sweep)                  # really the other path
    return prep, plan, w


def _check_grad(dev, Z, L, R, tag):
    from rpgp_amd import ops
    N, J = Z.shape
    T = L.shape[1]
    prep, plan = _panel_plan(Z)
    w = _weights(J, dev)
    Zh, Lh, Rh = _np(Z), _np(L), _np(R)
    gZ_ref, gs_ref = dense_gp.bilinear_grad(Zh, Lh, Rh, SCALE)
    gs_ref = float(gs_ref)
    gW_ref, gc_ref = fmo.bilinear_grad(Zh, Lh, Rh, "RBF", 1, _np(w), SCALE)
    # plain
    gZ, gs = ops.bilinear_grad_lowrank(plan, L, R, SCALE)
    sZ, ss = ops.bilinear_grad(Z, L, R, SCALE)
    e, es = _rel(_np(gZ), gZ_ref), _rel(_np(sZ), gZ_ref)
    r, rs = _rows(_np(gZ), gZ_ref), _rows(_np(sZ), gZ_ref)
    c, cs = abs(gs.item() - gs_ref) / abs(gs_ref), abs(ss.item() - gs_ref) / abs(gs_ref)
    print("derivative %s N %d J %d T %d P %d h_p %.3f p %d q %d: gZ %.2e (sweep %.2e) rows %.2e (sweep %.2e) gscale %.2e (sweep %.2e)"
          % (tag, N, J, T, plan.panels, plan.h_p, plan.p, plan.q, e, es, r, rs, c, cs))
    assert _held(e, 2e-6, es) and _held(r, 1e-5, rs), (e, es, r, rs)
    assert _held(c, 4e-6, cs), (c, cs)
    # weighted (gZ carries scale w_j, so its column of the zero weight is exactly zero; gcomp does not carry the weights)
    wZ, wc = ops.bilinear_grad_lowrank_weighted(plan, w, L, R, SCALE)
    fZ, fc = ops.family_bilinear_grad(ops.Family("RBF", 1, w), Z, L, R, SCALE)
    ew, esw = _rel(_np(wZ), gW_ref), _rel(_np(fZ), gW_ref)
    rw, rsw = _rows(_np(wZ), gW_ref), _rows(_np(fZ), gW_ref)
    cw, csw = _rel(_np(wc), gc_ref), _rel(_np(fc), gc_ref)
    print("  weighted: gZ %.2e (sweep %.2e) rows %.2e (sweep %.2e) gcomp %.2e (sweep %.2e)" % (ew, esw, rw, rsw, cw, csw))
    assert _held(ew, 2e-6, esw) and _held(rw, 1e-5, rsw), (ew, esw, rw, rsw)
    assert _held(cw, 4e-6, csw), (cw, csw)
    if J >= 3:
        assert float(wZ[:, 1].abs().max()) == 0.0 and float(wZ[:, 2].abs().max()) > 0.0 and wc[1].item() != 0.0
    # repeated calls are bit-identical; w = 1 gives gZ's bits
    again = ops.bilinear_grad_lowrank(plan, L, R, SCALE)
    assert torch.equal(again[0], gZ) and torch.equal(again[1], gs)
    again = ops.bilinear_grad_lowrank_weighted(plan, w, L, R, SCALE)
    assert torch.equal(again[0], wZ) and torch.equal(again[1], wc)
    oZ, oc = ops.bilinear_grad_lowrank_weighted(plan, torch.ones(J, device=dev), L, R, SCALE)
    assert torch.equal(oZ, gZ)
    # gscale is the sum of the components: both are float32 roundings (2^-24) of float64 sums, and the components cancel, so the
    # bound is that of their magnitudes, not of the sum's
    assert abs(float(oc.double().sum()) - gs.item()) <= 2e-7 * (float(oc.double().abs().sum()) + abs(gs.item()))
    return prep, plan, w, gZ, wZ, wc


@pytest.mark.parametrize("h", HALF_WIDTHS)
def test_product_and_derivative_at_every_half_width(gpu_device, h):
    """N = 2 049 rows over 2 ... 8 panels: every (column, panel) segment is a ragged projection block."""
    Z, L, R = _inputs(2049, 3, 2, h, gpu_device, seed=int(10 * h))
    prep, plan = _check_product(gpu_device, Z, L, "h %.1f" % h)[:2]
    assert plan.panels == {7.0: 2, 13.5: 3, 20.0: 4, 45.0: 8}[h]
    _check_grad(gpu_device, Z, L, R, "h %.1f" % h)


# two rows in the two end panels; a ragged wave; a wave and one row; T = 11 with segments of more than one block; J = 64: the
# output pass takes the projections in chunks of 31
@pytest.mark.parametrize("N,J,T", [(2, 1, 1), (63, 7, 5), (65, 7, 1), (4613, 7, 11), (130, 64, 1)])
def test_product_shapes(gpu_device, N, J, T):
    Z, V, _ = _inputs(N, J, T, 20.0, gpu_device, seed=N + 7 * T + J)
    _check_product(gpu_device, Z, V, "shape")


def test_product_with_64_projections_and_16_panels(gpu_device):
    """Half-width 100: 16 panels of rank about 61, the output pass's LDS holds 7 projections at a time."""
    Z, V, _ = _inputs(130, 64, 1, 100.0, gpu_device, seed=9)
    prep, plan, _ = _check_product(gpu_device, Z, V, "h 100")
    assert plan.panels == 16


# (two rows 2 h apart have a derivative of exactly zero: no relative error to take, as in the wide file)
@pytest.mark.parametrize("N,J,T", [(63, 7, 5), (65, 7, 1), (4613, 7, 11), (257, 64, 16)])
def test_derivative_shapes(gpu_device, N, J, T):
    Z, L, R = _inputs(N, J, T, 20.0, gpu_device, seed=N + 7 * T + J + 1)
    _check_grad(gpu_device, Z, L, R, "shape")


def test_two_rows(gpu_device):
    """Rows at +-w only: two end panels, nothing between them, a product that is scale v + noise v and a derivative that is
    zero up to the form's own bound: each row meets only itself, where the truncated D0 is within the tolerance of G(x, x) = 0."""
    from rpgp_amd import ops
    Z, V, R = _inputs(2, 1, 1, 20.0, gpu_device, seed=1)
    prep, plan = _panel_plan(Z)
    out = _raw_product(plan, prep, V, SCALE, 0.3)
    assert torch.allclose(out, (SCALE + 0.3) * V, rtol=1e-6, atol=0.0)
    gZ, gs = ops.bilinear_grad_lowrank(plan, V, R, SCALE)
    assert float(gZ.abs().max()) <= 2.0 * SCALE * TOL * float(V.abs().max() * R.abs().max())
    assert abs(gs.item() - float((V * R).sum())) <= 1e-6 * float((V * R).abs().sum())


# ---- 3. panel edge cases ----------------------------------------------------------------------------------------------------------
def _panel_counts(prep, plan):
    """Rows per (column, panel), from the prepared coordinates with the plan's own rule in float64."""
    N, J, P = plan.N, plan.J, plan.panels
    a = prep.buf[512:512 + 8 * N * J].view(torch.float32).view(N, J, 2)[:, :, 0].double()
    h = plan.h_p * P
    k = torch.clamp(torch.floor((a + h) / (2.0 * plan.h_p)), 0, P - 1).long()
    return torch.stack([(k == p).sum(0) for p in range(P)], 1).cpu().numpy(), a, k


def test_panel_edges_empty_panels_and_block_sized_segments(gpu_device):
    """Half-width 20, four panels with the edges -10, 0, 10 in prepared units.  Column 0: random with rows at +-w and one exactly
    on the inner edge 0 (the upper panel).  Column 1: the two end panels only.  Column 2: constant (one occupied panel, every row
    on the edge 0).  Column 3: 2 048 rows in panel 0 (exactly one projection block), 2 049 in panel 1 (a block and one row),
    none in panel 2, the rest in panel 3."""
    N, T, h = 4613, 3, 20.0
    g = torch.Generator().manual_seed(77)
    w = h / KAPPA
    Z = torch.empty(N, 4)
    Z[:, 0] = (torch.rand(N, generator=g) * 2.0 - 1.0) * w
    Z[2, 0] = 0.0
    side = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
    Z[:, 1] = side * (0.55 + 0.45 * torch.rand(N, generator=g)) * w
    Z[:, 2] = 0.3 * w
    u = torch.rand(N, generator=g)
    Z[:2048, 3] = (-1.0 + 0.49 * u[:2048]) * w
    Z[2048:4097, 3] = (-0.49 + 0.48 * u[2048:4097]) * w
    Z[4097:, 3] = (0.51 + 0.49 * u[4097:]) * w
    Z[0, :2], Z[0, 3] = w, -w                                  # the ends of the range (column 3: row 0 lies in panel 0)
    Z[1, :2], Z[4100, 3] = -w, w
    perm = torch.randperm(N, generator=g)                      # the sort has work to do
    Z = Z[perm].to(gpu_device)
    L = torch.randn(N, T, generator=g).to(gpu_device)
    R = torch.randn(N, T, generator=g).to(gpu_device)
    prep, plan, _ = _check_product(gpu_device, Z, L, "edges")
    assert plan.panels == 4
    counts, a, k = _panel_counts(prep, plan)
    print("rows per (column, panel):", counts.tolist())
    assert counts[3].tolist() == [2048, 2049, 0, 516]
    assert counts[1][1] == 0 and counts[1][2] == 0 and counts[1][0] > 0 and counts[1][3] > 0
    assert counts[2].tolist() == [0, 0, N, 0] and float(a[:, 2].abs().max()) == 0.0
    on_edge = (a[:, 0] == 0.0)
    assert int(on_edge.sum()) == 1 and int(k[on_edge, 0]) == 2
    _check_grad(gpu_device, Z, L, R, "edges")


# ---- 4. contracts of the entries ------------------------------------------------------------------------------------------------
def test_product_j_ranges_row_slices_and_aliasing(gpu_device):
    from rpgp_amd import ops
    N, J, T = 2049, 3, 2
    Z, V, _ = _inputs(N, J, T, 20.0, gpu_device, seed=40)
    prep, plan = _panel_plan(Z)
    w = _weights(J, gpu_device)
    Zh, Vh = _np(Z), _np(V)
    full = _raw_product(plan, prep, V, SCALE, 0.0)
    # j-ranges: each against the oracle on its columns, and their float64 sum against the whole
    parts = torch.zeros(N, T, dtype=torch.float64, device=gpu_device)
    for j0, j1 in ((0, 1), (1, 3)):
        o = _raw_product(plan, prep, V, SCALE, 0.0, j0=j0, j1=j1)
        ref = cmvm.mvm(Zh[:, j0:j1], Zh[:, j0:j1], Vh, SCALE)
        sweep = _np(ops.mvm_sym(Z, V, SCALE, 0.0, j0=j0, j1=j1))
        e, es = _rel(_np(o), ref), _rel(sweep, ref)
        print("columns [%d, %d): %.2e (sweep %.2e)" % (j0, j1, e, es))
        assert _held(e, 5e-7, es), (e, es)
        ow = _raw_product(plan, prep, V, SCALE, 0.0, j0=j0, j1=j1, w=w)
        refw = fmo.mvm(Zh[:, j0:j1], Zh[:, j0:j1], Vh, "RBF", 1, _np(w)[j0:j1], SCALE)
        if j0 == 0:
            assert _held(_rel(_np(ow), refw), 5e-7, es)
        parts += o.double()
    assert _rel(_np(parts), _np(full)) <= 2e-7
    # row slices of world 3: each rank writes its rows and zeros elsewhere, and the slices add up to the whole bit for bit
    total = torch.zeros_like(full)
    for rank in range(3):
        o = _raw_product(plan, prep, V, SCALE, 0.0, world=3, rank=rank)
        r0, r1 = N * rank // 3, N * (rank + 1) // 3
        assert float(o[:r0].abs().sum()) == 0.0 and float(o[r1:].abs().sum()) == 0.0
        assert torch.equal(o[r0:r1], full[r0:r1])
        total += o
    assert torch.equal(total, full)
    # out aliasing V, with the noise term that reads V
    for ww in (None, w):
        want = _raw_product(plan, prep, V, SCALE, 0.3, w=ww)
        buf, Va = _guarded(N, T, gpu_device)
        Va.copy_(V)
        got = _raw_product(plan, prep, Va, SCALE, 0.3, w=ww, out=Va)
        assert torch.equal(got, want) and _guards_untouched(buf, N, T)


def test_derivative_j_ranges_leave_the_rest_untouched(gpu_device):
    from rpgp_amd import ops
    N, J, T = 777, 7, 5
    Z, L, R = _inputs(N, J, T, 20.0, gpu_device, seed=3)
    prep, plan, w, gZ_full, wZ_full, wc_full = _check_grad(gpu_device, Z, L, R, "j-ranges")
    total, mag = torch.zeros((), dtype=torch.float64), 0.0
    for j0, j1 in ((0, 2), (2, 3), (3, 7)):
        gZ = torch.full((N, J), float("nan"), device=gpu_device)
        gs = torch.full((3,), float("nan"), device=gpu_device)
        assert _raw_grad(plan, L, R, gZ, gs[1:2], j0, j1, SCALE) == 0
        assert torch.isnan(gZ[:, :j0]).all() and torch.isnan(gZ[:, j1:]).all() and torch.isnan(gs[0]) and torch.isnan(gs[2])
        assert torch.equal(gZ[:, j0:j1], gZ_full[:, j0:j1])
        total += gs[1].double().cpu()
        mag += abs(gs[1].item())
        gZ = torch.full((N, J), float("nan"), device=gpu_device)
        gc = torch.full((J,), float("nan"), device=gpu_device)
        assert _raw_grad(plan, L, R, gZ, gc, j0, j1, SCALE, w=w) == 0
        assert torch.isnan(gZ[:, :j0]).all() and torch.isnan(gZ[:, j1:]).all()
        assert torch.isnan(gc[:j0]).all() and torch.isnan(gc[j1:]).all()
        assert torch.equal(gZ[:, j0:j1], wZ_full[:, j0:j1]) and torch.equal(gc[j0:j1], wc_full[j0:j1])
    gs_full = ops.bilinear_grad_lowrank(plan, L, R, SCALE)[1]
    assert abs(float(total) - gs_full.item()) <= 2e-7 * (mag + abs(gs_full.item()))     # (float32 roundings of the parts)


def test_error_codes_of_a_panel_plan(gpu_device):
    from rpgp_amd import _lib, ops
    lib = _lib.load()
    N, J, T = 300, 4, 3
    Z, L, R = _inputs(N, J, T, 20.0, gpu_device, seed=5)
    prep, plan = _panel_plan(Z)
    assert lib.rpgp_lowrank_grad_bytes(plan.handle) == 4 * 64 * 64 * 8
    need = lib.rpgp_mvm_sym_lowrank_workspace_bytes(plan.handle, N, T)
    gneed = lib.rpgp_bilinear_grad_lowrank_workspace_bytes(plan.handle, N, T)
    assert need > 0 and gneed > 0
    out = torch.zeros(N, T, device=gpu_device)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    args = (plan.handle, prep.buf.data_ptr(), L.data_ptr(), out.data_ptr())
    assert lib.rpgp_mvm_sym_lowrank_range(*args, N, J, T, 0, J, 1, 0, 1.0, 0.0, ws.data_ptr(), need - 1, ops._stream()) \
        == _lib.RPGP_EWORKSPACE
    assert lib.rpgp_mvm_sym_lowrank_range(*args, N + 1, J, T, 0, J, 1, 0, 1.0, 0.0, ws.data_ptr(), need, ops._stream()) \
        == _lib.RPGP_EINVAL
    assert lib.rpgp_mvm_sym_lowrank_range(*args, N, J, T, 2, 2, 1, 0, 1.0, 0.0, ws.data_ptr(), need, ops._stream()) \
        == _lib.RPGP_EINVAL
    assert lib.rpgp_mvm_sym_lowrank_range(*args, N, J, T, 0, J, 3, 3, 1.0, 0.0, ws.data_ptr(), need, ops._stream()) \
        == _lib.RPGP_EINVAL
    gZ = torch.zeros(N, J, device=gpu_device)
    go = torch.zeros(J, device=gpu_device)
    w = _weights(J, gpu_device)
    for ww in (None, w):
        assert _raw_grad(plan, L, R, gZ, go, 0, J, 1.0, w=ww, ws_bytes=gneed - 8) == _lib.RPGP_EWORKSPACE
        assert _raw_grad(plan, L, R, gZ, go, 0, J + 1, 1.0, w=ww) == _lib.RPGP_EINVAL
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(gZ.abs().max()) == 0.0 and float(go.abs().max()) == 0.0
    # a plan buffer too small for the selected panels
    P, p, hd = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_void_p(None)
    small = torch.empty(1024, dtype=torch.uint8, device=gpu_device)
    assert lib.rpgp_lowrank_create_panels(prep.buf.data_ptr(), N, J, prep.max_abs, TOL, 0, small.data_ptr(), small.numel(),
                                          ctypes.byref(P), ctypes.byref(p), ctypes.byref(hd), ops._stream()) == _lib.RPGP_EWORKSPACE
    assert P.value == 0 and not hd.value


# ---- 5. symmetry ----------------------------------------------------------------------------------------------------------------
def test_product_is_symmetric(gpu_device):
    """u^T (K v) against v^T (K u) at half-width 20.  Each product is within g = 5e-7 (relative 2-norm, the gate above) of the
    exact symmetric K, so the two bilinear forms differ by at most g (|u| |K v| + |v| |K u|); C0 is symmetric and the two orders of
    a neighbouring pair use C1 and its exact transpose, so what remains is float32 rounding."""
    N, J = 2049, 3
    Z, u, v = _inputs(N, J, 1, 20.0, gpu_device, seed=50)
    prep, plan = _panel_plan(Z)
    Kv, Ku = _raw_product(plan, prep, v, SCALE, 0.0).double(), _raw_product(plan, prep, u, SCALE, 0.0).double()
    a, b = float((u.double() * Kv).sum()), float((v.double() * Ku).sum())
    bound = 5e-7 * float(u.double().norm() * Kv.norm() + v.double().norm() * Ku.norm())
    print("symmetry: u^T K v %.9e, v^T K u %.9e, difference %.2e, bound %.2e" % (a, b, abs(a - b), bound))
    assert abs(a - b) <= bound


# ---- 6. the native executor -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_panel_operators_in_the_native_executor(gpu_device, weighted):
    """The bound of the executor tests in tests/test_lowrank_kernel_wide_gpu.py: mean residual below 2 tol and the solution
    within 100 tol of the float64 dense solve.  The iteration counts are printed beside the sweep's."""
    from rpgp_amd import settings, linear_cg as lcg
    from rpgp_amd.operators import AdditiveRPOperator, FamilyAdditiveOperator, AddedDiagOperator
    from rpgp_amd.precond import pivoted_cholesky, WoodburyPreconditioner
    N, J, T, noise, s, tol = 4613, 7, 11, 0.3, 0.8, 1e-4
    Z, rhs, _ = _inputs(N, J, T, 20.0, gpu_device, seed=4)
    w = _weights(J, gpu_device, signed=False)

    def make():
        if weighted:
            return FamilyAdditiveOperator(Z, outputscale=torch.tensor(s, device=gpu_device), comp_weights=w)
        return AdditiveRPOperator(Z, outputscale=torch.tensor(s, device=gpu_device))

    out, its, ranks, panels = {}, {}, None, None
    for on in (False, True):
        op = make()
        khat = AddedDiagOperator(op, torch.tensor(noise, device=gpu_device), noise_value=noise)
        pre = WoodburyPreconditioner(pivoted_cholesky(op._diagonal(), op._get_rows, 15), noise)
        with settings.lowrank_kernel(on), settings.lowrank_panels(on):
            before = lcg.stats.get("native_calls", 0)
            out[on] = lcg.linear_cg(khat._matmul, rhs, operator=khat, tolerance=tol, max_iter=500, preconditioner=pre)
            assert lcg.stats.get("native_calls", 0) == before + 1
            its[on] = lcg.stats["last_iterations"]
        assert op.lowrank_served == on
        if on:
            ranks, panels = op.lowrank_ranks, op.lowrank_panels
            assert panels >= 2 and 0 < ranks[0] <= 64 and 0 < ranks[1] <= 64 and not op._prep.fast_ok, (panels, ranks)
    # without the panels the same operator is the sweep, under either cap
    for cap in (64, 128):
        op = make()
        with settings.lowrank_kernel(True), settings.lowrank_max_rank(cap):
            assert op.lowrank_form(noise) is None and op.lowrank_panels is None
    Zd = _np(Z)
    Kh = fmo.kernel_matrix(Zd, Zd, "RBF", 1, _np(w) if weighted else np.ones(J), s) + noise * np.eye(N)
    b = _np(rhs)
    x_ref = np.linalg.solve(Kh, b)
    xd = _np(out[True])
    res = np.linalg.norm(Kh @ xd - b, axis=0) / np.linalg.norm(b, axis=0)
    err = np.linalg.norm(xd - x_ref) / np.linalg.norm(x_ref)
    err_sweep = np.linalg.norm(_np(out[False]) - x_ref) / np.linalg.norm(x_ref)
    print("executor %s: panels %s ranks %s, iterations panels %d sweep %d, residual %.2e, solution %.2e (sweep %.2e)"
          % ("weighted" if weighted else "plain", panels, ranks, its[True], its[False], res.mean(), err, err_sweep))
    assert res.mean() < 2.0 * tol, res
    assert err < 100.0 * tol, err


# ---- 7. - 9. end to end ---------------------------------------------------------------------------------------------------------
KINDS = {
    "plain": ("additive_rp", {"J": 8, "noise_prior": True, "kernel_type": "RBF", "learn_proj": False, "prescale": True}),
    "weighted": ("rp_poly", {"k": 1, "J": 8, "noise_prior": True, "kernel_type": "RBF", "learn_proj": False, "weighted": True}),
}
FIT_H = 20.0


class _Settings:
    def __init__(self, *more):
        from rpgp_amd import settings
        self.cms = [settings.deterministic_probes(True), settings.cg_tolerance(1e-3), settings.max_cg_iterations(2000)]
        self.cms += list(more)

    def __enter__(self):
        for c in self.cms:
            c.__enter__()

    def __exit__(self, *a):
        for c in reversed(self.cms):
            c.__exit__(*a)


def _data(which, dev, N=3000, d=8):
    """Synthetic inputs scaled by one factor so that the widest projected column of the freshly created model has the half-width
    FIT_H (the projected coordinates are linear in X; the model is created again from the same seed by every user)."""
    from rpgp_amd.training import create_exact_gp
    kind, mk = KINDS[which]
    g = torch.Generator().manual_seed(0)
    X = torch.randn(N + 100, d, generator=g)
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N + 100, generator=g)
    y = (y - y.mean()) / y.std()
    torch.manual_seed(0)
    np.random.seed(0)
    model, lik = create_exact_gp(X[:N].to(dev), y[:N].to(dev), kind, **mk)
    model = model.to(dev).train()
    with torch.no_grad():
        Z = model(X[:N].to(dev)).covariance.Z1
        h0 = KAPPA * float(((Z.max(0).values - Z.min(0).values) * 0.5).max())
    return X * (FIT_H / h0), y


def _fresh(which, X, y, dev, N=3000):
    from rpgp_amd.training import create_exact_gp
    from rpgp_amd.models import ExactMarginalLogLikelihood
    kind, mk = KINDS[which]
    torch.manual_seed(0)
    np.random.seed(0)
    model, lik = create_exact_gp(X[:N].to(dev), y[:N].to(dev), kind, **mk)
    model = model.to(dev)
    return model, lik, ExactMarginalLogLikelihood(lik, model)


def _step(model, mll, X, y, on, panels):
    from rpgp_amd import settings
    params = [p for p in model.parameters() if p.requires_grad]
    with settings.lowrank_kernel(on), settings.lowrank_panels(panels):
        model.train()
        for p in params:
            p.grad = None
        loss = mll.negative(model(X), y)
        loss.backward()
    return loss.item(), [p.grad.detach().clone() for p in params]


def _grad_rel(a, b):
    a = torch.cat([t.reshape(-1) for t in a]).double()
    b = torch.cat([t.reshape(-1) for t in b]).double()
    return float((a - b).norm() / b.norm())


def _record_forms(monkeypatch, cls):
    """Every decision of the operator's lowrank_form: (served, (P, p, q) or None, the Prepared's (max_abs, fast_ok))."""
    seen = []
    orig = cls.lowrank_form

    def rec(self, noise=None):
        undecided = self._lowrank is None
        r = orig(self, noise)
        if undecided:
            pr = self._prep
            seen.append((r is not None, (r.panels, r.p, r.q) if r is not None else None,
                         (pr.max_abs, pr.fast_ok) if pr is not None else None))
        return r
    monkeypatch.setattr(cls, "lowrank_form", rec)
    return seen


@pytest.mark.parametrize("which", ["plain", "weighted"])
def test_fit_at_half_width_20(gpu_device, monkeypatch, which):
    """The gates of tests/test_lowrank_train_gpu.py for the first step (value within 1e-4, all raw gradients as one vector within
    1e-3 of the settings-off step); with settings.lowrank_panels off the step IS the settings-off step; and a 4-step
    train_exact_gp fit, prediction included, whose every decision is served with two or more panels."""
    from rpgp_amd import operators, settings
    from rpgp_amd.training import train_exact_gp
    cls = operators.AdditiveRPOperator if which == "plain" else operators.FamilyAdditiveOperator
    dev = gpu_device
    N = 3000
    X, y = _data(which, dev)
    Xd, yd = X[:N].to(dev), y[:N].to(dev)
    seen = _record_forms(monkeypatch, cls)
    with _Settings():
        model, lik, mll = _fresh(which, X, y, dev)
        v_off, g_off = _step(model, mll, Xd, yd, False, False)
        assert not any(s[0] for s in seen), seen
        seen.clear()
        v_def, g_def = _step(model, mll, Xd, yd, True, False)
        assert seen and not any(s[0] for s in seen), seen     # decided, and not served without the panels
        assert v_def == v_off and all(torch.equal(a, b) for a, b in zip(g_def, g_off))
        seen.clear()
        v_on, g_on = _step(model, mll, Xd, yd, True, True)
        assert seen and all(s[0] for s in seen), seen
        (P, p, q), (max_abs, fast_ok) = seen[0][1], seen[0][2]
        rel = _grad_rel(g_on, g_off)
        print("%s first step: panels %d ranks (%d, %d) max_abs %.2f fast_ok %s, value on %.8f off %.8f, gradients %.2e"
              % (which, P, p, q, max_abs, fast_ok, v_on, v_off, rel))
        assert P >= 2 and 0 < p <= 64 and 0 < q <= 64
        assert abs(max_abs - FIT_H) <= 0.05 * FIT_H
        assert abs(v_on - v_off) <= 1e-4 * abs(v_off), (v_on, v_off)
        assert rel <= 1e-3, rel
    seen.clear()
    kind, mk = KINDS[which]
    losses = []
    tk = {"verbose": False, "optimizer": "adam", "max_iter": 4, "lr": 0.02, "patience": 20, "smooth": True, "init_iters": 1,
          "loss_log": losses}
    torch.manual_seed(0)
    np.random.seed(0)
    with _Settings(settings.lowrank_kernel(True), settings.lowrank_panels(True), settings.eval_cg_tolerance(1e-4)):
        metrics, pred, fitted = train_exact_gp(X[:N], y[:N], X[N:], y[N:], kind, mk, tk, devices=[str(dev)],
                                               skip_random_restart=True, skip_posterior_variances=True)
    print("%s fit: decisions %s, losses %s, test mse %s" % (which, seen, losses, metrics.get("test_mse")))
    assert metrics["trained_epochs"] == 4 and len(seen) >= 4
    assert all(s and pq[0] >= 2 and 0 < pq[1] <= 64 and 0 < pq[2] <= 64 for s, pq, _ in seen), seen
    assert torch.isfinite(pred).all() and all(np.isfinite(v) for v in losses)
    assert abs(losses[0] - v_on) <= 1e-4 * abs(v_on), (losses[0], v_on)


# ---- 10. what is not served -------------------------------------------------------------------------------------------------------
def test_a_nan_and_a_half_width_beyond_the_maximum_are_not_served(gpu_device):
    from rpgp_amd import ops, settings
    from rpgp_amd.operators import AdditiveRPOperator
    N, J, T = 601, 4, 2
    Z, V, _ = _inputs(N, J, T, 20.0, gpu_device, seed=12)
    prep = ops.Prepared(Z)
    plan = ops.lowrank_train_plan(prep, SCALE, 0.05, panels=True)
    assert plan is not None and plan.panels >= 2
    assert ops.lowrank_train_plan(prep, SCALE, 0.05, panels=True) is plan          # cached on the Prepared
    assert ops.lowrank_train_plan(prep, SCALE, 0.05) is None                       # without the keyword: the sweep, as today
    assert ops.lowrank_train_plan(prep, SCALE, 0.05, max_rank=128) is None
    assert prep.rank == 0                                                          # Prepared.rank is not touched
    # below the cap the keyword changes nothing: the single-interval plan serves, with its bits
    Zs, Vs, _ = _inputs(N, J, T, 4.0, gpu_device, seed=13)
    ps = ops.Prepared(Zs)
    single = ops.LowrankTrainPlan(ps, 2.0 ** -26)
    both = ops.LowrankTrainPlan(ps, 2.0 ** -26, panels=True)
    assert single.served and both.served and both.panels == 0 and (both.p, both.q) == (single.p, single.q)
    assert torch.equal(_raw_product(single, ps, Vs, SCALE, 0.3), _raw_product(both, ps, Vs, SCALE, 0.3))
    # one NaN in Z
    Zn = Z.clone()
    Zn[17, 2] = float("nan")
    pn = ops.Prepared(Zn)
    assert not pn.fast_ok
    assert ops.lowrank_train_plan(pn, SCALE, 0.05, panels=True) is None
    assert not ops.LowrankTrainPlan(pn, TOL, panels=True).served
    # a half-width beyond the 16 panels
    Zw, Vw, _ = _inputs(N, J, T, 150.0, gpu_device, seed=14)
    pw = ops.Prepared(Zw)
    assert ops.lowrank_train_plan(pw, SCALE, 0.05, panels=True) is None
    assert not ops.LowrankTrainPlan(pw, TOL, panels=True).served
    outs = []
    for on in (False, True):
        op = AdditiveRPOperator(Zw, outputscale=torch.tensor(SCALE, device=gpu_device))
        with settings.lowrank_kernel(on), settings.lowrank_panels(on):
            assert op.lowrank_form(0.05) is None and op.lowrank_panels is None
            outs.append(op._matmul(Vw))
    assert torch.equal(outs[0], outs[1])
