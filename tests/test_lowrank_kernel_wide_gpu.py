"""Chebyshev ranks 65 ... 128 in the low-rank product kernels (plans of rpgp_lowrank_create_cap; settings.lowrank_kernel under
settings.lowrank_max_rank above 64): the product and the bilinear derivative, plain and weighted, at every padded rank
72 ... 128 against the float64 oracles and the exact sweeps; shapes at which the rank-sliced projection, the split Clenshaw sum and
the 64-row output blocks can go wrong; j-ranges, row slices, aliasing, guard zones and run-to-run bit identity; the bits of a
rpgp_lowrank_create_tol plan wherever p, q <= 64; a Z beyond the factorised sweep's range guard; both operator kinds in the
native mBCG executor at half-width 10; and fits whose every step is served with 64 < p, q <= 128.

Accuracy conditions (each printed with (p, q) before it is asserted).  At half-widths of 8 and more the float32 coordinates
carry an absolute error of about ulp(h), which the sweep shares, so each result is held to the float64 oracle by the existing gate
or, where that is not met, by 1.25 x the error of the exact direct sweep on the same inputs + 1e-8:
  product: 5e-7 in relative 2-norm;  gZ: 2e-6 overall and 1e-5 on the worst row;  gscale / gcomp: 4e-6."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cmvm, dense_gp, family as fmo

pytestmark = pytest.mark.gpu

KAPPA = 0.8493218002880191        # the coordinate scale of rpgp_prepare: a = (z - mid) kappa
TAIL = 2.0 ** -26
TOL = 1e-12                       # the tolerance of the test plans: every padded rank 72 ... 128 of p and of q has a half-width
SCALE = 0.7
WIDE = tuple(range(72, 129, 8))


def _pad8(r):
    return (r + 7) // 8 * 8


_TABLE = {}


def _half_width_for(kind, padded, tol=TOL):
    """A half-width whose product rank (kind "p") or derivative rank (kind "q", the product rank served as well) pads to
    `padded`, by searching rpgp_lowrank_select's / rpgp_lowrank_grad_select's rank with p_max = 128 (the plan selects at
    h (1 + 2^-20)); the middle of the band, so that the float32 rounding of the range's ends does not leave it."""
    from rpgp_amd import ops
    if tol not in _TABLE:
        bands = {}
        for h in np.arange(0.2, 14.0, 0.05):
            he = float(h) * (1.0 + 2.0 ** -20)
            p = ops.lowrank_post_select(he, tol, p_max=128)[0]
            q = ops.lowrank_grad_select(he, 128, tol)[0]
            if p:
                bands.setdefault(("p", _pad8(p)), []).append(float(h))
                if q:
                    bands.setdefault(("q", _pad8(q)), []).append(float(h))
        _TABLE[tol] = {k: v[len(v) // 2] for k, v in bands.items()}
    assert (kind, padded) in _TABLE[tol], "no half-width with %s padded to %d" % (kind, padded)
    return _TABLE[tol][(kind, padded)]


def _inputs(N, J, T, h, dev, seed):
    """Z with every column spanning [-w, w] (w = h / kappa: the plan's half-width is h, rows 0 and 1 at +-w), L and R standard
    normal (L doubles as the product's V): tests/test_lowrank_grad_gpu.py::_inputs."""
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


def _cap_plan(Z, tol=TOL, cap=128):
    from rpgp_amd import ops
    prep = ops.Prepared(Z)
    return prep, ops.LowrankTrainPlan(prep, tol, max_rank=cap)


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


def _raw_grad(plan, L, R, gZ, gout, j0, j1, scale, w=None):
    from rpgp_amd import _lib, ops
    lib = _lib.load()
    N, J, T = plan.N, plan.J, L.shape[1]
    nbytes = lib.rpgp_bilinear_grad_lowrank_workspace_bytes(plan.handle, N, T)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=L.device)
    if w is None:
        rc = lib.rpgp_bilinear_grad_lowrank(plan.handle, L.data_ptr(), R.data_ptr(), gZ.data_ptr(), gout.data_ptr(), N, J, T,
                                            j0, j1, float(scale), ws.data_ptr(), ws.numel(), ops._stream())
    else:
        rc = lib.rpgp_bilinear_grad_lowrank_weighted(plan.handle, w.data_ptr(), L.data_ptr(), R.data_ptr(), gZ.data_ptr(),
                                                     gout.data_ptr(), N, J, T, j0, j1, float(scale), ws.data_ptr(), ws.numel(),
                                                     ops._stream())
    torch.cuda.synchronize()
    return rc


# ---- 1. the product -----------------------------------------------------------------------------------------------------------
def _check_product(dev, N, J, T, PB, seed):
    from rpgp_amd import ops
    h = _half_width_for("p", PB)
    Z, V, _ = _inputs(N, J, T, h, dev, seed)
    prep, plan = _cap_plan(Z)
    assert plan.p > 64 and _pad8(plan.p) == PB, (plan.p, PB)
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
        print("product N %d J %d T %d p %d q %d (PB %d, h %.2f) noise %.1f: plain %.2e (sweep %.2e), weighted %.2e (sweep %.2e)"
              % (N, J, T, plan.p, plan.q, PB, h, noise, e, es, ew, esw))
        assert _held(e, 5e-7, es), (e, es, plan.p)
        assert _held(ew, 5e-7, esw), (ew, esw, plan.p)
        # repeated calls are bit-identical; w = 1 gives the bits of the unweighted entry
        assert torch.equal(_raw_product(plan, prep, V, SCALE, noise), out)
        assert torch.equal(_raw_product(plan, prep, V, SCALE, noise, w=w), outw)
        assert torch.equal(_raw_product(plan, prep, V, SCALE, noise, w=ones), out)
        if N > 2:
            assert not torch.equal(out, sweep)                  # really the other path
    return Z, V, prep, plan, w


@pytest.mark.parametrize("PB", WIDE)
def test_product_at_every_padded_rank(gpu_device, PB):
    """N = 2 049: one row past a 2 048-row projection block (two blocks per slice, the second with one row), a ragged 64-row
    output block.  PB - 64 runs from 8 to 64: the upper rank slice from nearly empty to full."""
    _check_product(gpu_device, 2049, 3, 2, PB, seed=PB)


# a ragged wave, a wave and one row, three projection blocks with a ragged last one and T = 11; J = 7: waves with one and with two
# projections in the output pass.  (One row alone has the range 0 and the rank 1 whatever the cap: test_single_row.)
@pytest.mark.parametrize("N,J,T", [(2, 1, 1), (63, 7, 5), (65, 7, 1), (4613, 7, 11)])
@pytest.mark.parametrize("PB", [80, 120])
def test_product_shapes(gpu_device, N, J, T, PB):
    _check_product(gpu_device, N, J, T, PB, seed=N + 7 * T + J + PB)


def test_product_with_64_projections_at_the_largest_rank(gpu_device):
    """J = 64 at PB 128: U fills the output pass's 32 KB of LDS in 8 dwordx4 trips, every wave takes 16 projections."""
    _check_product(gpu_device, 130, 64, 1, 128, seed=9)


def test_single_row(gpu_device):
    """One point is a constant kernel: rank 1 under any cap, served by the cap plan with the kernels of rank 8."""
    from rpgp_amd import ops
    Z, V, R = _inputs(1, 1, 1, 9.0, gpu_device, seed=1)
    prep, plan = _cap_plan(Z)
    assert plan.served and (plan.p, plan.q) == (1, 1)
    out = _raw_product(plan, prep, V, SCALE, 0.3)
    assert abs(out.item() - (SCALE + 0.3) * V.item()) <= 1e-6 * abs(V.item())
    gZ, gs = ops.bilinear_grad_lowrank(plan, V, R, SCALE)
    assert float(gZ.abs().max()) == 0.0


@pytest.mark.parametrize("PB", [72, 128])
def test_product_j_ranges_row_slices_and_aliasing(gpu_device, PB):
    from rpgp_amd import ops
    N, J, T = 2049, 3, 2
    Z, V, _ = _inputs(N, J, T, _half_width_for("p", PB), gpu_device, seed=40 + PB)
    prep, plan = _cap_plan(Z)
    assert _pad8(plan.p) == PB
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
        print("PB %d columns [%d, %d): %.2e (sweep %.2e)" % (PB, j0, j1, e, es))
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


# ---- 2. the derivative --------------------------------------------------------------------------------------------------------
def _check_grad(dev, N, J, T, QB, seed):
    from rpgp_amd import ops
    h = _half_width_for("q", QB)
    Z, L, R = _inputs(N, J, T, h, dev, seed)
    prep, plan = _cap_plan(Z)
    assert plan.served and plan.q > 64 and _pad8(plan.q) == QB, (plan.p, plan.q, QB)
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
    print("derivative N %d J %d T %d p %d q %d (QB %d, h %.2f): gZ %.2e (sweep %.2e) rows %.2e (sweep %.2e) gscale %.2e (sweep %.2e)"
          % (N, J, T, plan.p, plan.q, QB, h, e, es, r, rs, c, cs))
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
    assert abs(float(oc.double().sum()) - gs.item()) <= 1e-6 * abs(gs.item())
    return Z, L, R, prep, plan, w, gZ, wZ, wc


@pytest.mark.parametrize("QB", WIDE)
def test_derivative_at_every_padded_rank(gpu_device, QB):
    """QB - 64 runs from 8 to 64: the upper part of the split Clenshaw sum from nearly empty to full."""
    _check_grad(gpu_device, 2049, 3, 2, QB, seed=100 + QB)


@pytest.mark.parametrize("N,J,T", [(63, 7, 5), (4613, 7, 11)])
@pytest.mark.parametrize("QB", [80, 120])
def test_derivative_shapes(gpu_device, N, J, T, QB):
    _check_grad(gpu_device, N, J, T, QB, seed=N + 7 * T + J + QB)


def test_derivative_with_64_projections_and_16_right_hand_sides(gpu_device):
    _check_grad(gpu_device, 257, 64, 16, 104, seed=13)


def test_derivative_j_ranges_leave_the_rest_untouched(gpu_device):
    N, J, T = 777, 7, 5
    Z, L, R, prep, plan, w, gZ_full, wZ_full, wc_full = _check_grad(gpu_device, N, J, T, 96, seed=3)
    total = torch.zeros((), dtype=torch.float64)
    for j0, j1 in ((0, 2), (2, 3), (3, 7)):
        gZ = torch.full((N, J), float("nan"), device=gpu_device)
        gs = torch.full((3,), float("nan"), device=gpu_device)
        assert _raw_grad(plan, L, R, gZ, gs[1:2], j0, j1, SCALE) == 0
        assert torch.isnan(gZ[:, :j0]).all() and torch.isnan(gZ[:, j1:]).all() and torch.isnan(gs[0]) and torch.isnan(gs[2])
        assert torch.equal(gZ[:, j0:j1], gZ_full[:, j0:j1])
        total += gs[1].double().cpu()
        gZ = torch.full((N, J), float("nan"), device=gpu_device)
        gc = torch.full((J,), float("nan"), device=gpu_device)
        assert _raw_grad(plan, L, R, gZ, gc, j0, j1, SCALE, w=w) == 0
        assert torch.isnan(gZ[:, :j0]).all() and torch.isnan(gZ[:, j1:]).all()
        assert torch.isnan(gc[:j0]).all() and torch.isnan(gc[j1:]).all()
        assert torch.equal(gZ[:, j0:j1], wZ_full[:, j0:j1]) and torch.equal(gc[j0:j1], wc_full[j0:j1])
    from rpgp_amd import ops
    gs_full = ops.bilinear_grad_lowrank(plan, L, R, SCALE)[1]
    assert abs(float(total) - gs_full.item()) <= 1e-6 * abs(gs_full.item())


def test_a_cap_plan_whose_q_exceeds_the_cap_answers_the_error_code(gpu_device):
    from rpgp_amd import _lib, ops
    Z, L, R = _inputs(300, 4, 3, _half_width_for("p", 88), gpu_device, seed=5)
    prep, wide = _cap_plan(Z)
    assert wide.served and wide.q > wide.p > 64
    prep, plan = _cap_plan(Z, cap=wide.p)                     # the product rank fits the cap, the derivative rank does not
    assert plan.p == wide.p and plan.q == 0 and not plan.served
    lib = _lib.load()
    assert lib.rpgp_bilinear_grad_lowrank_workspace_bytes(plan.handle, 300, 3) == 0
    assert lib.rpgp_lowrank_grad_bytes(plan.handle) == 2 * _pad8(wide.p) ** 2 * 8
    w = _weights(4, gpu_device)
    for ww in (None, w):
        gZ = torch.zeros(300, 4, device=gpu_device)
        go = torch.zeros(4, device=gpu_device)
        assert _raw_grad(plan, L, R, gZ, go, 0, 4, 1.0, w=ww) == _lib.RPGP_EINVAL
        assert float(gZ.abs().max()) == 0.0 and float(go.abs().max()) == 0.0
    with pytest.raises(ValueError):
        ops.bilinear_grad_lowrank(plan, L, R, 1.0)
    # the product of that plan is the wide plan's, bit for bit
    assert torch.equal(_raw_product(plan, prep, L, SCALE, 0.3), _raw_product(wide, prep, L, SCALE, 0.3))
    # grad_prepare asks for the plan's own size: the 64 KiB of the rank-64 plans are too small here
    small = torch.empty(_lib.RPGP_LOWRANK_GRAD_BYTES, dtype=torch.uint8, device=gpu_device)
    q = ctypes.c_int(0)
    assert lib.rpgp_lowrank_grad_prepare(wide.handle, TOL, small.data_ptr(), small.numel(), ctypes.byref(q),
                                         ops._stream()) == _lib.RPGP_EWORKSPACE


# ---- 3. the same bits below the old cap ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [8, 40, 63])
def test_same_bits_as_a_create_tol_plan_below_the_old_cap(gpu_device, target):
    from rpgp_amd import _lib, ops
    h = next(float(h) for h in np.arange(0.1, 9.0, 0.02)
             if target - 3 <= ops.lowrank_grad_select(float(h) * (1.0 + 2.0 ** -20), 128, TAIL)[0] <= target)
    N, J, T = 2049, 5, 3
    Z, L, R = _inputs(N, J, T, h, gpu_device, seed=target)
    prep = ops.Prepared(Z)
    old = ops.LowrankTrainPlan(prep, TAIL)
    new = ops.LowrankTrainPlan(prep, TAIL, max_rank=128)
    print("target %d: p %d q %d" % (target, new.p, new.q))
    assert (old.p, old.q) == (new.p, new.q) and 0 < new.p <= new.q <= 64 and target - 3 <= new.q <= target
    lib = _lib.load()
    assert lib.rpgp_lowrank_grad_bytes(old.handle) == 65536 and lib.rpgp_lowrank_grad_bytes(new.handle) == 2 * 128 * 128 * 8
    assert lib.rpgp_mvm_sym_lowrank_workspace_bytes(old.handle, N, T) == lib.rpgp_mvm_sym_lowrank_workspace_bytes(new.handle, N, T)
    w = _weights(J, gpu_device)
    for noise in (0.0, 0.3):
        assert torch.equal(_raw_product(old, prep, L, SCALE, noise), _raw_product(new, prep, L, SCALE, noise))
        assert torch.equal(_raw_product(old, prep, L, SCALE, noise, w=w), _raw_product(new, prep, L, SCALE, noise, w=w))
    assert torch.equal(_raw_product(old, prep, L, SCALE, 0.0, world=3, rank=1), _raw_product(new, prep, L, SCALE, 0.0, world=3, rank=1))
    a, b = ops.bilinear_grad_lowrank(old, L, R, SCALE), ops.bilinear_grad_lowrank(new, L, R, SCALE)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = ops.bilinear_grad_lowrank_weighted(old, w, L, R, SCALE), ops.bilinear_grad_lowrank_weighted(new, w, L, R, SCALE)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # and the default product of the Prepared (rank 64) is that plan's too
    assert prep.rank == old.p
    assert torch.equal(ops.mvm_sym_prepared(prep, L, SCALE, 0.3), _raw_product(new, prep, L, SCALE, 0.3))


class _RawPlan:
    """A plan made at the ctypes level, with what _raw_product and _raw_grad read of a LowrankTrainPlan."""

    def __init__(self, prep, entry, nbytes, *args):
        from rpgp_amd import _lib, ops
        self.N, self.J = prep.N, prep.J
        self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=prep.device)
        p, h = ctypes.c_int(0), ctypes.c_void_p(None)
        rc = getattr(_lib.load(), entry)(prep.buf.data_ptr(), prep.N, prep.J, prep.max_abs, *args, self.buf.data_ptr(),
                                         self.buf.numel(), ctypes.byref(p), ctypes.byref(h), ops._stream())
        assert rc == 0, (entry, rc)
        self.p, self.handle = p.value, h.value

    def grad_prepare(self, tol):
        from rpgp_amd import _lib, ops
        lib = _lib.load()
        self.dcoef = torch.empty(int(lib.rpgp_lowrank_grad_bytes(self.handle)), dtype=torch.uint8, device=self.buf.device)
        q = ctypes.c_int(0)
        assert lib.rpgp_lowrank_grad_prepare(self.handle, tol, self.dcoef.data_ptr(), self.dcoef.numel(), ctypes.byref(q),
                                             ops._stream()) == 0
        return q.value


def test_the_three_creators_give_the_same_plan_at_the_cap_64(gpu_device):
    """rpgp_lowrank_create, rpgp_lowrank_create_tol at 2^-26 and rpgp_lowrank_create_cap at 2^-26 with the cap 64 on one
    Prepared, at the ctypes level (ops builds every training plan through the cap entry, so no other test reaches
    rpgp_lowrank_create_tol): the same p, the same q after rpgp_lowrank_grad_prepare on the last two, and the same bits of the
    product (all three) and of the derivative (the two with one).  N = 2049: two projection blocks, the smallest N at which
    the block sum has more than one term."""
    from rpgp_amd import _lib, ops
    lib = _lib.load()
    N, J, T = 2049, 3, 2
    Z, L, R = _inputs(N, J, T, 3.0, gpu_device, seed=64)
    prep = ops.Prepared(Z)
    assert prep.fast_ok
    plans = [_RawPlan(prep, "rpgp_lowrank_create", lib.rpgp_lowrank_plan_bytes(N, J)),
             _RawPlan(prep, "rpgp_lowrank_create_tol", lib.rpgp_lowrank_plan_bytes(N, J), TAIL),
             _RawPlan(prep, "rpgp_lowrank_create_cap", lib.rpgp_lowrank_plan_bytes_cap(N, J, 64), TAIL, 64)]
    try:
        print("p %s" % [pl.p for pl in plans])
        assert 0 < plans[0].p <= 64 and plans[1].p == plans[0].p and plans[2].p == plans[0].p
        assert all(pl.handle for pl in plans)
        q = [pl.grad_prepare(TAIL) for pl in plans[1:]]
        print("q %s" % q)
        assert 0 < q[0] <= 64 and q[1] == q[0]
        outs = [_raw_product(pl, prep, L, SCALE, 0.3) for pl in plans]
        assert torch.isfinite(outs[0]).all() and torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])
        grads = []
        for pl in plans[1:]:
            gZ, gs = torch.zeros(N, J, device=gpu_device), torch.zeros(1, device=gpu_device)
            assert _raw_grad(pl, L, R, gZ, gs, 0, J, SCALE) == 0
            grads.append((gZ, gs))
        assert torch.isfinite(grads[0][0]).all() and float(grads[0][0].abs().max()) > 0.0
        assert torch.equal(grads[1][0], grads[0][0]) and torch.equal(grads[1][1], grads[0][1])
    finally:
        for pl in plans:
            lib.rpgp_lowrank_destroy(pl.handle)


# ---- 4. beyond fast_ok ----------------------------------------------------------------------------------------------------------
def test_half_width_12_is_served_beyond_the_sweeps_range_guard(gpu_device):
    from rpgp_amd import ops
    N, J, T = 3001, 6, 3
    Z, L, R = _inputs(N, J, T, 12.0, gpu_device, seed=12)
    prep = ops.Prepared(Z)
    assert not prep.fast_ok and abs(prep.max_abs - 12.0) <= 1e-3
    assert ops.lowrank_train_plan(prep, SCALE, 0.05) is None                       # the default cap: the sweep
    plan = ops.lowrank_train_plan(prep, SCALE, 0.05, max_rank=128)
    assert plan is not None and 64 < plan.p <= plan.q <= 128
    assert ops.lowrank_train_plan(prep, SCALE, 0.05, max_rank=128) is plan         # cached on the Prepared
    assert prep.rank == 0                                                          # Prepared.rank stays at 64 and fast_ok
    Zh, Lh, Rh = _np(Z), _np(L), _np(R)
    ref = cmvm.mvm(Zh, Zh, Lh, SCALE, 0.3)
    e = _rel(_np(_raw_product(plan, prep, L, SCALE, 0.3)), ref)
    es = _rel(_np(ops.mvm_sym(Z, L, SCALE, 0.3)), ref)
    gZ_ref, gs_ref = dense_gp.bilinear_grad(Zh, Lh, Rh, SCALE)
    gZ, gs = ops.bilinear_grad_lowrank(plan, L, R, SCALE)
    sZ, ss = ops.bilinear_grad(Z, L, R, SCALE)
    g, gsw = _rel(_np(gZ), gZ_ref), _rel(_np(sZ), gZ_ref)
    r, rs = _rows(_np(gZ), gZ_ref), _rows(_np(sZ), gZ_ref)
    c, cs = abs(gs.item() - float(gs_ref)) / abs(float(gs_ref)), abs(ss.item() - float(gs_ref)) / abs(float(gs_ref))
    print("h 12 p %d q %d: product %.2e (sweep %.2e) gZ %.2e (sweep %.2e) rows %.2e (sweep %.2e) gscale %.2e (sweep %.2e)"
          % (plan.p, plan.q, e, es, g, gsw, r, rs, c, cs))
    assert _held(e, 5e-7, es) and _held(g, 2e-6, gsw) and _held(r, 1e-5, rs) and _held(c, 4e-6, cs)
    # the same Z with one NaN is not served
    Zn = Z.clone()
    Zn[17, 2] = float("nan")
    pn = ops.Prepared(Zn)
    assert not pn.fast_ok
    assert ops.lowrank_train_plan(pn, SCALE, 0.05, max_rank=128) is None
    assert not ops.LowrankTrainPlan(pn, TOL, max_rank=128).served


# ---- 5. the native executor ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_wide_operators_in_the_native_executor(gpu_device, weighted):
    """The bound of the executor tests in tests/test_lowrank_train_gpu.py / tests/test_lowrank_family_gpu.py: mean residual below
    2 tol and the solution within 100 tol of the float64 dense solve.  The iteration counts are printed beside the sweep's."""
    from rpgp_amd import settings, linear_cg as lcg
    from rpgp_amd.operators import AdditiveRPOperator, FamilyAdditiveOperator, AddedDiagOperator
    from rpgp_amd.precond import pivoted_cholesky, WoodburyPreconditioner
    N, J, T, noise, s, tol = 4613, 7, 11, 0.3, 0.8, 1e-4
    Z, rhs, _ = _inputs(N, J, T, 10.0, gpu_device, seed=4)
    w = _weights(J, gpu_device, signed=False)

    def make():
        if weighted:
            return FamilyAdditiveOperator(Z, outputscale=torch.tensor(s, device=gpu_device), comp_weights=w)
        return AdditiveRPOperator(Z, outputscale=torch.tensor(s, device=gpu_device))

    out, its, ranks = {}, {}, None
    for on in (False, True):
        op = make()
        khat = AddedDiagOperator(op, torch.tensor(noise, device=gpu_device), noise_value=noise)
        pre = WoodburyPreconditioner(pivoted_cholesky(op._diagonal(), op._get_rows, 15), noise)
        with settings.lowrank_kernel(on), settings.lowrank_max_rank(128):
            before = lcg.stats.get("native_calls", 0)
            out[on] = lcg.linear_cg(khat._matmul, rhs, operator=khat, tolerance=tol, max_iter=500, preconditioner=pre)
            assert lcg.stats.get("native_calls", 0) == before + 1
            its[on] = lcg.stats["last_iterations"]
        assert op.lowrank_served == on
        if on:
            ranks = op.lowrank_ranks
            assert 64 < ranks[0] <= ranks[1] <= 128 and not op._prep.fast_ok, ranks
    # under the default cap the same operator is the sweep
    op = make()
    with settings.lowrank_kernel(True):
        assert op.lowrank_form(noise) is None
    Zd = _np(Z)
    Kh = fmo.kernel_matrix(Zd, Zd, "RBF", 1, _np(w) if weighted else np.ones(J), s) + noise * np.eye(N)
    b = _np(rhs)
    x_ref = np.linalg.solve(Kh, b)
    xd = _np(out[True])
    res = np.linalg.norm(Kh @ xd - b, axis=0) / np.linalg.norm(b, axis=0)
    err = np.linalg.norm(xd - x_ref) / np.linalg.norm(x_ref)
    err_sweep = np.linalg.norm(_np(out[False]) - x_ref) / np.linalg.norm(x_ref)
    print("executor %s: ranks %s, iterations low-rank %d sweep %d, residual %.2e, solution %.2e (sweep %.2e)"
          % ("weighted" if weighted else "plain", ranks, its[True], its[False], res.mean(), err, err_sweep))
    assert res.mean() < 2.0 * tol, res
    assert err < 100.0 * tol, err


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------
KINDS = {
    "plain": ("additive_rp", {"J": 8, "noise_prior": True, "kernel_type": "RBF", "learn_proj": False, "prescale": True}),
    "weighted": ("rp_poly", {"k": 1, "J": 8, "noise_prior": True, "kernel_type": "RBF", "learn_proj": False, "weighted": True}),
}
FIT_H = 9.5


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


def _step(model, mll, X, y, on, cap):
    from rpgp_amd import settings
    params = [p for p in model.parameters() if p.requires_grad]
    with settings.lowrank_kernel(on), settings.lowrank_max_rank(cap):
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
    """Every decision of the operator's lowrank_form: (served, (p, q) or None, the Prepared's (max_abs, fast_ok))."""
    seen = []
    orig = cls.lowrank_form

    def rec(self, noise=None):
        undecided = self._lowrank is None
        r = orig(self, noise)
        if undecided:
            pr = self._prep
            seen.append((r is not None, (r.p, r.q) if r is not None else None, (pr.max_abs, pr.fast_ok) if pr is not None else None))
        return r
    monkeypatch.setattr(cls, "lowrank_form", rec)
    return seen


@pytest.mark.parametrize("which", ["plain", "weighted"])
def test_fit_at_half_width_9_5(gpu_device, monkeypatch, which):
    """The gates of tests/test_lowrank_train_gpu.py for the first step (value within 1e-4, all raw gradients as one vector within
    1e-3 of the settings-off step); under the default cap the step IS the settings-off step; and a train_exact_gp fit, prediction
    included, whose every decision is served with 64 < p, q <= 128."""
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
        v_off, g_off = _step(model, mll, Xd, yd, False, 64)
        assert not any(s[0] for s in seen), seen
        seen.clear()
        v_def, g_def = _step(model, mll, Xd, yd, True, 64)
        assert seen and not any(s[0] for s in seen), seen     # decided, and not served under the default cap
        assert v_def == v_off and all(torch.equal(a, b) for a, b in zip(g_def, g_off))
        seen.clear()
        v_on, g_on = _step(model, mll, Xd, yd, True, 128)
        assert seen and all(s[0] for s in seen), seen
        (p, q), (max_abs, fast_ok) = seen[0][1], seen[0][2]
        rel = _grad_rel(g_on, g_off)
        print("%s first step: ranks (%d, %d) max_abs %.2f fast_ok %s, value on %.8f off %.8f, gradients %.2e"
              % (which, p, q, max_abs, fast_ok, v_on, v_off, rel))
        assert 64 < p <= 128 and 64 < q <= 128
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
    with _Settings(settings.lowrank_kernel(True), settings.lowrank_max_rank(128), settings.eval_cg_tolerance(1e-4)):
        metrics, pred, fitted = train_exact_gp(X[:N], y[:N], X[N:], y[N:], kind, mk, tk, devices=[str(dev)],
                                               skip_random_restart=True, skip_posterior_variances=True)
    print("%s fit: decisions %s, losses %s, test mse %s" % (which, seen, losses, metrics.get("test_mse")))
    assert metrics["trained_epochs"] == 4 and len(seen) >= 4
    assert all(s and 64 < pq[0] <= 128 and 64 < pq[1] <= 128 for s, pq, _ in seen), seen
    assert torch.isfinite(pred).all() and all(np.isfinite(v) for v in losses)
    assert abs(losses[0] - v_on) <= 1e-4 * abs(v_on), (losses[0], v_on)
