"""The float64 parity kernels (csrc/rpgp_f64.hip, csrc/rpgp_ski_f64.hip) against the float64 oracle, entry by entry, at every
tiling edge: |got - ref| <= C u A with the magnitudes A and the constants C of tests/f64_reference.py (measured on the CPU by
tests/test_f64_reference_host.py, which also shows by mutation that these cases reach every loop edge of the kernels).

Cases -> what they reach (rpgp_f64.hip): (4161, 4161, 5, 17) the second tile of a column split, a one-column ragged tile
after a full one, T chunks 12 + 5, pieces 4 + 1; (4097, ...) a last split of one column; (321, ., 35, 14) pieces 20 + 8 + 4 +
2 + 1 and chunks 12 + 2; (2305, 7361, 3, 16) rectangular multi-tile, chunks 12 + 4; (4161, 130) M > N; (7, 4500, 8, 13) the
8-wide piece, chunks 12 + 1; the raw-entry cases leading dimensions, J-slices and guard columns; (110000, 3, 20) the
projection's grid-stride loop.  rpgp_ski_f64.hip: every form at (130, 33, 3, 3), G = 16, for both grid rules, weighted and not,
every radial kind; T = 70 (host pieces 64 + 6); G = 8; N = 1; clamped rows (fr.SKI_SWEEP); the staged entries, each stage
with the constant measured for it.  No bitwise repeatability is
asserted: the column splits and the histograms add with float64 atomics.  Each test prints its figure (`F64GATE ...`, -s).

Worst |got - ref| / (u A) on an MI355X where this was written, beside the host's larger ratio and the constant in force
(the product and the derivative move in the second digit from run to run with the order of the atomics):
mvm 3.01 | 2.37 | 16; dense 4.58 | 4.53 | 32; bilinear 0.54 | 0.21 | 1; bilinear_dense 1.08 | 0.92 | 4; project 0.00 | 2.79 |
16 (the device's fma chain is numpy's, bit for bit); project_grad 1.88 | 1.76 | 8; ski 0.42 | 0.55 | 4 (both at the dense
block of (257, 5, 1, 2), G = 8; the starred forms stay below 0.05); ski_scatter 0.27 | 0.31 | 2; ski_gather 0.43 | 0.35 | 2;
ski_grid_product 1.69 | 0.95 | 4.  No kernel needed a fix."""
import numpy as np
import pytest
import torch

from tests import f64_reference as fr
from tests.oracle_backend import OracleBackend

pytestmark = pytest.mark.gpu

S = fr.SCALE


def _gate(entry, case, got, ref, A, column=False):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    r = (fr.column_ratio if column else fr.ratio)(got, ref, A)
    print("F64GATE %-16s %-44s ratio %8.3f  C %g" % (entry, case, r, fr.C[entry]))
    assert r <= fr.C[entry], (entry, case, r)
    return r


def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=dev)


def _lib():
    from rpgp_amd import _lib, ops
    return _lib.load(), ops._stream(), _lib


# ---- rpgp_mvm_f64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,J,T", fr.MVM_CASES)
def test_product(gpu_device, M, N, J, T):
    from rpgp_amd import ops
    Z1, Z2, V, noise = fr.mvm_inputs(M, N, J, T)
    Z1t, Z2t, Vt = _dev(gpu_device, Z1, Z2, V)
    out = ops.mvm_sym(Z2t, Vt, S, noise) if M == N else ops.mvm_rect(Z1t, Z2t, Vt, S)
    assert out.dtype == torch.float64 and tuple(out.shape) == (M, T)
    _gate("mvm", (M, N, J, T), out, fr.mvm_ref(Z1, Z2, V, S, noise), fr.mvm_mag(Z1, Z2, V, S, noise))


def test_product_slice_and_leading_dimensions(gpu_device):
    lib, st, _ = _lib()
    Z1, Z2, V = fr.mvm_slice_inputs()
    (M, ld1), (N, ld2), T, (j0, j1) = Z1.shape, Z2.shape, V.shape[1], fr.SLICE
    assert (ld1, ld2) == fr.SLICE_LD
    Z1t, Z2t, Vt = _dev(gpu_device, Z1, Z2, V)
    out = _nan(gpu_device, M, T)
    rc = lib.rpgp_mvm_f64(Z1t.data_ptr(), Z2t.data_ptr(), Vt.data_ptr(), out.data_ptr(), M, N, ld1, ld2, T, j0, j1, S, 0.0, st)
    torch.cuda.synchronize()
    assert rc == 0
    z1, z2 = Z1[:, j0:j1], Z2[:, j0:j1]
    _gate("mvm", "slice (3, 10), ldz 12 / 14", out, fr.mvm_ref(z1, z2, V, S), fr.mvm_mag(z1, z2, V, S))


def test_product_large_coordinates_and_duplicates(gpu_device):
    from rpgp_amd import ops
    Z, V = fr.large_coordinate_inputs()
    N, J = Z.shape
    Zt, Vt = _dev(gpu_device, Z, V)
    ref_d = fr.dense_ref(Z, Z, 1.0)
    assert (ref_d == 0.0).any() and (ref_d[np.arange(10), N - 1 - np.arange(10)] == J).all()   # underflows; duplicates are J
    Kd = ops.dense(Zt, Zt, 1.0).cpu().numpy()
    assert (Kd[np.arange(10), N - 1 - np.arange(10)] == J).all() and (np.diag(Kd) == J).all()
    _gate("dense", "Z = 30 x normal", Kd, ref_d, fr.dense_mag(Z, Z, 1.0))
    out = ops.mvm_sym(Zt, Vt, S, fr.NOISE)
    _gate("mvm", "Z = 30 x normal", out, fr.mvm_ref(Z, Z, V, S, fr.NOISE), fr.mvm_mag(Z, Z, V, S, fr.NOISE))


def test_product_overwrites_its_output(gpu_device):
    from rpgp_amd import ops
    Z1, Z2, V, noise = fr.mvm_inputs(65, 65, 3, 2)
    Zt, Vt = _dev(gpu_device, Z2, V)
    out = _nan(gpu_device, 65, 2)
    res = ops.mvm_sym(Zt, Vt, S, noise, out=out)
    assert res.data_ptr() == out.data_ptr()
    _gate("mvm", "out= pre-filled with NaN", out, fr.mvm_ref(Z2, Z2, V, S, noise), fr.mvm_mag(Z2, Z2, V, S, noise))


def test_product_error_codes(gpu_device):
    lib, st, L = _lib()
    Z1t, Z2t, Vt = _dev(gpu_device, *fr.mvm_slice_inputs())
    M, N, T = Z1t.shape[0], Z2t.shape[0], Vt.shape[1]
    out = _nan(gpu_device, M, T)
    call = lambda m, n, l1, l2, a, b, noise: lib.rpgp_mvm_f64(Z1t.data_ptr(), Z2t.data_ptr(), Vt.data_ptr(), out.data_ptr(), m, n,
                                                              l1, l2, T, a, b, S, noise, st)
    assert call(M, N, 12, 14, 3, 10, 0.2) == L.RPGP_EINVAL            # noise with M != N
    assert call(M, N, 12, 14, 5, 5, 0.0) == L.RPGP_EINVAL             # j1 <= j0
    assert call(M, N, 9, 14, 3, 10, 0.0) == L.RPGP_EINVAL and call(M, N, 12, 9, 3, 10, 0.0) == L.RPGP_EINVAL   # ldz < j1
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- rpgp_dense_f64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,J", fr.DENSE_CASES)
def test_dense_block(gpu_device, M, N, J):
    from rpgp_amd import ops
    Z1, Z2 = fr.dense_inputs(M, N, J)
    Kd = ops.dense(*_dev(gpu_device, Z1, Z2), S)
    _gate("dense", (M, N, J), Kd, fr.dense_ref(Z1, Z2, S), fr.dense_mag(Z1, Z2, S))


@pytest.mark.parametrize("sliced", [False, True])
def test_dense_block_raw_entry(gpu_device, sliced):
    """ldo = N + 3 with NaN guard columns; the slice (3, 10) of a 12-wide Z1 and a 14-wide Z2."""
    lib, st, _ = _lib()
    if sliced:
        Z1, Z2, _ = fr.mvm_slice_inputs()
        j0, j1 = fr.SLICE
    else:
        Z1, Z2 = fr.dense_inputs(33, 300, 11)
        j0, j1 = 0, 11
    M, N = Z1.shape[0], Z2.shape[0]
    Z1t, Z2t = _dev(gpu_device, Z1, Z2)
    buf = _nan(gpu_device, M, N + 3)
    rc = lib.rpgp_dense_f64(Z1t.data_ptr(), Z2t.data_ptr(), buf.data_ptr(), M, N, Z1.shape[1], Z2.shape[1], N + 3, j0, j1, S, st)
    torch.cuda.synchronize()
    assert rc == 0 and torch.isnan(buf[:, N:]).all()
    z1, z2 = Z1[:, j0:j1], Z2[:, j0:j1]
    _gate("dense", "raw, ldo = N + 3, slice %s" % ((j0, j1),), buf[:, :N], fr.dense_ref(z1, z2, S), fr.dense_mag(z1, z2, S))


# ---- rpgp_bilinear_grad_f64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,J,T", fr.BILINEAR_CASES)
def test_derivative(gpu_device, N, J, T):
    from rpgp_amd import ops
    Z, L, R = fr.bilinear_inputs(N, J, T)
    gZ, gs = ops.bilinear_grad(*_dev(gpu_device, Z, L, R), S)
    ref, gs_ref = fr.bilinear_ref(Z, L, R, S)
    A, Ags = fr.bilinear_mag(Z, L, R, S)
    _gate("bilinear", "gZ %s" % ((N, J, T),), gZ, ref, A)
    _gate("bilinear", "gscale %s" % ((N, J, T),), gs.reshape(1), np.array([gs_ref]), np.array([Ags]))


def _raw_bilinear(dev, Z, L, R, j0, j1, ldg):
    lib, st, _ = _lib()
    N, ldz = Z.shape
    Zt, Lt, Rt = _dev(dev, Z, L, R)
    gZ, gs, scratch = _nan(dev, N, ldg), _nan(dev, 1), _nan(dev, N)
    rc = lib.rpgp_bilinear_grad_f64(Zt.data_ptr(), Lt.data_ptr(), Rt.data_ptr(), gZ.data_ptr(), gs.data_ptr(), N, ldz, ldg,
                                    L.shape[1], j0, j1, S, scratch.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == 0
    return gZ, gs


def test_derivative_slice_and_guard_columns(gpu_device):
    N, J, T = 130, 12, 3
    (j0, j1), ldg = fr.SLICE, J + 2
    Z, L, R = fr.bilinear_inputs(N, J, T)
    gZ, gs = _raw_bilinear(gpu_device, Z, L, R, j0, j1, ldg)
    assert torch.isnan(gZ[:, :j0]).all() and torch.isnan(gZ[:, j1:]).all()
    ref, gs_ref = fr.bilinear_ref(Z[:, j0:j1], L, R, S)
    A, Ags = fr.bilinear_mag(Z[:, j0:j1], L, R, S)
    _gate("bilinear", "gZ slice (3, 10), ldg = J + 2", gZ[:, j0:j1], ref, A)
    _gate("bilinear", "gscale slice (3, 10)", gs, np.array([gs_ref]), np.array([Ags]))


# ---- rpgp_bilinear_grad_dense_f64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,J", fr.BILINEAR_DENSE_CASES)
def test_derivative_dense_form(gpu_device, N, J):
    from rpgp_amd import ops
    Z, Sm = fr.bilinear_dense_inputs(N, J)
    gZ, gs = ops.bilinear_grad_dense(*_dev(gpu_device, Z, Sm), S)
    ref, gs_ref = fr.bilinear_dense_ref(Z, Sm, S)
    A, Ags = fr.bilinear_mag(Z, None, None, S, S=Sm)
    _gate("bilinear_dense", "gZ %s" % ((N, J),), gZ, ref, A)
    _gate("bilinear_dense", "gscale %s" % ((N, J),), gs.reshape(1), np.array([gs_ref]), np.array([Ags]))


def _raw_bilinear_dense(dev, Z, Sbuf, j0, j1, ldg):
    lib, st, _ = _lib()
    N, ldz = Z.shape
    Zt, St = _dev(dev, Z, Sbuf)
    gZ, gs, scratch = _nan(dev, N, ldg), _nan(dev, 1), _nan(dev, N)
    rc = lib.rpgp_bilinear_grad_dense_f64(Zt.data_ptr(), St.data_ptr(), gZ.data_ptr(), gs.data_ptr(), N, ldz, ldg, Sbuf.shape[1],
                                          j0, j1, S, scratch.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == 0
    return gZ, gs


def test_derivative_dense_form_leading_dimension(gpu_device):
    N, J = 64, 3
    Z, Sbuf = fr.bilinear_dense_inputs(N, J, N + 5)
    assert np.isnan(Sbuf[:, N:]).all()                                # (a read behind column N would poison the result)
    gZ, gs = _raw_bilinear_dense(gpu_device, Z, Sbuf, 0, J, J)
    ref, gs_ref = fr.bilinear_dense_ref(Z, Sbuf[:, :N], S)
    A, Ags = fr.bilinear_mag(Z, None, None, S, S=Sbuf[:, :N])
    _gate("bilinear_dense", "gZ lds = N + 5", gZ, ref, A)
    _gate("bilinear_dense", "gscale lds = N + 5", gs, np.array([gs_ref]), np.array([Ags]))


def test_derivative_dense_form_slice(gpu_device):
    N, J = 130, 12
    (j0, j1), ldg = fr.SLICE, J + 2
    Z, Sm = fr.bilinear_dense_inputs(N, J)
    gZ, gs = _raw_bilinear_dense(gpu_device, Z, Sm, j0, j1, ldg)
    assert torch.isnan(gZ[:, :j0]).all() and torch.isnan(gZ[:, j1:]).all()
    ref, gs_ref = fr.bilinear_dense_ref(Z[:, j0:j1], Sm, S)
    A, Ags = fr.bilinear_mag(Z[:, j0:j1], None, None, S, S=Sm)
    _gate("bilinear_dense", "gZ slice (3, 10)", gZ[:, j0:j1], ref, A)
    _gate("bilinear_dense", "gscale slice (3, 10)", gs, np.array([gs_ref]), np.array([Ags]))


def test_derivative_forms_agree(gpu_device):
    """S = L R^T + R L^T given densely: the two entry points agree within the sum of their gates."""
    from rpgp_amd import ops
    N, J, T = 321, 35, 14
    Z, L, R = fr.bilinear_inputs(N, J, T)
    Sm = L @ R.T + R @ L.T
    Zt, Lt, Rt, St = _dev(gpu_device, Z, L, R, Sm)
    g1, s1 = ops.bilinear_grad(Zt, Lt, Rt, S)
    g2, s2 = ops.bilinear_grad_dense(Zt, St, S)
    A1, As1 = fr.bilinear_mag(Z, L, R, S)
    A2, As2 = fr.bilinear_mag(Z, None, None, S, S=Sm)
    bound = fr.U * (fr.C["bilinear"] * A1 + fr.C["bilinear_dense"] * A2)
    err = (g1 - g2).abs().cpu().numpy()
    print("F64GATE forms agree: worst |dense - low rank| / bound %.3f" % (err / bound).max())
    assert (err <= bound).all()
    assert abs(float(s1) - float(s2)) <= fr.U * (fr.C["bilinear"] * As1 + fr.C["bilinear_dense"] * As2)


# ---- rpgp_project_f64 / rpgp_project_grad_f64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,J", fr.PROJECT_CASES)
def test_projection_and_its_gradient(gpu_device, N, d, J):
    from rpgp_amd import ops
    X, P, G = fr.project_inputs(N, d, J)
    Xt, Pt, Gt = _dev(gpu_device, X, P, G)
    _gate("project", (N, d, J), ops.project(Xt, Pt), X @ P, fr.project_mag(X, P))
    _gate("project_grad", (N, d, J), ops.project_grad(Xt, Gt), X.T @ G, fr.project_grad_mag(X, G))


# ---- rpgp_ski_f64.hip -------------------------------------------------------------------------------------------------------
def _ski_setup(dev, N, M, J, T, G, rule, weighted, kind="RBF", seed=0):
    from rpgp_amd import ops
    Z, Zs, V, L, R, w = fr.ski_inputs(N, M, J, T, seed)
    host = dict(Z=Z, Zs=Zs, V=V, L=L, R=R)
    dev_t = {k: _dev(dev, a)[0] for k, a in host.items()}
    gp = ops.ski_grid(dev_t["Z"], dev_t["Zs"], G, weights=_dev(dev, w)[0] if weighted else None, rule=rule, kind=kind)
    assert gp.dtype == torch.float64
    cpu_t = {k: torch.from_numpy(a) for k, a in host.items()}
    return host, dev_t, cpu_t, gp, gp.cpu()


@pytest.mark.parametrize("case", fr.SKI_SWEEP, ids=fr.ski_case_id)
def test_ski_forms(gpu_device, case):
    """Every form a case asks for against the oracle with the device's own grid block.  starred: (130, 33, 3, 3) at G = 16, both
    grid rules, weighted and not, every radial kind.  T70: _ski64_mvm and _ski64_bilinear run 64 + 6 columns, gs and gc
    accumulate over the pieces.  single: N = 1 at G = 8, a zero range, the rule's clamp_min decides the grid (the point sits
    at position 2 and does not clamp, so its derivative is gated too).  G8: (257, 5, 1, 2) at the smallest grid.  clamp: the
    block is built from Z alone and every row of Zs clamps in `taps`; product and dense block only (the one-sided derivative
    at a clamped row is a convention, and a training row never clamps)."""
    from rpgp_amd import ops
    name, N, M, J, T, G, rule, weighted, kind, forms = case
    host, both = fr.ski_case_inputs(name, N, M, J, T)
    d = {k: _dev(gpu_device, host[k])[0] for k in ("Z", "Zs", "V", "L", "R")}
    gp = ops.ski_grid(d["Z"], d["Zs"] if both else None, G, weights=_dev(gpu_device, host["w"])[0] if weighted else None,
                      rule=rule, kind=kind)
    assert gp.dtype == torch.float64
    gpn = gp.cpu().numpy()
    g0, h, inv_h, _, _ = fr.ski_block(gpn, J)
    clamps = lambda Zx: np.stack([fr.ski_taps(Zx[:, j], g0[j], inv_h[j], G)[5] for j in range(J)], axis=1)
    assert not clamps(host["Z"]).any()
    if name == "clamp":
        assert clamps(host["Zs"]).all()
    if name == "single":
        assert float(h[0]) <= 1e-12                                   # (the clamp_min's spacing, not a zero one)
    got = {}
    if "product" in forms:
        got["product"] = ops.ski_mvm(d["Z"], d["Z"], gp, d["V"], S, fr.NOISE, G)
    if "rect" in forms:
        got["rect"] = ops.ski_mvm(d["Zs"], d["Z"], gp, d["V"], S, 0.0, G)
    if "diag" in forms:
        got["diag"] = ops.ski_diag(d["Z"], gp, S, G).reshape(-1, 1)
    if "dense" in forms:
        got["dense"] = ops.ski_dense(d["Zs"], d["Z"], gp, S, G)
    if "deriv" in forms:
        gZ, gs, gc = ops.ski_bilinear_grad_comp(d["Z"], gp, d["L"], d["R"], S, G)
        got["gZ"], got["gscale"], got["gcomp"] = gZ, gs.reshape(1, 1), gc.reshape(1, -1)
    oracle = fr.ski_oracle(host, gpn, G, forms)
    assert set(oracle) == set(got)
    for label, (ref, A) in oracle.items():
        assert got[label].dtype == torch.float64 and tuple(got[label].shape) == ref.shape
        _gate("ski", "%s %s" % (fr.ski_case_id(case), label), got[label], ref, A, True)


@pytest.mark.parametrize("rule,weighted", fr.SKI_STAGED)
def test_ski_staged_entries(gpu_device, rule, weighted):
    from rpgp_amd import ops
    lib, st, _ = _lib()
    ob = OracleBackend()
    N, M, J, T, G = 130, 33, 3, 3, 16
    h, d, c, gp, gpc = _ski_setup(gpu_device, N, M, J, T, G, rule, weighted)
    gpn = gpc.numpy()
    Z, L, R, V = d["Z"], d["L"], d["R"], d["V"]
    tag = "staged/%s/%s " % (rule[:3], "w" if weighted else "-")
    # scatter: [W^T L | W^T R] into one J x G x 2T buffer
    hist2 = _nan(gpu_device, J, G, 2 * T)
    scat = lambda src, hoff, zero: lib.rpgp_ski_f64_scatter(Z.data_ptr(), gp.data_ptr(), src.data_ptr(), hist2.data_ptr(), N, J, J, G,
                                                           T, 2 * T, hoff, zero, st)
    assert scat(L, 0, 1) == 0 and scat(R, T, 0) == 0
    torch.cuda.synchronize()
    ref2 = np.concatenate([fr.ski_hist_mag(h["Z"], gpn, h["L"], G, True), fr.ski_hist_mag(h["Z"], gpn, h["R"], G, True)], axis=2)
    A2 = np.concatenate([fr.ski_hist_mag(h["Z"], gpn, h["L"], G), fr.ski_hist_mag(h["Z"], gpn, h["R"], G)], axis=2)
    sep = torch.cat([ops.ski_scatter(Z, gp, L, G), ops.ski_scatter(Z, gp, R, G)], dim=2)
    _gate("ski_scatter", tag + "scatter vs oracle", hist2.reshape(J * G, -1), ob.ski_bilinear_scatter(c["Z"], gpc, c["L"], c["R"], G).reshape(J * G, -1),
          A2.reshape(J * G, -1), True)
    _gate("ski_scatter", tag + "scatter vs separate", hist2.reshape(J * G, -1), sep.reshape(J * G, -1), A2.reshape(J * G, -1), True)
    keep = hist2.clone()
    assert scat(R, T, 0) == 0                                          # zero_first = 0 adds
    torch.cuda.synchronize()
    twice, twiceA = ref2.copy(), A2.copy()                             # (the R half was scattered twice: value and magnitude)
    twice[:, :, T:] *= 2.0
    twiceA[:, :, T:] *= 2.0
    _gate("ski_scatter", tag + "scatter adds", hist2.reshape(J * G, -1), twice.reshape(J * G, -1), twiceA.reshape(J * G, -1), True)
    hist2 = keep
    # grid product, weighted and not, of the V histogram
    hist = ops.ski_scatter(Z, gp, V, G)
    hn = hist.cpu().numpy()
    sens = fr.ski_parts(h["Z"], gpn, G, True)
    H = {}
    for wflag in (1, 0):
        H[wflag] = _nan(gpu_device, J, G, T)
        assert lib.rpgp_ski_f64_grid_product(hist.data_ptr(), gp.data_ptr(), H[wflag].data_ptr(), J, G, T, wflag, st) == 0
        torch.cuda.synchronize()
        ref, A = fr.ski_grid_product_forms(hn, gpn, G, bool(wflag))
        for j in range(J):                                             # (per projection and column, as the constant was measured)
            _gate("ski_grid_product", tag + "grid product weighted=%d j=%d" % (wflag, j), H[wflag][j], ref[j], A[j], True)
    if weighted:
        assert not torch.equal(H[0], H[1])
    oracle_H = ob.ski_grid_product(hist.cpu(), gpc, G)
    for j in range(J):
        _gate("ski_grid_product", tag + "grid product vs oracle j=%d" % j, H[1][j], oracle_H[j], fr.ski_grid_product_forms(hn, gpn, G, True)[1][j], True)
    # gather with and without noise
    Hn = H[1].cpu().numpy()
    for noise in (0.0, fr.NOISE):
        out = _nan(gpu_device, N, T)
        assert lib.rpgp_ski_f64_gather(Z.data_ptr(), gp.data_ptr(), H[1].data_ptr(), V.data_ptr() if noise else None, out.data_ptr(), N,
                                       J, J, G, T, S, noise, st) == 0
        torch.cuda.synchronize()
        A = S * sum(sens[j][0] @ np.abs(Hn[j]) for j in range(J)) + abs(noise) * np.abs(h["V"])
        _gate("ski_gather", tag + "gather noise=%g" % noise, out, ob.ski_gather(c["Z"], gpc, H[1].cpu(), c["V"], S, noise, G), A, True)
    # finish on the staged histogram against the oracle and against the fused call
    nb = lambda n: (n * 8 + 255) // 256 * 256
    ws = torch.empty(nb(J * G * 2 * T) + nb(J), dtype=torch.uint8, device=gpu_device)
    gZ, gs, gc = _nan(gpu_device, N, J), _nan(gpu_device, 1), _nan(gpu_device, J)
    assert lib.rpgp_ski_f64_bilinear_finish(Z.data_ptr(), gp.data_ptr(), hist2.data_ptr(), L.data_ptr(), R.data_ptr(), gZ.data_ptr(),
                                            gs.data_ptr(), gc.data_ptr(), N, J, J, J, G, T, S, ws.data_ptr(), ws.numel(), st) == 0
    torch.cuda.synchronize()
    fZ, fs, fc = ops.ski_bilinear_grad_comp(Z, gp, L, R, S, G)
    rZ, rs, rc = ob.ski_bilinear_grad_comp(c["Z"], gpc, c["L"], c["R"], S, G)
    Ag, As, Ac = fr.ski_bilinear_mag(h["Z"], gpn, h["L"], h["R"], S, G)
    for name, got, fused, ref, A in [("gZ", gZ, fZ, rZ, Ag), ("gscale", gs.reshape(1, 1), fs.reshape(1, 1), rs.reshape(1, 1), np.array([[As]])),
                                     ("gcomp", gc.reshape(1, -1), fc.reshape(1, -1), rc.reshape(1, -1), Ac.reshape(1, -1))]:
        _gate("ski", tag + "finish %s vs oracle" % name, got, ref, A, True)
        _gate("ski", tag + "finish %s vs fused" % name, got, fused, A, True)


def test_ski_error_codes(gpu_device):
    lib, st, L = _lib()
    N, J, T, G = 40, 3, 3, 16
    h, d, c, gp, gpc = _ski_setup(gpu_device, N, 10, J, T, G, "shared", False)
    Z, V = d["Z"], d["V"]
    out, diag = _nan(gpu_device, N, T), _nan(gpu_device, N)
    need = lib.rpgp_ski_f64_workspace_bytes(J, G, T)
    assert need > 0 and lib.rpgp_ski_f64_workspace_bytes(J, 7, T) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    mvm = lambda g, nbytes: lib.rpgp_ski_f64_mvm(Z.data_ptr(), Z.data_ptr(), gp.data_ptr(), V.data_ptr(), out.data_ptr(), N, N, J, J, J,
                                                g, T, S, 0.0, ws.data_ptr(), nbytes, st)
    assert mvm(7, need) == L.RPGP_EINVAL                               # G = 7
    assert lib.rpgp_ski_f64_diag(Z.data_ptr(), gp.data_ptr(), diag.data_ptr(), N, J, J, 7, S, st) == L.RPGP_EINVAL
    assert mvm(G, need - 1) == L.RPGP_EWORKSPACE                       # one byte short
    hist = _nan(gpu_device, J, G, 2 * T)
    assert lib.rpgp_ski_f64_scatter(Z.data_ptr(), gp.data_ptr(), V.data_ptr(), hist.data_ptr(), N, J, J, G, T, 2 * T, T + 1, 1,
                                    st) == L.RPGP_EINVAL              # hoff + T > HT
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(diag).all() and torch.isnan(hist).all()
    assert mvm(G, need) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
