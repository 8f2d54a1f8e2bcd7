"""The native mBCG executor (rpgp_mbcg_solve, csrc/rpgp_cg.hip) against a plain float64 preconditioned CG of the same system,
coefficient by coefficient, after m = 4 iterations: every alpha, every beta, the iterate, the iteration count and the returned
mean residual.  A converged solve hides a wrong-but-SPD preconditioner application, a mis-masked lane or a slab left out of
a sum; four steps of a system whose coefficients are O(1) and tame do not (tests/cg_reference.py; the bound and the two
conditions on the inputs are checked on the CPU in tests/test_cg_reference_host.py).

With hist_len = max_iter = min_iter = m only the last iteration tests convergence (`hist_pending` in rpgp_mbcg_solve), the
tolerance 1e-30 is never met, the divergence rule needs an earlier snapshot and the stagnation window is off: the executor runs
min(m, N) iterations, pass C of the last one copies x into x_best with the same mean residual, and k_unnormalise hands back x
(`snap < mean_resid` is false) — the m-th iterate either way."""
import numpy as np
import pytest
import torch

from tests import cg_reference as R

pytestmark = pytest.mark.gpu

_worst = {}                 # group -> [alpha, beta, x, mean residual] largest GPU errors (printed when the module is done)


@pytest.fixture(scope="module")
def bounds():
    b = R.bounds()
    worst = np.array(list(R.case_distances().values())).max(axis=0)
    print("\nfloat32-to-float64 distances of the CPU emulation over the case table: alpha %.2e  beta %.2e  x %.2e" % tuple(worst))
    print("bounds (x %g): alpha %.2e  beta %.2e  x %.2e" % ((R.MARGIN,) + b))
    yield b
    for g, w in sorted(_worst.items()):
        print("largest GPU errors, %-16s alpha %.2e  beta %.2e  x %.2e  mean residual %.2e" % ((g + ":",) + tuple(w)))


_dev_cache = {}


def _on_device(key, make, dev):
    if key not in _dev_cache:
        _dev_cache[key] = make().to(dev)
    return _dev_cache[key]


def _descriptor(dev, N, J, kind):
    from rpgp_amd import ops, _lib
    sysm = R.system(N, J)
    if kind == "dense":
        Kd = _on_device(("Kd", N, J), lambda: torch.from_numpy(R.dense_system(N, J).Kd32), dev)
        return ops.make_operator_desc(_lib.RPGP_OP_DENSE, N, 0, 1.0, sysm.noise, Kd=Kd)
    Z = _on_device(("Z", N, J), lambda: torch.from_numpy(sysm.Z), dev)
    if kind == "prepared":
        if ("prep", N, J) not in _dev_cache:
            _dev_cache[("prep", N, J)] = ops.Prepared(Z)
        prep = _dev_cache[("prep", N, J)]
        assert prep.fast_ok, "the quantised coordinates must be inside the prepared sweep's range"
        return ops.make_operator_desc(_lib.RPGP_OP_FUSED_PREPARED, N, J, sysm.scale, sysm.noise, prep=prep)
    return ops.make_operator_desc(_lib.RPGP_OP_FUSED, N, J, sysm.scale, sysm.noise, Z=Z)


def _solve(dev, N, K, J, kind, B):
    """m iterations of the executor on the right-hand sides B (numpy float32 [N x T])."""
    from rpgp_amd import ops
    desc, keep = _descriptor(dev, N, J, kind)
    kw = {}
    if K:
        Lh = R.preconditioner(N, K)
        kw = dict(L=_on_device(("L", N, K), lambda: torch.from_numpy(Lh), dev),
                  Cinv=_on_device(("Cinv", N, K), lambda: torch.from_numpy(R.capacitance_inverse(Lh, R.NOISE)), dev),
                  sigma2=R.NOISE)
    rhs = torch.from_numpy(np.array(B, dtype=np.float32, order="C")).to(dev)       # (a copy: the shared inputs are read-only)
    x, ah, bh, it, mres = ops.mbcg_solve(desc, rhs, 1e-30, R.M_ITERS, min_iter=R.M_ITERS, hist_len=R.M_ITERS, **kw)
    del keep
    return x.double().cpu().numpy(), ah.astype(np.float64), bh.astype(np.float64), it, mres


def _check(group, bounds, got, ref_alpha, ref_beta, ref_x, ref_resid, N, label):
    """(a) alphas, (b) betas, (c) x within the bound; (d) the iteration count; (e) the mean residual to 1e-4."""
    x, ah, bh, it, mres = got
    n_iter = min(R.M_ITERS, N)
    assert it == n_iter and ah.shape == ref_alpha.shape and bh.shape == ref_beta.shape, (it, ah.shape, ref_alpha.shape)
    assert np.isfinite(ah).all() and np.isfinite(bh).all() and np.isfinite(x).all()
    exhausted = R.krylov_exhausted(n_iter, N)
    ea = R.coefficient_error(ah, ref_alpha)
    eb = R.coefficient_error(bh, ref_beta, exhausted)
    ex = R.iterate_error(x, ref_x)
    want = float(np.mean(ref_resid))
    # (N iterations on N rows: the residual is what rounding left of zero, 1e-16 in float64; it is held to 1e-4 of the
    #  normalised initial residual 1 instead of 1e-4 of itself)
    er = abs(mres - want) / (1.0 if exhausted else want)
    print("%s: alpha %.2e (bound %.2e)  beta %.2e (%.2e)  x %.2e (%.2e)  mean residual %.6g vs %.6g (%.1e)"
          % (label, ea, bounds[0], eb, bounds[1], ex, bounds[2], mres, want, er))
    w = _worst.setdefault(group, [0.0, 0.0, 0.0, 0.0])
    for i, e in enumerate((ea, eb, ex, er)):
        w[i] = max(w[i], e)
    assert ea < bounds[0], (label, "alpha", ea, bounds[0])
    assert eb < bounds[1], (label, "beta", eb, bounds[1])
    assert ex < bounds[2], (label, "x", ex, bounds[2])
    assert er < 1e-4, (label, "mean residual", mres, want)


def _run_case(dev, bounds, group, N, T, K, J, kind):
    ref = R.reference(N, K, J, kind="dense" if kind == "dense" else "quantised")
    got = _solve(dev, N, K, J, kind, R.rhs(N, K)[:, :T])
    _check(group, bounds, got, ref.alpha[:, :T], ref.beta[:, :T], ref.x[:, :T], ref.resid[:T], N,
           "%s N=%d T=%d K=%d %s" % (group, N, T, K, kind))


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_executor_steps_match_float64_pcg(gpu_device, bounds, monkeypatch, case):
    """The fused exact operator over every TT instantiation, the rank ladder, the row ladder, the slab counts of the
    consumer-side reduction, the k_reduce launches (65 slabs, and RPGP_CG_DIRECT=0) and two tiles per workgroup."""
    group, N, T, K, J, direct = case
    monkeypatch.delenv("RPGP_CG_DIRECT", raising=False)
    if not direct:
        monkeypatch.setenv("RPGP_CG_DIRECT", "0")
    _run_case(gpu_device, bounds, group, N, T, K, J, "fused")


@pytest.mark.parametrize("case", R.OPERATOR_CASES, ids=R.case_id)
def test_executor_steps_match_float64_pcg_other_operators(gpu_device, bounds, monkeypatch, case):
    """The N = 777 cases once more through RPGP_OP_FUSED_PREPARED (same float64 kernel) and RPGP_OP_DENSE (the reference runs
    on Kd.double() of the float32 matrix the operator is handed)."""
    group, N, T, K, J, kind = case
    monkeypatch.delenv("RPGP_CG_DIRECT", raising=False)
    _run_case(gpu_device, bounds, group + "/" + kind, N, T, K, J, kind)


@pytest.mark.parametrize("T", [3, 11, 16])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_zero_column_is_masked_and_leaves_the_others_alone(gpu_device, bounds, monkeypatch, T, where):
    monkeypatch.delenv("RPGP_CG_DIRECT", raising=False)
    N, K, J = 777, 15, 3
    c = {"first": 0, "middle": T // 2, "last": T - 1}[where]
    ref = R.reference(N, K, J)
    B = np.array(R.rhs(N, K)[:, :T])
    B[:, c] = 0.0
    got = _solve(gpu_device, N, K, J, "fused", B)
    x, ah, bh = got[0], got[1], got[2]
    assert (ah[:, c] == 0).all() and (x[:, c] == 0).all() and (bh[:, c] == 0).all()
    ra, rb, rx, rr = (np.array(a[..., :T]) for a in (ref.alpha, ref.beta, ref.x, ref.resid))
    ra[:, c], rb[:, c], rx[:, c], rr[c] = 0.0, 0.0, 0.0, 0.0
    _check("masks", bounds, got, ra, rb, rx, rr, N, "zero column %d of %d" % (c, T))


@pytest.mark.parametrize("N,K,col", [(777, 15, 0), (257, 16, 5)])
def test_column_scale_only_scales_the_iterate(gpu_device, bounds, monkeypatch, N, K, col):
    """One right-hand side beside itself times 2^20 and times 2^-20: the normalised systems are the same, so the
    coefficients agree within the bound (of each other and of the reference) and x scales."""
    monkeypatch.delenv("RPGP_CG_DIRECT", raising=False)
    J = 3
    ref = R.reference(N, K, J)
    s = np.array([1.0, 2.0 ** 20, 2.0 ** -20], dtype=np.float32)
    B = R.rhs(N, K)[:, [col, col, col]] * s
    got = _solve(gpu_device, N, K, J, "fused", B)
    x, ah, bh = got[0], got[1], got[2]
    cols = [col, col, col]
    _check("masks", bounds, got, ref.alpha[:, cols], ref.beta[:, cols], ref.x[:, cols] * s.astype(np.float64),
           ref.resid[cols], N, "scaled column N=%d K=%d" % (N, K))
    for j in (1, 2):
        assert R.coefficient_error(ah[:, [j]], ah[:, [0]]) < bounds[0]
        assert R.coefficient_error(bh[:, [j]], bh[:, [0]]) < bounds[1]
        assert R.iterate_error(x[:, [j]] / float(s[j]), x[:, [0]]) < bounds[2]
