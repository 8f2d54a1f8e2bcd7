"""tests/cg_reference.py held to dense float64 algebra on the CPU, the torch-op loop of linear_cg.py held to it step for step,
and the two conditions that make the bound of tests/test_native_cg_steps_gpu.py mean something (the inputs are tame; the
inputs notice one column of the preconditioner) over the whole case table.  Nothing here needs a GPU."""
import warnings

import numpy as np
import pytest
import torch

from tests import cg_reference as R


@pytest.mark.parametrize("K", [0, 5])
def test_reference_pcg_converges_to_the_dense_solve(K):
    N = 300
    op = R.system(N)
    L = R.make_L(N, K, R.NOISE, R.SEED)
    B = R.rhs(N)[:, :5]
    out = R.pcg(op.matvec, B, L, R.NOISE, N, np.float64)
    x = np.linalg.solve(op.dense(), B.astype(np.float64))
    assert out.alpha.shape == (N, 5) and out.beta.shape == (N, 5)
    assert np.linalg.norm(out.x - x) / np.linalg.norm(x) < 1e-10
    assert out.resid.max() < 1e-10


@pytest.mark.parametrize("N,J", [(1, 3), (2, 3), (300, 3), (1025, 3), (2049, 1)])
def test_quantised_product_is_the_dense_product(N, J):
    op = R.system(N, J)
    V = np.random.default_rng(N).standard_normal((N, 7))
    ref = op.dense() @ V
    assert np.abs(op.matvec(V) - ref).max() <= 1e-13 * np.abs(ref).max()
    # the float32 emulation's product is the same product up to float32 rounding (N terms, pairwise-ish sums)
    assert np.abs(op.matvec32(V) - ref).max() <= 2e-6 * np.abs(ref).max()
    assert op.Z.dtype == np.float32 and len(np.unique(op.Z[:, 0])) <= R.G_LEVELS


def test_dense_operator_is_its_float32_matrix():
    op, q = R.dense_system(777), R.system(777)
    V = np.random.default_rng(5).standard_normal((777, 3))
    assert op.Kd32.dtype == np.float32
    assert np.array_equal(op.matvec(V), op.Kd32.astype(np.float64) @ V + R.NOISE * V)
    assert np.abs(op.matvec(V) - q.matvec(V)).max() <= 1e-6 * np.abs(q.matvec(V)).max()


def test_preconditioner_of_the_reference_is_the_dense_woodbury_inverse():
    """One iteration from r0 = b / |b|: alpha_0 = r.z / z.A z with z = M^-1 r formed from the dense M."""
    N, K = 65, 9
    op, L = R.system(N), R.make_L(N, K, R.NOISE, R.SEED)
    B = R.rhs(N)[:, :3].astype(np.float64)
    M = L.astype(np.float64) @ L.astype(np.float64).T + R.NOISE * np.eye(N)
    r = B / np.linalg.norm(B, axis=0)
    z = np.linalg.solve(M, r)
    a0 = (r * z).sum(0) / (z * (op.dense() @ z)).sum(0)
    out = R.pcg(op.matvec, B, L, R.NOISE, 1, np.float64)
    assert np.abs(out.alpha[0] - a0).max() < 1e-13 * np.abs(a0).max()
    assert np.abs(out.x - a0 * z * np.linalg.norm(B, axis=0)).max() < 1e-13


def test_zero_column_and_short_systems():
    op = R.system(2)
    B = np.array(R.rhs(2)[:, :3])
    B[:, 1] = 0.0
    out = R.pcg(op.matvec, B, R.make_L(2, 1, R.NOISE, R.SEED), R.NOISE, R.M_ITERS, np.float64)
    assert out.alpha.shape == (2, 3)                            # n_iter = min(m, N)
    assert (out.alpha[:, 1] == 0).all() and (out.x[:, 1] == 0).all() and out.resid[1] == 0
    x = np.linalg.solve(op.dense(), B[:, [0, 2]].astype(np.float64))
    assert np.abs(out.x[:, [0, 2]] - x).max() < 1e-12          # N iterations solve an N x N system


def test_tridiagonals_match_the_library_formula():
    from rpgp_amd import linear_cg as lcg
    ref = R.reference(777, 15)
    t = R.tridiagonals(ref.alpha, ref.beta)
    lib = lcg._tridiag_from_history(ref.alpha, ref.beta, R.T_MAX, torch.float64, "cpu").numpy()
    assert t.shape == lib.shape == (R.T_MAX, R.M_ITERS, R.M_ITERS)
    assert np.abs(t - lib).max() <= 1e-14 * np.abs(t).max()
    # ... and they are what they claim to be: Q^T (M^-1/2 A M^-1/2) Q has the eigenvalues of a 4-step Lanczos run, all of them
    # inside the spectrum of the preconditioned matrix
    ev = np.linalg.eigvalsh(t)
    assert ev.min() > 0


@pytest.mark.parametrize("T", [1, 11])
@pytest.mark.parametrize("K", [0, 15])
def test_torch_loop_on_cpu_matches_the_reference_step_for_step(T, K):
    """linear_cg.linear_cg (torch ops, float32 CPU tensors, closure preconditioner) at m = 4, N = 777, held to the float64
    reference at the bound of the GPU tests.  The loop hands back the iterate and the Lanczos tridiagonals; all alphas and
    the first m - 1 betas are read back out of those (the last beta enters no tridiagonal entry)."""
    from rpgp_amd import linear_cg as lcg
    N, m = 777, R.M_ITERS
    op = R.dense_system(N)
    ref = R.reference(N, K, kind="dense")
    A = torch.from_numpy(op.Kd32)
    rhs = torch.from_numpy(np.array(R.rhs(N, K)[:, :T]))
    pre = None
    if K:
        Ld = torch.from_numpy(R.preconditioner(N, K)).double()
        Cinv = torch.from_numpy(R.capacitance_inverse(R.preconditioner(N, K), R.NOISE))

        def pre(r):
            rd = r.double()
            return ((rd - Ld @ (Cinv @ (Ld.t() @ rd))) / R.NOISE).float()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", lcg.NumericalWarning)
        x, tri = lcg.linear_cg(lambda v: A @ v + R.NOISE * v, rhs, n_tridiag=T, tolerance=1e-30, max_iter=m,
                               max_tridiag_iter=m, preconditioner=pre, min_iter=m)
    assert lcg.stats["last_iterations"] == m and tri.shape == (T, m, m)
    tri = tri.double().numpy()
    alpha, beta = np.zeros((m, T)), np.zeros((m - 1, T))
    for k in range(m):
        alpha[k] = 1.0 / (tri[:, k, k] - (beta[k - 1] / alpha[k - 1] if k else 0.0))
        if k + 1 < m:
            beta[k] = (tri[:, k, k + 1] * alpha[k]) ** 2
    ba, bb, bx = R.bounds()
    ea = R.coefficient_error(alpha, ref.alpha[:, :T])
    # (scaled by the column's largest beta over all m iterations, as everywhere)
    eb = float((np.abs(beta - ref.beta[:m - 1, :T]) / np.abs(ref.beta[:, :T]).max(axis=0)).max())
    ex = R.iterate_error(x.double().numpy(), ref.x[:, :T])
    print("torch loop T=%d K=%d: alpha %.2e (bound %.2e)  beta %.2e (%.2e)  x %.2e (%.2e)" % (T, K, ea, ba, eb, bb, ex, bx))
    assert ea < ba and eb < bb and ex < bx


def test_case_table_is_what_the_gpu_tests_need():
    tts = {(T, K) for (g, N, T, K, J, d) in R.CASES if g == "every_tt"}
    assert tts == {(T, K) for T in range(1, 17) for K in (0, 15)}
    assert {K for (g, N, T, K, J, d) in R.CASES if g == "rank_ladder"} == set(R.RANKS)
    assert {N for (g, N, T, K, J, d) in R.CASES if g == "row_ladder"} == set(R.ROWS)
    tiles = sorted({(N + 255) // 256 for (g, N, T, K, J, d) in R.CASES if g == "slabs"})
    assert tiles == [16, 17, 32, 33, 48, 64, 65]
    assert all((N + 255) // 256 > 1024 for (g, N, T, K, J, d) in R.CASES if g == "two_tiles")
    assert len({R.case_id(c) for c in R.CASES}) == len(R.CASES)
    assert len({R.case_id(c) for c in R.OPERATOR_CASES}) == len(R.OPERATOR_CASES) == 2 * (32 + 33)


def test_condition_1_inputs_are_tame_at_four_iterations():
    """Every case's own float32-to-float64 distance is below 1e-4: four iterations of these systems are not yet the regime
    where two correct implementations drift apart."""
    d = R.case_distances()
    worst = np.array(list(d.values())).max(axis=0)
    print("largest float32-to-float64 distances: alpha %.2e  beta %.2e  x %.2e" % tuple(worst))
    print("bounds (x %g): alpha %.2e  beta %.2e  x %.2e" % ((R.MARGIN,) + R.bounds()))
    for key, v in d.items():
        assert max(v) < R.TAME, (key, v)
    assert all(b > 0 for b in R.bounds())


def test_condition_2_inputs_notice_one_column_of_the_preconditioner():
    """For every case with N >= 17 and K >= 1 the float64 reference without the last column of L differs from the true one by
    at least 50 alpha bounds, in alpha: a one-column error of the preconditioner application cannot hide inside the bound."""
    s = R.sensitivities()
    ba = R.bounds()[0]
    least = min(s, key=s.get)
    print("least sensitivity %.2e at (N, K, J, kind) = %s: %.0f x the alpha bound %.2e" % (s[least], least, s[least] / ba, ba))
    assert len(s) >= 40
    for key, v in s.items():
        assert v >= R.SENSITIVITY * ba, (key, v, ba)
