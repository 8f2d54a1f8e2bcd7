"""Every device path of the pivoted-Cholesky factor (csrc/rpgp_pivchol.hip, dispatched by pivchol_common) held to float64
one greedy step at a time by tests/pivchol_reference.py: pivot, no repeat, greedy optimality, and every entry of the new
column within C u B of the float64 column computed from the factor's own earlier columns (C per operator kind: measured on
the host by tests/test_pivchol_reference_host.py, which also asserts that every main case is resolved).

Which case runs which kernel (removing a group leaves the kernel unexecuted by this module):
  one_workgroup      pivchol_kernel                     plain RBF, N <= 2048; rank 64 and J = 64 (slp[64], szp[64]), N < rank
  fast_step          pivchol_step_fast_kernel           plain RBF, J <= 32, rank <= 16, N > 2048; J = 1 and 32, ldz = 23
  general_step       pivchol_step_kernel, exact         J = 33 / rank 17 / rank 64 / J = 64 beyond the fast kernel's limits,
                                                        N = 131 073 (its row limit), N = 524 289 and 524 800: the 2 048-workgroup
                                                        cap, where a thread walks a second row
  family             pivchol_step_kernel + pivchol_entry  every (kind, group, weights) branch, at N = 2049 and N = 300; N = 5 < rank:
                                                        the step kernel's `ok == false` branch (columns 5 .. 7 exactly zero)
  grid_row_major     pivchol_step_kernel with gp         N < 65 536: pivchol_init_from_diag_kernel, row-major factor; N = 5 < rank
  grid_column_major  pivchol_step_kernel with gp and Lt  N >= 65 536 with J = 5 or rank 17, + pivchol_untranspose_kernel
                                                        (rank 17: a second panel one column wide; 65 537: last block one row)
  grid_fast          pivchol_step_ski_fast_kernel        N >= 65 536, J <= 4, rank <= 16, + pivchol_untranspose_kernel; Matern
                                                        sub-kernel, the reference grid rule, per-projection weights (the weights
                                                        ride in the grid block, so the weighted case runs this kernel as well)
Inputs: standard normal x 0.7 .. 1.0, scale = 0.8 / J.  Every case prints its per-step records before it asserts.

Where this was written (MI355X; the host restatement's figures behind the bar), largest ratio and smallest d_p / d0 per group:
  one_workgroup 7.75, 5.9e-2 | 7.28, 5.9e-2      fast_step 3.96, 3.0e-2 | 3.81, 3.0e-2      general_step 6.27, 6.1e-2 | 6.68, 6.1e-2
  family 3.04, 3.5e-2 | 4.92, 3.5e-2             grid_row_major 0.36, 1.9e-1 | 0.19, 1.8e-1
  grid_column_major 0.04, 6.6e-2 | 0.06, 5.8e-2  grid_fast 1.47, 5.6e-2 | 1.84, 4.4e-2
against C = 128 (exact, family) and 32 (grid): no gate fired on any path.  The grid operator's largest greedy gap is 0.10 of
the derived bound (the one bound of every operator)."""
import numpy as np
import pytest
import torch

from tests import pivchol_reference as pr

pytestmark = pytest.mark.gpu

CASES = pr.cases()
NAN = float("nan")


def _problem(case, dev):
    """(Z on the device, scale, provider, call): call(L, work, ldz_of_Z) runs the case's C entry on caller-owned buffers."""
    from rpgp_amd import ops, _lib
    lib = _lib.load()
    N, J, rank = case["N"], case["J"], case["rank"]
    Z, scale = pr.inputs(N, J)
    Zt = torch.from_numpy(Z).to(dev)
    if case["op"] == "exact":
        prov = pr.provider_of(case, Z)
        work_floats = N + _lib.RPGP_PIVCHOL_SCRATCH

        def call(Zd, ldz, L, work):
            _lib.check(lib.rpgp_pivoted_cholesky(Zd.data_ptr(), L.data_ptr(), work.data_ptr(), N, ldz, J, rank, scale, None),
                       "rpgp_pivoted_cholesky")
        run = lambda: ops.pivoted_cholesky(Zt, scale, rank)
    elif case["op"] == "family":
        prov = pr.provider_of(case, Z)
        fam = ops.Family(case["kind"], case["group"], torch.from_numpy(prov.w32).to(dev))
        wsum = pr.weight_sum32(prov.w32)
        work_floats = N + _lib.RPGP_PIVCHOL_SCRATCH

        def call(Zd, ldz, L, work):
            _lib.check(lib.rpgp_family_pivoted_cholesky(fam.ref, Zd.data_ptr(), L.data_ptr(), work.data_ptr(), N, ldz, rank,
                                                        scale, wsum, None), "rpgp_family_pivoted_cholesky")
        run = lambda: ops.family_pivoted_cholesky(fam, Zt, scale, rank, wsum)
    else:
        G = case["G"]
        w = pr.grid_weights(J) if case["weighted"] else None
        gp = ops.ski_grid(Zt, None, G, weights=None if w is None else torch.from_numpy(w), rule=case["rule"], kind=case["kind"])
        blk = gp.cpu().numpy()
        assert int(blk[3]) == (1 if case["weighted"] else 0) + (2 if case["rule"] == "reference" else 0) + 4 * ops.KINDS[case["kind"]]
        if case["rule"] == "reference":
            g = blk[4 + J:].reshape(J, 3)
            grid = (g[:, 0].copy(), g[:, 1].copy(), g[:, 2].copy())
        else:
            grid = tuple(np.full(J, blk[q], dtype=np.float32) for q in range(3))
        # the reference runs on the kernel's own (float32) grid block, which is the host rule's to float32 rounding
        for got, want in zip(grid, pr.host_grid_block(Z, G, case["rule"])):
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)       # (the gates of test_ski_gpu.py)
        prov = pr.provider_of(case, Z, grid)
        work_floats = lib.rpgp_ski_pivoted_cholesky_work_floats(N, rank)
        assert work_floats == N + _lib.RPGP_PIVCHOL_SCRATCH + (N * rank if N >= 65536 else 0)

        def call(Zd, ldz, L, work):
            _lib.check(lib.rpgp_ski_pivoted_cholesky(Zd.data_ptr(), gp.data_ptr(), L.data_ptr(), work.data_ptr(), work_floats,
                                                     N, ldz, J, G, rank, scale, None), "rpgp_ski_pivoted_cholesky")
        run = lambda: ops.ski_pivoted_cholesky(Zt, gp, scale, rank, G)
    return Zt, scale, prov, run, call, work_floats


def _held(case, L, prov, scale):
    """Print the records, then assert: `check` raises on any gate; a main case has no skipped step."""
    try:
        records = pr.check(L, prov, scale, case=case["id"])
    except pr.CheckFailure as e:
        pr.show(case["id"], e.records)
        print(e)
        raise
    pr.show(case["id"], records)
    worst, dmin, skipped = pr.summary(records)
    print("%s: largest ratio %.3f (C = %g), smallest d_p/d0 %.3e, skipped %.2f"
          % (case["id"], worst, pr.C[prov.name], dmin, skipped))
    pr.assert_resolved(case, records)
    return records


@pytest.mark.parametrize("case_id", [c["id"] for c in CASES])
def test_every_step_against_float64(gpu_device, case_id):
    case = next(c for c in CASES if c["id"] == case_id)
    Zt, scale, prov, run, _, _ = _problem(case, gpu_device)
    L = run()
    assert L.shape == (case["N"], case["rank"])
    Lh = L.cpu().numpy()
    _held(case, Lh, prov, scale)
    if case["N"] < case["rank"]:                          # N < rank: every row has been a pivot, the rest is exactly zero
        assert not Lh[:, case["N"]:].any()


def _buffers(dev, N, rank, work_floats, fill):
    """L and the work buffer inside NaN guard zones of 4096 floats, pre-filled with `fill`."""
    guard = 4096
    Lb = torch.full((2 * guard + N * rank,), NAN, dtype=torch.float32, device=dev)
    Wb = torch.full((2 * guard + work_floats,), NAN, dtype=torch.float32, device=dev)
    L = Lb[guard:guard + N * rank].view(N, rank)
    W = Wb[guard:guard + work_floats]
    L.fill_(fill)
    W.fill_(fill)
    return Lb, Wb, L, W, guard


CONTRACT = ["one_workgroup-N65-J32-r16", "fast_step-N2049-J20-r15", "general_step-N2049-J33-r17",
            "family-Matern-g1-c6-N300-r17", "grid_row_major-N3000-J3-r15-G256-RBF-shared",
            "grid_column_major-N65537-J3-r17-G512-RBF-shared", "grid_fast-N65537-J4-r15-G512-RBF-reference"]


@pytest.mark.parametrize("case_id", CONTRACT)
def test_contract_of_the_c_entry(gpu_device, case_id):
    """Through the raw C entry on caller-owned buffers, once per path: L and the work buffer pre-filled with NaN give the
    bits of a zero pre-fill and of `ops`; a repeated call on the used buffers gives them again; the guard zones around L and
    around the work buffer stay NaN."""
    case = next(c for c in CASES if c["id"] == case_id)
    N, J, rank = case["N"], case["J"], case["rank"]
    Zt, scale, prov, run, call, work_floats = _problem(case, gpu_device)
    want = run().view(torch.int32)
    outs = []
    for fill in (NAN, 0.0):
        Lb, Wb, L, W, guard = _buffers(gpu_device, N, rank, work_floats, fill)
        for rep in range(2 if fill != 0.0 else 1):        # the second call finds the first one's factor and scratch
            call(Zt, J, L, W)
            torch.cuda.synchronize()
            outs.append(L.clone().view(torch.int32))
        for buf, n in ((Lb, N * rank), (Wb, work_floats)):
            assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all()
    assert torch.isfinite(outs[0].view(torch.float32)).all()
    for o in outs:
        assert torch.equal(o, want)


def test_padded_coordinate_rows(gpu_device):
    """ldz = 23 > J = 20 through the C entry (fast step kernel), the padding NaN: the factor has the bits of the packed
    call, and is held to float64 like it."""
    N, J, rank, ldz = pr.LDZ_CASE
    case = next(c for c in CASES if c["id"] == "fast_step-N%d-J%d-r%d" % (N, J, rank))
    Zt, scale, prov, run, call, work_floats = _problem(case, gpu_device)
    Zp = torch.full((N, ldz), NAN, dtype=torch.float32, device=gpu_device)
    Zp[:, :J] = Zt
    Lb, Wb, L, W, guard = _buffers(gpu_device, N, rank, work_floats, NAN)
    call(Zp, ldz, L, W)
    torch.cuda.synchronize()
    _held(dict(case, id=case["id"] + "-ldz%d" % ldz), L.cpu().numpy(), prov, scale)
    assert torch.equal(L.view(torch.int32), run().view(torch.int32))
    assert torch.isnan(Lb[:guard]).all() and torch.isnan(Lb[guard + N * rank:]).all()
