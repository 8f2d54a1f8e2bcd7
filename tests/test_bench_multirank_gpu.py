"""`bench.py --gpus N` END TO END on the one-GPU test box: the ranks are started by bench.py itself, all on device 0
(`--all-ranks-on-device 0`: gloo bootstrap, rpgp_comm all-reduce — RCCL refuses two ranks per device), each runs its share
of the sharded MVM, the partials are all-reduced on the launch stream, the timings are MAX-reduced and rank 0 prints the
JSON line.  The reduced product is checked against the float64 oracle (oracle/cmvm.c) on a seeded row sample, the JSON
against the driver's contract (n_gpus, config.parallelism / split / comm, per-rank kernel and all-reduce times).  On a real
multi-GPU node the same command without `--all-ranks-on-device` runs one rank per GPU over RCCL — this test exists so
that the first 8-GPU run is not the first run of that code (replaces `MultiDeviceKernel`, training_routines.py:407-408;
3-device run script run_scripts/additive_spread_prescale_Jd.sh:6)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, J = 20, 20


def _oracle_rows(N, rows):
    import torch
    import bench
    from oracle import cmvm, dense_gp as orc
    X, P, ls, V = bench.make_inputs(N, D, J, 1, torch.device("cpu"))
    Z = orc.project(X.numpy(), P.numpy(), ls.numpy())
    Vh = V.double().numpy()
    return cmvm.mvm(Z[rows], Z, Vh, 1.0 / J) + 0.1 * Vh[rows]


# (world, split that is `value`, N): every --full run times BOTH splits (the other one lands in multi_gpu.other_split), so
# the last case is north_star's uneven J = 20 -> (3,3,3,3,2,2,2,2) split AND the equal-pairs split at world 8 on the BASELINE
# size N = 50 000 (VERDICT r5 #1b).  Eight ranks sharing one device exceed the number of processes a GPU test may keep on
# a device at once, so that case runs one rank per GPU and needs 8 of them; the 4-rank case keeps the BASELINE size on one
# device.
@pytest.mark.parametrize("world,shard,N", [(2, "pairs", 20000), (3, "j", 20000), (4, "pairs", 50000), (8, "pairs", 50000)])
def test_bench_gpus_n_runs_on_one_device(gpu_device, tmp_path, world, shard, N):
    import torch
    shared = world < 8
    if not shared and torch.cuda.device_count() < world:
        pytest.skip("needs %d GPUs (one rank each), found %d" % (world, torch.cuda.device_count()))
    dump = str(tmp_path / "res.npy")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--shard", shard, "--full",
           "--n", str(N), "--steps", "5", "--warmup", "2", "--no-extras", "--cpu-budget", "0", "--dump-result", dump]
    cmd += ["--all-ranks-on-device", "0"] if shared else ["--comm", "ipc"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == world and res["steps"] == 5 and res["warmup"] == 2 and res["unit"] == "MVM/s"
    assert res["value"] > 0 and abs(res["value"] * res["ms_per_step"] / 1e3 - 1.0) < 1e-3
    assert res["config"]["parallelism"] == "%s-shard x%d + all-reduce" % (shard, world)
    assert res["config"]["split"].startswith(shard) and "rpgp_comm" in res["config"]["comm"]
    sys.path.insert(0, ROOT)
    from rpgp_amd.distributed import j_partition
    jtab = ", ".join("%d:%d" % ab for ab in j_partition(J, world))
    assert "j-shard x%d [%s]" % (world, jtab) in res["config"]["north_star_split"]
    if world == 8:
        assert jtab == "0:3, 3:6, 6:9, 9:12, 12:14, 14:16, 16:18, 18:20"
    mg = res["multi_gpu"]
    assert len(mg["per_rank_kernel_ms"]) == world and all(k > 0 for k in mg["per_rank_kernel_ms"])
    assert len(mg["per_rank_allreduce_us"]) == world and mg["allreduce_us"] > 0 and mg["allreduce_bytes"] == 4 * N
    if shared:
        assert mg["all_ranks_on_device"] == 0 and "NOT a scaling measurement" in mg["note"]
    else:
        assert "all_ranks_on_device" not in mg
    assert abs(res["roofline"]["kernel_ms"] - max(mg["per_rank_kernel_ms"])) < 1e-3
    assert res["roofline"]["traffic"] is None and "cpu_baseline" not in res
    # the kernel the line names is the one the split launches (the hand-scheduled kernel serves the pair shares)
    other = mg["other_split"]
    names = {shard: res["roofline"]["kernel"], ("j" if shard == "pairs" else "pairs"): other["kernel"]}
    assert names["pairs"] == "mvm_fact_asm_kernel" and names["j"].startswith("mvm_fact_asm_thin_kernel<" if N >= 10240 else "mvm_fact_kernel<")
    assert other["parallelism"] == "%s-shard x%d + all-reduce" % ("j" if shard == "pairs" else "pairs", world)
    assert other["value"] > 0 and len(other["per_rank_kernel_ms"]) == world and other["rel_diff_vs_value_split"] < 1e-5
    # the all-reduced products of the last step of BOTH splits against the oracle (identical inputs: bench.make_inputs seeds)
    rows = np.sort(np.random.default_rng(world).choice(N, size=384, replace=False))
    ref = _oracle_rows(N, rows)
    for path in (dump, dump + ".other.npy"):
        out = np.load(path).astype(np.float64)
        assert out.shape == (N, 1)
        assert np.linalg.norm(out[rows] - ref) / np.linalg.norm(ref) < 1e-5, path


def test_bench_plain_run_times_the_steps_and_dumps_the_last_product(gpu_device, tmp_path):
    """A plain `bench.py --gpus 1` run: the headline line only (nothing that `--full` adds), exactly --steps timed steps, and
    `--dump-outputs` writes the product of the last timed step, checked against the float64 oracle on a seeded row sample."""
    N = 20000
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(N), "--steps", "7", "--warmup", "1",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 1 and res["steps"] == 7 and res["warmup"] == 1 and res["unit"] == "MVM/s"
    assert res["higher_is_better"] is True and res["dtype"] == "f32" and res["metric"].startswith("additive-RP kernel MVMs/sec")
    # value = steps / elapsed and ms_per_step = 1e3 elapsed / steps are printed rounded to 3 and to 4 decimals: they agree to
    # half a unit of ms_per_step's last decimal (a step at this size is ~0.026 ms, where that half unit is 2e-3 relative: a
    # relative 1e-3 held or not by the luck of the rounding; above 0.05 ms this is the tighter statement)
    assert res["value"] > 0 and abs(res["ms_per_step"] - 1e3 / res["value"]) <= 0.5e-4 + 1e-7
    assert not {"extras", "cpu_baseline", "cpu_baseline_best", "prepare_us", "multi_gpu"} & set(res)
    assert sorted(os.listdir(out_dir)) == ["mvm_out.npy"]
    out = np.load(out_dir / "mvm_out.npy")
    assert out.dtype == np.float32 and out.shape == (N, 1)
    rows = np.sort(np.random.default_rng(1).choice(N, size=384, replace=False))
    ref = _oracle_rows(N, rows)
    assert np.linalg.norm(out[rows].astype(np.float64) - ref) / np.linalg.norm(ref) < 1e-5
