"""Timing of the full radial kernels (csrc/rpgp_radial.hip, settings.fused_full) on the MI355X.  One JSON line per
record, appended to --out (profiles/radial_full_bench.jsonl).  Every arm: device events, warm-up, >= 9 repetitions ALTERNATING
between the arms in one process, min / median / max reported, outputs compared across the arms on the same seeded inputs.

  --arms product   (a) out = K V at N = 50 000, d in {8, 20, 90}, T in {1, 11}, RBF: the radial kernel, the dense path of the
                       flag-off operator (K built once, K @ V timed; the build is timed apart) and, for d <= 20, the family
                       tile kernel (ops.family_mvm_sym, one component of group = d); (c) the achieved fp32 FLOP/s of the radial
                       kernel, Gram 2 N^2 d plus the V product as issued (2 N^2 16), against the 157 TF matrix peak.
  --arms step      (b) one optimiser step (Adam) of the ARD RBF `full` model at N in {7 372, 14 939, 50 000} (d = 8, 18, 20):
                       --modes on (settings.fused_full as committed), on_radial (the same without the family tile route of
                       d <= 20) and off (the dense path; where its step raises, the error is the record).
  --constant       the largest error of the direct-difference family kernels in the unit scale u (1 + d2 |phi'|): the
                   constant c of tests/radial_reference.py."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(ts):
    s = sorted(ts)
    return {"ms_min": s[0], "ms_median": s[len(s) // 2], "ms_max": s[-1], "reps": len(s)}


def _emit(rec, out):
    print(json.dumps(rec), flush=True)
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")


def product_arms(out, N, dims, widths, reps, warmup, tag):
    from rpgp_amd import ops
    dev = torch.device("cuda:0")
    for d in dims:
        g = torch.Generator().manual_seed(d)
        Z = torch.randn(N, d, generator=g) * min(1.0, 2.0 / d ** 0.5)
        Z = (Z - Z.mean(0)).to(dev)
        t_build, K = _timed(lambda: torch.exp(-0.5 * (Z.pow(2).sum(1, keepdim=True) - 2.0 * Z @ Z.t() + Z.pow(2).sum(1)[None, :])
                                              .clamp_min_(0.0)))
        fam = ops.Family("RBF", d, torch.ones(1, device=dev)) if d in ops.FAMILY_GROUPS else None
        for T in widths:
            V = torch.randn(N, T, generator=g).to(dev)
            arms = {"radial": lambda: ops.radial_mvm("RBF", Z, None, V, 1.0, 0.1),
                    "dense": lambda: torch.addmm(V, K, V, beta=0.1)}
            if fam is not None:
                arms["family"] = lambda: ops.family_mvm_sym(fam, Z, V, 1.0, 0.1)
            times, outs = {k: [] for k in arms}, {}
            for it in range(warmup + reps):
                for k, fn in arms.items():                     # alternating: one repetition of every arm per round
                    t, o = _timed(fn)
                    if it >= warmup:
                        times[k].append(t)
                    outs[k] = o
            ref = outs["dense"].double()
            for k in arms:
                rec = {"arm": "product", "impl": k, "N": N, "d": d, "T": T, "kind": "RBF", "tag": tag, **_stats(times[k]),
                       "rel_vs_dense": float((outs[k].double() - ref).norm() / ref.norm())}
                if k == "radial":
                    fl = 2.0 * N * N * d + 2.0 * N * N * 16
                    rec.update(flops_issued=fl, tflops=fl / (rec["ms_median"] * 1e-3) / 1e12,
                               fraction_of_157tf=fl / (rec["ms_median"] * 1e-3) / 157.3e12)
                if k == "dense":
                    rec["build_ms"] = t_build
                _emit(rec, out)
        del K
        torch.cuda.empty_cache()


def step_arms(out, sizes, reps, reps_off_large, warmup, tag, modes=("on", "on_radial", "off")):
    """`on`: settings.fused_full as committed (the RBF with d <= 20 on the family tile route); `on_radial`: the same with the
    private switch operators._FULL_FAMILY_ROUTE off (every full kernel on the radial kernels); `off`: the dense torch path.  An
    arm whose step raises (the dense path at N = 50 000: the library's triangular solve) is recorded with its error and dropped;
    the other arms go on."""
    from rpgp_amd import operators, settings, linear_cg as lcg
    from rpgp_amd.models import ExactMarginalLogLikelihood
    from rpgp_amd.training import create_exact_gp, make_optimizer
    dev = torch.device("cuda:0")
    for N, d in sizes:
        g = torch.Generator().manual_seed(0)
        X = torch.randn(N, d, generator=g)
        y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
        y = ((y - y.mean()) / y.std()).to(dev)
        X = X.to(dev)
        arms = {}
        for mode in modes:
            torch.manual_seed(0)
            model, lik = create_exact_gp(X, y, "full", noise_prior=True, ard=True, kernel_type="RBF",
                                         init_lengthscale_range=(d ** 0.5, d ** 0.5))
            model = model.to(dev)
            model.train()
            opt = make_optimizer(torch.optim.Adam, [p for p in model.parameters() if p.requires_grad], 0.1)
            arms[mode] = (model, ExactMarginalLogLikelihood(lik, model), opt)
        n_off = reps if N < 30000 else reps_off_large
        times, losses, iters, errors = {m: [] for m in modes}, {m: [] for m in modes}, {m: [] for m in modes}, {}

        def step(mode):
            model, mll, opt = arms[mode]
            operators._FULL_FAMILY_ROUTE = mode != "on_radial"
            try:
                with settings.fused_full(mode != "off"):
                    opt.zero_grad()
                    loss = mll.negative(model(X), y)
                    loss.backward()
                    opt.step()
            finally:
                operators._FULL_FAMILY_ROUTE = True
            return loss.detach()
        for it in range(warmup + reps):
            for mode in modes:                                 # alternating: one step of every arm per round
                if mode in errors or (mode == "off" and it >= warmup + n_off):
                    continue
                lcg.stats["iterations"] = 0
                try:
                    t, loss = _timed(lambda: step(mode))
                except RuntimeError as e:
                    errors[mode] = " ".join(str(e).split())[:300]
                    continue
                if it >= warmup:
                    times[mode].append(t)
                    iters[mode].append(lcg.stats["iterations"])
                losses[mode].append(float(loss))
        for mode in modes:
            rec = {"arm": "step", "model": "ARD RBF full", "mode": mode, "fused_full": mode != "off", "N": N, "d": d, "tag": tag}
            if mode in errors:
                rec["error"] = errors[mode]
            if times[mode]:
                rec.update(_stats(times[mode]), loss_first=losses[mode][0], loss_last=losses[mode][-1],
                           cg_iters_per_step=(sum(iters[mode]) / len(iters[mode])) if mode != "off" else None)
            _emit(rec, out)
        del arms
        torch.cuda.empty_cache()
    from rpgp_amd import precond
    precond.finish_factorisation_warmup()


def family_constant(out, tag):
    from rpgp_amd import ops
    from oracle import family as fmo
    from tests import radial_reference as rr
    dev = torch.device("cuda:0")
    res = {}
    for kind in rr.KINDS:
        worst = 0.0
        for d in (1, 3, 4, 5, 20):
            for (N, M) in ((257, 129), (1237, 301)):
                Z, Z1 = rr.inputs(N, d, d + N), rr.inputs(M, d, d + N + 1)
                fam = ops.Family(kind, d, torch.ones(1, device=dev))
                got = ops.family_dense(fam, torch.from_numpy(Z1).to(dev), torch.from_numpy(Z).to(dev), 1.3).cpu().numpy()
                d2 = rr.sqdist(Z1, Z)
                unit = 1.3 * rr.U * (1.0 + d2 * np.abs(fmo._dphi(kind, d2, fmo._phi(kind, d2))))
                worst = max(worst, float((np.abs(got.astype(np.float64) - rr.kernel(Z1, Z, kind, 1.3)) / unit).max()))
        res[kind] = worst
    _emit({"arm": "constant", "family_dense_error_over_unit": res, "twice_max": 2.0 * max(res.values()), "tag": tag}, out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="product,step")
    ap.add_argument("--constant", action="store_true")
    ap.add_argument("--N", type=int, default=50000)
    ap.add_argument("--dims", default="8,20,90")
    ap.add_argument("--widths", default="1,11")
    ap.add_argument("--sizes", default="7372:8,14939:18,50000:20")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--reps_off_large", type=int, default=9, help="repetitions of the flag-off step from N = 30 000 (O(N^3) each)")
    ap.add_argument("--modes", default="on,on_radial,off", help="--arms step: on, on_radial, off (see above)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.constant:
        family_constant(a.out, a.tag)
    arms = [] if a.constant else a.arms.split(",")
    if "product" in arms:
        product_arms(a.out, a.N, [int(v) for v in a.dims.split(",")], [int(v) for v in a.widths.split(",")], a.reps, a.warmup,
                     a.tag)
    if "step" in arms:
        step_arms(a.out, [tuple(int(v) for v in s.split(":")) for s in a.sizes.split(",")], a.reps, a.reps_off_large, a.warmup,
                  a.tag, tuple(a.modes.split(",")))
