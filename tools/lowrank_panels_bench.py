"""Timing of the panel plans of the low-rank product kernels (settings.lowrank_panels; csrc/rpgp_lowrank.hip) on
synthetic stand-ins of the BASELINE configs.  Two kinds of record, one JSON line each, appended to --out:

  steps:   optimiser steps at a first-step half-width, in the modes
             panels  settings.lowrank_kernel and settings.lowrank_panels on, rank cap 64
             parent  what runs without this setting: settings.lowrank_kernel on under the rank cap 128 (the cap-128 plan up to a
                     half-width of about 13, the sweep beyond), code that the panels leave untouched
           alternating, --rounds times, so that a drift of the device shows in both; median, minimum and maximum per mode, the
           panel count and the ranks of the last step and how many of the timed steps the low-rank form served.
  kernels: the plan creation (rpgp_lowrank_create_panels + rpgp_lowrank_grad_prepare, host time with the stream drained), the
           product and the derivative of a panel plan at T right-hand sides, device time by events over --reps calls; the split of
           the product into its three kernels comes from a kernel trace of this tool (rocprofv3 --kernel-trace --stats).

--weighted times the weighted rp_poly model (k = 1) with the lengthscales spread --spread times across the projections."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from rpgp_amd import settings, operators, ops, linear_cg as lcg
from rpgp_amd.training import create_exact_gp, make_optimizer
from rpgp_amd.models import ExactMarginalLogLikelihood
from lowrank_step_bench import _set_half_width, _weighted_model, _last      # (its recording lowrank_form wrappers are installed)

def _record_panels(cls):
    inner = cls.lowrank_form

    def form(self, noise=None):
        r = inner(self, noise)
        _last["panels"] = int(getattr(r, "panels", 0)) if r is not None else None
        return r
    cls.lowrank_form = form


_record_panels(operators.AdditiveRPOperator)
_record_panels(operators.FamilyAdditiveOperator)

KAPPA = 0.8493218002880191
TABLE = {"C2": ("C2 kin8nm-shaped RPA-GP", 7372, 8, 20), "C4": ("C4 synthetic 50k RPA-GP", 50000, 20, 20),
         "S": ("small", 3000, 8, 20)}
MODES = {"panels": (True, 64, True), "parent": (True, 128, False), "off": (False, 64, False)}


def _emit(res, out):
    print(json.dumps(res), flush=True)
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(res) + "\n")


def _model(N, d, J, half_width, weighted, spread, dev):
    g = torch.Generator().manual_seed(0)
    X = torch.randn(N, d, generator=g)
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
    y = (y - y.mean()) / y.std()
    Xtr, ytr = X.to(dev), y.to(dev)
    torch.manual_seed(0)
    import numpy as np
    np.random.seed(0)
    if weighted:
        model, lik = _weighted_model(Xtr, ytr, J, half_width, spread, dev)
    else:
        model, lik = create_exact_gp(Xtr, ytr, "additive_rp", J=J, noise_prior=True, kernel_type="RBF", learn_proj=False,
                                     prescale=True, space_proj=False)
        model = model.to(dev)
        _set_half_width(model, Xtr, half_width)
    return model, lik, Xtr, ytr


def steps(cfg, half_width, mode, nsteps, warmup, cg_tol, lr, weighted, spread, tag, out, rnd):
    name, N, d, J = TABLE[cfg]
    dev = torch.device("cuda:0")
    model, lik, Xtr, ytr = _model(N, d, J, half_width, weighted, spread, dev)
    mll = ExactMarginalLogLikelihood(lik, model)
    opt = make_optimizer(torch.optim.Adam, [p for p in model.parameters() if p.requires_grad], lr)
    on, cap, panels = MODES[mode]
    times, iters, served, forms = [], [], [], []
    with settings.cg_tolerance(cg_tol), settings.max_cg_iterations(10000), settings.lowrank_kernel(on), \
            settings.lowrank_max_rank(cap), settings.lowrank_panels(panels):
        model.train()
        for it in range(warmup + nsteps):
            _last.clear()
            lcg.stats["iterations"] = 0
            torch.cuda.synchronize(); t0 = time.perf_counter()
            opt.zero_grad()
            out_ = model(Xtr)
            loss = mll.negative(out_, ytr)
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            if it >= warmup:
                times.append(time.perf_counter() - t0)
                iters.append(lcg.stats["iterations"])
                served.append(bool(_last.get("served", False)))
                forms.append((_last.get("panels"), _last.get("pq")))
    st = sorted(times)
    res = {"record": "steps", "config": name, "N": N, "J": J, "mode": mode, "round": rnd, "half_width": half_width,
           "weighted": weighted, "spread": spread if weighted else None, "steps": nsteps, "warmup": warmup, "cg_tol": cg_tol,
           "lr": lr, "step_ms_median": 1e3 * st[len(st) // 2], "step_ms_min": 1e3 * st[0], "step_ms_max": 1e3 * st[-1],
           "cg_iters_per_step": sum(iters) / len(iters), "served_steps": sum(served), "panels_last": forms[-1][0],
           "pq_last": forms[-1][1], "tag": tag}
    _emit(res, out)


def lbfgs(cfg, half_width, mode, max_iter, cg_tol, tag, out):
    """One L-BFGS fit (strong-Wolfe, fixed probes) from a first-step half-width: the evaluations the low-rank form served, with
    how many panels, and the half-widths of the ones it did not."""
    name, N, d, J = TABLE[cfg]
    dev = torch.device("cuda:0")
    model, lik, Xtr, ytr = _model(N, d, J, half_width, False, 1.0, dev)
    mll = ExactMarginalLogLikelihood(lik, model)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.LBFGS(params, lr=1.0, max_iter=max_iter, line_search_fn="strong_wolfe")
    on, cap, panels = MODES[mode]
    evals = []

    def closure():
        opt.zero_grad()
        _last.clear()
        out_ = model(Xtr)
        loss = mll.negative(out_, ytr)
        loss.backward()
        pr = getattr(out_.covariance, "_prep", None)
        evals.append((bool(_last.get("served", False)), _last.get("panels"), None if pr is None else pr.max_abs))
        return loss

    with settings.cg_tolerance(cg_tol), settings.max_cg_iterations(10000), settings.deterministic_probes(True), \
            settings.lowrank_kernel(on), settings.lowrank_max_rank(cap), settings.lowrank_panels(panels):
        model.train()
        first = float(closure())
        del evals[:]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        opt.step(closure)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        final = float(mll.negative(model(Xtr), ytr))
    st = opt.state[opt._params[0]]
    unserved = sorted(round(h, 1) for s_, _, h in evals if not s_ and h is not None)
    _emit({"record": "lbfgs", "config": name, "N": N, "J": J, "mode": mode, "half_width": half_width, "max_iter": max_iter,
           "lbfgs_iterations": int(st["n_iter"]), "evaluations": len(evals), "served_evaluations": sum(e[0] for e in evals),
           "served_with_panels": sum(1 for e in evals if e[0] and e[1]), "panel_counts": sorted({e[1] for e in evals if e[1]}),
           "unserved_half_widths": unserved, "wall_s": wall, "loss_first": first, "loss_final": final, "tag": tag}, out)


def kernels(cfg, half_width, T, reps, tag, out):
    name, N, d, J = TABLE[cfg]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    w = half_width / KAPPA
    Z = ((torch.rand(N, J, generator=g) * 2.0 - 1.0) * w)
    Z[0], Z[1] = w, -w
    Z = Z.to(dev)
    L, R = torch.randn(N, T, generator=g).to(dev), torch.randn(N, T, generator=g).to(dev)
    prep = ops.Prepared(Z)
    tol = ops.lowrank_train_tol(N, J, 1.0 / J, 0.05)
    plan = None
    create = []
    for _ in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        plan = ops.LowrankTrainPlan(prep, tol, panels=True)
        torch.cuda.synchronize()
        create.append(1e3 * (time.perf_counter() - t0))
    if not plan.served or not plan.panels:
        _emit({"record": "kernels", "config": name, "half_width": half_width, "served": False, "tag": tag}, out)
        return
    outb = torch.empty(N, T, device=dev)

    def timed(fn):
        for _ in range(3):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        return ms[len(ms) // 2], ms[0], ms[-1]

    wts = torch.ones(J, device=dev)
    prod = timed(lambda: ops.mvm_sym_lowrank_weighted(plan, prep, wts, L, 1.0 / J, 0.05, out=outb))
    grad = timed(lambda: ops.bilinear_grad_lowrank(plan, L, R, 1.0 / J))
    sweep = timed(lambda: ops.mvm_sym(Z, L, 1.0 / J, 0.05))
    cs = sorted(create)
    _emit({"record": "kernels", "config": name, "N": N, "J": J, "T": T, "half_width": half_width, "served": True,
           "panels": plan.panels, "h_p": plan.h_p, "p": plan.p, "q": plan.q, "tol": tol,
           "plan_create_ms_median_min_max": [cs[len(cs) // 2], cs[0], cs[-1]], "product_ms_median_min_max": list(prod),
           "derivative_ms_median_min_max": list(grad), "direct_sweep_product_ms_median_min_max": list(sweep), "reps": reps,
           "tag": tag}, out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--half_widths", default="8,10,16,24,40")
    ap.add_argument("--modes", default="panels,parent")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cg_tol", type=float, default=0.05)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--weighted", action="store_true")
    ap.add_argument("--spread", type=float, default=8.0)
    ap.add_argument("--kernels", action="store_true", help="the plan creation, the product and the derivative instead of steps")
    ap.add_argument("--lbfgs", type=int, default=0, help="one L-BFGS fit of at most this many iterations per mode instead")
    ap.add_argument("--T", type=int, default=11)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hs = [float(h) for h in a.half_widths.split(",")]
    if a.lbfgs:
        for m in a.modes.split(","):
            lbfgs(a.config, hs[0], m, a.lbfgs, a.cg_tol, a.tag, a.out)
    elif a.kernels:
        for h in hs:
            kernels(a.config, h, a.T, a.reps, a.tag, a.out)
    else:
        for h in hs:
            for rnd in range(a.rounds):
                for m in a.modes.split(","):
                    steps(a.config, h, m, a.steps, a.warmup, a.cg_tol, a.lr, a.weighted, a.spread, a.tag, a.out, rnd)
    from rpgp_amd import precond
    precond.finish_factorisation_warmup()
