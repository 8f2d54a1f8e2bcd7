"""Optimiser-step timing of the exact additive-RP GP with settings.lowrank_kernel off and on (the Chebyshev low-rank solve
and derivative of csrc/rpgp_lowrank.hip), on synthetic stand-ins of the BASELINE configs.  Prints one JSON line per
(configuration, setting): the median step time over the timed steps (after warm-up steps), the CG iterations per step, the
ranks p, q of the training plan and whether the low-rank form served every timed step.  --weighted times the weighted rp_poly
model instead (k = 1: one lengthscale and one weight per projection, the FamilyAdditiveOperator), with the lengthscales spread
--spread times across the projections.  --max_rank sets settings.lowrank_max_rank for the run (64 by default; up to 128, which
serves half-widths up to about 13).  The parent of a change is timed by running its own copy of this tool with --modes off."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rpgp_amd import settings, operators, linear_cg as lcg
from rpgp_amd.training import create_exact_gp, make_optimizer
from rpgp_amd.models import ExactMarginalLogLikelihood

_last = {}
_orig_form = operators.AdditiveRPOperator.lowrank_form


def _recording_form(self, noise=None):
    r = _orig_form(self, noise)
    _last["served"] = r is not None
    _last["pq"] = (r.p, r.q) if r is not None else None
    return r


operators.AdditiveRPOperator.lowrank_form = _recording_form
_orig_family_form = operators.FamilyAdditiveOperator.lowrank_form


def _recording_family_form(self, noise=None):
    r = _orig_family_form(self, noise)
    _last["served"] = r is not None
    _last["pq"] = (r.p, r.q) if r is not None else None
    return r


operators.FamilyAdditiveOperator.lowrank_form = _recording_family_form


def _set_half_width(model, X, h):
    """One factor on every lengthscale so that the first step's widest projected column has half-width h (plan units)."""
    pk = model.covar_module.base_kernel
    with torch.no_grad():
        Z = pk.project(X) * (pk.base_kernel.input_scale_factor() or 1.0)
        h0 = 0.8493218002880191 * float(((Z.max(0).values - Z.min(0).values) * 0.5).max())
        pk.initialize(lengthscale=pk.lengthscale.detach().reshape(-1) * (h0 / h))


def _weighted_model(X, y, J, half_width, spread, dev):
    """The weighted rp_poly model (k = 1) of tools/lowrank_mll_bench.py --weighted: lengthscale of projection j proportional to
    spread^(j / (J - 1)), scaled so that the widest column has the half-width; the mixing weights as the kernel initialises
    them."""
    from rpgp_amd.kernels import inv_softplus
    model, lik = create_exact_gp(X, y, "rp_poly", J=J, k=1, noise_prior=True, kernel_type="RBF", learn_proj=False,
                                 weighted=True)
    model = model.to(dev)
    kern = model.covar_module.base_kernel
    with torch.no_grad():
        ls = torch.tensor([spread ** (j / max(J - 1, 1)) for j in range(J)], dtype=torch.float64, device=dev)
        Z = (X.double() @ kern.projection_module.weight.double().t()) / ls
        h0 = 0.8493218002880191 * float(((Z.max(0).values - Z.min(0).values) * 0.5).max())
        if half_width is not None:
            ls = ls * (h0 / half_width)
        kern.raw_lengthscales.data = inv_softplus(ls).reshape(1, -1).to(kern.raw_lengthscales)
    return model, lik


def run(name, N, d, J, steps, warmup, on, space_proj, cg_tol, half_width=None, lr=0.1, quiet=False, weighted=False,
        spread=1.0, tag=None, out=None, max_rank=64):
    dev = torch.device("cuda:0")
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
                                     prescale=True, space_proj=space_proj)
        model = model.to(dev)
        if half_width is not None:
            _set_half_width(model, Xtr, half_width)
    mll = ExactMarginalLogLikelihood(lik, model)
    opt = make_optimizer(torch.optim.Adam, [p for p in model.parameters() if p.requires_grad], lr)
    res = {"config": name, "N": N, "d": d, "J": J, "lowrank_kernel": on, "steps": steps, "warmup": warmup,
           "half_width": half_width, "lr": lr, "cg_tol": cg_tol, "max_rank": max_rank}
    if weighted:
        res.update(model="rp_poly weighted k=1", spread=spread)
    if tag is not None:
        res["tag"] = tag
    times, iters, losses, served, ranks = [], [], [], [], []
    with settings.cg_tolerance(cg_tol), settings.max_cg_iterations(10000), settings.lowrank_kernel(on), \
            settings.lowrank_max_rank(max_rank):
        model.train()
        for it in range(warmup + steps):
            _last.clear()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            lcg.stats["iterations"] = 0
            opt.zero_grad()
            loss = mll.negative(model(Xtr), ytr)
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            if it >= warmup:
                times.append(time.perf_counter() - t0)
                iters.append(lcg.stats["iterations"])
                served.append(bool(_last.get("served", False)))
                ranks.append(_last.get("pq"))
            losses.append(loss.item())
            if not quiet:
                print("%s on=%s step %d: %.2f ms, %d CG iterations, served %s" % (name, on, it, 1e3 * (time.perf_counter() - t0),
                      lcg.stats["iterations"], _last.get("served", False)), file=sys.stderr, flush=True)
    st = sorted(times)
    pq = [r for r in ranks if r is not None]
    res.update({"step_ms_median": 1e3 * st[len(st) // 2], "step_ms_min": 1e3 * st[0], "step_ms_max": 1e3 * st[-1],
                "cg_iters_per_step": sum(iters) / len(iters), "served_all": all(served), "served_steps": sum(served),
                "p": [r[0] for r in pq][-1] if pq else None, "q": [r[1] for r in pq][-1] if pq else None,
                "p_range": [min(r[0] for r in pq), max(r[0] for r in pq)] if pq else None,
                "q_range": [min(r[1] for r in pq), max(r[1] for r in pq)] if pq else None,
                "loss_first": losses[0], "loss_last": losses[-1]})
    if not quiet:
        print(json.dumps(res), flush=True)
        if out:
            with open(out, "a") as f:
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C4")
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cg_tol", type=float, default=0.05)
    ap.add_argument("--half_width", type=float, default=None,
                    help="scale the initial lengthscales so that the first step's plan half-width is this (default: as built)")
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--weighted", action="store_true", help="the weighted rp_poly model (k = 1) instead of additive_rp")
    ap.add_argument("--spread", type=float, default=1.0, help="--weighted: longest / shortest lengthscale across projections")
    ap.add_argument("--max_rank", type=int, default=64,
                    help="settings.lowrank_max_rank: the largest p, q the low-rank form serves (1 ... 128, default 64)")
    ap.add_argument("--tag", default=None, help="a label copied into every record (which run, which build)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    table = {"C2": ("C2 kin8nm-shaped RPA-GP", 7372, 8, 20, False), "C3": ("C3 elevators-shaped DPA-GP", 14939, 18, 20, True),
             "C4": ("C4 synthetic 50k RPA-GP", 50000, 20, 20, False),
             # C5's N with the exact kernel (no SKI): a synthetic stand-in with J = 20
             "C5X": ("C5-sized exact RPA-GP (synthetic, J=20, no SKI)", 391386, 20, 20, False),
             "S": ("small", 3000, 8, 20, False)}
    run("warm-up", 3000, 8, 20, 1, 1, True, False, a.cg_tol, quiet=True, weighted=a.weighted,
        spread=a.spread)                                                       # first use of every library, untimed
    for c in a.configs.split(","):
        name, N, d, J, sp = table[c]
        for m in a.modes.split(","):
            run(name, N, d, J, a.steps, a.warmup, m == "on", sp, a.cg_tol, a.half_width, a.lr, weighted=a.weighted,
                spread=a.spread, tag=a.tag, out=a.out, max_rank=a.max_rank)
    # (the preconditioner's library warm-up runs in a helper thread: a run of a few fast steps must not end underneath it)
    from rpgp_amd import precond
    precond.finish_factorisation_warmup()
