"""Optimiser-step timing of the exact additive-RP GP with the closed-form features objective (settings.lowrank_mll) against the
setting off and against settings.lowrank_kernel, on synthetic stand-ins of the BASELINE configs, plus the stages of one
features-mode evaluation (features, Gram, Cholesky, Y = B M^-1, the adjoint kernel and its read bandwidth, beside the features
kernel at the same N, J, p, r) and optionally one L-BFGS fit.  --weighted builds the weighted rp_poly model (J = 20, k = 1: one
lengthscale and one weight per projection, served on column forms) with the lengthscales spread --spread times across the
projections; --max_forms 1 holds it to a single form for comparison.  Prints, and appends to --out, one JSON line per
measurement."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rpgp_amd import settings, ops, operators
from rpgp_amd.training import create_exact_gp, make_optimizer
from rpgp_amd.models import ExactMarginalLogLikelihood

KAPPA = 0.8493218002880191
_last = {}
_orig = operators.AdditiveRPOperator.lowrank_mll_form


def _recording(self, noise=None):
    r = _orig(self, noise)
    _last["served"] = r is not None
    _last["ranks"] = r.ranks if r is not None else None
    _last["class_ranks"] = getattr(r, "class_ranks", None)
    _last["reason"] = self.lowrank_mll_reason
    return r


operators.AdditiveRPOperator.lowrank_mll_form = _recording


WEIGHTED = {"on": False, "spread": 1.0}


def _weighted_problem(X, y, J, half_width, spread, dev):
    """The weighted rp_poly model (k = 1): lengthscale of projection j proportional to spread^(j / (J - 1)), scaled so that the
    widest column has the half-width; the mixing weights as the kernel initialises them."""
    from rpgp_amd.kernels import inv_softplus
    model, lik = create_exact_gp(X, y, "rp_poly", J=J, k=1, noise_prior=True, kernel_type="RBF", learn_proj=False,
                                 weighted=True)
    model = model.to(dev)
    kern = model.covar_module.base_kernel
    with torch.no_grad():
        ls = torch.tensor([spread ** (j / max(J - 1, 1)) for j in range(J)], dtype=torch.float64, device=dev)
        Z = (X.double() @ kern.projection_module.weight.double().t()) / ls
        h0 = KAPPA * float(((Z.max(0).values - Z.min(0).values) * 0.5).max())
        if half_width is not None:
            ls = ls * (h0 / half_width)
        kern.raw_lengthscales.data = inv_softplus(ls).reshape(1, -1).to(kern.raw_lengthscales)
    return model, lik


def _problem(N, d, J, half_width, dev):
    g = torch.Generator().manual_seed(0)
    X = torch.randn(N, d, generator=g)
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
    y = (y - y.mean()) / y.std()
    X, y = X.to(dev), y.to(dev)
    torch.manual_seed(0)
    if WEIGHTED["on"]:
        return _weighted_problem(X, y, J, half_width, WEIGHTED["spread"], dev) + (X, y)
    model, lik = create_exact_gp(X, y, "additive_rp", J=J, noise_prior=True, kernel_type="RBF", learn_proj=False,
                                 prescale=True)
    model = model.to(dev)
    if half_width is not None:
        pk = model.covar_module.base_kernel
        with torch.no_grad():
            Z = pk.project(X) * (pk.base_kernel.input_scale_factor() or 1.0)
            h0 = KAPPA * float(((Z.max(0).values - Z.min(0).values) * 0.5).max())
            pk.initialize(lengthscale=pk.lengthscale.detach().reshape(-1) * (h0 / half_width))
    return model, lik, X, y


def _timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for _ in range(reps):
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    return sorted(ts)[len(ts) // 2], out


def steps(name, N, d, J, mode, n_steps, warmup, half_width, out):
    dev = torch.device("cuda:0")
    model, lik, X, y = _problem(N, d, J, half_width, dev)
    mll = ExactMarginalLogLikelihood(lik, model)
    opt = make_optimizer(torch.optim.Adam, [p for p in model.parameters() if p.requires_grad], 0.1)
    times, served, ranks = [], [], []
    with settings.lowrank_mll(mode == "mll"), settings.lowrank_kernel(mode == "kernel"), settings.cg_tolerance(0.05), \
            settings.max_cg_iterations(10000):
        model.train()
        for it in range(warmup + n_steps):
            _last.clear()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            opt.zero_grad()
            loss = mll.negative_and_backward(model(X), y)
            opt.step()
            torch.cuda.synchronize()
            if it >= warmup:
                times.append(time.perf_counter() - t0)
                served.append(bool(_last.get("served", False)))
                ranks.append(_last.get("ranks"))
            print("%s %s step %d: %.2f ms loss %.6f" % (name, mode, it, 1e3 * (time.perf_counter() - t0), float(loss)),
                  file=sys.stderr, flush=True)
    st = sorted(times)
    res = {"kind": "step", "config": name, "N": N, "d": d, "J": J, "mode": mode, "half_width": half_width,
           "max_rank": settings.lowrank_max_rank.value(), "steps": n_steps, "warmup": warmup, "step_ms_median": 1e3 * st[len(st) // 2], "step_ms_min": 1e3 * st[0],
           "step_ms_max": 1e3 * st[-1], "served_steps": sum(served) if mode == "mll" else None,
           "ranks_pr_F": ranks[-1] if mode == "mll" else None}
    if WEIGHTED["on"]:
        res.update(_weighted_tags(), class_ranks_p_r_columns=_last.get("class_ranks") if mode == "mll" else None)
    _emit(res, out)


def _weighted_tags():
    from rpgp_amd import lowrank_posterior
    return {"model": "rp_poly weighted k=1", "spread": WEIGHTED["spread"], "max_forms": getattr(lowrank_posterior, "MAX_FORMS", None)}


def stages_weighted(name, N, d, J, half_width, out):
    """The stages of one features-mode evaluation of the weighted model: the feature and adjoint launches of every class
    (summed), the Gram matrix, its factor and Y = B M^-1."""
    from rpgp_amd import backend
    from rpgp_amd.lowrank_posterior import column_forms
    dev = torch.device("cuda:0")
    be = backend.get_backend()
    model, lik, X, y = _problem(N, d, J, half_width, dev)
    kern = model.covar_module.base_kernel
    cap = settings.lowrank_max_rank.value()
    with torch.no_grad():
        Z = kern.project(X).double().contiguous()
        s, noise = float(model.covar_module.outputscale), float(lik.noise)
        forms, why = column_forms(be, Z, Z.min(0).values, Z.max(0).values, kern.outputscales.double(), s, noise)
        if forms is None:
            _emit(dict(_weighted_tags(), kind="stages", config=name, N=N, J=J, half_width=half_width, max_rank=cap,
                       served=False, reason=why), out)
            return
        t_feat, B = _timed(lambda: forms.features(be, Z))
        t_gram, M = _timed(lambda: B.t() @ B)
        M.diagonal().add_(noise)
        t_chol, L = _timed(lambda: torch.linalg.cholesky_ex(M)[0])
        t_minv, Minv = _timed(lambda: torch.cholesky_inverse(L))
        t_y, Y = _timed(lambda: B @ Minv)
        alpha = torch.randn(N, 1, dtype=torch.float64, device=dev)
        v = (B.t() @ alpha).reshape(-1)
        gZ = torch.empty_like(Z)

        def adjoint():
            for c in forms.classes:
                be.lowrank_features_grad_cols(Z, c.cols, c.mid, c.inv_w, c.G, forms.col_scale[c.cols], Y[:, c.f0:c.f1], alpha,
                                              v[c.f0:c.f1], -1.0, 1.0, out=gZ, **forms.kw)
            return gZ
        t_grad, _ = _timed(adjoint)
    res = dict(_weighted_tags(), kind="stages", config=name, N=N, J=J, p=forms.p, r=forms.r, F=forms.F,
               class_ranks_p_r_columns=forms.class_ranks, half_width=half_width, max_rank=cap, tail=forms.tail,
               features_ms=t_feat, gram_ms=t_gram, cholesky_ms=t_chol, cholesky_inverse_ms=t_minv, Y_ms=t_y,
               grad_kernel_ms=t_grad)
    _emit(res, out)


def stages(name, N, d, J, half_width, out):
    """The stages of one features-mode evaluation at the model's first step."""
    if WEIGHTED["on"]:
        return stages_weighted(name, N, d, J, half_width, out)
    from rpgp_amd.lowrank_posterior import _Form, LowrankPosterior, tail_tolerance
    dev = torch.device("cuda:0")
    model, lik, X, y = _problem(N, d, J, half_width, dev)
    pk = model.covar_module.base_kernel
    with torch.no_grad():
        Z = (pk.project(X) * (pk.base_kernel.input_scale_factor() or 1.0)).double().contiguous()
        s = float(model.covar_module.outputscale) / J
        noise = float(lik.noise)
        mid, h = LowrankPosterior._interval(Z.min(0).values, Z.max(0).values)
        cap = settings.lowrank_max_rank.value()
        tol = tail_tolerance(N, s * J, noise)
        p, r, tail, G = ops.lowrank_post_select(h, tol, cap)
        if p == 0:
            _emit({"kind": "stages", "config": name, "N": N, "J": J, "half_width": half_width, "max_rank": cap, "served": False},
                  out)
            return
        ts = []
        for _ in range(5):                                # the host selection (no device work)
            t0 = time.perf_counter()
            ops.lowrank_post_select(h, tol, cap)
            ts.append(time.perf_counter() - t0)
        t_select = 1e3 * sorted(ts)[2]
        f = _Form(mid, h, p, r, tail, G)
        F = J * r
        t_feat, B = _timed(lambda: ops.lowrank_features(Z, f.mid, f.inv_w, f.G, s, max_rank=cap))
        t_gram, M = _timed(lambda: B.t() @ B)
        M.diagonal().add_(noise)
        t_chol, L = _timed(lambda: torch.linalg.cholesky_ex(M)[0])
        t_minv, Minv = _timed(lambda: torch.cholesky_inverse(L))
        t_y, Y = _timed(lambda: B @ Minv)
        alpha = torch.randn(N, 1, dtype=torch.float64, device=dev)
        v = B.t() @ alpha
        t_grad, _ = _timed(lambda: ops.lowrank_features_grad(Z, f.mid, f.inv_w, f.G, s, Y, alpha, v, -1.0, 1.0, max_rank=cap))
    read = 8.0 * (N * F + N * J + N + F)                 # Y, Z, alpha, v
    res = {"kind": "stages", "config": name, "N": N, "J": J, "p": p, "r": r, "F": F, "half_width": half_width,
           "max_rank": cap, "tail": tail, "select_host_ms": t_select,
           "features_ms": t_feat, "gram_ms": t_gram, "cholesky_ms": t_chol, "cholesky_inverse_ms": t_minv, "Y_ms": t_y,
           "grad_kernel_ms": t_grad, "grad_kernel_read_TBps": read / (t_grad * 1e-3) / 1e12,
           "features_write_TBps": 8.0 * N * F / (t_feat * 1e-3) / 1e12, "grad_over_features": t_grad / t_feat}
    _emit(res, out)


def lbfgs_fit(name, N, d, J, half_width, max_iter, out):
    dev = torch.device("cuda:0")
    model, lik, X, y = _problem(N, d, J, half_width, dev)
    mll = ExactMarginalLogLikelihood(lik, model)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.LBFGS(params, lr=1.0, max_iter=max_iter, line_search_fn="strong_wolfe")
    evals, served, reasons = [0], [0], []

    def closure():
        opt.zero_grad()
        _last.clear()
        loss = mll.negative(model(X), y)
        loss.backward()
        evals[0] += 1
        served[0] += bool(_last.get("served", False))
        if evals[0] > 1 and not _last.get("served", False):
            reasons.append(_last.get("reason"))
        return loss

    with settings.lowrank_mll(True):
        model.train()
        first = float(closure())
        torch.cuda.synchronize(); t0 = time.perf_counter()
        opt.step(closure)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        final = float(mll.negative(model(X), y))
    st = opt.state[opt._params[0]]
    res = {"kind": "lbfgs", "config": name, "N": N, "J": J, "half_width": half_width, "max_iter": max_iter,
           "max_rank": settings.lowrank_max_rank.value(),
           "lbfgs_iterations": int(st["n_iter"]), "evaluations": evals[0] - 1, "served_evaluations": served[0] - 1,
           "unserved_reasons": reasons, "wall_s": wall, "loss_first": first, "loss_final": final}
    _emit(res, out)


def _emit(res, out):
    if globals().get("TAG"):
        res = dict(res, tag=TAG)
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C4")
    ap.add_argument("--modes", default="off,kernel,mll")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--half_width", type=float, default=4.6)
    ap.add_argument("--stages", action="store_true", help="also time the stages of one features-mode evaluation")
    ap.add_argument("--lbfgs", type=int, default=0, help="also run one L-BFGS fit of at most this many iterations")
    ap.add_argument("--max_rank", type=int, default=64, help="settings.lowrank_max_rank for every measurement (1 ... 128)")
    ap.add_argument("--weighted", action="store_true", help="the weighted rp_poly model (k = 1) instead of additive_rp")
    ap.add_argument("--spread", type=float, default=1.0, help="--weighted: longest / shortest lengthscale across projections")
    ap.add_argument("--max_forms", type=int, default=None, help="--weighted: at most this many column forms (default: 4)")
    ap.add_argument("--tag", default=None, help="a label copied into every record (which run, which build)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    TAG = a.tag
    settings.lowrank_max_rank._set(a.max_rank)
    WEIGHTED.update(on=a.weighted, spread=a.spread)
    if a.max_forms is not None:
        from rpgp_amd import lowrank_posterior
        lowrank_posterior.MAX_FORMS = a.max_forms
    table = {"C4": ("C4 synthetic 50k RPA-GP", 50000, 20, 20),
             "C5X": ("C5-sized exact RPA-GP (synthetic, J=20, no SKI)", 391386, 20, 20)}
    for c in a.configs.split(","):
        name, N, d, J = table[c]
        for m in a.modes.split(","):
            if m:
                steps(name, N, d, J, m, a.steps, a.warmup, a.half_width, a.out)
        if a.stages:
            stages(name, N, d, J, a.half_width, a.out)
        if a.lbfgs:
            lbfgs_fit(name, N, d, J, a.half_width, a.lbfgs, a.out)
