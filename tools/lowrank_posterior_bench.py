"""Prediction with settings.lowrank_posterior on and off (the closed-form posterior of the explicit Chebyshev low-rank features,
lowrank_posterior.py), on synthetic stand-ins: the stages of the feature posterior (features, Gram, factor, test features,
solves), the feature kernel's time and write bandwidth, and each prediction mode (full: mean + covariance + test NLL; mean +
variances + test NLL; mean only) in a warmed process.  --weighted: the weighted rp_poly model (J = 20, k = 1) with the
lengthscales spread --spread times across the projections, served on column forms.  One JSON line per record, appended to
--out."""
import argparse, json, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rpgp_amd import backend, settings
from rpgp_amd.kernels import AdditiveStructureRBFKernel, ScaledProjectionKernel, ScaleKernel
from rpgp_amd.likelihoods import GaussianLikelihood, SmoothedBoxPrior
from rpgp_amd.models import ExactGPModel, ExactMarginalLogLikelihood

KAPPA = 0.84932180028801907


def model_of(N, d, J, n_test, half_width, dev, noise=0.1):
    g = torch.Generator().manual_seed(0)
    X = torch.randn(N, d, generator=g)
    P = torch.randn(d, J, generator=torch.Generator().manual_seed(1))
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
    y = (y - y.mean()) / y.std()
    Xs = torch.randn(n_test, d, generator=g) * 0.8
    ys = torch.sin(Xs).sum(1) / float(torch.sin(X).sum(1).std())
    ls = torch.full((d,), math.sqrt(d))
    if half_width is not None:                       # one factor on the lengthscale: the widest column has this half-width
        Z = (X / ls) @ P
        ls = ls * (KAPPA * float(((Z.max(0).values - Z.min(0).values) * 0.5).max()) / half_width)
    lin = torch.nn.Linear(d, J, bias=False)
    lin.weight.data = P.t().contiguous()
    k = ScaledProjectionKernel(lin, AdditiveStructureRBFKernel(J), prescale=True, ard_num_dims=d)
    k.initialize(lengthscale=ls)
    sk = ScaleKernel(k)
    lik = GaussianLikelihood(noise_prior=SmoothedBoxPrior(1e-4, 10, sigma=0.01))
    lik.noise = noise
    model = ExactGPModel(X.to(dev), y.to(dev), lik, sk).to(dev)
    model.eval()
    return model, lik, ExactMarginalLogLikelihood(lik, model), Xs.to(dev), ys.to(dev)


def weighted_model_of(N, d, J, n_test, half_width, spread, dev, noise=0.1):
    """model_of for the weighted rp_poly kernel (k = 1): lengthscale of projection j proportional to spread^(j / (J - 1)),
    scaled so that the widest column has the half-width."""
    from rpgp_amd.kernels import PolynomialProjectionKernel, inv_softplus
    g = torch.Generator().manual_seed(0)
    X = torch.randn(N, d, generator=g)
    P = torch.randn(d, J, generator=torch.Generator().manual_seed(1)) / math.sqrt(d)
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
    y = (y - y.mean()) / y.std()
    Xs = torch.randn(n_test, d, generator=g) * 0.8
    ys = torch.sin(Xs).sum(1) / float(torch.sin(X).sum(1).std())
    ls = torch.tensor([spread ** (j / max(J - 1, 1)) for j in range(J)])
    if half_width is not None:
        Z = (X @ P) / ls
        ls = ls * (KAPPA * float(((Z.max(0).values - Z.min(0).values) * 0.5).max()) / half_width)
    kern = PolynomialProjectionKernel(J, 1, d, "RBF", [P[:, j:j + 1].clone() for j in range(J)], weighted=True)
    kern.raw_lengthscales.data = inv_softplus(ls).reshape(1, -1).float()
    sk = ScaleKernel(kern)
    lik = GaussianLikelihood(noise_prior=SmoothedBoxPrior(1e-4, 10, sigma=0.01))
    lik.noise = noise
    model = ExactGPModel(X.to(dev), y.to(dev), lik, sk).to(dev)
    model.eval()
    return model, lik, ExactMarginalLogLikelihood(lik, model), Xs.to(dev), ys.to(dev)


def timed(fn, reps=1):
    ts, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2], out


def predict_mode(model, lik, mll, Xs, ys, mode):
    def run():
        with torch.no_grad(), settings.skip_posterior_variances(mode == "mean"):
            out = model(Xs)
            m = out.mean
            if mode == "mean":
                return float(m[0])
            nll = -mll(out, ys).item()
            if mode == "full":
                return float(out.covariance[0, 0]) + nll
            return float(out.variance[0]) + nll
    return run


def bench(name, N, d, J, n_test, half_width, sides, modes, out_path, reps, spread=None, tag=None):
    dev = torch.device("cuda:0")
    if spread is not None:
        model, lik, mll, Xs, ys = weighted_model_of(N, d, J, n_test, half_width, spread, dev)
    else:
        model, lik, mll, Xs, ys = model_of(N, d, J, n_test, half_width, dev)
    recs = []
    for on in sides:
        with settings.lowrank_posterior(on):
            model.prediction_strategy = None
            t_build, _ = timed(lambda: model(Xs[:1]))        # strategy build (+ one row)
            st = model.prediction_strategy
            rec = {"config": name, "N": N, "d": d, "J": J, "n_test": n_test, "half_width": half_width, "setting": on,
                   "max_rank": settings.lowrank_max_rank.value(),
                   "served": st.lowrank is not None, "strategy_build_s": round(t_build, 4)}
            if tag:
                rec["tag"] = tag
            if spread is not None:
                rec.update({"model": "rp_poly weighted k=1", "spread": spread})
            if on and st.lowrank is not None:
                lr = st.lowrank
                p, r, F = lr.ranks
                rec.update({"p": p, "r": r, "F": F, "tail": lr.form.tail, "rebuilds": lr.rebuilds})
                be = backend.get_backend()
                f = lr.form
                if spread is not None:
                    rec["class_ranks_p_r_columns"] = lr.class_ranks
                t_feat, _ = timed(lambda: lr._evaluate(be, lr.Z, f, lr.scale), reps=5)
                t_gram, M = timed(lambda: lr.B.t() @ lr.B, reps=3)
                t_fac, L = timed(lambda: torch.linalg.cholesky(lr.M), reps=3)
                Zs = lr._test_coordinates(Xs)
                t_tfeat, Bs = timed(lambda: lr._evaluate(be, Zs, f, lr.scale), reps=3)
                t_solve, _ = timed(lambda: lr._lower_solve(Bs.t()), reps=3)
                rec.update({"features_ms": round(1e3 * t_feat, 3),
                            "features_write_TBps": round(8.0 * N * F / t_feat / 1e12, 3),
                            "gram_ms": round(1e3 * t_gram, 3), "factor_ms": round(1e3 * t_fac, 3),
                            "test_features_ms": round(1e3 * t_tfeat, 3), "test_solve_ms": round(1e3 * t_solve, 3)})
                del M, L, Bs
            elif on:
                rec["reason"] = st.lowrank_fallback_reason
            for mode in modes.get(on, ()):
                model(Xs[:1])                                  # warm
                t, _ = timed(predict_mode(model, lik, mll, Xs, ys, mode), reps=reps)
                rec["predict_%s_s" % mode] = round(t, 4)
            model.prediction_strategy = None
            torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    with open(out_path, "a") as fh:
        for rec in recs:
            fh.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["c4", "c5x"], default="c4")
    ap.add_argument("--half_width", type=float, default=4.6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--off", action="store_true", help="also time the setting-off path")
    ap.add_argument("--max_rank", type=int, default=64, help="settings.lowrank_max_rank for every measurement (1 ... 128)")
    ap.add_argument("--weighted", action="store_true", help="the weighted rp_poly model (k = 1) instead of additive_rp")
    ap.add_argument("--spread", type=float, default=1.0, help="--weighted: longest / shortest lengthscale across projections")
    ap.add_argument("--tag", default=None, help="a label copied into every record (which run, which build)")
    ap.add_argument("--sides", default=None, help="which sides to run: on, off or on,off (default: on, and off with --off)")
    ap.add_argument("--out", default="profiles/lowrank_posterior_bench_c4.jsonl")
    a = ap.parse_args()
    settings.lowrank_max_rank._set(a.max_rank)
    sides = [True, False] if a.off else [True]
    if a.sides:
        sides = [x == "on" for x in a.sides.split(",")]
    if a.config == "c4" and a.weighted:
        # mean + variances + test NLL on 2 000 rows, either side
        bench("C4 weighted", 50000, 20, 20, 2000, a.half_width, sides, {True: ["var", "mean"], False: ["var", "mean"]}, a.out,
              a.reps, spread=a.spread, tag=a.tag)
    elif a.config == "c4":
        bench("C4", 50000, 20, 20, 2000, a.half_width, sides,
              {True: ["full", "var", "mean"], False: ["full", "mean"]}, a.out, a.reps)
    else:
        # the exact N = 391 386 model (3droad's size, J = 20, no grid) with 3droad's ~43 000 test rows: mean, variances and test
        # NLL on; the off side refuses the full covariance and is timed mean-only (--skip_posterior_variances)
        bench("C5x exact", 391386, 3, 20, 43487, a.half_width, [True, False] if a.off else [True],
              {True: ["var", "mean"], False: ["mean"]}, a.out, a.reps)


if __name__ == "__main__":
    main()
