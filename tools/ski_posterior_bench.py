"""Times the closed-form posterior of the grid-interpolation models (settings.ski_posterior) on one MI355X and
writes one JSON line per measurement (default profiles/ski_posterior_bench.jsonl).

  c5       synthetic N = 391 386, d = J = 3, grid 1024, 43 488 test rows (the shape of configuration C5): the Gram pass, the whole
           build (grid block, eigen step, Gram pass, factorisation), mean + variances + test NLL; with the setting off the
           strategy's build and the mean-only prediction, and what the variance request does.
  both     N = 14 939, J = 20, grid 1024, 1 660 test rows — a shape both paths serve: both timed, and the largest difference of
           their means and variances (three grids and a CG tolerance against one grid in closed form: reported, not asserted).
  gram     the Gram pass alone at J = 20, N = 50 000, grid 1024, with its rate against the N J coordinates it must read.

Every time is a host clock around work that ends in a device synchronise, after one warm-up of the same shape; the median of
`--reps` repeats.  The two settings are timed alternately in the same process."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _Rows(list):
    """The measurements; each is printed as it arrives."""

    def append(self, row):
        print(json.dumps(row), flush=True)
        super().append(row)


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def _model(N, M, d, J, G, dev, seed, noise=0.1):
    from rpgp_amd.kernels import AdditiveStructureRBFKernel, ScaledProjectionKernel, ScaleKernel
    from rpgp_amd.likelihoods import GaussianLikelihood, SmoothedBoxPrior
    from rpgp_amd.models import ExactGPModel
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g)
    y = torch.sin(X).sum(1) + 0.1 * torch.randn(N, generator=g)
    Xs = torch.randn(M, d, generator=g)
    ys = torch.sin(Xs).sum(1) + 0.1 * torch.randn(M, generator=g)
    lin = torch.nn.Linear(d, J, bias=False)
    lin.weight.data = torch.randn(J, d, generator=g) / d ** 0.5
    k = ScaledProjectionKernel(lin, AdditiveStructureRBFKernel(J, ski=True, ski_options={"grid_size": G, "num_dims": 1}),
                               prescale=True, ard_num_dims=d)
    k.initialize(lengthscale=torch.ones(d))
    sk = ScaleKernel(k)
    sk.outputscale = 1.0
    lik = GaussianLikelihood(noise_prior=SmoothedBoxPrior(1e-4, 10, sigma=0.01))
    lik.noise = noise
    model = ExactGPModel(X.to(dev), y.to(dev), lik, sk).to(dev)
    model.eval()
    return model, lik, Xs.to(dev), ys.to(dev)


def _closed_form(model, lik, Xs, ys, reps, tag, rows):
    """Build and prediction with the setting on; returns the predictive."""
    from rpgp_amd import backend, settings
    from rpgp_amd.models import PredictionStrategy

    def build():
        model.prediction_strategy = PredictionStrategy(model)
        return model.prediction_strategy

    with settings.ski_posterior(True), torch.no_grad():
        t_build, st = _timed(build, reps)
        post = st.ski_post
        if post is None:
            rows.append(dict(shape=tag, what="closed form not served", reason=st.ski_posterior_reason))
            return None
        be = backend.get_backend()
        r64 = post._residual(st)
        t_gram, _ = _timed(lambda: be.ski_gram(post.Z, post.state.gp, r64, post.G), reps)

        def predict():
            out = model(Xs)
            return out, float(lik(out).log_prob(ys.double()))
        t_pred, (out, lp) = _timed(predict, reps)
        N, J = post.Z.shape
        rows.append(dict(shape=tag, what="closed form", N=N, J=J, G=post.G, M=Xs.shape[0], F=post.features, rebuilds=post.rebuilds,
                         build_ms=1e3 * t_build, gram_ms=1e3 * t_gram, gram_rows_GBps=8e-9 * N * J / t_gram,
                         mean_var_nll_ms=1e3 * t_pred, test_nll=-lp / Xs.shape[0]))
        return out


def _exact(model, lik, Xs, ys, reps, tag, rows, variances):
    """The strategy with the setting off: build (mean cache) and the mean-only prediction; with `variances` the full prediction."""
    from rpgp_amd import settings
    from rpgp_amd.models import PredictionStrategy

    def build():
        model.prediction_strategy = PredictionStrategy(model)

    with torch.no_grad():
        t_build, _ = _timed(build, reps)
        with settings.skip_posterior_variances(True):
            t_mean, m_only = _timed(lambda: model(Xs), reps)
        row = dict(shape=tag, what="setting off", build_ms=1e3 * t_build, mean_only_ms=1e3 * t_mean)
        out = None
        try:
            if variances:
                def full():
                    o = model(Xs)
                    o.variance
                    return o
                t_var, out = _timed(full, 1)
                row["mean_var_ms"] = 1e3 * t_var
            else:
                model(Xs).variance
                row["variance_request"] = "served"
        except RuntimeError as e:
            row["variance_request"] = "RuntimeError: %s" % e
        rows.append(row)
        return out if out is not None else m_only


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--out", default=os.path.join("profiles", "ski_posterior_bench.jsonl"))
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--parts", default="c5,both,gram")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing can be timed here")
    dev = torch.device("cuda:0")
    rows = _Rows()
    parts = args.parts.split(",")
    if "c5" in parts:
        model, lik, Xs, ys = _model(391386, 43488, 3, 3, 1024, dev, seed=0)
        _closed_form(model, lik, Xs, ys, args.reps, "c5", rows)
        _exact(model, lik, Xs, ys, 1, "c5", rows, variances=False)
        del model
        torch.cuda.empty_cache()
    if "both" in parts:
        model, lik, Xs, ys = _model(14939, 1660, 20, 20, 1024, dev, seed=1)
        on = _closed_form(model, lik, Xs, ys, args.reps, "both", rows)
        off = _exact(model, lik, Xs, ys, 1, "both", rows, variances=True)
        if on is not None:
            rows.append(dict(shape="both", what="closed form against the setting off",
                             max_mean_diff=float((on.mean.double() - off.mean.double()).abs().max()),
                             max_var_diff=float((on.variance.double() - off.variance.double()).abs().max()),
                             max_var=float(off.variance.max())))
        del model, on, off
        torch.cuda.empty_cache()
    if "gram" in parts:
        from rpgp_amd import ops
        N, J, G = 50000, 20, 1024
        g = torch.Generator().manual_seed(2)
        Z = torch.randn(N, J, generator=g, dtype=torch.float64).to(dev)
        gp = ops.ski_grid(Z, None, G)
        r = torch.randn(N, 1, generator=g, dtype=torch.float64).to(dev)
        t, _ = _timed(lambda: ops.ski_gram(Z, gp, r, G), args.reps)
        rows.append(dict(shape="gram", what="Gram pass", N=N, J=J, G=G, gram_ms=1e3 * t, row_bytes=8 * N * J,
                         gram_rows_GBps=8e-9 * N * J / t, output_bytes=8 * (J * G) ** 2, output_GBps=8e-9 * (J * G) ** 2 / t))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
