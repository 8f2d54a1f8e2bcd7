"""Timing of `kind: sgpr` (csrc/rpgp_inducing.hip, rpgp_amd/sgpr.py) on the MI355X.  One JSON line per record,
appended to --out (profiles/sgpr_bench.jsonl).  Device events, warm-up, repetitions ALTERNATING between the arms in one process,
min / median / max reported, losses compared across the arms on the same seeded inputs.

  --arms step     one optimiser step (Adam; forward, backward, update) of the ARD RBF model at the C2 / C3 / C4 shapes
                  (N = 7 372, 14 939, 50 000; d = 8, 18, 20) with M = 400 and 800 inducing points:
                    native        the inducing-point sums (one rpgp_inducing_gram, one rpgp_inducing_grad)
                    materialised  the same objective with K_fu (N x M float32) from ops.radial_dense and torch float64 matmuls
                                  on the device for G, g, K C, S^T Z — the entries of the backend replaced, nothing else
                    exact         the exact ARD step of `kind: full` under settings.fused_full (not the same model: what the
                                  sparse baseline is compared against)
  --arms kernels  the two entries alone at the same shapes, with the float64 operations they issue (Gram 2 N M (M + T); derivative
                  2 N M M + 2 N M T + 2 N M (2 d + 1)) over the time: an end-to-end rate of the entry (slab pass included), not a
                  kernel's share of peak."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def _data(N, d, dev):
    g = torch.Generator().manual_seed(0)
    X = torch.randn(N, d, generator=g)
    y = torch.sin(X).sum(1) + 0.05 * torch.randn(N, generator=g)
    return X.to(dev), ((y - y.mean()) / y.std()).to(dev)


def _materialised_backend():
    """The HIP backend with the two inducing-point entries served from a materialised K_fu (RBF only: phi' = -phi / 2)."""
    from rpgp_amd import backend, ops

    class Materialised(backend.HipBackend):
        @staticmethod
        def inducing_gram(kind, Z, U, Y=None, rows=None):
            K = ops.radial_dense(kind, Z, U, 1.0).double()
            return K.t() @ K, K.t() @ Y.double()

        @staticmethod
        def inducing_grad(kind, Z, U, Y, C, v, rows=None):
            assert kind == "RBF"
            K = ops.radial_dense(kind, Z, U, 1.0).double()
            S = (2.0 * (K @ C) + Y.double() @ v.t()) * (-0.5 * K)
            Z64, U64 = Z.double(), U.double()
            P, cs = S.t() @ Z64, S.sum(0)
            gU = 2.0 * (cs[:, None] * U64 - P)
            q = (S.sum(1)[:, None] * Z64 * Z64).sum(0) - 2.0 * (U64 * P).sum(0) + (cs[:, None] * U64 * U64).sum(0)
            return gU, q
    return Materialised()


def step_arms(out, sizes, points, reps, warmup, tag):
    from rpgp_amd import backend, settings
    from rpgp_amd.models import ExactMarginalLogLikelihood
    from rpgp_amd.training import create_exact_gp, make_optimizer
    dev = torch.device("cuda:0")
    mat = _materialised_backend()
    for N, d in sizes:
        X, y = _data(N, d, dev)
        for M in points:
            arms = {}
            for mode in ("native", "materialised", "exact"):
                torch.manual_seed(0)
                kw = dict(noise_prior=True, ard=True, kernel_type="RBF", init_lengthscale_range=(d ** 0.5, d ** 0.5))
                if mode != "exact":
                    kw["inducing_points"] = M
                model, lik = create_exact_gp(X, y, "full" if mode == "exact" else "sgpr", **kw)
                model = model.to(dev)
                model.train()
                opt = make_optimizer(torch.optim.Adam, [p for p in model.parameters() if p.requires_grad], 0.01)
                arms[mode] = (model, ExactMarginalLogLikelihood(lik, model), opt)

            def step(mode):
                model, mll, opt = arms[mode]
                prev = backend.set_backend(mat) if mode == "materialised" else None
                try:
                    with settings.fused_full(mode == "exact"):
                        opt.zero_grad()
                        loss = mll.negative(model(X), y)
                        loss.backward()
                        opt.step()
                finally:
                    if prev is not None:
                        backend.set_backend(prev)
                return loss.detach()
            times, losses = {m: [] for m in arms}, {m: [] for m in arms}
            for it in range(warmup + reps):
                for mode in arms:                                  # alternating: one step of every arm per round
                    t, loss = _timed(lambda: step(mode))
                    if it >= warmup:
                        times[mode].append(t)
                    losses[mode].append(float(loss))
            for mode in arms:
                _emit({"arm": "step", "mode": mode, "N": N, "d": d, "M": M if mode != "exact" else None, "tag": tag,
                       **_stats(times[mode]), "loss_first": losses[mode][0], "loss_last": losses[mode][-1],
                       "loss_rel_vs_native": [abs(a - b) / abs(b) for a, b in zip(losses[mode], losses["native"])][-1]
                       if mode == "materialised" else None}, out)
            del arms
            torch.cuda.empty_cache()
    from rpgp_amd import precond
    precond.finish_factorisation_warmup()


def kernel_arms(out, sizes, points, reps, warmup, tag):
    from rpgp_amd import ops
    dev = torch.device("cuda:0")
    T = 2
    for N, d in sizes:
        X, y = _data(N, d, dev)
        Z = ((X - X.mean(0)) / d ** 0.5).contiguous()
        Y = torch.stack([y, torch.ones_like(y)], 1).contiguous()
        for M in points:
            U = Z[:M].clone()
            g = torch.Generator().manual_seed(1)
            C = torch.randn(M, M, generator=g, dtype=torch.float64) / M
            C, v = (0.5 * (C + C.t())).to(dev), torch.randn(M, T, generator=g, dtype=torch.float64).to(dev)
            arms = {"gram": (lambda: ops.inducing_gram("RBF", Z, U, Y), 2.0 * N * M * (M + T)),
                    "grad": (lambda: ops.inducing_grad("RBF", Z, U, Y, C, v), 2.0 * N * M * M + 2.0 * N * M * T +
                             2.0 * N * M * (2 * d + 1))}
            times = {k: [] for k in arms}
            for it in range(warmup + reps):
                for k, (fn, _) in arms.items():
                    t, _o = _timed(fn)
                    if it >= warmup:
                        times[k].append(t)
            for k, (_, fl) in arms.items():
                st = _stats(times[k])
                _emit({"arm": "kernels", "entry": k, "N": N, "d": d, "M": M, "T": T, "tag": tag, **st, "f64_flops_issued": fl,
                       "entry_tflops_f64": fl / (st["ms_median"] * 1e-3) / 1e12}, out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="kernels,step")
    ap.add_argument("--sizes", default="7372:8,14939:18,50000:20")
    ap.add_argument("--points", default="400,800")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sgpr_bench needs the GPU: nothing is timed without one")
    sizes = [tuple(int(v) for v in s.split(":")) for s in a.sizes.split(",")]
    points = [int(v) for v in a.points.split(",")]
    if "kernels" in a.arms.split(","):
        kernel_arms(a.out, sizes, points, a.reps, a.warmup, a.tag)
    if "step" in a.arms.split(","):
        step_arms(a.out, sizes, points, a.reps, a.warmup, a.tag)
