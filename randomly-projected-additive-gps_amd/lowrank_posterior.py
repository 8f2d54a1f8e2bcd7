"""Closed-form posterior of the exact additive-RP GP through the explicit features of its Chebyshev low-rank form
(settings.lowrank_posterior).

Every 1-D term is exp2(-h^2 (x - y)^2) ~= T(x)^T C T(y) on x = (z - mid) kappa / h in [-1, 1] (csrc/rpgp_lowrank.hip), and C
(p x p, positive semi-definite) ~= G G^T with G = Q_r Lambda_r^1/2 (rpgp_lowrank_post_select).  The truncated kernel is then
an explicit feature model
    K_lr = B B^T,   B = sqrt(scale) [T(x_1) G | ... | T(x_J) G]   (N x F,  F = J r;  rpgp_lowrank_features_f64)
(p <= settings.lowrank_max_rank: 64 by default, up to 128)
whose posterior needs no N x N object.  With M = sigma^2 I + B^T B = L L^T (F x F) and w = M^-1 B^T (y - c):
    mean* = B* w + c,   Sigma* = sigma^2 B* M^-1 B*^T = sigma^2 V^T V  (V = L^-1 B*^T),   alpha = (r - B w) / sigma^2,
    Khat^-1 X = (X - B M^-1 B^T X) / sigma^2,
and the noisy log-density at any inputs (B* = B at the training inputs) by Woodbury and the determinant lemma in F x F:
    Sigma* + sigma^2 I = sigma^2 (I + B* M^-1 B*^T),   (...)^-1 = (I - B* P^-1 B*^T) / sigma^2,   P = M + B*^T B*,
    log|Sigma* + sigma^2 I| = m log sigma^2 + log|P| - log|M|.
Everything runs in float64; the accuracy is set by the per-entry tail of the truncation alone (no CG tolerance)."""
import math

import torch

from . import backend as _backend
from . import ops
from .hostvals import host_float
from .likelihoods import LOG2PI, MultivariateNormal
from .models import TrainPosterior

KAPPA = 0.84932180028801907      # (2 ln 2)^-1/2: exp(-(z - z')^2 / 2) = exp2(-(kappa (z - z'))^2)
TAIL_TOL = 1e-10                 # largest per-entry tail of one 1-D term (selection + dropped eigenpairs)
TAIL_FLOOR = 1e-12               # smallest: the selection's own rounding allowance is 1e-13
REL_ACCURACY = 1e-6              # a tail eps per entry moves Khat by <= N s eps in the 2-norm (s: outputscale), the posterior
                                 # by <= N s eps / sigma^2 relative: eps = 1e-6 sigma^2 / (N s) keeps that bound below 1e-6


def tail_tolerance(N, outputscale, noise):
    """Per-entry tail tolerance of the posterior's features for N rows, outputscale s and noise sigma^2."""
    if not (outputscale > 0.0) or not (noise > 0.0):
        return TAIL_TOL
    return min(TAIL_TOL, max(TAIL_FLOOR, REL_ACCURACY * noise / (N * outputscale)))
MAX_J = 64
MAX_FEATURES = 4096
MEMORY_SHARE = 0.25              # B (8 N F bytes) may take this share of the device memory
_PANEL = 4096                    # columns per triangular solve


def rank_cap():
    """(cap, kw): settings.lowrank_max_rank and the keyword that carries it to the backend's feature kernels.  At the default
    the keyword is left out, so a backend written against the rank-64 interface keeps serving it."""
    from . import settings
    cap = settings.lowrank_max_rank.value()
    return cap, ({} if cap == 64 else {"max_rank": cap})


class _Form:
    """The features of one interval: mid (J), inv_w, ranks, tail and G, and B with its F x F factor."""

    def __init__(self, mid, h, p, r, tail, G):
        self.mid, self.h, self.p, self.r, self.tail, self.G = mid, h, p, r, tail, G
        self.inv_w = KAPPA / h if h > 0.0 else 0.0
        self.kw = rank_cap()[1]                     # the cap this form was selected under goes with it to the kernels


class LowrankPosterior:
    """The closed-form feature posterior of one prediction strategy.  Construct with `LowrankPosterior.build(strategy)`,
    which returns (posterior or None, reason)."""

    def __init__(self, strategy, op64, form, B, M, L, w):
        self.strategy = strategy
        self.model = strategy.model
        self.scale = float(op64._scale)
        self.noise = host_float(strategy.noise)
        self.c = host_float(strategy.mean_const.reshape(-1)[0]) if strategy.mean_const.numel() else 0.0
        self.zmin = op64.Z1.min(0).values
        self.zmax = op64.Z1.max(0).values
        self.Z = op64.Z1
        self.rebuilds = 0
        self._set(form, B, M, L, w)

    # ---- construction -------------------------------------------------------------------------------------------------
    @staticmethod
    def _interval(zmin, zmax):
        mid = 0.5 * (zmin + zmax)
        h = KAPPA * float((0.5 * (zmax - zmin)).max()) * (1.0 + 2.0 ** -20)
        return mid, h

    @staticmethod
    def _form(be, Z, zmin, zmax, scale, noise):
        """(form, None) for the interval of [zmin, zmax], or (None, reason)."""
        N, J = Z.shape
        mid, h = LowrankPosterior._interval(zmin, zmax)
        cap = rank_cap()[0]
        p, r, tail, G = be.lowrank_post_select(h, tail_tolerance(N, scale * J, noise), cap)
        if p == 0:
            return None, "half-width %.3g needs a Chebyshev rank above %d" % (h, cap)
        F = J * r
        if F > MAX_FEATURES:
            return None, "%d features exceed %d" % (F, MAX_FEATURES)
        if Z.is_cuda and 8.0 * N * F > MEMORY_SHARE * torch.cuda.get_device_properties(Z.device).total_memory:
            return None, "the %d x %d features exceed %.0f%% of the device memory" % (N, F, 100 * MEMORY_SHARE)
        return _Form(mid, h, p, r, tail, G), None

    @staticmethod
    def _factor(be, Z, form, scale, noise, r64):
        """(B, M, L, w) of one form, or None when M = sigma^2 I + B^T B does not factor."""
        B = be.lowrank_features(Z, form.mid, form.inv_w, form.G, scale, **form.kw)
        M = B.t() @ B
        M.diagonal().add_(noise)
        L, info = torch.linalg.cholesky_ex(M)
        if int(info) != 0:
            return None
        w = torch.cholesky_solve(B.t() @ r64, L)
        return B, M, L, w

    @classmethod
    def build(cls, strategy):
        model = strategy.model
        x = model.train_inputs
        cm = model.covar_module
        if getattr(cm, "shard", None) is not None and getattr(cm.shard, "world_size", 1) > 1:
            return None, "sharded model"
        if getattr(strategy.op, "row_shard", None) is not None:
            return None, "sharded model"
        if not ops.lowrank_enabled():
            return None, "the low-rank form is switched off (RPGP_LOWRANK=0 or RPGP_FACT_ASM)"
        be = _backend.get_backend()
        if getattr(be, "lowrank_post_select", None) is None or getattr(be, "lowrank_features", None) is None:
            return None, "the backend has no low-rank features"
        f64 = getattr(cm, "float64_operator", None)
        op64 = f64(x) if f64 is not None else None
        if op64 is None:
            return None, "the kernel has no float64 form (grid interpolation, family kernel, k > 1 or memory-efficient)"
        Z = op64.Z1
        if Z.shape[1] > MAX_J:
            return None, "J = %d exceeds %d" % (Z.shape[1], MAX_J)
        noise = host_float(strategy.noise)
        form, why = cls._form(be, Z, Z.min(0).values, Z.max(0).values, float(op64._scale), noise)
        if form is None:
            return None, why
        r64 = cls._residual(strategy)
        fac = cls._factor(be, Z, form, float(op64._scale), noise, r64)
        if fac is None:
            return None, "sigma^2 I + B^T B is not positive definite"
        return cls(strategy, op64, form, *fac), None

    @staticmethod
    def _residual(strategy):
        model = strategy.model
        return (model.train_targets.double().reshape(-1, 1) - strategy.mean_const.double().reshape(-1, 1))

    def _set(self, form, B, M, L, w):
        self.form, self.B, self.M, self.L, self.w = form, B, M, L, w
        self.logdet_M = 2.0 * float(torch.log(L.diagonal()).sum())
        r64 = self._residual(self.strategy)
        a64 = (r64 - B @ w) / self.noise
        s = self.strategy
        s.alpha64 = a64
        s.alpha = a64.to(s.r.dtype)

    @property
    def ranks(self):
        """(p, r, F) of the current form."""
        return self.form.p, self.form.r, self.B.shape[1]

    # ---- features at other inputs --------------------------------------------------------------------------------------
    def _test_coordinates(self, xs):
        return self.model.covar_module.float64_operator(xs).Z1

    def _features(self, Zs):
        """B* for projected test coordinates, or None (with strategy.lowrank_fallback_reason set) when the interval that
        covers them is not served.  A coordinate outside the interval rebuilds the form once on the union of the ranges."""
        f = self.form
        be = _backend.get_backend()
        if f.inv_w > 0.0:
            outside = bool((((Zs - f.mid) * f.inv_w).abs() > 1.0).any())
        else:
            outside = bool(((Zs.min(0).values < self.zmin) | (Zs.max(0).values > self.zmax)).any())
        if outside:
            zmin = torch.minimum(self.zmin, Zs.min(0).values)
            zmax = torch.maximum(self.zmax, Zs.max(0).values)
            form, why = self._form(be, self.Z, zmin, zmax, self.scale, self.noise)
            fac = None
            if form is not None:
                fac = self._factor(be, self.Z, form, self.scale, self.noise, self._residual(self.strategy))
                if fac is None:
                    why = "sigma^2 I + B^T B is not positive definite"
            if fac is None:
                self.strategy.lowrank_fallback_reason = why
                return None
            self.zmin, self.zmax = zmin, zmax
            self._set(form, *fac)
            self.rebuilds += 1
        return be.lowrank_features(Zs, self.form.mid, self.form.inv_w, self.form.G, self.scale, **self.form.kw)

    # ---- prediction ----------------------------------------------------------------------------------------------------
    def predict(self, xs, at_train=False):
        """The posterior at xs (a LowrankPredictive, or mean-only under skip_posterior_variances), or None when this call
        must take the exact path (the reason is in strategy.lowrank_fallback_reason)."""
        from . import settings
        with torch.no_grad():
            Bs = self.B if at_train else self._features(self._test_coordinates(xs))
            if Bs is None:
                return None
            mean64 = (Bs @ self.w).reshape(-1) + self.c
            mean = mean64.to(xs.dtype)
            if settings.skip_posterior_variances.on():
                return MultivariateNormal(mean, torch.zeros_like(mean), diagonal_only=True)
            V = self._lower_solve(Bs.t())                                           # F x m
            var64 = self.noise * (V * V).sum(0)
            return LowrankPredictive(mean, mean64, var64, self, Bs, V, xs)

    def _lower_solve(self, R):
        """L^-1 R in column panels (the library's triangular solve runs out of workspace on very wide right-hand sides)."""
        out = torch.empty((R.shape[0], R.shape[1]), dtype=R.dtype, device=R.device)
        for c0 in range(0, R.shape[1], _PANEL):
            out[:, c0:c0 + _PANEL] = torch.linalg.solve_triangular(self.L, R[:, c0:c0 + _PANEL], upper=False)
        return out

    def _lower_solve_t(self, R):
        """L^-T R in column panels."""
        out = torch.empty_like(R)
        for c0 in range(0, R.shape[1], _PANEL):
            out[:, c0:c0 + _PANEL] = torch.linalg.solve_triangular(self.L.t(), R[:, c0:c0 + _PANEL], upper=True)
        return out

    def solve(self, X):
        """Khat^-1 X = (X - B M^-1 B^T X) / sigma^2 (float64, returned in X's dtype)."""
        X64 = X.double()
        Y = self._lower_solve(self.B.t() @ X64)
        out = (X64 - self.B @ self._lower_solve_t(Y)) / self.noise
        return out.to(X.dtype)

    def log_prob(self, Bs, mean64, value):
        """log N(value | mean, sigma^2 (I + B* M^-1 B*^T)) in F x F (Woodbury, determinant lemma)."""
        d = value.double().reshape(-1, 1) - mean64.reshape(-1, 1)
        m = d.shape[0]
        P = Bs.t() @ Bs + self.M
        Lp = torch.linalg.cholesky(P)
        u = torch.linalg.solve_triangular(Lp, Bs.t() @ d, upper=False)
        quad = (float((d * d).sum()) - float((u * u).sum())) / self.noise
        logdet = m * math.log(self.noise) + 2.0 * float(torch.log(Lp.diagonal()).sum()) - self.logdet_M
        return -0.5 * (quad + logdet + m * LOG2PI)

    def train_log_prob(self, target):
        """log N(target | mu_train, Sigma_train + sigma^2 I) at the training inputs (B* = B)."""
        mean64 = (self.B @ self.w).reshape(-1) + self.c
        return self.log_prob(self.B, mean64, target)


class LowrankPredictive(TrainPosterior):
    """Posterior of the feature model at m inputs: mean and variances eager, the m x m covariance sigma^2 V^T V formed only
    when it is read; the noisy version's log-density is closed-form in F x F when its noise is the strategy's."""

    def __init__(self, mean, mean64, var64, post, Bs, V, xs, noise=None):
        self.mean = mean
        self.diagonal_only = False
        self._mean64, self._var64, self._post, self._Bs, self._V = mean64, var64, post, Bs, V
        self._strategy, self._xs, self._noise, self._cov = post.strategy, xs, noise, None

    @property
    def variance(self):
        v = self._var64 if self._noise is None else self._var64 + float(self._noise)
        return v.to(self.mean.dtype)

    @property
    def covariance(self):
        if self._cov is None:
            cov = self._post.noise * (self._V.t() @ self._V)
            if self._noise is not None:
                cov.diagonal().add_(float(self._noise))
            self._cov = cov.to(self.mean.dtype)
        return self._cov

    @property
    def covariance_materialized(self):
        return self._cov is not None

    def with_observation_noise(self, noise):
        return LowrankPredictive(self.mean, self._mean64, self._var64, self._post, self._Bs, self._V, self._xs, noise=noise)

    def log_prob(self, value):
        post = self._post
        same_noise = self._noise is not None and abs(float(self._noise) - post.noise) <= 1e-12 * post.noise
        if not same_noise:
            return MultivariateNormal.log_prob(self, value)
        lp = post.log_prob(self._Bs, self._mean64, value)
        return torch.as_tensor(lp, dtype=value.dtype, device=value.device)
