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
Everything runs in float64; the accuracy is set by the per-entry tail of the truncation alone (no CG tolerance).

A kernel with one lengthscale and one weight per projection (GeneralizedProjectionKernel with RBF sub-kernels and k = 1:
K = s sum_c w_c exp(-(z_c - z'_c)^2 / 2)) is the same feature model on column forms (column_forms): its columns are put into
up to MAX_FORMS classes by half-width, each class with the form of its widest column; B is class-major, the columns of component
c carry the factor sqrt(s w_c) (rpgp_lowrank_features_cols_f64), and F = sum_g nc_g r_g."""
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
MAX_FORMS = 4                    # classes of columns with a Chebyshev form each (column_forms)
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


class _ColumnForm:
    """One class of columns and its form: the columns (ascending), their midpoints, the class half-width with inv_w, ranks,
    tail and G, and the first of its nc r feature columns in B."""

    def __init__(self, cols, mid, h, p, r, tail, G, f0):
        self.cols, self.mid, self.h, self.p, self.r, self.tail, self.G, self.f0 = cols, mid, h, p, r, tail, G, f0
        self.inv_w = KAPPA / h if h > 0.0 else 0.0
        self.f1 = f0 + len(cols) * r


class ColumnForms:
    """The forms of a kernel with one lengthscale and one weight per projection, K = s sum_c w_c exp(-(z_c - z'_c)^2 / 2):
    up to MAX_FORMS classes of columns by half-width (column_forms), B class-major with class g in columns [f0_g, f1_g)."""

    def __init__(self, classes, cls, comp, weights, scale, tail):
        self.classes = classes              # the non-empty classes, widest first
        self.cls = cls                      # class index (into `classes`) of every column
        self.comp = comp                    # component of every feature column (F, host int64)
        self.weights, self.scale = weights, scale          # w_c (host float64) and s
        self.col_scale = (scale * weights).sqrt()          # sqrt(s w_c)
        self.tail = tail                    # sum_g (sum_{c in g} w_c) tail_g / sum_c w_c
        self.kw = rank_cap()[1]
        self.F = classes[-1].f1
        self.p = max(c.p for c in classes)
        self.r = max(c.r for c in classes)

    @property
    def class_ranks(self):
        """(p, r, columns) of every class."""
        return [(c.p, c.r, len(c.cols)) for c in self.classes]

    def features(self, be, Z):
        """B (rows of Z x F, float64): one launch per class, each into its own columns."""
        B = torch.empty((Z.shape[0], self.F), dtype=torch.float64, device=Z.device)
        for c in self.classes:
            be.lowrank_features_cols(Z, c.cols, c.mid, c.inv_w, c.G, self.col_scale[c.cols], out=B[:, c.f0:c.f1], **self.kw)
        return B


def column_classes(hj):
    """Class of every column from its half-width h_j (a sequence of host floats): min(MAX_FORMS - 1, floor(log2(h_max / h_j)));
    a column with h_j = 0 joins the last non-empty class; h_max = 0 is one class."""
    hmax = max(hj)
    if not hmax > 0.0:
        return [0] * len(hj)
    cls = [min(MAX_FORMS - 1, int(math.floor(math.log2(hmax / h)))) if h > 0.0 else -1 for h in hj]
    last = max(cls)
    return [last if c < 0 else c for c in cls]


def column_forms(be, Z, zmin, zmax, weights, scale, noise):
    """(ColumnForms, None) for N x J coordinates Z with the column ranges [zmin, zmax], component weights w (J) and outputscale
    s, or (None, reason).  Every class takes the form of its widest column, selected at the tolerance of the whole kernel
    (tail_tolerance(N, s sum_c w_c, sigma^2)): a column that needs few Chebyshev terms no longer pays for the widest one."""
    N, J = Z.shape
    w = torch.as_tensor(weights, dtype=torch.float64).detach().reshape(-1).cpu()
    half = (0.5 * (zmax - zmin)).double().cpu()
    mid_all = (0.5 * (zmin + zmax)).double()
    hj = (KAPPA * half).tolist()
    cls = column_classes(hj)
    cap = rank_cap()[0]
    tol = tail_tolerance(N, scale * float(w.sum()), noise)
    classes, index, f0 = [], {}, 0
    comp = []
    for g in sorted(set(cls)):
        cols = [j for j in range(J) if cls[j] == g]
        h = max(hj[j] for j in cols) * (1.0 + 2.0 ** -20)
        p, r, tail, G = be.lowrank_post_select(h, tol, cap)
        if p == 0:
            return None, "half-width %.3g needs a Chebyshev rank above %d" % (h, cap)
        index[g] = len(classes)
        classes.append(_ColumnForm(cols, mid_all[cols].contiguous(), h, p, r, tail, G, f0))
        f0 = classes[-1].f1
        for j in cols:
            comp.extend([j] * r)
    tail = sum(float(w[c.cols].sum()) * c.tail for c in classes) / float(w.sum())
    forms = ColumnForms(classes, [index[g] for g in cls], torch.tensor(comp, dtype=torch.int64), w, scale, tail)
    return forms, None


def size_reason(N, F, device, copies, what):
    """Why N x F features are not served (None when they are): MAX_FEATURES and `copies` N x F float64 matrices within
    MEMORY_SHARE of the device memory."""
    if F > MAX_FEATURES:
        return "%d features exceed %d" % (F, MAX_FEATURES)
    if device.type == "cuda" and 8.0 * copies * N * F > MEMORY_SHARE * torch.cuda.get_device_properties(device).total_memory:
        return "the %d x %d %s exceed %.0f%% of the device memory" % (N, F, what, 100 * MEMORY_SHARE)
    return None


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
        self.weights = self._weights(op64)
        self.rebuilds = 0
        self._set(form, B, M, L, w)

    # ---- construction -------------------------------------------------------------------------------------------------
    @staticmethod
    def _interval(zmin, zmax):
        mid = 0.5 * (zmin + zmax)
        h = KAPPA * float((0.5 * (zmax - zmin)).max()) * (1.0 + 2.0 ** -20)
        return mid, h

    @staticmethod
    def _form(be, Z, zmin, zmax, scale, noise, weights=None):
        """(form, None) for the interval of [zmin, zmax], or (None, reason).  `weights` (one per column: the kernel has a
        weight and a lengthscale per projection) selects the column forms."""
        N, J = Z.shape
        if weights is not None:
            form, why = column_forms(be, Z, zmin, zmax, weights, scale, noise)
            if form is None:
                return None, why
            why = size_reason(N, form.F, Z.device, 1, "features")
            return (None, why) if why else (form, None)
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
    def _evaluate(be, Z, form, scale):
        """B of `form` at the coordinates Z."""
        if isinstance(form, ColumnForms):
            return form.features(be, Z)
        return be.lowrank_features(Z, form.mid, form.inv_w, form.G, scale, **form.kw)

    @staticmethod
    def _factor(be, Z, form, scale, noise, r64):
        """(B, M, L, w) of one form, or None when M = sigma^2 I + B^T B does not factor."""
        B = LowrankPosterior._evaluate(be, Z, form, scale)
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
        if getattr(be, "lowrank_post_select", None) is None:
            return None, "the backend has no low-rank features"
        op64 = cls._float64_operator(cm, x)
        if op64 is None:
            return None, "the kernel has no float64 form (grid interpolation, non-RBF kind, k > 1 or memory-efficient)"
        Z = op64.Z1
        if Z.shape[1] > MAX_J:
            return None, "J = %d exceeds %d" % (Z.shape[1], MAX_J)
        weights = cls._weights(op64)
        if getattr(be, "lowrank_features" if weights is None else "lowrank_features_cols", None) is None:
            return None, "the backend has no low-rank features"
        if weights is not None and not bool((weights > 0.0).all()):
            return None, "a component weight is not positive"
        noise = host_float(strategy.noise)
        form, why = cls._form(be, Z, Z.min(0).values, Z.max(0).values, float(op64._scale), noise, weights)
        if form is None:
            return None, why
        r64 = cls._residual(strategy)
        fac = cls._factor(be, Z, form, float(op64._scale), noise, r64)
        if fac is None:
            return None, "sigma^2 I + B^T B is not positive definite"
        return cls(strategy, op64, form, *fac), None

    @staticmethod
    def _float64_operator(cm, x):
        """The float64 twin of the model's kernel on x, the kinds with per-component weights included."""
        f64 = getattr(cm, "float64_operator", None)
        if f64 is None:
            return None
        return f64(x, weighted=True)

    @staticmethod
    def _weights(op64):
        """The component weights of the float64 operator on the host (None: the unweighted operator, one shared form)."""
        w = getattr(op64, "comp_weights", None)
        return None if w is None else w.detach().double().reshape(-1).cpu()

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
        """(p, r, F) of the current form; with column forms the largest p and r (`class_ranks` has every class)."""
        return self.form.p, self.form.r, self.B.shape[1]

    @property
    def class_ranks(self):
        """[(p, r, columns)] per class of columns (one entry for the shared form)."""
        if isinstance(self.form, ColumnForms):
            return self.form.class_ranks
        return [(self.form.p, self.form.r, self.Z.shape[1])]

    # ---- features at other inputs --------------------------------------------------------------------------------------
    def _test_coordinates(self, xs):
        return self._float64_operator(self.model.covar_module, xs).Z1

    def _features(self, Zs):
        """B* for projected test coordinates, or None (with strategy.lowrank_fallback_reason set) when the interval that
        covers them is not served.  A coordinate outside the interval rebuilds the form once on the union of the ranges."""
        f = self.form
        be = _backend.get_backend()
        if isinstance(f, ColumnForms):
            bad = [(((Zs[:, c.cols] - c.mid) * c.inv_w).abs() > 1.0).any() if c.inv_w > 0.0 else
                   ((Zs[:, c.cols].min(0).values < self.zmin[c.cols]) | (Zs[:, c.cols].max(0).values > self.zmax[c.cols])).any()
                   for c in f.classes]
            outside = bool(torch.stack(bad).any())
        elif f.inv_w > 0.0:
            outside = bool((((Zs - f.mid) * f.inv_w).abs() > 1.0).any())
        else:
            outside = bool(((Zs.min(0).values < self.zmin) | (Zs.max(0).values > self.zmax)).any())
        if outside:
            zmin = torch.minimum(self.zmin, Zs.min(0).values)
            zmax = torch.maximum(self.zmax, Zs.max(0).values)
            form, why = self._form(be, self.Z, zmin, zmax, self.scale, self.noise, self.weights)
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
        return self._evaluate(be, Zs, self.form, self.scale)

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
