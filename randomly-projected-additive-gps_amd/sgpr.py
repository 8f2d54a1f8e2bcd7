"""`kind: sgpr` — the inducing-point GP of training_routines.py:296-322 (`ScaleKernel(InducingPointKernel(base, X[:M], likelihood))`)
on Titsias' collapsed bound, with the N training rows entering only through two float64 sums.

With Z = (X - mu) / l, U = (U_raw - mu) / l, K_fu = phi(|z_i - u_j|^2), K_uu = phi(U, U) + jitter I, r = y - c,
    G = K_uf K_fu (M x M),   g_r = K_uf r (M),   A = K_uu + (s / sigma^2) G,
the objective is log N(y | c, s Q + sigma^2 I) - (s / (2 sigma^2)) tr(K_ff - Q), Q = K_fu K_uu^-1 K_uf:
    logdet   = N log sigma^2 - log|K_uu| + log|A|
    inv_quad = (r^T r - (s / sigma^2) g_r^T A^-1 g_r) / sigma^2
    trace    = s (N phi(0) - tr(K_uu^-1 G))
and the prediction at x* is c + (s / sigma^2) K_*u A^-1 g_r with covariance s (K_** - K_*u (K_uu^-1 - A^-1) K_u*).

Native path (settings.sgpr_native, the default): G and g = K_uf [y, 1] from ONE call of the backend's inducing_gram (float32
kernel entries, exact products, float64 sums — csrc/rpgp_inducing.hip), the M x M algebra in float64 torch, and in the backward
pass C = dL/dG and v = dL/dg from autograd handed to ONE call of inducing_grad.  K_uu is formed by torch in float64 from the same
float32 U the kernels read, and brings its own share of the gradients of U and l through autograd.  No N x M object is held.
Dense path: the same objective with K_fu materialised in float64 by torch, on any device and dtype (CPU, --double, M > 1024).

[GPT-mem] The GPyTorch of the reference's era leaves the outputscale out of the trace term (its InducingPointKernel adds the
term through the likelihood it holds, inside the ScaleKernel) and the sign of that term in that era is uncertain from memory;
neither is replicated: the bound here carries s in the trace term, with the sign of Titsias (2009)."""
import math

import torch

from . import backend as _backend
from . import settings
from .likelihoods import LOG2PI, MultivariateNormal

KINDS = ("RBF", "Matern", "InverseMQ")
ROW_CHUNK = 8192                  # rows of a dense float64 K_*u block


def phi(kind, d2):
    """phi_kind(d2) in torch (any floating dtype); phi(0) = 1 for every kind."""
    if kind == "RBF":
        return torch.exp(-0.5 * d2)
    if kind == "InverseMQ":
        return (d2 + 1.0).rsqrt()
    if kind == "Matern":
        r = (d2 + 1e-30).sqrt() * math.sqrt(3.0)
        return (1.0 + r) * torch.exp(-r)
    raise ValueError("Unknown kernel type")


def sqdist(A, B=None):
    """Squared distances of the rows of A and B (B None: A with itself, exact zero diagonal)."""
    na = (A * A).sum(-1, keepdim=True)
    if B is None:
        d2 = (na + na.t() - 2.0 * (A @ A.t())).clamp_min(0.0)
        return d2 * (1.0 - torch.eye(A.shape[0], dtype=A.dtype, device=A.device))
    return (na + (B * B).sum(-1).unsqueeze(0) - 2.0 * (A @ B.t())).clamp_min(0.0)


def inducing_gram_matrix(kind, U, jitter):
    """K_uu = phi(U, U) + jitter I in the dtype of U."""
    K = phi(kind, sqdist(U))
    return K + jitter * torch.eye(U.shape[0], dtype=U.dtype, device=U.device)


def collapsed_bound(G, g_r, rr, Kuu, s, noise, n, with_factors=False):
    """The collapsed bound (no priors, not divided by N) from the sums G (M x M), g_r (M), rr = r^T r and K_uu, all float64."""
    a = s / noise
    G = 0.5 * (G + G.t())
    A = Kuu + a * G
    Lu = torch.linalg.cholesky(Kuu)
    La = torch.linalg.cholesky(A)
    beta = torch.cholesky_solve(g_r.reshape(-1, 1), La).reshape(-1)
    logdet = n * torch.log(noise) - 2.0 * torch.log(Lu.diagonal()).sum() + 2.0 * torch.log(La.diagonal()).sum()
    inv_quad = (rr - a * (g_r * beta).sum()) / noise
    trace = s * (n - torch.cholesky_solve(G, Lu).diagonal().sum())
    value = -0.5 * (inv_quad + logdet + n * LOG2PI) - 0.5 * trace / noise
    if with_factors:
        return value, Lu, La, beta
    return value


class _InducingSums(torch.autograd.Function):
    """(G, g) of the backend for Z = Xc / l and U.  Backward: one inducing_grad call gives dU and, through q, the share of dl that
    comes through Z (the share through U = (U_raw - mu) / l is autograd's, outside)."""

    @staticmethod
    def forward(ctx, ls, U, Xc, Y, kind):
        be = _backend.get_backend()
        Z = (Xc / ls).contiguous()
        Ud = U.detach().contiguous()
        G, g = be.inducing_gram(kind, Z, Ud, Y)
        ctx.save_for_backward(ls, Ud, Z, Y)
        ctx.kind = kind
        return G, g

    @staticmethod
    def backward(ctx, C, v):
        ls, U, Z, Y = ctx.saved_tensors
        be = _backend.get_backend()
        C = torch.zeros(U.shape[0], U.shape[0], dtype=torch.float64, device=U.device) if C is None else C
        v = torch.zeros(U.shape[0], Y.shape[1], dtype=torch.float64, device=U.device) if v is None else v
        gU, q = be.inducing_grad(ctx.kind, Z, U, Y, (0.5 * (C + C.t())).contiguous(), v.contiguous())
        g_ls = g_U = None
        if ctx.needs_input_grad[0]:
            # d / dl_m through Z alone = -(1 / l_m) sum_i gZ_im z_im = (-2 q_m + sum_j gU_jm u_jm) / l_m
            per = (-2.0 * q + (gU * U.double()).sum(0)) / ls.double().reshape(-1)
            g_ls = (per.sum().reshape(ls.shape) if ls.numel() == 1 else per.reshape(ls.shape)).to(ls.dtype)
        if ctx.needs_input_grad[1]:
            g_U = gU.to(U.dtype)
        return g_ls, g_U, None, None, None


class InducingPointOperator:
    """What `InducingPointKernel.forward` returns on the training inputs: the pieces of the objective, not a matrix.  The
    marginal log-likelihood and the prediction strategy recognise it."""

    def __init__(self, kernel, x, outputscale, reason):
        self.kernel, self.x, self.outputscale, self.reason = kernel, x, outputscale, reason
        self.shape = (x.shape[0], x.shape[0])

    @property
    def native(self):
        return self.reason is None

    def _scalars(self, noise):
        s = self.outputscale if self.outputscale is not None else torch.ones((), dtype=self.x.dtype, device=self.x.device)
        return s.reshape(()).double(), noise.reshape(()).double()

    def sums(self, target, mean):
        """(G, g_r, rr, K_uu, U64) in float64, autograd-tracked."""
        k = self.kernel
        n = self.x.shape[0]
        jitter = float(settings.sgpr_jitter.value())
        ls, Xc, U = k.coordinates(self.x)
        if self.native and not (mean.dim() == 1 and (n == 1 or mean.stride(0) == 0)):
            self.reason = k.sgpr_reason = "the mean is not one constant: r = y - mean has to be formed row by row"
        if self.native:
            # a constant mean c: r = y - c only through g = K_uf [y, 1] and two sums of the targets
            c = mean[0].double()
            y = target.detach()
            Y = torch.stack([y, torch.ones_like(y)], dim=1).contiguous()
            G, g = _InducingSums.apply(ls, U, Xc, Y, k.kernel_type)
            y64 = y.double()
            g_r = g[:, 0] - c * g[:, 1]
            rr = (y64 * y64).sum() - 2.0 * c * y64.sum() + n * c * c
            U64 = U.double()
        else:
            ls64 = ls.double()
            U64 = (k.inducing_points.double() - k.center(self.x).double()) / ls64
            r = (target - mean).double()
            G = torch.zeros(U64.shape[0], U64.shape[0], dtype=torch.float64, device=self.x.device)
            g_r = torch.zeros(U64.shape[0], dtype=torch.float64, device=self.x.device)
            step = n if torch.is_grad_enabled() else ROW_CHUNK          # (under autograd the N x M block is kept anyway)
            for r0 in range(0, n, step):
                Kfu = phi(k.kernel_type, sqdist(Xc[r0:r0 + step].double() / ls64, U64))
                G = G + Kfu.t() @ Kfu
                g_r = g_r + Kfu.t() @ r[r0:r0 + Kfu.shape[0]]
            rr = (r * r).sum()
        return G, g_r, rr, inducing_gram_matrix(k.kernel_type, U64, jitter), U64

    def log_prob(self, noise, target, mean):
        """The collapsed bound (no priors, not divided by N) as a scalar of the targets' dtype."""
        s, n2 = self._scalars(noise)
        G, g_r, rr, Kuu, _ = self.sums(target, mean)
        return collapsed_bound(G, g_r, rr, Kuu, s, n2, self.x.shape[0]).to(target.dtype)


class InducingPosterior:
    """Closed-form prediction from the factors of the bound: mean c + (s / sigma^2) K_*u A^-1 g_r, covariance
    s (K_** - K_*u (K_uu^-1 - A^-1) K_u*), the latter formed only when read."""

    def __init__(self, strategy):
        model = strategy.model
        self.op, self.model = strategy.op, model
        with torch.no_grad():
            s, noise = self.op._scalars(strategy.noise)
            mean = model.mean_module(model.train_inputs)
            G, g_r, rr, Kuu, U64 = self.op.sums(model.train_targets, mean)
            _, Lu, La, beta = collapsed_bound(G, g_r, rr, Kuu, s, noise, self.op.x.shape[0], with_factors=True)
            self.s, self.noise, self.U = s, noise, U64
            self.w = (s / noise) * beta                                        # mean weights
            eye = torch.eye(Kuu.shape[0], dtype=torch.float64, device=Kuu.device)
            D = torch.cholesky_solve(eye, Lu) - torch.cholesky_solve(eye, La)  # K_uu^-1 - A^-1 (positive semi-definite)
            self.D = 0.5 * (D + D.t())

    def _cross(self, xs):
        k = self.op.kernel
        ls = k.base_kernel.lengthscale.detach().double()
        return phi(k.kernel_type, sqdist((xs.double() - k.center(xs).double()) / ls, self.U))

    def mean_and_variance(self, xs, want_variance=True):
        means, variances = [], []
        for r0 in range(0, xs.shape[0], ROW_CHUNK):
            Ks = self._cross(xs[r0:r0 + ROW_CHUNK])
            means.append(Ks @ self.w)
            if want_variance:
                variances.append(self.s * (1.0 - ((Ks @ self.D) * Ks).sum(1)))
        return torch.cat(means), (torch.cat(variances) if want_variance else None)

    def covariance(self, xs):
        k = self.op.kernel
        ls = k.base_kernel.lengthscale.detach().double()
        Zs = (xs.double() - k.center(xs).double()) / ls
        Ks = self._cross(xs)
        cov = self.s * (phi(k.kernel_type, sqdist(Zs)) - Ks @ self.D @ Ks.t())
        return 0.5 * (cov + cov.t())

    def predict(self, xs):
        with torch.no_grad():
            skip = settings.skip_posterior_variances.on()
            m, var = self.mean_and_variance(xs, want_variance=not skip)
            mean = (m + self.model.mean_module(xs).double()).to(xs.dtype)
            if skip:
                return MultivariateNormal(mean, torch.zeros_like(mean), diagonal_only=True)
            return InducingPredictive(mean, var.to(xs.dtype), self, xs)


class InducingPredictive(MultivariateNormal):
    """Posterior of the inducing-point GP at xs: mean and marginal variances are held, the N* x N* covariance is formed when
    somebody reads it (a dense log-density does)."""

    def __init__(self, mean, var, post, xs, noise=None):
        self.mean, self.diagonal_only = mean, False
        self._var, self._post, self._xs, self._noise, self._cov = var, post, xs, noise, None

    @property
    def variance(self):
        return self._var if self._noise is None else self._var + self._noise

    @property
    def covariance(self):
        if self._cov is None:
            with torch.no_grad():
                cov = self._post.covariance(self._xs).to(self.mean.dtype)
            if self._noise is not None:
                cov.diagonal().add_(self._noise)
            self._cov = cov
        return self._cov

    def with_observation_noise(self, noise):
        return InducingPredictive(self.mean, self._var, self._post, self._xs, noise=noise)
