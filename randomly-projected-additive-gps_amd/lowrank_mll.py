"""The exact marginal likelihood of the truncated Chebyshev low-rank kernel in closed form (settings.lowrank_mll): the third
mode of inv_quad_logdet.InvQuadLogDet ("features").

The features of lowrank_posterior.py make the truncated kernel an explicit feature model K_lr = B B^T (B: N x F, F = J r;
rpgp_lowrank_features_f64; p <= settings.lowrank_max_rank).  With r = y - c, M = sigma^2 I + B^T B = L L^T, w = M^-1 B^T r and alpha = (r - B w) / sigma^2
(= Khat^-1 r), everything is F x F algebra in float64:
    inv_quad = r^T alpha,                    logdet = (N - F) log sigma^2 + log|M|,
    tr(Khat^-1) = (N - F) / sigma^2 + tr(M^-1),          tr(Khat^-1 K_lr) = F - sigma^2 tr(M^-1),
and for the objective g_iq inv_quad + g_ld logdet
    dB = W = -2 g_iq alpha (B^T alpha)^T + 2 g_ld Y,   Y = B M^-1   (Khat^-1 B = B M^-1),
    dZ = the adjoint of the features applied to W (rpgp_lowrank_features_grad_f64; W is never stored),
    dsigma^2 = -g_iq alpha^T alpha + g_ld tr(Khat^-1),
    doutputscale = (1 / outputscale) (-g_iq |B^T alpha|^2 + g_ld (F - sigma^2 tr(M^-1))),
    drhs = 2 g_iq alpha.
The interval (mid, h) of the features is fixed within one evaluation: the kernel depends on it only through the tail.  Value
and gradient are deterministic and belong to the same function, exact for the truncated kernel; the distance to the exact
kernel is set by the per-entry tail eps of lowrank_posterior.tail_tolerance alone.  dZ is the exact derivative of the
truncated kernel; Markov's inequality (|P'| <= n^2 max |P| on [-1, 1] for a polynomial of degree n) puts it roughly
(p - 1)^2 eps inv_w per kernel entry (times the scale) from the exact kernel's: an estimate, since the dropped Chebyshev terms
are of higher degree, held to by the rapid decay of their coefficients."""
import math

import torch

from . import backend as _backend
from . import ops, settings
from .lowrank_posterior import MAX_FEATURES, MAX_J, MEMORY_SHARE, LowrankPosterior, rank_cap, tail_tolerance


class FeatureForm:
    """What serves one operator: its float64 coordinates, the features' interval, ranks and G, B and the factor L of
    M = sigma^2 I + B^T B."""

    def __init__(self, form, Z, B, L, noise, scale, weight):
        self.Z = Z                                              # the operator's coordinates in float64 (N x J)
        self.mid, self.inv_w, self.h, self.p, self.r, self.tail, self.G = \
            form.mid, form.inv_w, form.h, form.p, form.r, form.tail, form.G
        self.B, self.L, self.noise, self.scale, self.weight = B, L, noise, scale, weight
        self.kw = form.kw

    @property
    def ranks(self):
        """(p, r, F)."""
        return self.p, self.r, self.B.shape[1]


def decide(op, noise):
    """(FeatureForm, None) when the features mode serves the operator `op` at noise sigma^2 (a host float), else
    (None, reason).  Cheap conditions first: B is only formed once every size condition holds."""
    from .operators import AdditiveRPOperator
    if not settings.lowrank_mll.on():
        return None, "settings.lowrank_mll is off"
    if type(op) is not AdditiveRPOperator or not op.symmetric:
        return None, "not a plain symmetric additive-RP RBF operator (grid, family, k > 1 or rectangular)"
    if getattr(op, "memory_efficient", False) or settings.memory_efficient.on():
        return None, "memory-efficient kernel"
    if (op.shard is not None and getattr(op.shard, "world_size", 1) > 1) or getattr(op, "row_shard", None) is not None:
        return None, "sharded operator"
    N, J = op.Z1.shape
    if J > MAX_J:
        return None, "J = %d exceeds %d" % (J, MAX_J)
    if not ops.lowrank_enabled():
        return None, "the low-rank form is switched off (RPGP_LOWRANK=0 or RPGP_FACT_ASM)"
    be = _backend.get_backend()
    if any(getattr(be, name, None) is None for name in ("lowrank_post_select", "lowrank_features", "lowrank_features_grad")):
        return None, "the backend has no low-rank features"
    if noise is None or not (noise > 0.0):
        return None, "no positive noise value"
    scale = float(op._scale)
    Z = op.Z1.detach().double().contiguous()
    mid, h = LowrankPosterior._interval(Z.min(0).values, Z.max(0).values)
    cap = rank_cap()[0]
    p, r, tail, G = be.lowrank_post_select(h, tail_tolerance(N, scale * J, noise), cap)
    if p == 0:
        return None, "half-width %.3g needs a Chebyshev rank above %d" % (h, cap)
    F = J * r
    if F >= N:
        return None, "%d features for %d rows (F >= N)" % (F, N)
    if F > MAX_FEATURES:
        return None, "%d features exceed %d" % (F, MAX_FEATURES)
    if Z.is_cuda and 16.0 * N * F > MEMORY_SHARE * torch.cuda.get_device_properties(Z.device).total_memory:
        return None, "the %d x %d features and B M^-1 exceed %.0f%% of the device memory" % (N, F, 100 * MEMORY_SHARE)
    from .lowrank_posterior import _Form
    form = _Form(mid, h, p, r, tail, G)
    B = be.lowrank_features(Z, form.mid, form.inv_w, form.G, scale, **form.kw)
    M = B.t() @ B
    M.diagonal().add_(noise)
    L, info = torch.linalg.cholesky_ex(M)
    if int(info) != 0:
        return None, "sigma^2 I + B^T B is not positive definite"
    return FeatureForm(form, Z, B, L, noise, scale, op.weight), None


def forward(ctx, Z, r, op, fm):
    """InvQuadLogDet.forward in the features mode: (inv_quad, logdet) in Z's dtype."""
    N = Z.shape[0]
    B, L, noise = fm.B, fm.L, fm.noise
    F = B.shape[1]
    r64 = r.detach().double().reshape(N, 1)
    w = torch.cholesky_solve(B.t() @ r64, L)
    alpha = (r64 - B @ w) / noise
    inv_quad = (r64 * alpha).sum()
    if settings.skip_logdet_forward.on():
        logdet = torch.zeros((), dtype=torch.float64, device=B.device)
    else:
        logdet = (N - F) * math.log(noise) + 2.0 * torch.log(L.diagonal()).sum()
    ctx.mode = "features"
    ctx.fm = fm
    ctx.alpha64 = alpha
    ctx.rdtype = r.dtype
    return inv_quad.to(Z.dtype), logdet.to(Z.dtype)


def backward(ctx, g_inv_quad, g_logdet):
    """(gZ, gs, gn, gr) of the features mode (InvQuadLogDet.backward's convention; gs is d / d outputscale)."""
    op, fm, alpha, need = ctx.op, ctx.fm, ctx.alpha64, ctx.needs_input_grad
    B, L, noise = fm.B, fm.L, fm.noise
    N, F = B.shape
    g_iq, g_ld = float(g_inv_quad), float(g_logdet)
    Minv = torch.cholesky_inverse(L)
    tr_minv = Minv.diagonal().sum()
    v = B.t() @ alpha                                                            # F x 1
    dtype = op.Z1.dtype
    gZ = gs = gn = gr = None
    if need[0]:
        Y = B @ Minv                                                             # Khat^-1 B = B M^-1
        be = _backend.get_backend()
        gZ = be.lowrank_features_grad(fm.Z, fm.mid, fm.inv_w, fm.G, fm.scale, Y, alpha, v, -2.0 * g_iq,
                                      2.0 * g_ld, **fm.kw).to(dtype)
    if need[1]:
        # K = scale k with scale = outputscale * weight: dK / doutputscale = weight K / scale
        gs = (fm.weight / fm.scale) * (-g_iq * (v * v).sum() + g_ld * (F - noise * tr_minv))
        gs = gs.to(op.outputscale.dtype)
    if need[2]:
        gn = (-g_iq * (alpha * alpha).sum() + g_ld * ((N - F) / noise + tr_minv)).to(dtype)
    if need[3]:
        gr = (2.0 * g_iq * alpha).reshape(-1).to(ctx.rdtype)
    return gZ, gs, gn, gr
