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
are of higher degree, held to by the rapid decay of their coefficients.

The weighted kinds (FamilyAdditiveOperator, RBF, 1-D sub-kernels: K = s sum_c w_c exp(-(z_c - z'_c)^2 / 2), one lengthscale per
projection folded into z_c) are served on column forms (lowrank_posterior.column_forms): B is class-major, its column f
belongs to component c(f) and carries the factor sqrt(s w_c), and the algebra above is unchanged.  With
    per_f = -g_iq v_f^2 + g_ld (1 - sigma^2 (M^-1)_ff),   v = B^T alpha      (the diagonal of B^T dB / 2),
    doutputscale = (1 / s) sum_f per_f,          dw_c = (1 / w_c) sum_{f in c} per_f,
and dZ is one adjoint call per class (rpgp_lowrank_features_grad_cols_f64), each writing its own columns of one N x J buffer."""
import math

import torch

from . import backend as _backend
from . import ops, settings
from .lowrank_posterior import (MAX_FEATURES, MAX_J, MEMORY_SHARE, LowrankPosterior, column_forms, rank_cap, size_reason,
                                tail_tolerance)


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


class ColumnFeatureForm:
    """What serves one weighted operator: its float64 coordinates, the column forms (lowrank_posterior.ColumnForms), B and the
    factor L of M = sigma^2 I + B^T B."""

    def __init__(self, forms, Z, B, L, noise, weight):
        self.forms, self.Z, self.B, self.L, self.noise, self.weight = forms, Z, B, L, noise, weight
        self.scale, self.tail, self.p, self.r, self.kw = forms.scale, forms.tail, forms.p, forms.r, forms.kw

    @property
    def ranks(self):
        """(max p, max r, F); `class_ranks` has (p, r, columns) of every class."""
        return self.p, self.r, self.B.shape[1]

    @property
    def class_ranks(self):
        return self.forms.class_ranks


def _served_kind(op):
    """None when `op` is of a kind the features mode serves, else the reason."""
    if op.feature_form_kind is None:
        return "not a plain symmetric additive-RP RBF operator (grid, family, k > 1 or rectangular)"
    return None


def _decide_weighted(op, noise, be, Z):
    """decide() for the weighted kinds, after the conditions the two share."""
    N, J = Z.shape
    w = op.comp_weights.detach().double().reshape(-1).cpu()
    if not bool((w > 0.0).all()):
        return None, "a component weight is not positive"
    forms, why = column_forms(be, Z, Z.min(0).values, Z.max(0).values, w, float(op._scale), noise)
    if forms is None:
        return None, why
    F = forms.F
    if F >= N:
        return None, "%d features for %d rows (F >= N)" % (F, N)
    why = size_reason(N, F, Z.device, 2, "features and B M^-1")
    if why:
        return None, why
    B = forms.features(be, Z)
    M = B.t() @ B
    M.diagonal().add_(noise)
    L, info = torch.linalg.cholesky_ex(M)
    if int(info) != 0:
        return None, "sigma^2 I + B^T B is not positive definite"
    return ColumnFeatureForm(forms, Z, B, L, noise, op.weight), None


_decisions = [0, 0]          # operators served / decided with the setting on, in this process


def served_counts():
    """(served, decided): how many operators (= objective evaluations) the features mode has served, of those that asked
    with the setting on.  The difference of two readings gives a fit's served share (training.train_exact_gp reports it)."""
    return tuple(_decisions)


def decide(op, noise):
    """(FeatureForm or ColumnFeatureForm, None) when the features mode serves the operator `op` at noise sigma^2 (a host
    float), else (None, reason)."""
    out = _decide(op, noise)
    if settings.lowrank_mll.on():
        _decisions[0] += out[0] is not None
        _decisions[1] += 1
    return out


def _decide(op, noise):
    """decide() itself.  Cheap conditions first: B is only formed once every size condition holds."""
    if not settings.lowrank_mll.on():
        return None, "settings.lowrank_mll is off"
    why = _served_kind(op)
    if why:
        return None, why
    weighted = op.feature_form_kind == "weighted"
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
    names = ("lowrank_post_select", "lowrank_features_cols", "lowrank_features_grad_cols") if weighted else \
        ("lowrank_post_select", "lowrank_features", "lowrank_features_grad")
    if any(getattr(be, name, None) is None for name in names):
        return None, "the backend has no low-rank features"
    if noise is None or not (noise > 0.0):
        return None, "no positive noise value"
    scale = float(op._scale)
    Z = op.Z1.detach().double().contiguous()
    if weighted:
        return _decide_weighted(op, noise, be, Z)
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
    """(gZ, gs, gn, gr, gw) of the features mode (InvQuadLogDet.backward's convention; gs is d / d outputscale, gw
    d / d component weights: None for the unweighted operator)."""
    op, fm, alpha, need = ctx.op, ctx.fm, ctx.alpha64, ctx.needs_input_grad
    B, L, noise = fm.B, fm.L, fm.noise
    N, F = B.shape
    g_iq, g_ld = float(g_inv_quad), float(g_logdet)
    Minv = torch.cholesky_inverse(L)
    tr_minv = Minv.diagonal().sum()
    v = B.t() @ alpha                                                            # F x 1
    dtype = op.Z1.dtype
    gZ = gs = gn = gr = gw = None
    forms = getattr(fm, "forms", None)                                           # column forms: the weighted kinds
    if need[0]:
        Y = B @ Minv                                                             # Khat^-1 B = B M^-1
        be = _backend.get_backend()
        if forms is None:
            gZ = be.lowrank_features_grad(fm.Z, fm.mid, fm.inv_w, fm.G, fm.scale, Y, alpha, v, -2.0 * g_iq,
                                          2.0 * g_ld, **fm.kw).to(dtype)
        else:
            gZ = torch.empty_like(fm.Z)                                          # every column belongs to exactly one class
            vf = v.reshape(-1)
            for c in forms.classes:
                be.lowrank_features_grad_cols(fm.Z, c.cols, c.mid, c.inv_w, c.G, forms.col_scale[c.cols], Y[:, c.f0:c.f1],
                                              alpha, vf[c.f0:c.f1], -2.0 * g_iq, 2.0 * g_ld, out=gZ, **fm.kw)
            gZ = gZ.to(dtype)
    if forms is not None and (need[1] or (len(need) > 5 and need[5])):
        per_f = -g_iq * (v * v).reshape(-1) + g_ld * (1.0 - noise * Minv.diagonal())
        if need[1]:
            gs = ((fm.weight / fm.scale) * per_f.sum()).to(op.outputscale.dtype)
        if len(need) > 5 and need[5]:
            comp = forms.comp.to(per_f.device)
            gw = torch.zeros(forms.weights.numel(), dtype=torch.float64, device=per_f.device).index_add_(0, comp, per_f)
            gw = gw / forms.weights.to(per_f.device)
    elif need[1]:
        # K = scale k with scale = outputscale * weight: dK / doutputscale = weight K / scale
        gs = (fm.weight / fm.scale) * (-g_iq * (v * v).sum() + g_ld * (F - noise * tr_minv))
        gs = gs.to(op.outputscale.dtype)
    if need[2]:
        gn = (-g_iq * (alpha * alpha).sum() + g_ld * ((N - F) / noise + tr_minv)).to(dtype)
    if need[3]:
        gr = (2.0 * g_iq * alpha).reshape(-1).to(ctx.rdtype)
    return gZ, gs, gn, gr, gw
