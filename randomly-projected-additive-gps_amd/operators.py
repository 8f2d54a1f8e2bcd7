"""LinearOperator-shaped classes for the additive randomly-projected kernel (drop-in boundary).

Method names follow GPyTorch's LazyTensor / `linear_operator.LinearOperator` protocol (`_matmul`, `_size`,
`_transpose_nonbatch`, `_diagonal`, `_bilinear_derivative`/`_quad_form_derivative`, `to_dense`/`evaluate`,
`representation`) so the solver stack (linear_cg, pivoted Cholesky, prediction strategy) reads like the
reference's dependency.  All arithmetic goes through the compute backend (HIP library); K is never stored unless
`to_dense()` / the cached mode is requested.

`AdditiveRPOperator` writes the protocol once; the other kernel families override its hooks.
"""
import torch

from . import backend as _backend
from .hostvals import host_float
from . import settings
# group sizes the family tile kernels are instantiated for; other sizes are padded with zero columns
from .ops import FAMILY_GROUPS as _FAMILY_GROUPS

# FullKernelOperator._family_route (private: False keeps every full kernel on the radial kernels, for measurements)
_FULL_FAMILY_ROUTE = True


def padded_group_size(k):
    """Smallest instantiated group size >= k (an RBF group padded with all-zero coordinates is the same kernel:
    exp(-0.5 sum d^2) gains factors exp(0))."""
    for g in _FAMILY_GROUPS:
        if g >= k:
            return g
    raise NotImplementedError("multiplicative groups of more than %d dimensions are not built" % _FAMILY_GROUPS[-1])


def _plan_keywords(plan_fn):
    """The keywords of a backend's lowrank_train_plan(prep, scale, noise[, mass=...]) under the settings.  At the defaults there
    are none, so that a backend written against the older signature keeps working: `max_rank` is passed only above 64 (64 is
    the plan's own cap), `panels=True` only under settings.lowrank_panels and to a plan function that takes the keyword (one
    that does not: no panels)."""
    kw = {}
    cap = settings.lowrank_max_rank.value()
    if cap > 64:
        kw["max_rank"] = cap
    if settings.lowrank_panels.on():
        import inspect
        try:
            params = inspect.signature(plan_fn).parameters
        except (TypeError, ValueError):
            params = {}
        if "panels" in params or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values()):
            kw["panels"] = True
    return kw


def _rows(Z, idx):
    """The left operand of a dense block: all rows of Z (to_dense), or a contiguous copy of the rows `idx` (_get_rows)."""
    return Z if idx is None else Z.index_select(0, idx).contiguous()


class LinearOperator:
    """Minimal protocol base."""

    def _size(self):
        raise NotImplementedError

    @property
    def shape(self):
        return self._size()

    def size(self, dim=None):
        s = self._size()
        return s if dim is None else s[dim]

    @property
    def dtype(self):
        raise NotImplementedError

    @property
    def device(self):
        raise NotImplementedError

    def _matmul(self, rhs):
        raise NotImplementedError

    def matmul(self, rhs):
        if rhs.dim() == 1:
            return self._matmul(rhs.unsqueeze(-1)).squeeze(-1)
        return self._matmul(rhs)

    __matmul__ = matmul

    def _transpose_nonbatch(self):
        raise NotImplementedError

    def t(self):
        return self._transpose_nonbatch()

    def _diagonal(self):
        raise NotImplementedError

    def diagonal(self):
        return self._diagonal()

    diag = diagonal

    def _get_rows(self, idx):
        """Dense rows K[idx, :] (the `_getitem` use of pivoted Cholesky)."""
        raise NotImplementedError

    def to_dense(self):
        raise NotImplementedError

    def evaluate(self):
        return self.to_dense()

    def representation(self):
        raise NotImplementedError

    def _bilinear_derivative(self, left_vecs, right_vecs):
        """Gradients of sum((left right^T) * self) w.r.t. each tensor of `representation()`."""
        raise NotImplementedError

    def _quad_form_derivative(self, left_vecs, right_vecs):
        return self._bilinear_derivative(left_vecs, right_vecs)

    def add_diag(self, diag_value):
        return AddedDiagOperator(self, diag_value)

    add_diagonal = add_diag


class AdditiveRPOperator(LinearOperator):
    """K(Z1, Z2) = outputscale * weight * sum_j exp(-0.5 (Z1[:,j]-Z2[:,j]^T)^2)  (SURVEY.md A.1).

    Z1, Z2: projected inputs (N x J), produced by `ScaledProjectionKernel` (scaled_projection_kernel.py:21-37).
    `Z2 is None` means the symmetric train-train kernel: each unordered pair is evaluated once.
    `shard` (rpgp_amd.distributed.JShard) splits the J terms across ranks with one all-reduce per MVM.

    Also the skeleton of the protocol for every kernel family: the guards, the detach, the transpose of a
    symmetric operator, `_get_rows` / `to_dense` and `representation` are written here once, over the hooks `_local_matmul`,
    `_diagonal_value`, `_dense_block`, `_swapped` and `_bilinear_grads` (and, where a family has them, `native_descriptor`,
    `fused_pivoted_cholesky`, `lowrank_form`, `dense_weight_derivative`).
    """

    plain = True               # this class's own kernel: False on every other family, which has none of its fast paths (the fused
    #                            pivoted Cholesky, the padded dense block, the packed symmetric cache, the Chebyshev plan)
    cacheable = True           # a dense or packed copy of K may be built for the solves (kernel_copy_ok: and float32)
    comp_weights = None        # per-component output scales: the families that have them add them to representation()

    def __init__(self, Z1, Z2=None, outputscale=None, weight=1.0, shard=None):
        self.Z1 = Z1
        self.Z2 = Z2
        self.symmetric = Z2 is None
        if outputscale is None:
            outputscale = torch.ones((), dtype=Z1.dtype, device=Z1.device)
        self.outputscale = outputscale
        self.weight = float(weight)
        self.shard = shard
        # kernels take the scale by value: fetched on first use (hostvals: the marginal log-likelihood prefetches it together
        # with the noise in ONE device-to-host copy per optimiser step)
        self._scale_value = None
        self._prep = None          # rpgp_prepare tables for the factorised fast path (built on first use)
        self._lowrank = None       # settings.lowrank_kernel: None undecided, False the sweep, else the ops.LowrankTrainPlan
        self._lowrank_mll = None   # settings.lowrank_mll: None undecided, else (lowrank_mll.FeatureForm or None, reason)

    @property
    def _scale(self):
        if self._scale_value is None:
            self._scale_value = host_float(self.outputscale) * self.weight
        return self._scale_value

    @_scale.setter
    def _scale(self, value):
        self._scale_value = float(value)

    # ---- what the call sites ask instead of the operator's class ---------------------------------------------------
    @property
    def _sharded(self):
        return self.shard is not None and self.shard.world_size > 1

    @property
    def kernel_copy_ok(self):
        """Whether a dense or packed copy of K may be built for the solves (cached-K mode)."""
        return self.cacheable and self.dtype == torch.float32

    def densify_for_wide_solve(self, n):
        """Whether a solve with many right-hand sides may run on the dense matrix at n rows."""
        return True

    @property
    def plain_unsharded(self):
        """The plain operator on one rank: its derivative is the backend's bilinear_grad and one factor `weight`."""
        return self.plain and not self._sharded

    @property
    def feature_form_kind(self):
        """Which feature form lowrank_mll.decide may serve this operator with: "plain", "weighted" or None."""
        return "plain" if self.plain and self.symmetric else None

    # ---- protocol -------------------------------------------------------------------------------------------
    def _size(self):
        n2 = self.Z1.shape[0] if self.symmetric else self.Z2.shape[0]
        return torch.Size((self.Z1.shape[0], n2))

    @property
    def dtype(self):
        return self.Z1.dtype

    @property
    def device(self):
        return self.Z1.device

    @property
    def num_projections(self):
        return self.Z1.shape[1]

    def _jrange(self):
        if self.shard is None:
            return 0, self.num_projections
        return self.shard.j0, self.shard.j1

    def _local_matmul(self, rhs, noise=0.0):
        be = _backend.get_backend()
        j0, j1 = self._jrange()
        z1 = self.Z1.detach()
        if self.symmetric:
            kw = {}
            if self._sharded:
                ps = self.shard.pair_shard(be)
                if ps is not None and z1.dtype == torch.float32:    # pair-sharding: all projections, 1/world of the pairs
                    j0, j1 = 0, self.num_projections
                    kw = {"shard": ps}
                elif j1 <= j0:                      # J-sharding with more ranks than projections: nothing to do here
                    return torch.zeros_like(rhs) if not noise else rhs * noise
            prepare = getattr(be, "prepare", None)
            if prepare is not None and z1.dtype == torch.float32:
                if self._prep is None:
                    self._prep = prepare(z1)        # once per operator (= per hyper-parameter step), one host sync
                if self._prep.fast_ok:
                    return be.mvm_sym_prepared(self._prep, rhs, self._scale, noise, j0=j0, j1=j1, **kw)
            return be.mvm_sym(z1, rhs, self._scale, noise, j0=j0, j1=j1, **kw)
        return be.mvm_rect(z1, self.Z2.detach(), rhs, self._scale, j0=j0, j1=j1)

    def _matmul(self, rhs, noise=0.0):
        if noise and not self.symmetric:
            raise ValueError("a diagonal can only be added to the square symmetric operator")
        rhs = rhs.detach()
        if self._sharded:
            return self.shard.sharded_mvm(lambda j0, j1, nz: self._local_matmul(rhs, nz), rhs, float(noise))
        return self._local_matmul(rhs, noise if self.symmetric else 0.0)

    def fused_pivoted_cholesky(self, rank):
        """Single-launch pivoted Cholesky (rpgp_pivoted_cholesky) when the backend has it and the kernel is not sharded;
        None otherwise (callers fall back to the generic row-by-row version)."""
        be = _backend.get_backend()
        if not self.plain_unsharded or not self.symmetric or not hasattr(be, "pivoted_cholesky") or \
                self.Z1.dtype != torch.float32 or self.num_projections > 64 or rank > 64:
            return None
        return be.pivoted_cholesky(self.Z1.detach().contiguous(), self._scale, min(rank, self.Z1.shape[0]))

    def lowrank_form(self, noise=None):
        """The training plan of the Chebyshev low-rank form that serves this operator's solves and derivative
        (settings.lowrank_kernel), or None for the exact sweep.  Decided ONCE per operator (= per hyper-parameter step) from
        N, the scale and the noise (default: the host value the marginal likelihood recorded), so that the solve and the
        derivative of a step use the same form.  Ranks p, q up to settings.lowrank_max_rank (64 by default; above it a Z
        beyond the factorised sweep's range guard is served too, and its Python-path products run the direct sweep)."""
        return self._decide_lowrank(noise, lambda be, noise: self.plain_unsharded)

    def _decide_lowrank(self, noise, mine, mass=None, sweep_guard=False):
        """lowrank_form of this class and of its weighted subclass.  `mine(be, noise)`: the class's own conditions, asked once
        the setting is on and the noise is known, before the shared ones: a symmetric float32 operator with
        J <= 64 and a backend with prepare and lowrank_train_plan.  `mass()`: the diagonal mass passed as mass=, read (one host
        sync) only when a plan is asked for.  `sweep_guard`: at the default cap without panels a Z that is not fast_ok asks for
        no plan."""
        if self._lowrank is None:
            self._lowrank = False
            be = _backend.get_backend()
            plan_fn, prepare = getattr(be, "lowrank_train_plan", None), getattr(be, "prepare", None)
            if noise is None:
                noise = getattr(self, "_noise_host", None)
            if settings.lowrank_kernel.on() and noise is not None and mine(be, noise) and self.symmetric and \
                    self.Z1.dtype == torch.float32 and self.num_projections <= 64 and plan_fn is not None and \
                    prepare is not None:
                if self._prep is None:
                    self._prep = prepare(self.Z1.detach())
                kw = _plan_keywords(plan_fn)
                if self._prep.fast_ok or kw or not sweep_guard:
                    if mass is not None:
                        kw = dict(mass=mass(), **kw)
                    plan = plan_fn(self._prep, self._scale, float(noise), **kw)
                    if plan is not None:
                        self._lowrank = plan
        return self._lowrank or None

    def _lowrank_in_use(self, noise=None):
        """lowrank_form(noise) under settings.lowrank_kernel or once a plan serves this operator, else None without deciding."""
        return self.lowrank_form(noise) if (settings.lowrank_kernel.on() or self._lowrank) else None

    def lowrank_mll_form(self, noise=None):
        """The explicit features (lowrank_mll.FeatureForm) on which settings.lowrank_mll evaluates this operator's marginal
        likelihood in closed form, or None when that mode does not serve it (the reason: `lowrank_mll_reason`).  Decided ONCE
        per operator (= per hyper-parameter step), from the noise (default: the host value the marginal likelihood recorded)."""
        if self._lowrank_mll is None:
            from . import lowrank_mll
            if noise is None:
                noise = getattr(self, "_noise_host", None)
            self._lowrank_mll = lowrank_mll.decide(self, None if noise is None else float(noise))
        return self._lowrank_mll[0]

    @property
    def lowrank_mll_served(self):
        """Whether the closed-form features mode serves this operator (False while undecided)."""
        return bool(self._lowrank_mll and self._lowrank_mll[0] is not None)

    @property
    def lowrank_mll_reason(self):
        """Why the features mode does not serve this operator (None when it does or while undecided)."""
        return self._lowrank_mll[1] if self._lowrank_mll else None

    @property
    def lowrank_served(self):
        """Whether the low-rank form serves this operator (False while undecided)."""
        return bool(self._lowrank)

    @property
    def lowrank_ranks(self):
        """(p, q) of the low-rank form that serves this operator, or None."""
        return (self._lowrank.p, self._lowrank.q) if self._lowrank else None

    @property
    def lowrank_panels(self):
        """Panel count P >= 2 of the panel plan that serves this operator (settings.lowrank_panels), 0 for a single-interval
        plan, None when the low-rank form does not serve it."""
        return int(getattr(self._lowrank, "panels", 0)) if self._lowrank else None

    def native_descriptor(self, noise=0.0):
        """`struct rpgp_operator` for the native mBCG executor, or None when the operator must stay on the Python path
        (rectangular, float64, or a backend without the executor).  A sharded operator describes THIS RANK's share —
        its (world, rank) pair-shard with all projections, or its [j0, j1) slice of the projections — and
        `native_sharding()` tells the executor to sum the partial products over the ranks."""
        be = _backend.get_backend()
        if not self.symmetric or not hasattr(be, "mbcg_solve") or self.Z1.dtype != torch.float32:
            return None
        if self._sharded and not settings.native_sharded_cg.on():
            return None
        from . import _lib
        z1 = self.Z1.detach()
        lr = self._lowrank_in_use(noise)
        if lr is not None:
            return be.make_operator_desc(_lib.RPGP_OP_LOWRANK, z1.shape[0], z1.shape[1], self._scale, noise, lowrank=lr)
        j0, j1 = self._jrange()
        kw = {}
        if self._sharded:
            ps = self.shard.pair_shard(be)
            if ps is not None:
                j0, j1 = 0, self.num_projections
                kw = {"world": ps[0], "rank": ps[1]}
        prepare = getattr(be, "prepare", None)
        if prepare is not None:
            if self._prep is None:
                self._prep = prepare(z1)
            if self._prep.fast_ok:
                return be.make_operator_desc(_lib.RPGP_OP_FUSED_PREPARED, z1.shape[0], z1.shape[1], self._scale, noise,
                                             prep=self._prep, j0=j0, j1=j1, **kw)
        return be.make_operator_desc(_lib.RPGP_OP_FUSED, z1.shape[0], z1.shape[1], self._scale, noise, Z=z1.contiguous(),
                                     j0=j0, j1=j1, **kw)

    def native_sharding(self):
        """(mode, reducer, global_N) for the native executor, or None for an unsharded operator."""
        if not self._sharded:
            return None
        return ("partial", self.shard.reducer, self.Z1.shape[0])

    def _transpose_nonbatch(self):
        return self if self.symmetric else self._swapped()

    def _swapped(self):
        """The same operator with its two inputs exchanged (hook of `_transpose_nonbatch`; only asked of a rectangular one)."""
        return AdditiveRPOperator(self.Z2, self.Z1, self.outputscale, self.weight, self.shard)

    def _diagonal(self):
        if not self.symmetric:
            raise RuntimeError("diagonal of a rectangular cross-covariance requested")
        d = self._diagonal_value()
        if isinstance(d, torch.Tensor):
            return d
        return torch.full((self.Z1.shape[0],), d, dtype=self.dtype, device=self.device)

    def _diagonal_value(self):
        """k(x, x): one value for all rows, or the backend's vector (hook of `_diagonal`)."""
        return self._scale * self.num_projections       # (diag(K) = s*w*J)

    def _dense_block(self, idx=None):
        """K[idx, :] as a dense matrix, all rows for idx = None (hook of `_get_rows` and `to_dense`)."""
        z2 = self.Z1 if self.symmetric else self.Z2
        return _backend.get_backend().dense(_rows(self.Z1.detach(), idx), z2.detach(), self._scale)

    def _get_rows(self, idx):
        return self._dense_block(idx)

    def to_dense(self):
        return self._dense_block()

    def to_dense_cached(self):
        """The matrix of the cached-K mode: same entries as to_dense(), rows padded to 256 bytes when the backend can
        (a view with stride(0) >= N), so that the HBM stream of DenseOperator runs on aligned 16-byte loads."""
        be = _backend.get_backend()
        if self.plain and self.symmetric and self.Z1.dtype == torch.float32 and getattr(be, "supports_padded_dense", False):
            return be.dense(self.Z1.detach(), self.Z1.detach(), self._scale, pad=True)
        return self.to_dense()

    def to_symcache(self, wide=False):
        """Packed symmetric cache of this operator (every unordered pair once: half the bytes of to_dense_cached()), or
        None when the backend / operator cannot provide one (then the dense matrix is the cached-K form).  `wide`: the
        matrix-core tile layout for blocks of 5..16 right-hand sides (training), else the rotation order (thin solves)."""
        be = _backend.get_backend()
        if not self.plain or not self.symmetric or self.Z1.dtype != torch.float32 or \
                not getattr(be, "supports_symcache", False):
            return None
        if not self._sharded:
            return be.symcache(self.Z1.detach(), wide=wide)
        ps = self.shard.pair_shard(be)          # multi-GPU: this rank's share of the pairs (pair-sharding only)
        if ps is None:
            return None
        return be.symcache(self.Z1.detach(), shard=ps, wide=wide)

    def representation(self):
        zs = (self.Z1,) if self.symmetric else (self.Z1, self.Z2)
        return zs + (self.outputscale,) + (() if self.comp_weights is None else (self.comp_weights,))

    def _bilinear_derivative(self, left_vecs, right_vecs):
        if not self.symmetric:
            raise NotImplementedError("derivatives are only needed for the train-train kernel")
        return self._bilinear_grads(left_vecs.detach(), right_vecs.detach())

    def _bilinear_grads(self, L, R):
        """Hook of `_bilinear_derivative` on the symmetric operator: L, R are detached."""
        be = _backend.get_backend()
        j0, j1 = self._jrange()
        lr = self._lowrank_in_use()
        if lr is not None:
            gZ, gs = be.bilinear_grad_lowrank(lr, L, R, self._scale)
        elif j1 > j0:
            gZ, gs = be.bilinear_grad(self.Z1.detach(), L, R, self._scale, j0=j0, j1=j1)
        else:
            gZ = torch.zeros_like(self.Z1)
            gs = torch.zeros((), dtype=self.dtype, device=self.device)
        if self._sharded:
            from .distributed import all_reduce_sum_
            all_reduce_sum_(gZ, self.shard.group)
            gs = gs.reshape(1)
            all_reduce_sum_(gs, self.shard.group)
            gs = gs.reshape(())
        return gZ, (gs if self.weight == 1.0 else gs * self.weight)

    def dense_weight_derivative(self, S):
        """Gradients of 0.5*sum(S * self) for an explicit symmetric S (Cholesky regime)."""
        be = _backend.get_backend()
        gZ, gs = be.bilinear_grad_dense(self.Z1.detach(), S, self._scale)
        return gZ, gs * self.weight


class SKIAdditiveOperator(AdditiveRPOperator):
    """K ~= outputscale * weight * sum_j W_j Tm W_j^T  — the `ski=True` variant (training_routines.py:157-158;
    SURVEY.md Appendix E): cubic interpolation of every projection onto one shared regular grid of `grid_size` points
    and a Toeplitz matrix of the wrapped 1-D sub-kernel (`kind`: RBF by default) on the grid.  O(N) per MVM (scatter / Toeplitz / gather kernels); same protocol as the exact
    operator so the whole solve stack is unchanged.  The grid is recomputed from the data range at construction
    (once per hyper-parameter step) and is not differentiated (it is a buffer in GPyTorch as well); `gp`: the grid block of the
    operator this one is the transpose of, instead of a new one."""

    plain = False
    cacheable = False              # (its O(N) product is the point; a wide solve may still densify it: densify_for_wide_solve)

    def __init__(self, Z1, Z2=None, outputscale=None, weight=1.0, shard=None, grid_size=1024, comp_weights=None,
                 row_shard=None, grid_rule="shared", kind="RBF", gp=None):
        super().__init__(Z1, Z2, outputscale, weight, shard=None)     # (no J-sharding: the SKI product is O(N))
        self.grid_size = int(grid_size)
        # the wrapped 1-D sub-kernel (training_routines.py:157-158 wraps whatever `_map_to_kernel` returned): only the
        # grid-to-grid Toeplitz entries depend on it; scatter, gather and the derivative's staging are kernel-agnostic
        self.kind = kind
        self._plan = None
        self._local_plan = None       # plan of this rank's rows (row-sharded solve + derivative)
        # Multi-GPU: the N training rows are split over the ranks (distributed.RowShard).  The operator itself keeps the
        # replicated interface (full Z, full vectors: prediction and the generic call sites are unchanged); the solves of
        # the marginal likelihood and of the mean cache run on `row_sharded(noise)` — every rank scatters / gathers ITS rows.
        self.row_shard = row_shard if (row_shard is not None and Z2 is None and row_shard.world_size > 1 and
                                       row_shard.N == Z1.shape[0]) else None
        # per-projection output scales (weighted rp_poly / strictly_additive kinds with `ski: true`): they ride in the
        # grid parameter block and every SKI kernel applies them on the Toeplitz stage
        self.comp_weights = comp_weights
        # grid rule: "shared" = one grid over all projections (this build's rule for the additive_rp kinds, whose reference
        # `GridInterpolationKernel(kernel, **ski_options)` at training_routines.py:157-158 passes no bounds); "reference" =
        # the per-projection bounds of polynomial_projection_kernels.py:54-63 (rp_poly / strictly_additive / additive kinds)
        self.grid_rule = grid_rule
        if gp is None:
            kw = {} if grid_rule == "shared" else {"rule": grid_rule}
            if kind != "RBF":
                kw["kind"] = kind
            if comp_weights is not None:
                kw = dict(weights=comp_weights.detach(), **kw)
            gp = _backend.get_backend().ski_grid(Z1.detach(), None if Z2 is None else Z2.detach(), self.grid_size, **kw)
        self.gp = gp

    def densify_for_wide_solve(self, n):
        # the operator's own wide scatter / gather is O(N J T) and wins above N ~ 32k (models.PredictionStrategy.solve)
        return n <= 32768

    def fused_pivoted_cholesky(self, rank):
        be = _backend.get_backend()
        if not self.symmetric or not hasattr(be, "ski_pivoted_cholesky") or self.Z1.shape[1] > 64 or rank > 64 or \
                self.Z1.dtype != torch.float32:            # (float64 parity path: the generic greedy factor on _get_rows)
            return None
        return be.ski_pivoted_cholesky(self.Z1.detach().contiguous(), self.gp, self._scale,
                                       min(rank, self.Z1.shape[0]), self.grid_size)

    def _get_plan(self):
        """rpgp_ski_plan of the square operator (points sorted by interpolation cell), built on first use — once per
        operator = once per hyper-parameter step; None when the backend has no planned product."""
        be = _backend.get_backend()
        if not self.symmetric or not hasattr(be, "ski_plan") or self.Z1.dtype != torch.float32:
            return None
        if self._plan is None:
            self._plan = be.ski_plan(self.Z1.detach().contiguous(), self.gp, self.grid_size)
        return self._plan if self._plan.ok else None

    def _local_matmul(self, rhs, noise=0.0):
        be = _backend.get_backend()
        z1 = self.Z1.detach()
        z2 = z1 if self.symmetric else self.Z2.detach()
        plan = self._get_plan() if rhs.shape[-1] <= 12 or rhs.dim() == 1 else None
        if plan is not None:
            return be.ski_mvm(z1, z2, self.gp, rhs, self._scale, noise, self.grid_size, plan=plan)
        return be.ski_mvm(z1, z2, self.gp, rhs, self._scale, noise if self.symmetric else 0.0, self.grid_size)

    def native_descriptor(self, noise=0.0):
        be = _backend.get_backend()
        if not self.symmetric or not hasattr(be, "mbcg_solve") or self.Z1.dtype != torch.float32:
            return None
        from . import _lib
        z1 = self.Z1.detach().contiguous()
        return be.make_operator_desc(_lib.RPGP_OP_SKI, z1.shape[0], z1.shape[1], self._scale, noise, Z=z1, gp=self.gp,
                                     G=self.grid_size, prep=self._get_plan())

    def _swapped(self):
        # on the SAME grid block (building one is a backend call and a host sync); no row shard, and the plans start empty
        return SKIAdditiveOperator(self.Z2, self.Z1, self.outputscale, self.weight, grid_size=self.grid_size,
                                   comp_weights=self.comp_weights, grid_rule=self.grid_rule, kind=self.kind, gp=self.gp)

    def row_sharded(self, noise):
        """This rank's rows of (self + noise I) as a RowShardedSKIOperator on the SAME grid block (and weights)."""
        rs = self.row_shard
        op = RowShardedSKIOperator(self.Z1.detach()[rs.r0:rs.r1], self._scale, 1.0, rs, grid_size=self.grid_size,
                                   noise=noise, gp=self.gp)
        # one plan of the local rows per hyper-parameter step, shared by the forward solve and the derivative
        if self._local_plan is None:
            self._local_plan = op._get_plan()
        else:
            op._plan = self._local_plan
        return op

    def _get_local_plan(self, Zl):
        be = _backend.get_backend()
        if not hasattr(be, "ski_plan") or Zl.dtype != torch.float32 or Zl.shape[0] == 0:
            return None
        if self._local_plan is None:
            self._local_plan = be.ski_plan(Zl, self.gp, self.grid_size)
        return self._local_plan if self._local_plan.ok else None

    def row_sharded_bilinear_derivative(self, left_local, right_local):
        """`_bilinear_derivative` with the vectors given as this rank's rows: per 12-column piece the 2T-column grid
        histogram is all-reduced (J x G x 2T float64), the Toeplitz stage is replicated and every rank differentiates ITS
        rows; the d+1 (+J) parameter sums are all-reduced once.  Returns the same tuple as `_bilinear_derivative`, with
        gZ assembled for all N rows (zero-padded all-reduce) so that the projection's backward runs replicated."""
        be = _backend.get_backend()
        rs = self.row_shard
        Zl = self.Z1.detach()[rs.r0:rs.r1].contiguous()
        comp = self.comp_weights is not None
        J = self.Z1.shape[1]
        gZ = torch.zeros_like(self.Z1.detach())
        tail = torch.zeros(1 + (J if comp else 0), dtype=self.dtype, device=self.device)
        for t0 in range(0, left_local.shape[1], 12):
            Lc = left_local[:, t0:t0 + 12].detach().contiguous()
            Rc = right_local[:, t0:t0 + 12].detach().contiguous()
            lplan = self._get_local_plan(Zl)            # cell-sorted scatters of the local rows (same sums as one process)
            hist = be.ski_bilinear_scatter(Zl, self.gp, Lc, Rc, self.grid_size, plan=lplan) if lplan is not None else \
                be.ski_bilinear_scatter(Zl, self.gp, Lc, Rc, self.grid_size)
            rs.all_reduce_(hist, "sum")
            gzl, gs, gc = be.ski_bilinear_finish(Zl, self.gp, hist, Lc, Rc, self._scale, self.grid_size, comp=comp)
            gZ[rs.r0:rs.r1] += gzl
            tail[0] += gs.reshape(())
            if comp:
                tail[1:] += gc.reshape(-1)
        rs.all_reduce_(gZ, "sum")
        rs.all_reduce_(tail, "sum")
        if comp:
            w = self.comp_weights.detach().to(tail)
            return gZ, tail[0] * self.weight, self._scale * tail[1:] / w
        return gZ, tail[0] * self.weight

    def _diagonal_value(self):
        return _backend.get_backend().ski_diag(self.Z1.detach(), self.gp, self._scale, self.grid_size)

    def _dense_block(self, idx=None):
        be = _backend.get_backend()
        z1 = self.Z1.detach()
        z2 = z1 if self.symmetric else self.Z2.detach()
        if hasattr(be, "ski_dense") and z1.shape[1] <= 64:
            # straight from the interpolation weights and the Toeplitz lags (no N x N identity through the MVM)
            return be.ski_dense(_rows(z1, idx), z2, self.gp, self._scale, self.grid_size)
        if idx is None:
            eye = torch.eye(z2.shape[0], dtype=self.dtype, device=self.device)
            return be.ski_mvm(z1, z2, self.gp, eye, self._scale, 0.0, self.grid_size)
        eye = torch.eye(idx.numel(), dtype=self.dtype, device=self.device)
        # K[idx, :] = (K(Z2, Z1[idx]))^T : interpolate the k selected points, gather at all columns
        return be.ski_mvm(z2, _rows(z1, idx), self.gp, eye, self._scale, 0.0, self.grid_size).t().contiguous()

    def _bilinear_grads(self, L, R):
        be = _backend.get_backend()
        z, comp = self.Z1.detach(), self.comp_weights is not None
        plan = self._get_plan()
        if plan is not None and hasattr(be, "ski_bilinear_scatter"):
            # staged form on the operator's plan: cell-sorted scatters of L and R (no atomics), the 2T-column Toeplitz product
            # on the matrix cores, then the per-row derivative — 12 columns per piece
            gZ = gs = gc = None
            for t0 in range(0, L.shape[1], 12):
                Lc = L[:, t0:t0 + 12].contiguous()
                Rc = R[:, t0:t0 + 12].contiguous()
                hist = be.ski_bilinear_scatter(z, self.gp, Lc, Rc, self.grid_size, plan=plan)
                gz_p, gs_p, gc_p = be.ski_bilinear_finish(z, self.gp, hist, Lc, Rc, self._scale, self.grid_size, comp=comp)
                gZ = gz_p if gZ is None else gZ.add_(gz_p)
                gs = gs_p if gs is None else gs.add_(gs_p)
                if comp:
                    gc = gc_p if gc is None else gc.add_(gc_p)
        elif comp:
            gZ, gs, gc = be.ski_bilinear_grad_comp(z, self.gp, L, R, self._scale, self.grid_size)
        else:
            gZ, gs = be.ski_bilinear_grad(z, self.gp, L, R, self._scale, self.grid_size)
        if comp:
            w = self.comp_weights.detach().to(gc)
            return gZ, gs * self.weight, self._scale * gc / w       # d/dZ, d/d outputscale, d/d comp_weights
        return gZ, gs * self.weight

    def dense_weight_derivative(self, S):
        """Gradients of 0.5*sum(S * self) for an explicit symmetric S: bilinear form with L = S/2, R = I."""
        eye = torch.eye(S.shape[0], dtype=self.dtype, device=self.device)
        return self._bilinear_derivative((0.5 * S).contiguous(), eye)


class RowShardedSKIOperator(LinearOperator):
    """The SKI operator (+ noise I) with the N data rows split across ranks — the MI355X counterpart of wrapping the
    SKI kernel in `MultiDeviceKernel` (training_routines.py:407-408 with :157-158).  Every vector it touches is a
    rank's LOCAL block of rows:
        hist_r = W_r^T v_r  (J x G x T float64, rpgp_ski_scatter)  ->  all-reduce SUM (RCCL; 270 KB at J = 3, T = 11)
        H = Tm hist         (replicated float64 Toeplitz product, rpgp_ski_grid_product)
        out_r = scale * W_r H + noise * v_r                        (rpgp_ski_gather)
    The interpolation grid is built from the GLOBAL coordinate range (MIN / MAX all-reduce), so all ranks interpolate onto
    the same grid and the sharded product equals the single-process SKI product up to the float64 summation order of the
    histogram.  CG on it runs with all-reduced inner products (`linear_cg(..., reduce=shard.all_reduce_)`); the rank-k
    pivoted-Cholesky preconditioner is built from distributed pivots (`row_sharded_preconditioner`)."""

    def __init__(self, Z_local, outputscale, weight, row_shard, grid_size=1024, noise=0.0, gp=None, kind="RBF"):
        self.Z1 = Z_local.detach().contiguous()
        self.row_shard = row_shard
        self.grid_size = int(grid_size)
        self._scale = float(outputscale) * float(weight)
        self._noise = float(noise)
        be = _backend.get_backend()
        self._plan = None
        if gp is not None:                 # the grid block of the replicated operator this one was split from
            self.gp = gp
            return
        if self.Z1.shape[0] > 0:
            rng = torch.stack([self.Z1.min(), -self.Z1.max()])
        else:
            rng = torch.full((2,), float("inf"), device=self.Z1.device, dtype=self.Z1.dtype)
        row_shard.all_reduce_(rng, "min")                     # one collective for (min, -max)
        kw = {} if kind == "RBF" else {"kind": kind}
        if self.Z1.dtype == torch.float64:
            kw["dtype"] = torch.float64
        self.gp = be.ski_grid_from_range(float(rng[0]), float(-rng[1]), self.grid_size, self.Z1.device, **kw)

    def _size(self):
        n = self.Z1.shape[0]
        return torch.Size((n, n))

    @property
    def dtype(self):
        return self.Z1.dtype

    @property
    def device(self):
        return self.Z1.device

    def _matmul(self, rhs):
        be = _backend.get_backend()
        rhs = rhs.detach()
        squeeze = rhs.dim() == 1
        V = rhs.reshape(self.Z1.shape[0], rhs.shape[1] if rhs.dim() == 2 else 1).contiguous()
        outs = []
        for c0 in range(0, V.shape[1], 12):                   # the staged entry points take T <= 12 columns
            Vp = V[:, c0:c0 + 12].contiguous()
            J = self.Z1.shape[1]
            if self.Z1.shape[0] > 0:
                plan = self._get_plan()
                hist = be.ski_scatter(self.Z1, self.gp, Vp, self.grid_size, plan=plan) if plan is not None else \
                    be.ski_scatter(self.Z1, self.gp, Vp, self.grid_size)
            else:
                hist = torch.zeros(J, self.grid_size, Vp.shape[1], dtype=torch.float64, device=self.Z1.device)
            self.row_shard.all_reduce_(hist, "sum")
            if self.Z1.shape[0] > 0:
                H = be.ski_grid_product(hist, self.gp, self.grid_size)
                if plan is not None:
                    outs.append(be.ski_gather(self.Z1, self.gp, H, Vp, self._scale, self._noise, self.grid_size, plan=plan))
                else:
                    outs.append(be.ski_gather(self.Z1, self.gp, H, Vp, self._scale, self._noise, self.grid_size))
            else:
                outs.append(Vp.clone())
        out = outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)
        return out.reshape(-1) if squeeze else out

    def _diagonal(self):
        if self.Z1.shape[0] == 0:
            return torch.zeros(0, dtype=self.dtype, device=self.device)
        return _backend.get_backend().ski_diag(self.Z1, self.gp, self._scale, self.grid_size) + self._noise

    def _get_plan(self):
        be = _backend.get_backend()
        if not hasattr(be, "ski_plan") or self.Z1.dtype != torch.float32 or self.Z1.shape[0] == 0:
            return None
        if self._plan is None:
            self._plan = be.ski_plan(self.Z1, self.gp, self.grid_size)
        return self._plan if self._plan.ok else None

    def native_descriptor(self):
        """The local rows as an RPGP_OP_SKI descriptor (noise included); with `native_sharding()` the executor all-reduces
        the grid histogram and the inner products, so the solve is the row-sharded one."""
        be = _backend.get_backend()
        if not hasattr(be, "mbcg_solve") or self.Z1.dtype != torch.float32 or not settings.native_sharded_cg.on():
            return None
        from . import _lib
        z = self.Z1 if self.Z1.shape[0] > 0 else torch.zeros(1, self.Z1.shape[1], dtype=self.dtype, device=self.device)
        return be.make_operator_desc(_lib.RPGP_OP_SKI, self.Z1.shape[0], self.Z1.shape[1], self._scale, self._noise, Z=z,
                                     gp=self.gp, G=self.grid_size, prep=self._get_plan())

    def native_sharding(self):
        return ("rows", self.row_shard.reducer, self.row_shard.N)

    def kernel_rows(self, z_rows):
        """scale * K_ski(z_rows, local rows): k x N_local block for rows given by their (global) coordinates."""
        return _backend.get_backend().ski_dense(z_rows.contiguous(), self.Z1, self.gp, self._scale, self.grid_size)


class RowShardedWoodbury:
    """M = L L^T + noise I with L split by rows: every product with L^T is a k x T all-reduce."""

    def __init__(self, L_local, noise, row_shard):
        self.L = L_local
        self.noise = float(noise)
        self.row_shard = row_shard
        from .precond import gram64
        be = _backend.get_backend()
        on_device = L_local.is_cuda or getattr(be, "name", "") != "hip-gfx950"
        # in-tree float64 Gram / update kernels on the fp32 factor (rpgp_gram_f64, rpgp_woodbury_apply), as in
        # precond.WoodburyPreconditioner; a rank without rows contributes zeros
        self._be = be if (L_local.dtype == torch.float32 and 0 < L_local.shape[1] <= 64 and hasattr(be, "gram_f64")
                          and on_device and L_local.shape[0] > 0) else None
        self._L64 = L_local.double() if self._be is None else None
        cap = self._be.gram_f64(L_local, L_local) if self._be is not None else gram64(self._L64, self._L64)
        row_shard.all_reduce_(cap, "sum")
        self._cinv = self._logdet_cap = None
        if hasattr(be, "woodbury_setup") and on_device and cap.shape[0] <= 64:
            self._cap_chol, self._cinv, self._logdet_cap = be.woodbury_setup(cap, self.noise)   # one launch, no sync
        else:
            cap.diagonal().add_(self.noise)
            self._cap_chol = torch.linalg.cholesky(cap)

    def solve(self, r):
        """(r - L C^-1 L^T r) / noise on the local rows.  As in precond.WoodburyPreconditioner.solve the subtraction
        cancels to ~sigma^2 / |K| of r along the range of L (1e-6 at N = 391k), so t and r - L t stay float64; wide
        blocks go through in 64-column panels (one k x T all-reduce per panel)."""
        from .precond import gram64, _PANEL
        squeeze = r.dim() == 1
        if squeeze:
            r = r.unsqueeze(-1)
        out = torch.empty_like(r)
        for c0 in range(0, max(r.shape[1], 1), _PANEL):
            if self._be is not None and r.dtype == torch.float32:
                rp = r[:, c0:c0 + _PANEL]
                t = self._be.gram_f64(self.L, rp)
                self.row_shard.all_reduce_(t, "sum")
                t = self._cinv @ t if self._cinv is not None else torch.cholesky_solve(t, self._cap_chol)
                out[:, c0:c0 + _PANEL] = self._be.woodbury_apply(self.L, rp, t, self.noise)
                continue
            if self._L64 is None:
                self._L64 = self.L.double()
            rd = r[:, c0:c0 + _PANEL].double()
            t = gram64(self._L64, rd)
            self.row_shard.all_reduce_(t, "sum")
            t = torch.cholesky_solve(t, self._cap_chol)
            out[:, c0:c0 + _PANEL] = torch.addmm(rd, self._L64, t, alpha=-1.0).div_(self.noise).to(r.dtype)
        return out.squeeze(-1) if squeeze else out

    def logdet(self):
        """log|M| = log|noise I_k + L^T L| + (N - k) log noise with the GLOBAL N."""
        import math
        if self._logdet_cap is not None:
            ld_cap = float(self._logdet_cap)
            if ld_cap != ld_cap:
                raise RuntimeError("the preconditioner's capacitance matrix is not positive definite")
        else:
            ld_cap = float(2.0 * torch.log(self._cap_chol.diagonal()).sum())
        return ld_cap + (self.row_shard.N - self.L.shape[1]) * math.log(self.noise)

    def cinv(self):
        """(noise I + L^T L)^-1 in float64 (k x k), identical on every rank, for the native mBCG executor."""
        if self._cinv is not None:
            return self._cinv
        return torch.cholesky_inverse(self._cap_chol).contiguous()

    __call__ = solve


def row_sharded_preconditioner(op, rank):
    """Rank-`rank` pivoted Cholesky of the noise-free row-sharded SKI operator with GLOBAL greedy pivots: per step one
    MAX all-reduce of (largest local residual diagonal), one broadcast of the pivot's J coordinates from its owner, and
    the usual downdate of the local rows.  Same pivots as the single-process factorisation (ties go to the lowest rank)."""
    sh = op.row_shard
    dev, dt = op.device, op.dtype
    nloc, J = op.Z1.shape
    d = (op._diagonal() - op._noise).clone() if nloc else torch.zeros(0, device=dev, dtype=dt)
    dmax0 = torch.tensor([float(d.max()) if nloc else 0.0], device=dev, dtype=torch.float64)
    sh.all_reduce_(dmax0, "max")
    L = torch.zeros(rank, nloc, dtype=dt, device=dev)
    for m in range(rank):
        # (value, -rank) packed so that ONE max all-reduce picks the largest value and, among ties, the lowest rank
        loc = float(d.max()) if nloc else -1.0
        key = torch.tensor([loc], device=dev, dtype=torch.float64)
        sh.all_reduce_(key, "max")
        best = float(key[0])
        claim = torch.tensor([sh.rank if (nloc and loc == best) else sh.world_size], device=dev, dtype=torch.float64)
        sh.all_reduce_(claim, "min")
        owner = int(claim[0])
        zp = torch.zeros(1, J, device=dev, dtype=dt)
        lp = torch.zeros(m + 1, device=dev, dtype=dt)             # the pivot's own entries in the previous columns
        if sh.rank == owner:
            p = int(torch.argmax(d))
            zp[0] = op.Z1[p]
            lp[:m] = L[:m, p]
            lp[m] = d[p]
            d[p] = 0.0
            own_p = p
        sh.broadcast_(zp, owner)
        sh.broadcast_(lp, owner)
        dp = float(lp[m])
        if not dp > 1e-10 * float(dmax0[0]):
            continue                                              # exhausted: zero column (as the single-process loop)
        if nloc:
            row = op.kernel_rows(zp)[0]
            if m > 0:
                row = row - L[:m].t() @ lp[:m]
            l = row / (dp ** 0.5)
            if sh.rank == owner:
                l[own_p] = dp ** 0.5
            L[m] = l
            d = (d - l * l).clamp_min(0.0)
            if sh.rank == owner:
                d[own_p] = 0.0
    return RowShardedWoodbury(L.t().contiguous(), op._noise, sh)


class _WeightedOperator(AdditiveRPOperator):
    """What the family, full and mixed-group operators share: a sum of components phi(.) with phi(0) = 1 and output scales
    summing to `_wsum`, replicated (no shard, no operator weight), and none of the plain operator's own fast paths."""

    plain = False

    def __init__(self, Z1, Z2, outputscale):
        super().__init__(Z1, Z2, outputscale, 1.0, shard=None)

    def _diagonal_value(self):
        return self._scale * self._wsum             # k(x, x) = outputscale * sum_c w_c


class FamilyAdditiveOperator(_WeightedOperator):
    """K = outputscale * sum_c w_c phi_kind(group c of Z's columns) — the other members of the family behind the same
    operator: `kernel_type` Matern / InverseMQ / Cosine sub-kernels (training_routines.py:47-88),
    k > 1 RBF sub-kernels (:172-174) and per-component output scales (polynomial_projection_kernels.py:88-98).
    Z is already divided by the lengthscales.  Same fused tile kernels with a different kernel-function policy
    (rpgp_family_*); runs replicated (no J-sharding), fp32 only."""

    def __init__(self, Z1, Z2=None, outputscale=None, comp_weights=None, kind="RBF", group=1, product=False):
        super().__init__(Z1, Z2, outputscale)
        self.kind, self.group = kind, int(group)
        # a k > 1 group as the PRODUCT of its 1-D sub-kernels (polynomial_projection_kernels.py:70-86) instead of the radial
        # k-dimensional sub-kernel of `additive_rp` (training_routines.py:172-174); one and the same for the RBF
        self.product = bool(product) and self.group > 1 and kind != "RBF"
        if Z1.shape[1] % self.group:
            raise ValueError("the number of columns must be a multiple of the sub-kernel dimension")
        ncomp = Z1.shape[1] // self.group
        if comp_weights is None:
            comp_weights = torch.full((ncomp,), 1.0 / ncomp, dtype=Z1.dtype, device=Z1.device)
        self.comp_weights = comp_weights
        # float64 operators (`--double`) keep float64 weights: the backend then serves them with the runtime-(kind, group)
        # kernels (csrc/rpgp_family_generic.hip), as it does k > 1 sub-kernels of the non-RBF types
        wdt = torch.float64 if Z1.dtype == torch.float64 else torch.float32
        w = comp_weights.detach().to(device=Z1.device, dtype=wdt).reshape(-1).contiguous()
        self.fam = _backend.get_backend().make_family(kind, self.group, w, self.product) if self.product else \
            _backend.get_backend().make_family(kind, self.group, w)
        self._generic = bool(getattr(self.fam, "generic", False))
        self._wsum = float(w.sum())                 # one host sync per construction (= per optimiser step)

    @property
    def _one_form(self):
        """ONE Chebyshev form serves every column: 1-D RBF components (a weight is a factor, a lengthscale is in the column)."""
        return self.kind == "RBF" and self.group == 1 and not self.product

    @property
    def feature_form_kind(self):
        return "weighted" if self._one_form and self.symmetric else None

    def lowrank_form(self, noise=None):
        """The plain operator's protocol for the weighted kinds: the training plan of the ONE Chebyshev form shared by every
        column of Z (the lengthscales are folded into the columns; a component weight is a factor of the combine pass) that
        serves this operator's solves and derivative under settings.lowrank_kernel, or None for the family sweep.  Served: a
        symmetric float32 RBF operator with k = 1 and J <= 64, a backend with the weighted entries, a known positive noise and
        a plan with p, q <= settings.lowrank_max_rank (64 by default) at the tolerance of the kernel's diagonal mass scale * sum_c |w_c| (weights of any sign: the
        product is linear in them).  Decided ONCE per operator, like the plain operator's."""
        def mine(be, noise):
            return self._one_form and not self._generic and hasattr(be, "mvm_sym_lowrank_weighted") and \
                hasattr(be, "bilinear_grad_lowrank_weighted") and float(noise) > 0.0

        # (sweep_guard: above 64 or with panels the plan decides on a finite range; at the defaults the sweep's guard does)
        return self._decide_lowrank(noise, mine, mass=lambda: self._scale * float(self.fam.weights.abs().sum()),
                                    sweep_guard=True)

    def _local_matmul(self, rhs, noise=0.0):
        be = _backend.get_backend()
        z1 = self.Z1.detach()
        if self.symmetric:
            if self._lowrank:                           # (only a plan decided under settings.lowrank_kernel: lowrank_form)
                return be.mvm_sym_lowrank_weighted(self._lowrank, self._prep, self.fam.weights, rhs, self._scale, noise)
            return be.family_mvm_sym(self.fam, z1, rhs, self._scale, noise)
        return be.family_mvm_rect(self.fam, z1, self.Z2.detach(), rhs, self._scale)

    def fused_pivoted_cholesky(self, rank):
        be = _backend.get_backend()
        if not self.symmetric or not hasattr(be, "family_pivoted_cholesky") or self.Z1.shape[1] > 64 or rank > 64 or \
                self._generic:
            return None
        return be.family_pivoted_cholesky(self.fam, self.Z1.detach().contiguous(), self._scale,
                                          min(rank, self.Z1.shape[0]), self._wsum)

    def native_descriptor(self, noise=0.0):
        be = _backend.get_backend()
        if not self.symmetric or not hasattr(be, "mbcg_solve") or self._generic:
            return None
        from . import _lib
        lr = self._lowrank_in_use(noise)
        if lr is not None:
            return be.make_operator_desc(_lib.RPGP_OP_LOWRANK_FAMILY, self.Z1.shape[0], self.Z1.shape[1], self._scale, noise,
                                         family=self.fam, lowrank=lr)
        z1 = self.Z1.detach().contiguous()
        return be.make_operator_desc(_lib.RPGP_OP_FAMILY, z1.shape[0], z1.shape[1], self._scale, noise, Z=z1,
                                     family=self.fam)

    def _swapped(self):
        return FamilyAdditiveOperator(self.Z2, self.Z1, self.outputscale, self.comp_weights, self.kind, self.group, self.product)

    def _dense_block(self, idx=None):
        z2 = self.Z1 if self.symmetric else self.Z2
        return _backend.get_backend().family_dense(self.fam, _rows(self.Z1.detach(), idx), z2.detach(), self._scale)

    def _finish_grads(self, gZ, gcomp):
        w = self.comp_weights.detach().to(gcomp)
        return gZ, (w * gcomp).sum(), self._scale * gcomp          # d/dZ, d/d outputscale, d/d comp_weights

    def _bilinear_grads(self, L, R):
        be = _backend.get_backend()
        lr = self._lowrank_in_use()
        if lr is not None:
            return self._finish_grads(*be.bilinear_grad_lowrank_weighted(lr, self.fam.weights, L, R, self._scale))
        return self._finish_grads(*be.family_bilinear_grad(self.fam, self.Z1.detach(), L, R, self._scale))

    def dense_weight_derivative(self, S):
        return self._finish_grads(*_backend.get_backend().family_bilinear_grad_dense(self.fam, self.Z1.detach(), S, self._scale))


class _FamilyRoute:
    """A full RBF kernel with d <= 20 columns as ONE component of group g >= d of the family tile kernels: owns the zero columns
    up to the instantiated group size g, and takes them off the derivatives again."""

    def __init__(self, fam, Z1, Z2, g):
        self.fam, self.d = fam, Z1.shape[1]

        def pad(Z):
            return None if Z is None else torch.nn.functional.pad(Z.detach(), (0, g - self.d)).contiguous()
        self.z1, self.z2 = pad(Z1), pad(Z2)

    def matmul(self, be, rhs, scale, noise):
        if self.z2 is None:
            return be.family_mvm_sym(self.fam, self.z1, rhs, scale, noise)
        return be.family_mvm_rect(self.fam, self.z1, self.z2, rhs, scale)

    def dense(self, be, idx, scale):
        return be.family_dense(self.fam, _rows(self.z1, idx), self.z1 if self.z2 is None else self.z2, scale)

    def _unpadded(self, gZ, gc):
        return gZ[:, :self.d].contiguous(), gc.reshape(-1)[0]

    def bilinear_grad(self, be, L, R, scale):
        return self._unpadded(*be.family_bilinear_grad(self.fam, self.z1, L, R, scale))

    def bilinear_grad_dense(self, be, S, scale):
        return self._unpadded(*be.family_bilinear_grad_dense(self.fam, self.z1, S, scale))

    def descriptor(self, be, scale, noise):
        from . import _lib
        z1 = self.z1
        return be.make_operator_desc(_lib.RPGP_OP_FAMILY, z1.shape[0], z1.shape[1], scale, noise, Z=z1, family=self.fam)


class _RadialRoute:
    """A full kernel of any kind and d <= 1024 on the radial kernels (csrc/rpgp_radial.hip): owns the radial family of the native
    executor, made on first use."""

    def __init__(self, kind, Z1, Z2):
        self.kind, self.z1, self.z2, self.fam = kind, Z1.detach(), None if Z2 is None else Z2.detach(), None

    def matmul(self, be, rhs, scale, noise):
        return be.radial_mvm(self.kind, self.z1, self.z2, rhs, scale, noise if self.z2 is None else 0.0)

    def dense(self, be, idx, scale):
        z1 = self.z1.contiguous()
        rows = be.radial_dense(self.kind, _rows(z1, idx), z1 if self.z2 is None else self.z2, scale)
        if idx is not None and self.z2 is None:
            # the selected rows are a copy, so the kernel cannot know which entries are diagonal ones: they get the value
            # _diagonal() claims, scale * phi(0), exactly as in the product and the square dense block
            rows[torch.arange(idx.numel(), device=rows.device), idx] = scale
        return rows

    def bilinear_grad(self, be, L, R, scale):
        return be.radial_bilinear_grad(self.kind, self.z1, L, R, scale)

    def bilinear_grad_dense(self, be, S, scale):
        return be.radial_bilinear_grad_dense(self.kind, self.z1, S, scale)

    def descriptor(self, be, scale, noise):
        if not hasattr(be, "make_radial_family"):
            return None
        from . import _lib
        if self.fam is None:
            self.fam = be.make_radial_family(self.kind, self.z1.shape[1])
        z1 = self.z1.contiguous()
        return be.make_operator_desc(_lib.RPGP_OP_RADIAL, z1.shape[0], z1.shape[1], scale, noise, Z=z1, family=self.fam)


class FullKernelOperator(_WeightedOperator):
    """K = outputscale * phi_kind(|z_i - z_i'|^2) over ALL d columns of Z — the `full` kinds (training_routines.py:275-293: one
    RBF / Matern / InverseMQ / Cosine kernel on all inputs, ARD or not) matrix-free (settings.fused_full): the family's single
    component of group = d on the radial kernels (csrc/rpgp_radial.hip), whose squared distance is a Gram product on the fp32
    matrix cores, for any d <= 1024.  Z is already CENTRED (the Gram form's rounding error grows with the norms of the rows,
    not with their distance) and divided by the lengthscales, both inside autograd, so that the lengthscale gradient comes
    from gZ by the chain rule.  Same protocol as the additive operators: the marginal likelihood and the prediction strategy
    take their CG / SLQ / pivoted-Cholesky / LOVE routes.  Unsharded, float32, never cached as an N x N matrix.  Which kernels
    evaluate it (`_route`: _FamilyRoute or _RadialRoute) is chosen once per operator."""

    cacheable = False              # (solve_operator / PredictionStrategy: no dense or packed copy of K; the product is the point)
    _wsum = 1.0                    # one component: phi(0) = 1, and the symmetric product forces d2 = 0 on the diagonal, so
    #                                k(x, x) = outputscale exactly

    def __init__(self, Z1, Z2=None, outputscale=None, kind="RBF"):
        super().__init__(Z1, Z2, outputscale)
        self.kind = kind
        self._chosen = None

    @property
    def _route(self):
        """The RBF with d <= 20 columns on the family tile kernels, everything else on the radial kernels.  Measured on the MI355X
        at N = 50 000: the tile kernel takes 0.8 / 1.4 ms (T = 1) and 2.1 / 2.7 ms (T = 11) at d = 8 / 20 against
        4.0 - 4.7 ms of the radial kernel, far beyond the 5 % spread; the other kinds have no tile kernel for a radial group, and
        d > 20 none at all.  The entries are called directly (no FamilyAdditiveOperator in between: no low-rank decision of its
        own, no host read of the weight); `_FULL_FAMILY_ROUTE` (private: tools/radial_bench.py times both) switches the family
        route off."""
        if self._chosen is None:
            be = _backend.get_backend()
            d = self.Z1.shape[1]
            names = ("make_family", "family_mvm_sym", "family_mvm_rect", "family_dense", "family_bilinear_grad",
                     "family_bilinear_grad_dense")
            self._chosen = _RadialRoute(self.kind, self.Z1, self.Z2)
            if _FULL_FAMILY_ROUTE and self.kind == "RBF" and d <= _FAMILY_GROUPS[-1] and self.Z1.dtype == torch.float32 and \
                    all(hasattr(be, n) for n in names):
                g = padded_group_size(d)
                fam = be.make_family("RBF", g, torch.ones(1, dtype=torch.float32, device=self.Z1.device))
                if not getattr(fam, "generic", False):
                    self._chosen = _FamilyRoute(fam, self.Z1, self.Z2, g)
        return self._chosen

    def _family_route(self):
        """The family route when it serves this operator, None on the radial kernels."""
        return self._route if isinstance(self._route, _FamilyRoute) else None

    def lowrank_form(self, noise=None):
        return None

    def lowrank_mll_form(self, noise=None):
        self._lowrank_mll = (None, "the full kernel has no low-rank feature form")
        return None

    def _local_matmul(self, rhs, noise=0.0):
        return self._route.matmul(_backend.get_backend(), rhs, self._scale, noise)

    def native_descriptor(self, noise=0.0):
        be, route = _backend.get_backend(), self._route
        if not self.symmetric or not hasattr(be, "mbcg_solve"):
            return None
        return route.descriptor(be, self._scale, noise)

    def _swapped(self):
        return FullKernelOperator(self.Z2, self.Z1, self.outputscale, self.kind)

    def _dense_block(self, idx=None):
        return self._route.dense(_backend.get_backend(), idx, self._scale)

    def _bilinear_grads(self, L, R):
        return self._route.bilinear_grad(_backend.get_backend(), L, R, self._scale)

    def dense_weight_derivative(self, S):
        return self._route.bilinear_grad_dense(_backend.get_backend(), S, self._scale)


class MixedGroupOperator(_WeightedOperator):
    """K = outputscale * sum_c w_c prod_{m in group c} k1(z_m - z_m') with multiplicative groups of DIFFERENT sizes
    (`general_rp_poly` with e.g. degrees [1, 1, 2, 3], training_routines.py:192-207; `create_multi_additive_kernel`,
    :247-258: every feature subset up to a degree).  The components are bucketed by group size and every bucket is one
    FamilyAdditiveOperator on its own column slice of Z — same fused tile kernels, one launch per distinct size per
    product; sums, diagonals, rows and derivatives are assembled here.  Runs replicated, fp32; solves in the native mBCG
    executor as an RPGP_OP_SUM of the buckets."""

    def __init__(self, Z1, Z2=None, outputscale=None, comp_weights=None, kind="RBF", degrees=(1,), product=False):
        super().__init__(Z1, Z2, outputscale)
        self.kind = kind
        self.product = bool(product)
        self.degrees = [int(dg) for dg in degrees]
        if sum(self.degrees) != Z1.shape[1]:
            raise ValueError("the group sizes must add up to the number of columns")
        ncomp = len(self.degrees)
        if comp_weights is None:
            comp_weights = torch.full((ncomp,), 1.0 / ncomp, dtype=Z1.dtype, device=Z1.device)
        self.comp_weights = comp_weights
        starts = [0]
        for dg in self.degrees:
            starts.append(starts[-1] + dg)
        self.buckets = []               # (component indices, column indices, operator, group size before padding) per distinct size
        def gather(Zm, co, k, kp, ncomp):
            z = Zm.detach().index_select(1, co)
            if kp == k:
                return z.contiguous()
            zp = torch.zeros(z.shape[0], ncomp, kp, dtype=z.dtype, device=z.device)     # zero-padded groups (see padded_group_size)
            zp[:, :, :k] = z.reshape(z.shape[0], ncomp, k)
            return zp.reshape(z.shape[0], ncomp * kp)

        for k in sorted(set(self.degrees)):
            comps = [c for c, dg in enumerate(self.degrees) if dg == k]
            cols = [starts[c] + m for c in comps for m in range(k)]
            kp = padded_group_size(k) if kind == "RBF" else k
            ci = torch.as_tensor(comps, dtype=torch.long, device=Z1.device)
            co = torch.as_tensor(cols, dtype=torch.long, device=Z1.device)
            z1 = gather(Z1, co, k, kp, len(comps))
            z2 = None if Z2 is None else gather(Z2, co, k, kp, len(comps))
            part = FamilyAdditiveOperator(z1, z2, outputscale, comp_weights.detach().index_select(0, ci), kind, kp, product)
            self.buckets.append((ci, co, part, k))
        self._wsum = sum(bucket[2]._wsum for bucket in self.buckets)

    def _bucket_sum(self, term):
        """Sum of term(bucket's operator, whether it is the first one: the noise rides on the first only) over the buckets."""
        out = None
        for i, bucket in enumerate(self.buckets):
            o = term(bucket[2], i == 0)
            out = o if out is None else out.add_(o)
        return out

    def _local_matmul(self, rhs, noise=0.0):
        return self._bucket_sum(lambda part, first: part._local_matmul(rhs, noise if first else 0.0))

    def native_descriptor(self, noise=0.0):
        """RPGP_OP_SUM of the buckets' RPGP_OP_FAMILY descriptors (the noise rides on the first one)."""
        be = _backend.get_backend()
        if not self.symmetric or not hasattr(be, "make_sum_operator_desc"):
            return None
        parts = []
        for i, bucket in enumerate(self.buckets):
            made = bucket[2].native_descriptor(noise if i == 0 else 0.0)
            if made is None:
                return None
            parts.append(made)
        return be.make_sum_operator_desc(parts)

    def _swapped(self):
        return MixedGroupOperator(self.Z2, self.Z1, self.outputscale, self.comp_weights, self.kind, self.degrees, self.product)

    def _dense_block(self, idx=None):
        return self._bucket_sum(lambda part, first: part._dense_block(idx))

    def _assemble(self, grads):
        gZ = torch.zeros_like(self.Z1)
        gc = torch.zeros(len(self.degrees), dtype=self.Z1.dtype, device=self.Z1.device)
        gs = torch.zeros((), dtype=self.Z1.dtype, device=self.Z1.device)
        for (ci, co, part, k), (gz_p, gs_p, gc_p) in zip(self.buckets, grads):
            kp = part.group
            if kp != k:                              # drop the derivatives of the padding columns
                gz_p = gz_p.reshape(gz_p.shape[0], -1, kp)[:, :, :k].reshape(gz_p.shape[0], -1)
            gZ.index_copy_(1, co, gz_p.to(gZ))
            gc.index_copy_(0, ci, gc_p.to(gc).reshape(-1))
            gs = gs + gs_p.to(gs)
        return gZ, gs, gc

    def _bilinear_grads(self, L, R):
        return self._assemble([bucket[2]._bilinear_grads(L, R) for bucket in self.buckets])

    def dense_weight_derivative(self, S):
        return self._assemble([bucket[2].dense_weight_derivative(S) for bucket in self.buckets])


class AddedDiagOperator(LinearOperator):
    """base + noise * I  (the likelihood's AddedDiagLazyTensor); the noise term is fused into the MVM kernel."""

    def __init__(self, base, noise, noise_value=None):
        if not isinstance(noise, torch.Tensor):
            noise = torch.as_tensor(float(noise), dtype=base.dtype, device=base.device)
        self.base = base
        self.noise = noise
        # host value of the noise: given by the caller, or the one `hostvals.prefetch` / the step kernels left on the tensor —
        # a plain `float(noise)` is a device-to-host copy and a synchronisation in the middle of the step's set-up
        self._noise = float(noise_value) if noise_value is not None else host_float(noise)

    def _size(self):
        return self.base._size()

    @property
    def dtype(self):
        return self.base.dtype

    @property
    def device(self):
        return self.base.device

    def _matmul(self, rhs):
        if isinstance(self.base, AdditiveRPOperator):
            return self.base._matmul(rhs, noise=self._noise)
        return self.base._matmul(rhs) + self._noise * rhs

    def native_descriptor(self):
        fn = getattr(self.base, "native_descriptor", None)
        return fn(self._noise) if fn is not None else None

    def native_sharding(self):
        fn = getattr(self.base, "native_sharding", None)
        return fn() if fn is not None else None

    def _transpose_nonbatch(self):
        return self

    def _diagonal(self):
        return self.base._diagonal() + self._noise

    def _get_rows(self, idx):
        rows = self.base._get_rows(idx)
        rows[torch.arange(idx.numel(), device=rows.device), idx] += self._noise
        return rows

    def to_dense(self):
        d = self.base.to_dense()
        d.diagonal().add_(self._noise)
        return d

    evaluate = to_dense

    def representation(self):
        return self.base.representation() + (self.noise,)

    def _bilinear_derivative(self, left_vecs, right_vecs):
        g_noise = (left_vecs * right_vecs).sum()
        return self.base._bilinear_derivative(left_vecs, right_vecs) + (g_noise,)

    _quad_form_derivative = _bilinear_derivative


class SymCachedOperator(LinearOperator):
    """Cached-K mode on the packed symmetric cache (rpgp_symcache_*): Khat = scale * K + noise I applied as ONE stream
    over N^2 / 2 stored kernel values per block of up to 12 right-hand sides.  `diag_value` = scale * (number of
    projections), the constant diagonal of the additive RBF kernel."""

    def __init__(self, cache, scale, noise=0.0, diag_value=None, shard=None):
        self.cache = cache
        self._scale = float(scale)
        self._noise = float(noise)
        self._diag_value = diag_value
        self.shard = shard if (shard is not None and shard.world_size > 1) else None   # cache = this rank's pair share

    def _size(self):
        return torch.Size((self.cache.N, self.cache.N))

    @property
    def dtype(self):
        return torch.float32

    @property
    def device(self):
        return self.cache.device

    def _matmul(self, rhs):
        be = _backend.get_backend()
        if self.shard is None:
            return be.symcache_mvm(self.cache, rhs.detach(), self._scale, self._noise)
        # one all-reduce of the N x T partial products per MVM, the noise term added by rank 0's slab reduce only
        return self.shard.sharded_mvm(lambda j0, j1, nz: be.symcache_mvm(self.cache, rhs.detach(), self._scale, nz), rhs,
                                      self._noise)

    def native_descriptor(self):
        be = _backend.get_backend()
        if not hasattr(be, "mbcg_solve") or (self.cache.world != 1) != (self.shard is not None):
            return None
        if self.shard is not None and not settings.native_sharded_cg.on():
            return None
        from . import _lib
        return be.make_operator_desc(_lib.RPGP_OP_SYMCACHE, self.cache.N, 0, self._scale, self._noise, symcache=self.cache)

    def native_sharding(self):
        return None if self.shard is None else ("partial", self.shard.reducer, self.cache.N)

    def _transpose_nonbatch(self):
        return self

    def _diagonal(self):
        if self._diag_value is None:
            raise RuntimeError("SymCachedOperator was built without its diagonal value")
        return torch.full((self.cache.N,), float(self._diag_value) + self._noise, dtype=torch.float32, device=self.device)

    def to_dense(self):
        n = self.cache.N
        out = torch.empty((n, n), dtype=torch.float32, device=self.device)
        eye = torch.zeros((n, 12), dtype=torch.float32, device=self.device)
        for c0 in range(0, n, 12):
            w = min(12, n - c0)
            eye.zero_()
            eye[c0:c0 + w, :w].fill_diagonal_(1.0)
            out[:, c0:c0 + w] = self._matmul(eye)[:, :w]
        return out

    evaluate = to_dense


class DenseOperator(LinearOperator):
    """Cached-K mode: an explicit symmetric kernel matrix in HBM; every MVM is an HBM stream
    (rpgp_dense_mvm for thin right-hand sides, a library GEMM for wide ones)."""

    def __init__(self, Kd, noise=0.0):
        self.Kd = Kd
        self._noise = float(noise)

    def _size(self):
        return self.Kd.shape

    @property
    def dtype(self):
        return self.Kd.dtype

    @property
    def device(self):
        return self.Kd.device

    def _matmul(self, rhs):
        rhs = rhs.detach()
        if rhs.shape[-1] <= 32 and rhs.is_cuda and rhs.dtype == torch.float32:
            return _backend.get_backend().dense_mvm(self.Kd, rhs, self._noise)      # HBM-bound MFMA thin GEMM
        out = self.Kd @ rhs                                                        # wide blocks: library GEMM
        if self._noise:
            out.add_(rhs, alpha=self._noise)
        return out

    def native_descriptor(self):
        be = _backend.get_backend()
        if not hasattr(be, "mbcg_solve") or not self.Kd.is_cuda or self.Kd.dtype != torch.float32 or \
                self.Kd.stride(1) != 1 or self.Kd.shape[0] >= 2 ** 31:
            return None
        from . import _lib
        return be.make_operator_desc(_lib.RPGP_OP_DENSE, self.Kd.shape[0], 0, 1.0, self._noise, Kd=self.Kd)

    def _transpose_nonbatch(self):
        return self

    def _diagonal(self):
        return self.Kd.diagonal() + self._noise

    def _get_rows(self, idx):
        rows = self.Kd.index_select(0, idx).clone()
        if self._noise:
            rows[torch.arange(idx.numel(), device=rows.device), idx] += self._noise
        return rows

    def to_dense(self):
        d = self.Kd.clone()
        if self._noise:
            d.diagonal().add_(self._noise)
        return d

    evaluate = to_dense
