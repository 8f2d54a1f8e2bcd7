"""Closed-form posterior of the grid-interpolation (SKI) models from Gram sums over the grid nodes (settings.ski_posterior;
DESIGN.md 7.13).

The SKI kernel is an explicit feature model on J G grid nodes.  With w_i the 4 J cubic-convolution weights of point i placed in a
vector of J G entries, W (N x JG) their stack and Kuu = blockdiag_j(s w_j Tm_j) the symmetric Toeplitz matrices of the wrapped
1-D sub-kernel, K = W Kuu W^T.  ONE grid block covers the training and the test coordinates (the exact path uses three: K(X, X),
K(X*, X), K(X*, X*)): what is computed is the posterior of one consistent kernel.  Kuu is numerically singular (RBF), so it is
never inverted or factored: per projection w_j Tm_j = U Lambda U^T (eigh, float64), the eigenpairs above 1e-14 lambda_max are
kept and S = blockdiag_j(sqrt(s) U_j Lambda_j^1/2) (JG x F).  Then
    A = W^T W (JG x JG),  g = W^T (y - c)                  the only passes over the N rows (rpgp_ski_gram_f64)
    M = sigma^2 I_F + S^T A S = L L^T                       (cond <= 1 + ||K|| / sigma^2)
    m_u = S M^-1 S^T g,            mean* = W* m_u + c       (the float64 gather)
    C = sigma^2 S M^-1 S^T,        var*_i = w*_i^T C w*_i   (rpgp_ski_quadform_f64: 16 J^2 terms per test row)
    cov* = (W* Q)(W* Q)^T,  Q = sigma S L^-T                (only when it is read)
    alpha = (r - W m_u) / sigma^2
    log N(y* | mean*, cov* + sigma^2 I):  P = M + S^T A* S (A* = W*^T W*),  u = L_P^-1 S^T W*^T d,
        quad = (d^T d - u^T u) / sigma^2,   logdet = m log sigma^2 + log|P| - log|M|
(at the training inputs A* = A and W^T d = g - A m_u: no further pass).  No CG, no preconditioner, no N x N* array."""
import math

import torch

from . import backend as _backend
from .hostvals import host_float
from .likelihoods import LOG2PI, MultivariateNormal
from .models import TrainPosterior

EIG_FLOOR = 1e-14                # eigenpairs of w_j Tm_j kept above this share of the largest
MAX_FEATURES = 4096
MEMORY_SHARE = 0.25              # A, C and one more JG x JG temporary may take this share of the device memory
_COPIES = 3
_PANEL = 4096                    # columns per triangular solve


class _State:
    """Everything that depends on the grid block: the block, the sums over the rows and the F x F factors."""

    def __init__(self, gp, lo, hi, A, g, S, M, L, m_u, logdet_M):
        self.gp, self.lo, self.hi = gp, lo, hi            # lo / hi (J): the coordinate range the block was built over
        self.A, self.g, self.S, self.M, self.L, self.m_u, self.logdet_M = A, g, S, M, L, m_u, logdet_M
        self.C = self.Q = None                            # built when variances / a covariance are first asked for


class SKIPosterior:
    """The closed-form posterior of one prediction strategy over an unsharded SKIAdditiveOperator.  Construct with
    `SKIPosterior.build(strategy)`, which returns (posterior or None, reason)."""

    def __init__(self, strategy, Z, state):
        op = strategy.op
        self.strategy = strategy
        self.model = strategy.model
        self.Z = Z
        self.J, self.G = Z.shape[1], op.grid_size
        self.scale = float(op._scale)
        self.noise = host_float(strategy.noise)
        self.c = host_float(strategy.mean_const.reshape(-1)[0]) if strategy.mean_const.numel() else 0.0
        self.rebuilds = 0
        self._set(state)

    # ---- construction -------------------------------------------------------------------------------------------------
    @staticmethod
    def _grid_kw(op):
        kw = {} if op.grid_rule == "shared" else {"rule": op.grid_rule}
        if op.kind != "RBF":
            kw["kind"] = op.kind
        if op.comp_weights is not None:
            kw["weights"] = op.comp_weights.detach().double()
        return kw

    @staticmethod
    def _residual(strategy):
        return (strategy.model.train_targets.detach().double().reshape(-1, 1) -
                strategy.mean_const.detach().double().reshape(-1, 1))

    @staticmethod
    def _root(be, op, gp, J, G, scale):
        """S (JG x F): per projection the first column of w_j Tm_j from the device's own grid product (a unit histogram: the
        kind and the weights exactly as the operator applies them), the symmetric Toeplitz matrix of it, and its eigenpairs
        above EIG_FLOOR.  One G x G problem under the shared grid without weights."""
        shared = op.grid_rule == "shared" and op.comp_weights is None
        Jh = 1 if shared else J
        hist = torch.zeros((Jh, G, 1), dtype=torch.float64, device=gp.device)
        hist[:, 0, 0] = 1.0
        col = be.ski_grid_product(hist, gp, G).reshape(Jh, G).double()
        lag = (torch.arange(G, device=gp.device).reshape(-1, 1) - torch.arange(G, device=gp.device).reshape(1, -1)).abs()
        lam, U = torch.linalg.eigh(col[:, lag])                               # Jh x G x G
        blocks = []
        for j in range(Jh):
            keep = lam[j] > EIG_FLOOR * lam[j].max()
            blocks.append(U[j][:, keep] * (scale * lam[j][keep]).sqrt())
        if shared:
            blocks = blocks * J
        return torch.block_diag(*blocks)

    @classmethod
    def _state(cls, be, op, Z, lo, hi, r64, scale, noise):
        """(state, None) for the block over [lo, hi] (J each), or (None, reason)."""
        N, J = Z.shape
        G = op.grid_size
        ext = torch.stack([lo, hi])
        gp = be.ski_grid(Z, ext, G, **cls._grid_kw(op))
        S = cls._root(be, op, gp, J, G, scale)
        F = S.shape[1]
        if F > MAX_FEATURES:
            return None, "%d features exceed %d" % (F, MAX_FEATURES)
        if F >= N:
            return None, "%d features for %d rows" % (F, N)
        A, g = be.ski_gram(Z, gp, r64, G)
        M = S.t() @ (A @ S)
        M = 0.5 * (M + M.t())
        M.diagonal().add_(noise)
        L, info = torch.linalg.cholesky_ex(M)
        if int(info) != 0:
            return None, "sigma^2 I + S^T A S is not positive definite"
        m_u = S @ torch.cholesky_solve(S.t() @ g, L)
        return _State(gp, lo, hi, A, g, S, M, L, m_u, 2.0 * float(torch.log(L.diagonal()).sum())), None

    @classmethod
    def build(cls, strategy):
        from . import settings
        op = strategy.op
        cm = strategy.model.covar_module
        if getattr(op, "row_shard", None) is not None or \
                (getattr(cm, "shard", None) is not None and getattr(cm.shard, "world_size", 1) > 1):
            return None, "sharded model"
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            return None, "a world larger than 1"
        be = _backend.get_backend()
        if getattr(be, "ski_gram", None) is None or getattr(be, "ski_quadform", None) is None:
            return None, "the backend has no SKI Gram sums"
        if isinstance(be, _backend.HipBackend) and not op.Z1.is_cuda:
            return None, "host tensors"
        N, J = op.Z1.shape
        G = op.grid_size
        cap = settings.ski_posterior_max_nodes.value()
        if J * G > cap:
            return None, "J G = %d nodes exceed %d" % (J * G, cap)
        if op.Z1.is_cuda and 8.0 * _COPIES * (J * G) ** 2 > MEMORY_SHARE * torch.cuda.get_device_properties(op.Z1.device).total_memory:
            return None, "the %d x %d node arrays exceed %.0f%% of the device memory" % (J * G, J * G, 100 * MEMORY_SHARE)
        if op.comp_weights is not None and not bool((op.comp_weights.detach() >= 0.0).all()):
            return None, "a component weight is negative"
        noise = host_float(strategy.noise)
        Z = op.Z1.detach().double().contiguous()
        lo, hi = Z.min(0).values, Z.max(0).values
        with torch.no_grad():
            state, why = cls._state(be, op, Z, lo, hi, cls._residual(strategy), float(op._scale), noise)
            if state is None:
                return None, why
            return cls(strategy, Z, state), None

    def _set(self, state):
        self.state = state
        be = _backend.get_backend()
        s = self.strategy
        fit = be.ski_gather(self.Z, state.gp, state.m_u.reshape(self.J, self.G, 1), None, 1.0, 0.0, self.G)
        a64 = (self._residual(s) - fit.reshape(-1, 1)) / self.noise
        s.alpha64 = a64
        s.alpha = a64.to(s.r.dtype)

    @property
    def features(self):
        """F: the eigenpairs kept over all projections."""
        return self.state.S.shape[1]

    # ---- other inputs --------------------------------------------------------------------------------------------------
    def _test_coordinates(self, xs):
        return self.model.covar_module(xs, self.model.train_inputs).Z1.detach().double().contiguous()

    def _cover(self, Zs):
        """The state whose block covers Zs, or None (strategy.ski_posterior_reason says why).  A coordinate outside the current
        block rebuilds the block and the sums once on the union of the ranges."""
        st = self.state
        zlo, zhi = Zs.min(0).values, Zs.max(0).values
        if self.strategy.op.grid_rule == "shared":
            outside = bool((zlo.min() < st.lo.min()) | (zhi.max() > st.hi.max()))
        else:
            outside = bool(((zlo < st.lo) | (zhi > st.hi)).any())
        if not outside:
            return st
        new, why = self._state(_backend.get_backend(), self.strategy.op, self.Z, torch.minimum(st.lo, zlo),
                               torch.maximum(st.hi, zhi), self._residual(self.strategy), self.scale, self.noise)
        if new is None:
            self.strategy.ski_posterior_reason = why
            return None
        self._set(new)
        self.rebuilds += 1
        return new

    def _Q(self, st):
        """Q = sigma S L^-T (JG x F), the triangular solve in column panels (the library's runs out of workspace on very wide
        blocks)."""
        if st.Q is None:
            St = st.S.t().contiguous()
            V = torch.empty_like(St)
            for c0 in range(0, St.shape[1], _PANEL):
                V[:, c0:c0 + _PANEL] = torch.linalg.solve_triangular(st.L, St[:, c0:c0 + _PANEL], upper=False)
            st.Q = math.sqrt(self.noise) * V.t().contiguous()
        return st.Q

    def _C(self, st):
        """C = sigma^2 S M^-1 S^T = Q Q^T (JG x JG)."""
        if st.C is None:
            Q = self._Q(st)
            st.C = Q @ Q.t()
        return st.C

    # ---- prediction ----------------------------------------------------------------------------------------------------
    def predict(self, xs, at_train=False):
        """The posterior at xs (an SKIPredictive, or mean-only under skip_posterior_variances), or None when this call must
        take the exact path (the reason is in strategy.ski_posterior_reason)."""
        from . import settings
        be = _backend.get_backend()
        with torch.no_grad():
            Zs = self.Z if at_train else self._test_coordinates(xs)
            st = self.state if at_train else self._cover(Zs)
            if st is None:
                return None
            mean64 = be.ski_gather(Zs, st.gp, st.m_u.reshape(self.J, self.G, 1), None, 1.0, 0.0, self.G).reshape(-1) + self.c
            mean = mean64.to(xs.dtype)
            if settings.skip_posterior_variances.on():
                return MultivariateNormal(mean, torch.zeros_like(mean), diagonal_only=True)
            var64 = be.ski_quadform(Zs, st.gp, self._C(st), self.G)
            return SKIPredictive(mean, mean64, var64, self, st, Zs, xs, at_train)

    def log_prob(self, st, Zs, mean64, value, at_train=False):
        """log N(value | mean, cov* + sigma^2 I) in F x F (Woodbury, determinant lemma)."""
        be = _backend.get_backend()
        d = value.double().reshape(-1, 1) - mean64.reshape(-1, 1)
        m = d.shape[0]
        y = self.model.train_targets
        if at_train and (value is y or (value.shape == y.shape and torch.equal(value.double(), y.double()))):
            As, gs = st.A, st.g - st.A @ st.m_u                               # W^T (y - c - W m_u)
        else:
            As, gs = be.ski_gram(Zs, st.gp, d, self.G)
        P = st.S.t() @ (As @ st.S)
        P = 0.5 * (P + P.t()) + st.M
        Lp = torch.linalg.cholesky(P)
        u = torch.linalg.solve_triangular(Lp, st.S.t() @ gs, upper=False)
        quad = (float((d * d).sum()) - float((u * u).sum())) / self.noise
        logdet = m * math.log(self.noise) + 2.0 * float(torch.log(Lp.diagonal()).sum()) - st.logdet_M
        return -0.5 * (quad + logdet + m * LOG2PI)

    def train_log_prob(self, target):
        """log N(target | mu_train, Sigma_train + sigma^2 I) at the training inputs (W* = W)."""
        st = self.state
        be = _backend.get_backend()
        mean64 = be.ski_gather(self.Z, st.gp, st.m_u.reshape(self.J, self.G, 1), None, 1.0, 0.0, self.G).reshape(-1) + self.c
        return self.log_prob(st, self.Z, mean64, target, at_train=True)


class SKIPredictive(TrainPosterior):
    """Posterior of the grid model at m inputs: mean and variances eager, the m x m covariance (W* Q)(W* Q)^T formed only when
    it is read; the noisy version's log-density is closed-form in F x F when its noise is the strategy's."""

    def __init__(self, mean, mean64, var64, post, state, Zs, xs, at_train, noise=None):
        self.mean = mean
        self.diagonal_only = False
        self._mean64, self._var64, self._post, self._state, self._Zs, self._at_train = mean64, var64, post, state, Zs, at_train
        self._strategy, self._xs, self._noise, self._cov = post.strategy, xs, noise, None

    @property
    def variance(self):
        v = self._var64 if self._noise is None else self._var64 + float(self._noise)
        return v.to(self.mean.dtype)

    @property
    def covariance64(self):
        """The m x m covariance (without observation noise) in float64."""
        post, st = self._post, self._state
        Q = post._Q(st)
        R = _backend.get_backend().ski_gather(self._Zs, st.gp, Q.reshape(post.J, post.G, Q.shape[1]), None, 1.0, 0.0, post.G)
        return R @ R.t()

    @property
    def covariance(self):
        if self._cov is None:
            cov = self.covariance64
            if self._noise is not None:
                cov.diagonal().add_(float(self._noise))
            self._cov = cov.to(self.mean.dtype)
        return self._cov

    @property
    def covariance_materialized(self):
        return self._cov is not None

    def with_observation_noise(self, noise):
        return SKIPredictive(self.mean, self._mean64, self._var64, self._post, self._state, self._Zs, self._xs, self._at_train,
                             noise=noise)

    def log_prob(self, value):
        post = self._post
        same_noise = self._noise is not None and abs(float(self._noise) - post.noise) <= 1e-12 * post.noise
        if not same_noise:
            return MultivariateNormal.log_prob(self, value)
        lp = post.log_prob(self._state, self._Zs, self._mean64, value, self._at_train)
        return torch.as_tensor(lp, dtype=value.dtype, device=value.device)
