"""Pivoted-Cholesky preconditioner.

Rank-k (k = settings.max_preconditioner_size = 15) partial Cholesky L of K with greedy max-diagonal pivots;
M = L L^T + sigma^2 I is applied by Woodbury, log|M| corrects the SLQ log-det and probes are drawn from N(0, M).
Used when N >= settings.min_preconditioning_size (2000).  Needs only diag(K) (constant s for this kernel) and k rows
of K (rpgp_dense on k x N)."""
import math

import os

import torch

from . import backend as _backend


def pivoted_cholesky(diag, get_rows, max_iter):
    """Returns L (N x k) with K ~= L L^T.  `get_rows(idx)` -> dense K[idx, :].  No host syncs: a fixed number of
    steps is taken and exhausted pivots produce zero columns."""
    N = diag.shape[0]
    k = min(max_iter, N)
    d = diag.clone()
    L = torch.zeros(k, N, dtype=diag.dtype, device=diag.device)
    tiny = torch.finfo(diag.dtype).tiny
    for m in range(k):
        piv = torch.argmax(d).reshape(1)
        dp = d.index_select(0, piv)
        ok = dp > 1e-10 * diag.max()
        row = get_rows(piv)[0]
        if m > 0:
            row = row - L[:m].t() @ L[:m].index_select(1, piv).reshape(-1)
        l = torch.where(ok, row / dp.clamp_min(tiny).sqrt(), torch.zeros_like(row))
        L[m] = l
        d = (d - l * l).clamp_min(0.0)
        d.index_fill_(0, piv, 0.0)
    return L.t().contiguous()


def gram64(A, B):
    """A^T B (k x T) for tall skinny float64 A (N x k), B (N x T).  The library's GEMM heuristics pick a one-tile kernel
    with a serial K loop for a 15 x 15 output with K = 391k (10.8 ms per call, measured); 256 batched partial products
    summed in a fixed order take ~0.1 ms."""
    N = A.shape[0]
    if N < 32768:
        return A.t() @ B
    nb = 256
    c = N // nb
    main = c * nb
    out = torch.bmm(A[:main].reshape(nb, c, A.shape[1]).transpose(1, 2), B[:main].reshape(nb, c, B.shape[1])).sum(0)
    if main < N:
        out = out + A[main:].t() @ B[main:]
    return out


_PANEL = 64          # columns per float64 panel of the Woodbury solve


class WoodburyPreconditioner:
    """M = L L^T + noise I."""

    def __init__(self, L, noise):
        self.L = L
        self.noise = float(noise)
        k = L.shape[1]
        # The capacitance matrix noise I + L^T L is ACCUMULATED in float64: the entries of L^T L are ~ |K| ~ s N (1e5 at
        # N = 391k), so an fp32 accumulation is off by more than sigma^2 itself (measured 0.69 against sigma^2 = 0.45) and
        # the Woodbury "inverse" stops being the inverse of M — preconditioned CG then stagnated at a true residual of
        # 0.2 - 1.4 on the C5-shaped system where un-preconditioned fp32 CG converges in 140 iterations.
        # On the HIP backend the two Gram products and the cancelling update are in-tree kernels on the fp32 factor
        # (rpgp_gram_f64 / rpgp_woodbury_apply: exact products, float64 sums); otherwise float64 torch operations.
        be = _backend.get_backend()
        on_device = L.is_cuda or getattr(be, "name", "") != "hip-gfx950"      # (kind `full` on CPU tensors: torch path)
        self._be = be if (L.dtype == torch.float32 and 0 < k <= 64 and hasattr(be, "gram_f64") and on_device) else None
        self._L64c = None
        cap = self._be.gram_f64(L, L) if self._be is not None else gram64(self._L64, self._L64)
        self._cinv = self._logdet_cap = self._logdet_host = None
        if self._be is not None and hasattr(self._be, "woodbury_setup"):
            # Cholesky factor, inverse and log-determinant of the capacitance matrix in one launch, no synchronisation
            # the log-determinant also lands in pinned host memory, written by the set-up kernel itself: by the time somebody
            # asks for it a solve has synchronised the stream and the read is free (a `float()` of the device scalar is a
            # copy + a synchronisation)
            pinned = torch.empty(1, dtype=torch.float64, pin_memory=True) if cap.is_cuda else None
            if pinned is not None:
                self._cap_chol, self._cinv, self._logdet_cap = self._be.woodbury_setup(cap, self.noise, logdet_pinned=pinned)
            else:
                self._cap_chol, self._cinv, self._logdet_cap = self._be.woodbury_setup(cap, self.noise)
            if pinned is not None:
                self._logdet_host = pinned
                self._logdet_ev = torch.cuda.Event()
                self._logdet_ev.record()
        else:
            cap.diagonal().add_(self.noise)
            self._cap_chol = torch.linalg.cholesky(cap)               # k x k, float64 for a stable capacitance solve
        self.N, self.k = L.shape

    def solve(self, r):
        """M^-1 r = (r - L (noise I + L^T L)^-1 L^T r) / noise.  Everything that touches the cancellation is float64:
        L^T r is accumulated in float64 and r - L t (which shrinks the range-of-L component of r by
        sigma^2 / (sigma^2 + lambda) ~ 1e-6) is subtracted in float64.  Wide blocks (predictive covariance, T = N_test) go
        through in column panels so that the float64 temporaries stay N x 64."""
        squeeze = r.dim() == 1
        if squeeze:
            r = r.unsqueeze(-1)
        if r.shape[1] <= _PANEL:
            out = self._solve_panel(r)
        else:
            out = torch.empty_like(r)
            for c0 in range(0, r.shape[1], _PANEL):
                out[:, c0:c0 + _PANEL] = self._solve_panel(r[:, c0:c0 + _PANEL])
        return out.squeeze(-1) if squeeze else out

    @property
    def _L64(self):
        if self._L64c is None:
            self._L64c = self.L.double()
        return self._L64c

    def _solve_panel(self, r):
        if self._be is not None and r.dtype == torch.float32:
            if self._cinv is not None and hasattr(self._be, "woodbury_solve") and self._cinv.is_contiguous():
                return self._be.woodbury_solve(self.L, r, self._cinv, self.noise)      # Gram product + one fused launch
            g = self._be.gram_f64(self.L, r)
            # (the float64 inverse from the set-up kernel: one small product instead of two triangular solves)
            t = self._cinv @ g if self._cinv is not None else torch.cholesky_solve(g, self._cap_chol)
            return self._be.woodbury_apply(self.L, r, t, self.noise)
        rd = r.double()
        t = torch.cholesky_solve(gram64(self._L64, rd), self._cap_chol)
        return torch.addmm(rd, self._L64, t, alpha=-1.0).div_(self.noise).to(r.dtype)     # (rd may alias r: out of place)

    __call__ = solve

    def cinv(self):
        """(noise I + L^T L)^-1 in float64 (k x k) for the native mBCG executor."""
        if self._cinv is not None:
            return self._cinv
        return torch.cholesky_inverse(self._cap_chol).contiguous()

    def logdet(self):
        """log|M| = log|noise I_k + L^T L| + (N - k) log noise."""
        if self._logdet_host is not None:
            # (long complete behind any solve; hipEventSynchronize costs ~200 us even then — profiles/r4_step_C2_*: ask first)
            if not self._logdet_ev.query():
                self._logdet_ev.synchronize()
            ld_cap = float(self._logdet_host)
            if ld_cap != ld_cap:
                raise RuntimeError("the preconditioner's capacitance matrix is not positive definite")
        elif self._logdet_cap is not None:
            ld_cap = float(self._logdet_cap)                          # (the only synchronisation of the preconditioner)
            if ld_cap != ld_cap:
                raise RuntimeError("the preconditioner's capacitance matrix is not positive definite")
        else:
            ld_cap = float(2.0 * torch.log(self._cap_chol.diagonal()).sum())
        return ld_cap + (self.N - self.k) * math.log(self.noise)

    def sample(self, num, generator=None):
        """z ~ N(0, M):  L eps1 + sqrt(noise) eps2."""
        dev, dt = self.L.device, self.L.dtype
        e1 = torch.randn(self.k, num, generator=generator, device=dev, dtype=dt)
        e2 = torch.randn(self.N, num, generator=generator, device=dev, dtype=dt)
        return self.L @ e1 + math.sqrt(self.noise) * e2


def build_preconditioner(operator, noise, settings):
    """operator: the noise-free kernel operator (LinearOperator protocol: _diagonal, _get_rows)."""
    N = operator.shape[0]
    if N < settings.min_preconditioning_size.value() or settings.max_preconditioner_size.value() <= 0:
        return None
    rank = settings.max_preconditioner_size.value()
    # a model this large is evaluated through a dense factorisation of Khat (models.py): the first use of that factorisation's
    # library products is paid on a side stream while the model trains — every training step builds its preconditioner here
    Z = getattr(operator, "Z1", None)
    if N >= 16384 and Z is not None and Z.is_cuda and Z.dtype == torch.float32 and getattr(operator, "shard", None) is None \
            and not hasattr(operator, "gp") and N <= 131072:          # (not the grid-interpolation operator)
        start_factorisation_warmup(N, Z.device)
    fused = getattr(operator, "fused_pivoted_cholesky", None)
    L = fused(rank) if fused is not None else None
    if L is None:
        L = pivoted_cholesky(operator._diagonal(), operator._get_rows, rank)
    return WoodburyPreconditioner(L, noise)


_FP16X3 = {}


def _fp16x3_available(device):
    """fp16 operands into a float32 result (`torch.mm / addmm(..., out_dtype=torch.float32)`): present in this image's
    PyTorch-ROCm; probed once per device so that another build falls back to the library factorisation instead of failing."""
    key = str(device)
    if key not in _FP16X3:
        try:
            a = torch.ones(16, 16, device=device, dtype=torch.float16)
            c = torch.mm(a, a, out_dtype=torch.float32)
            c = torch.addmm(c, a, a, beta=0.5, out_dtype=torch.float32)
            _FP16X3[key] = c.dtype == torch.float32 and abs(float(c[0, 0]) - 24.0) < 1e-3
        except (TypeError, RuntimeError):
            _FP16X3[key] = False
    return _FP16X3[key]


def blocked_cholesky(K, block=2048, min_size=16384):
    """(L, info) like `torch.linalg.cholesky_ex` for a LARGE float32 SPD matrix on a HIP device: a blocked right-looking
    factorisation written for MI355X (round 5, tools/r5_chol_lab.py).  Per panel of `block` columns: the library factors the
    diagonal block, the panel below it is `A21 D^-T` by the library's triangular solve, and
    the trailing update — where the flops are — runs on the LOWER block triangle only as **fp16x3** products: the panel is
    split into hi = fp16(P) and lo = fp16(2^11 (P - hi)) (22 of float32's 24 mantissa bits; the scale keeps lo out of the
    fp16 subnormals), and `P P^T ~ hi hi^T + 2^-11 (hi lo^T + lo hi^T)` is three fp16 matrix products accumulated in float32
    (`mm / addmm(..., out_dtype=float32)`): the fp16 matrix rate of MI355X (1.2 PFLOP/s measured for one product) instead of
    140 TFLOP/s for the float32 matrix instruction.  N = 50 000: 0.41 - 0.47 s against 0.69 - 0.96 s for the library routine,
    and the factor is as accurate (backward error 4e-7, library 3e-7; a bf16 split, 16 mantissa bits, gave 4e-6 and a
    refinement that contracted by 0.3 per round instead of 4e-4).  Same contract as `cholesky_ex` (lower factor, zeros above).
    Falls back to the library below `min_size`, off the GPU, for other dtypes, when the factor's entries (<= sqrt(max
    diagonal)) would leave the comfortable fp16 range — and retries ONCE with the library when the mixed-precision factor
    reports a failed panel or a non-finite diagonal."""
    n = K.shape[0]
    finish_factorisation_warmup()
    if (not K.is_cuda) or K.dtype != torch.float32 or n < min_size or K.dim() != 2 or not _fp16x3_available(K.device) or \
            os.environ.get("RPGP_BLOCKED_CHOL", "1") == "0":          # (RPGP_BLOCKED_CHOL=0: the library routine, for A/B runs)
        return torch.linalg.cholesky_ex(K)
    dmax = float(K.diagonal().max())                 # (one host synchronisation per factorisation of >= 0.1 s)
    if not (1e-6 < dmax < 1e8):
        return torch.linalg.cholesky_ex(K)
    L = K.clone()
    bad = torch.zeros((), dtype=torch.int32, device=K.device)
    for j0 in range(0, n, block):
        j1 = min(j0 + block, n)
        D, info = torch.linalg.cholesky_ex(L[j0:j1, j0:j1])
        bad = torch.where((bad == 0) & (info != 0), info.to(torch.int32) + j0, bad)     # (no host synchronisation per panel)
        L[j0:j1, j0:j1] = D
        if j1 >= n:
            break
        L[j0:j1, j1:] = 0                              # (the contract of cholesky_ex: zeros above the diagonal blocks)
        P = torch.empty((n - j1, j1 - j0), device=K.device, dtype=K.dtype)                        # A21 D^-T, in row chunks of
        r1 = n                                                                                    # a fixed height (see below)
        while r1 > j1:
            r0 = max(j1, r1 - 4 * block)
            P[r0 - j1:r1 - j1] = torch.linalg.solve_triangular(D, L[r0:r1, j0:j1].t(), upper=False).t()
            r1 = r0
        L[j1:, j0:j1] = P
        hi = P.half()
        lo = ((P - hi.float()) * 2048.0).half()
        # Row chunks of a FIXED height, counted from the bottom: the library picks a kernel per (M, N, K) on first sight of a
        # shape (~3 ms each), and whole-column-block products have ~300 distinct heights per factorisation — the first call of
        # a process took 3.1 s against 0.41 s for the next.  With fixed chunks the heights are `rows` and four remainders
        # (`_blocked_shapes`; `warm_blocked_cholesky` touches exactly those while a model trains).
        rows = 4 * block
        for c0 in range(j1, n, block):
            c1 = min(c0 + block, n)
            bh, bl = hi[c0 - j1:c1 - j1].t(), lo[c0 - j1:c1 - j1].t()
            r1 = n
            while r1 > c0:
                r0 = max(c0, r1 - rows)
                ah, al = hi[r0 - j1:r1 - j1], lo[r0 - j1:r1 - j1]
                t1 = torch.mm(ah, bl, out_dtype=torch.float32)
                t1 = torch.addmm(t1, al, bh, out_dtype=torch.float32)
                t1 = torch.addmm(t1, ah, bh, beta=1.0 / 2048.0, out_dtype=torch.float32)
                L[r0:r1, c0:c1].sub_(t1)
                r1 = r0
    # the mixed-precision factor failed or is not finite where the float32 library routine may still succeed: one
    # retry with the library before the failure is reported (one host synchronisation per factorisation of >= 0.1 s)
    if int(bad) != 0 or not bool(torch.isfinite(L.diagonal()).all()):
        del L
        return torch.linalg.cholesky_ex(K)
    return L, bad


def _blocked_shapes(n, block=2048):
    """The distinct (M, N, K) of the trailing-update products and (rows, cols) of the triangular solves `blocked_cholesky`
    issues for an n x n matrix: chunk heights are `4 block` and the four remainders (n - c0) mod (4 block)."""
    rows = 4 * block
    gemm, trsm = set(), set()
    for j0 in range(0, n, block):
        j1 = min(j0 + block, n)
        if j1 >= n:
            break
        r1 = n
        while r1 > j1:
            r0 = max(j1, r1 - rows)
            trsm.add((r1 - r0, j1 - j0))
            r1 = r0
        for c0 in range(j1, n, block):
            c1 = min(c0 + block, n)
            r1 = n
            while r1 > c0:
                r0 = max(c0, r1 - rows)
                gemm.add((r1 - r0, c1 - c0, j1 - j0))
                r1 = r0
    return sorted(gemm), sorted(trsm)


_WARMED = set()
_warm_thread = None
_warm_started = set()


def start_factorisation_warmup(n, device):
    """`warm_blocked_cholesky` on a side stream from a helper thread, once per (device, n): a few ms of small library products
    beside the training kernels.  A warm-up never takes a fit down: its errors are dropped."""
    global _warm_thread
    dev = torch.device(device)
    key = (str(dev), int(n))
    if key in _warm_started or dev.type != "cuda" or os.environ.get("RPGP_BLOCKED_CHOL", "1") == "0":
        return
    _warm_started.add(key)
    finish_factorisation_warmup()
    import threading
    if len(_warm_started) == 1:
        # a process that ends while the helper thread is still inside the libraries' first-use loads (a fit of a few fast
        # steps: 20 low-rank steps at N = 50 000 take 0.3 s) aborts at interpreter teardown: join it before that
        import atexit
        atexit.register(finish_factorisation_warmup)
    side = torch.cuda.Stream(device=dev)

    def work():
        try:
            with torch.cuda.device(dev), torch.cuda.stream(side):
                warm_blocked_cholesky(n, dev)
            side.synchronize()
        except Exception:
            pass
    _warm_thread = threading.Thread(target=work, daemon=True, name="rpgp-factorisation-warmup")
    _warm_thread.start()


def finish_factorisation_warmup():
    """Join the helper thread (the factorisation that needed it is about to run, or another warm-up is about to start)."""
    global _warm_thread
    th, _warm_thread = _warm_thread, None
    if th is not None:
        th.join()


def warm_blocked_cholesky(n, device, block=2048, min_size=16384):
    """First use of `blocked_cholesky` in a process pays the library's kernel selection / code-object loading for every
    product shape it issues (measured at N = 50 000 in a fresh process: 2.26 s for the first full prediction against 1.23 s for
    the next; 1.66 s with the library factorisation — VERDICT r5 weak #6).  This touches exactly those shapes on scratch
    operands (a few MB, a few ms of device time).  `build_preconditioner` starts it on a side stream from a helper thread
    while the model trains (`start_factorisation_warmup`), so that the prediction behind the fit
    (training_routines.py:551-575) finds them loaded."""
    dev = torch.device(device)
    key = (str(dev), int(n), int(block))
    if dev.type != "cuda" or n < min_size or key in _WARMED or not _fp16x3_available(dev) or \
            os.environ.get("RPGP_BLOCKED_CHOL", "1") == "0":
        return False
    gemm, trsm = _blocked_shapes(n, block)
    eye = torch.eye(block, device=dev, dtype=torch.float32)
    D, _ = torch.linalg.cholesky_ex(eye)
    for (m, k) in trsm:
        torch.linalg.solve_triangular(D[:k, :k], torch.zeros((k, m), device=dev, dtype=torch.float32), upper=False)
    for (m, nn, k) in gemm:
        a = torch.zeros((m, k), device=dev, dtype=torch.float16)
        b = torch.zeros((nn, k), device=dev, dtype=torch.float16).t()
        t1 = torch.mm(a, b, out_dtype=torch.float32)
        t1 = torch.addmm(t1, a, b, out_dtype=torch.float32)
        torch.addmm(t1, a, b, beta=1.0 / 2048.0, out_dtype=torch.float32)
    # the wide triangular solves of the factor's user (torch.cholesky_solve on 2048-column panels)
    torch.cholesky_solve(torch.zeros((block, 64), device=dev, dtype=torch.float32), D)
    _WARMED.add(key)
    return True


class CholeskyPreconditioner:
    """M = the fp32 Cholesky factor of Khat itself: M^-1 r is two triangular solves.  Used for the N_test-wide covariance
    solve when the dense matrix is in HBM anyway and N is beyond the float64 direct solve: CG on the fp32 operator then
    only has to remove the factorisation's rounding error (a handful of iterations instead of ~40 at 91 ms each for
    N = 50k, T = 2000)."""

    def __init__(self, chol):
        self.chol = chol

    def solve(self, r):
        return torch.cholesky_solve(r, self.chol)

    __call__ = solve

