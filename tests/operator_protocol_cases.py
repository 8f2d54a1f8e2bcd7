"""The fixed set of small operators and protocol calls behind tests/golden/operator_protocol.{json,npz}: what every protocol
method of the additive operators asks of the backend (entry names in order, shapes / dtypes / strides of tensor arguments,
values of scalar and keyword arguments, host_float reads) and what it returns.  tests/golden/make_operator_protocol.py
records it, tests/test_operator_protocol_host.py replays it and compares.  No GPU: the backend is tests/oracle_backend.py
behind a recording wrapper, extended with stand-ins for the entries only the HIP backend has."""
import contextlib

import torch

from tests.oracle_backend import OracleBackend
from tests.test_fused_full_host import _radial_entries

N, M, T = 8, 3, 3                    # training rows, test rows, right-hand sides


class _Obj:
    """A stand-in for a backend object (tables, plan, descriptor); the trace records its label."""

    def __init__(self, label, **kw):
        self.label = label
        self.__dict__.update(kw)


class RichBackend(OracleBackend):
    """The test double with stand-ins for the entries the host logic probes for with hasattr / getattr: the prepared sweep, the
    padded dense block, the fused pivoted Choleskys, the native executor's descriptors, the SKI plan and the low-rank plan."""
    supports_padded_dense = True
    mbcg_solve = True                                   # (only probed for)

    def __init__(self, fast_ok=True):
        super().__init__()
        self.fast_ok = fast_ok
        _radial_entries(self)

    def prepare(self, Z):
        return _Obj("prep", Z=Z, fast_ok=self.fast_ok)

    def mvm_sym_prepared(self, prep, V, scale, noise=0.0, j0=0, j1=None, shard=None):
        return OracleBackend.mvm_sym(self, prep.Z, V, scale, noise, j0=j0, j1=j1, shard=shard)

    def dense(self, Z1, Z2, scale, j0=0, j1=None, pad=False):
        K = OracleBackend.dense(self, Z1, Z2, scale, j0, j1)
        if not pad:
            return K
        wide = torch.zeros(K.shape[0], K.shape[1] + 8, dtype=K.dtype)
        wide[:, :K.shape[1]] = K
        return wide[:, :K.shape[1]]

    def pivoted_cholesky(self, Z, scale, rank):
        return OracleBackend.dense(self, Z, Z, scale)[:, :rank].contiguous()

    def family_pivoted_cholesky(self, fam, Z, scale, rank, wsum):
        return self.family_dense(fam, Z, Z, scale)[:, :rank].contiguous()

    def ski_pivoted_cholesky(self, Z, gp, scale, rank, grid_size):
        return self.ski_dense(Z, Z, gp, scale, grid_size)[:, :rank].contiguous()

    def make_family(self, kind, group, weights, product=False):
        fam = OracleBackend.make_family(self, kind, group, weights, product)
        fam.weights = weights
        fam.generic = weights.dtype == torch.float64
        return fam

    def make_radial_family(self, kind, d):
        return _Obj("radial_family", kind=kind, d=d)

    def make_operator_desc(self, op, n, j, scale, noise, **kw):
        return _Obj("desc", op=op, n=n, j=j, scale=scale, noise=noise, kw=sorted(kw))

    def make_sum_operator_desc(self, parts):
        return _Obj("sum_desc", parts=len(parts))

    def ski_plan(self, Z, gp, grid_size):
        return _Obj("ski_plan", ok=True)

    def ski_mvm(self, Z1, Z2, gp, V, scale, noise=0.0, grid_size=1024, plan=None):
        return OracleBackend.ski_mvm(self, Z1, Z2, gp, V, scale, noise, grid_size)

    def lowrank_train_plan(self, prep, scale, noise, mass=None):
        return _Obj("lowrank_plan", prep=prep, p=4, q=4, panels=0)

    def mvm_sym_lowrank_weighted(self, lr, prep, weights, V, scale, noise=0.0):
        return self.family_mvm_sym(OracleBackend.make_family(self, "RBF", 1, weights), prep.Z, V, scale, noise)

    def bilinear_grad_lowrank(self, lr, L, R, scale):
        return self.bilinear_grad(lr.prep.Z, L, R, scale)

    def bilinear_grad_lowrank_weighted(self, lr, weights, L, R, scale):
        return self.family_bilinear_grad(OracleBackend.make_family(self, "RBF", 1, weights), lr.prep.Z, L, R, scale)


def _quantise(x):
    """Backend outputs on a bfloat16 grid.  The oracle's float64 exponentials and BLAS sums may differ in their last bits from
    one CPU to another; on this grid they do not, and everything the host code does with them afterwards (exactly rounded
    elementwise arithmetic, copies, views) is reproducible, so the returned tensors can be compared bit for bit."""
    if isinstance(x, torch.Tensor) and x.is_floating_point():
        return x.to(torch.bfloat16).to(x.dtype) if x.is_contiguous() else \
            x.copy_(x.to(torch.bfloat16).to(x.dtype))          # (the padded dense view keeps its strides)
    if isinstance(x, tuple):
        return tuple(_quantise(v) for v in x)
    return x


def describe(x, deep=False):
    """JSON form of an argument: a tensor by shape / dtype / strides, a scalar by value, an object by its label (`deep`: and what
    it was made from)."""
    if isinstance(x, torch.Tensor):
        return "%s%s/%s" % (str(x.dtype).replace("torch.", ""), list(x.shape), list(x.stride()))
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, (tuple, list)):
        return [describe(v, deep) for v in x]
    if deep and isinstance(x, _Obj):
        return {"obj": x.label, "of": {k: describe(v) for k, v in sorted(vars(x).items()) if k != "label"}}
    return {"obj": getattr(x, "label", type(x).__name__)}


class Recorder:
    """The backend the operators see: every call of an entry is appended to `events` before it runs.  Attribute probes (hasattr,
    getattr with a default) answer as the wrapped backend does."""

    def __init__(self, inner):
        self._inner = inner
        self.events = []

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr) or isinstance(attr, type):
            return attr

        def entry(*args, **kw):
            self.events.append({"entry": name, "args": [describe(a) for a in args],
                                "kw": {k: describe(v) for k, v in sorted(kw.items())}})
            out = attr(*args, **kw)
            return out if name == "ski_grid" else _quantise(out)      # (the grid block: exactly rounded already, and h, 1/h agree)
        return entry


class ShardStub:
    """A world-size-2 distributed.JShard without a process group: rank 0's [j0, j1) slice, or its share of the pairs."""
    world_size, rank, group, reducer = 2, 0, None, "reducer"

    def __init__(self, j0, j1, pairs, events):
        self.j0, self.j1, self.pairs, self.events = j0, j1, pairs, events

    def pair_shard(self, backend):
        return (2, 0) if self.pairs else None

    def sharded_mvm(self, local_mvm, V, noise):
        self.events.append({"entry": "shard.sharded_mvm", "args": [describe(V), describe(noise)], "kw": {}})
        return local_mvm(self.j0, self.j1, noise)


def _rand(seed, *shape, dtype=torch.float32):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 0.6).to(dtype)


def _cases():
    """name -> (backend factory, operator factory(rect, events)).  The factories build fresh tensors with fixed seeds."""
    from rpgp_amd.operators import (AdditiveRPOperator, FamilyAdditiveOperator, FullKernelOperator, MixedGroupOperator,
                                    SKIAdditiveOperator)
    out = {}

    def add(name, backend, cls, J, dtype=torch.float32, rect=True, **kw):
        def make(rectangular, events):
            z1, z2 = _rand(1, N, J, dtype=dtype), _rand(2, M, J, dtype=dtype)
            s = torch.tensor(1.7, dtype=dtype)
            k = dict(kw)
            if "shard" in k:
                k["shard"] = ShardStub(*k["shard"], events)
            if "comp_weights" in k:
                k["comp_weights"] = torch.tensor(k["comp_weights"], dtype=dtype)
            return cls(z2, z1, s, **k) if rectangular else cls(z1, None, s, **k)
        out[name] = (backend, make, rect)

    plain = lambda: _radial_entries(OracleBackend())
    rich, slow = (lambda: RichBackend(True)), (lambda: RichBackend(False))
    for tag, be in (("oracle", plain), ("rich", rich), ("slow", slow)):
        add("plain_f32_" + tag, be, AdditiveRPOperator, 5)
    add("plain_f64", rich, AdditiveRPOperator, 5, dtype=torch.float64)
    add("plain_weight", rich, AdditiveRPOperator, 5, weight=0.25)
    add("plain_jshard", rich, AdditiveRPOperator, 5, rect=False, shard=(0, 3, False))
    add("plain_jshard_oracle", plain, AdditiveRPOperator, 5, rect=False, shard=(0, 3, False))
    add("plain_jshard_empty", rich, AdditiveRPOperator, 5, rect=False, shard=(3, 3, False))
    add("plain_pairshard", rich, AdditiveRPOperator, 5, rect=False, shard=(0, 3, True))
    for kind in ("RBF", "Matern", "InverseMQ", "Cosine"):
        add("family_%s_g1" % kind, rich, FamilyAdditiveOperator, 4, kind=kind, comp_weights=[0.4, 0.3, 0.2, 0.6])
    add("family_RBF_g1_oracle", plain, FamilyAdditiveOperator, 4, kind="RBF")
    add("family_RBF_g2", rich, FamilyAdditiveOperator, 6, kind="RBF", group=2, comp_weights=[0.5, 0.3, 0.4])
    add("family_Matern_g2_product", rich, FamilyAdditiveOperator, 6, kind="Matern", group=2, product=True)
    add("family_generic_f64", rich, FamilyAdditiveOperator, 4, dtype=torch.float64, kind="Matern", group=2)
    add("full_RBF_d8", rich, FullKernelOperator, 8, kind="RBF")
    add("full_RBF_d8_oracle", plain, FullKernelOperator, 8, kind="RBF")
    add("full_RBF_d24", rich, FullKernelOperator, 24, kind="RBF")
    add("full_Matern_d8", rich, FullKernelOperator, 8, kind="Matern")
    add("full_RBF_d8_route_off", rich, FullKernelOperator, 8, kind="RBF")
    add("mixed_1123", rich, MixedGroupOperator, 7, kind="RBF", degrees=[1, 1, 2, 3], comp_weights=[0.4, 0.3, 0.2, 0.6])
    add("mixed_1123_oracle", plain, MixedGroupOperator, 7, kind="RBF", degrees=[1, 1, 2, 3])
    add("ski_J5", rich, SKIAdditiveOperator, 5, grid_size=32)
    add("ski_J5_oracle", plain, SKIAdditiveOperator, 5, grid_size=32)
    add("ski_J5_weights", rich, SKIAdditiveOperator, 5, grid_size=32, comp_weights=[0.4, 0.3, 0.2, 0.6, 0.5])
    add("ski_J5_weights_oracle", plain, SKIAdditiveOperator, 5, grid_size=32, comp_weights=[0.4, 0.3, 0.2, 0.6, 0.5])
    add("ski_J5_reference_rule", rich, SKIAdditiveOperator, 5, grid_size=32, grid_rule="reference")
    add("ski_J5_Matern", rich, SKIAdditiveOperator, 5, grid_size=32, kind="Matern")
    add("ski_J66", rich, SKIAdditiveOperator, 66, grid_size=16)
    return out


def case_names():
    return sorted(_cases())


def _calls(rectangular):
    """label -> call(op) of the protocol, each made on a FRESH operator (`sequence`: several on one, for what an operator keeps
    between calls: tables, plans, the route)."""
    from rpgp_amd import settings
    n = M if rectangular else N                      # rows of the operator; its columns are always the N training rows
    V, L, R = _rand(3, N, T), _rand(4, N, 4), _rand(5, N, 4)
    S = _rand(6, N, N)
    S = (S + S.t()) / 2
    idx = torch.tensor([n - 1, 0, n // 2])

    def like(t, op):
        return t.to(op.dtype)

    def lowrank(on):
        def call(op):
            with settings.lowrank_kernel(on):
                return op.lowrank_form(0.1)
        return call

    def lowrank_products(op):
        with settings.lowrank_kernel(True):
            return (op.lowrank_form(0.1), op._matmul(like(V, op), 0.1), op.native_descriptor(0.1),
                    op._bilinear_derivative(like(L, op), like(R, op)), op.lowrank_served, op.lowrank_ranks, op.lowrank_panels)

    calls = {
        "matmul": lambda op: op._matmul(like(V, op)),
        "matmul_noise": lambda op: op._matmul(like(V, op), 0.1),
        "matmul_wide": lambda op: op._matmul(like(_rand(7, N, 14), op)),
        "matmul_vector": lambda op: op.matmul(like(V, op)[:, 0]),
        "diagonal": lambda op: op._diagonal(),
        "get_rows": lambda op: op._get_rows(idx),
        "to_dense": lambda op: op.to_dense(),
        "evaluate": lambda op: op.evaluate(),
        "to_dense_cached": lambda op: op.to_dense_cached(),
        "to_symcache": lambda op: op.to_symcache(),
        "to_symcache_wide": lambda op: op.to_symcache(wide=True),
        "transpose": lambda op: op.t() is op,
        "transpose_matmul": lambda op: op.t()._matmul(like(_rand(8, n, T), op)),
        "transpose_get_rows": lambda op: op.t()._get_rows(torch.tensor([1, N - 1])),
        # (public attributes of the transpose; a tensor with whether it IS one of the operator's own: the grid block, the weights)
        "transpose_state": lambda op: sorted((k, describe(v), any(v is w for w in vars(op).values()))
                                             for k, v in vars(op.t()).items() if not k.startswith("_") and k != "buckets"),
        "representation": lambda op: op.representation(),
        "native_descriptor": lambda op: op.native_descriptor(0.1),
        "native_sharding": lambda op: op.native_sharding(),
        "fused_pivoted_cholesky": lambda op: op.fused_pivoted_cholesky(6),
        "fused_pivoted_cholesky_rank65": lambda op: op.fused_pivoted_cholesky(65),
        "bilinear_derivative": lambda op: op._bilinear_derivative(like(L, op), like(R, op)),
        "quad_form_derivative": lambda op: op._quad_form_derivative(like(L, op), like(R, op)),
        "dense_weight_derivative": lambda op: op.dense_weight_derivative(like(S, op)),
        "lowrank_form_on": lowrank(True),
        "lowrank_form_off": lowrank(False),
        "lowrank_mll_form": lambda op: (op.lowrank_mll_form(0.1), op.lowrank_mll_served, op.lowrank_mll_reason),
        "shape": lambda op: (tuple(op.shape), op.num_projections, op.lowrank_served, op.lowrank_ranks, op.lowrank_panels),
        "sequence": lambda op: (op._matmul(like(V, op)), op.native_descriptor(0.0), op._get_rows(idx), op.to_dense(),
                                op._matmul(like(V, op)), op.t()._matmul(like(_rand(8, n, T), op))),
    }
    if rectangular:
        for name in ("to_symcache_wide", "dense_weight_derivative", "lowrank_form_on", "lowrank_form_off", "lowrank_mll_form",
                     "evaluate", "matmul_vector", "fused_pivoted_cholesky_rank65", "quad_form_derivative"):
            del calls[name]
    else:
        calls["sequence_derivative"] = lambda op: (op._matmul(like(V, op), 0.1), op._bilinear_derivative(like(L, op), like(R, op)),
                                                   op.dense_weight_derivative(like(S, op)), op.native_descriptor(0.1))
        calls["lowrank_products"] = lowrank_products
    return calls


@contextlib.contextmanager
def _recording(backend):
    """Install the recording backend and count operators.host_float reads."""
    from rpgp_amd import backend as _backend, operators
    rec = Recorder(backend)
    reads = [0]
    real = operators.host_float

    def counted(t):
        reads[0] += 1
        return real(t)
    prev = _backend.set_backend(rec)
    operators.host_float = counted
    try:
        yield rec, reads
    finally:
        operators.host_float = real
        _backend.set_backend(prev)


def run_case(name):
    """(trace, tensors, operators) of one case.  trace: "sym/<call>" or "rect/<call>" -> {"events", "host_reads", "returns" |
    "raises"}, the construction's own backend calls under ".../construct".  tensors: every tensor returned, in the order of the
    calls and of their `returns`.  operators: "sym" / "rect" -> a constructed operator (for the capability answers)."""
    from rpgp_amd import operators
    backend, make, rect = _cases()[name]
    trace, tensors, ops = {}, [], {}
    route = operators._FULL_FAMILY_ROUTE
    if name.endswith("route_off"):
        operators._FULL_FAMILY_ROUTE = False
    try:
        for rectangular in ((False, True) if rect else (False,)):
            side = "rect" if rectangular else "sym"
            for label, call in _calls(rectangular).items():
                with _recording(backend()) as (rec, reads):
                    op = make(rectangular, rec.events)
                    built = len(rec.events)
                    entry = {}
                    try:
                        ret = call(op)
                        entry["returns"] = _returned(ret, tensors)
                        entry["events"], entry["host_reads"] = rec.events[built:], reads[0]
                    except Exception as err:   # what raises today raises the same tomorrow; what was asked before is no contract
                        entry["raises"] = [type(err).__name__, str(err)]
                    trace.setdefault(side + "/construct", {"events": rec.events[:built]})
                    trace[side + "/" + label] = entry
                    ops[side] = op
    finally:
        operators._FULL_FAMILY_ROUTE = route
    return trace, tensors, ops


def _returned(x, tensors):
    if isinstance(x, torch.Tensor):
        tensors.append(x.detach().clone())
        return describe(x)
    if isinstance(x, (tuple, list)):
        return [_returned(v, tensors) for v in x]
    return describe(x, deep=True)
