"""Training routines: counterparts of training_routines.py (create_additive_rp_kernel :131-189, create_full_kernel
:275-293, create_exact_gp :325-410, train_exact_gp :469-585) and fitting/optimizing.py (train_to_convergence :14-108,
mean_squared_error :111-113) with the same argument names, defaults, return contract and error behaviour
(SURVEY.md §3.2, Appendix D)."""
import copy
import os
import warnings

import numpy as np
import torch
import torch.distributed as dist

from . import rp
from .distributed import JShard, RowShard, is_distributed
from .kernels import (AdditiveStructureRBFKernel, CustomAdditiveKernel, InducingPointKernel, MemoryEfficientGamKernel,
                      PolynomialProjectionKernel, RBFKernel, ScaledProjectionKernel, ScaleKernel, StrictlyAdditiveKernel)
from .likelihoods import GaussianLikelihood, SmoothedBoxPrior
from .models import ExactGPModel, ExactMarginalLogLikelihood
from .ops import trace_range
from . import fused_mll

EXACT_GP_KINDS = ("full", "additive_rp", "strictly_additive", "additive", "rp_poly", "general_rp_poly", "sgpr")
REFERENCE_ONLY_KINDS = ("rp", "deep_rp_poly", "multi_full", "duvenaud_additive")


def _map_to_optim(optimizer):
    """training_routines.py:24-34."""
    table = {"adam": torch.optim.Adam, "sgd": torch.optim.SGD, "lbfgs": torch.optim.LBFGS}
    if optimizer not in table:
        raise ValueError("Unknown optimizer")
    return table[optimizer]


def make_optimizer(optimizer, params, lr):
    """`optimizer(params, lr=lr)` as fitting/optimizing.py:52 builds it; Adam on device parameters uses torch's single-launch
    (`fused=True`) implementation of the SAME update — the exact-GP step has d + 3 scalars to update and is bound by the
    host's launch rate (seven multi-tensor launches per step otherwise)."""
    params = list(params)
    if optimizer is torch.optim.Adam and params and all(p.is_cuda and p.is_floating_point() for p in params):
        try:
            return optimizer(params, lr=lr, fused=True)
        except (RuntimeError, TypeError, ValueError):
            pass
    return optimizer(params, lr=lr)


def _sample_from_range(num_samples, range_):
    """training_routines.py:47-48 (always consumes `num_samples` uniforms, also for a degenerate range)."""
    return torch.rand(num_samples) * (range_[1] - range_[0]) + range_[0]


def mean_squared_error(y_pred, y_true):
    return ((y_pred - y_true) ** 2).mean().item()


def create_additive_rp_kernel(d, J, learn_proj=False, kernel_type="RBF", space_proj=False, prescale=False, ard=True,
                              init_lengthscale_range=(1., 1.), ski=False, ski_options=None, proj_dist="gaussian",
                              batch_kernel=True, mem_efficient=False, k=1, keops=False):
    """Additive randomly-projected kernel (RPA-GP; DPA-GP when `space_proj`).  Same options and validation errors as
    training_routines.py:131-189.  `ski=True` selects the 1-D grid-interpolation operator.
    k > 1 RBF sub-kernels of ANY k <= 20 run on the family kernels (k outside (2, 3, 4, 5, 8, 10, 20) zero-padded to the next
    instantiated group size: the same function); k > 1 Matern / InverseMQ / Cosine sub-kernels (radial form of the
    per-dimension AdditiveKernel, `batch_kernel=False`) run on the runtime-(kind, group) kernels of
    csrc/rpgp_family_generic.hip for k <= 32 and J k <= 64 projected columns; NotImplementedError outside those limits."""
    if k > 1 and (mem_efficient or batch_kernel or space_proj):
        raise ValueError("Can't have k > 1 with memory efficient GAM kernel or a batch kernel or spaced projections.")
    if mem_efficient:
        if ski:
            raise ValueError("Not implemented yet")
        if batch_kernel:
            raise ValueError("Impossible to have batch kernel and memory efficient GAM")
        if kernel_type != "RBF":
            raise ValueError("Memory efficient GAM with alternative sub-kernels not implemented yet.")
    if kernel_type not in ("RBF", "Matern", "InverseMQ", "Cosine"):
        raise ValueError("Unknown kernel type")
    if k > 1 and kernel_type != "RBF" and (batch_kernel or k > 32 or J * k > 64):
        raise NotImplementedError("k > 1 sub-kernels of the non-RBF types: the radial form of the per-dimension AdditiveKernel "
                                  "(batch_kernel=False), k <= 32 and J k <= 64 columns")
    if k > 20 and kernel_type == "RBF":
        raise NotImplementedError("k-dimensional RBF sub-kernels are built up to k = 20 (the reference's largest: "
                                  "additive_rp_prescale_J1_K20.json); other k are padded to the next instantiated size")
    if ski and k > 1:
        raise NotImplementedError("grid interpolation is built for 1-D sub-kernels (k == 1)")
    if keops:
        warnings.warn("keops=True is ignored: the fused HIP kernel already is the matrix-free path")

    projs = [rp.gen_rp(d, k, dist=proj_dist) for _ in range(J)]
    if space_proj:
        newW, _ = rp.space_equally(torch.cat(projs, dim=1).t(), lr=0.1, niter=5000)
        newW.requires_grad = False
        projs = [newW[i:i + k, :].t() for i in range(0, J * k, k)]
    proj_module = torch.nn.Linear(d, J * k, bias=False)
    proj_module.weight.data = torch.cat(projs, dim=1).t().contiguous()

    if mem_efficient:
        add_kernel = MemoryEfficientGamKernel(J)
    else:
        # batch_kernel (AdditiveStructureKernel) and the per-dimension AdditiveKernel variant are the same function:
        # (1/J) sum_j RBF_1(z_j)  (training_routines.py:169-174)
        add_kernel = AdditiveStructureRBFKernel(J, ski=ski, ski_options=ski_options, kernel_type=kernel_type, group=k)
    if ard:
        ard_num_dims = d if prescale else J * k
        initial_ls = _sample_from_range(ard_num_dims, init_lengthscale_range)
    else:
        ard_num_dims = None
        initial_ls = _sample_from_range(1, init_lengthscale_range)
    proj_kernel = ScaledProjectionKernel(proj_module, add_kernel, prescale=prescale, ard_num_dims=ard_num_dims,
                                         learn_proj=learn_proj)
    proj_kernel.initialize(lengthscale=initial_ls)
    return proj_kernel


def create_rp_poly_kernel(d, k, J, activation=None, learn_proj=False, weighted=False, kernel_type="RBF",
                          space_proj=False, init_mixin_range=(1.0, 1.0), init_lengthscale_range=(1.0, 1.0), ski=False,
                          ski_options=None, X=None, proj_dist="gaussian", keops=False):
    """training_routines.py:107-128: J groups of k random projections, product of 1-D sub-kernels inside a group,
    per-component output scales."""
    projs = [rp.gen_rp(d, k, dist=proj_dist) for _ in range(J)]
    if space_proj:
        newW, _ = rp.space_equally(torch.cat(projs, dim=1).t(), lr=0.1, niter=5000)
        newW.requires_grad = False
        projs = [newW[i:i + 1, :].t() for i in range(J)]
    if kernel_type not in ("RBF", "Matern", "InverseMQ", "Cosine"):
        raise ValueError("Unknown kernel type")
    kernel = PolynomialProjectionKernel(J, k, d, kernel_type, projs, None, activation=activation, learn_proj=learn_proj,
                                        weighted=weighted, ski=ski, ski_options=ski_options, X=X)
    kernel.initialize(init_mixin_range, init_lengthscale_range)
    return kernel


def create_strictly_additive_kernel(d, weighted=False, kernel_type="RBF", init_lengthscale_range=(1.0, 1.0),
                                    init_mixin_range=(1.0, 1.0), ski=False, ski_options=None, X=None,
                                    memory_efficient=False, keops=False):
    """training_routines.py:210-225: one sub-kernel per input dimension (GAM)."""
    if kernel_type == "RBF" and memory_efficient:
        if ski:
            raise NotImplementedError("the memory-efficient GAM has no grid-interpolation form (use memory_efficient=False)")
        kernel = MemoryEfficientGamKernel(ard_num_dims=d)
        kernel.initialize(lengthscale=_sample_from_range(d, init_lengthscale_range))
        return kernel
    if kernel_type not in ("RBF", "Matern", "InverseMQ", "Cosine"):
        raise ValueError("Unknown kernel type")
    kernel = StrictlyAdditiveKernel(d, kernel_type, weighted, ski=ski, ski_options=ski_options, X=X)
    kernel.initialize(init_mixin_range, init_lengthscale_range)
    return kernel


def create_additive_kernel(d, groups, weighted=False, kernel_type="RBF", init_lengthscale_range=(1.0, 1.0),
                           init_mixin_range=(1.0, 1.0), ski=False, ski_options=None, X=None, keops=False):
    """training_routines.py:228-235: additive kernel over explicit (equally sized) feature groups."""
    if kernel_type not in ("RBF", "Matern", "InverseMQ", "Cosine"):
        raise ValueError("Unknown kernel type")
    kernel = CustomAdditiveKernel(groups, d, kernel_type, weighted=weighted, ski=ski, ski_options=ski_options, X=X)
    kernel.initialize(init_mixin_range, init_lengthscale_range)
    return kernel


def create_general_rp_poly_kernel(d, degrees, learn_proj=False, weighted=False, kernel_type="RBF",
                                  init_lengthscale_range=(1.0, 1.0), init_mixin_range=(1.0, 1.0), ski=False,
                                  ski_options=None, X=None, keops=False):
    """training_routines.py:192-207 (model_specs/polynomial_rp.json): sum(degrees) Gaussian random projections, grouped in
    order into multiplicative groups of the given sizes — the sizes may differ (operators.MixedGroupOperator)."""
    from .kernels import GeneralizedProjectionKernel
    out_dim = sum(degrees)
    W = torch.cat([rp.gen_rp(d, 1) for _ in range(out_dim)], dim=1).t()
    projection_module = torch.nn.Linear(d, out_dim, bias=False)
    projection_module.weight = torch.nn.Parameter(W.contiguous())
    if kernel_type not in ("RBF", "Matern", "InverseMQ", "Cosine"):
        raise ValueError("Unknown kernel type")
    kernel = GeneralizedProjectionKernel(degrees, d, kernel_type, projection_module, learn_proj, weighted, ski, ski_options,
                                         X=X)
    kernel.initialize(init_mixin_range, init_lengthscale_range)
    return kernel


def create_multi_additive_kernel(d, max_degree, weighted=False, kernel_type="RBF", init_lengthscale_range=(1.0, 1.0),
                                 init_mixin_range=(1.0, 1.0), ski=False, ski_options=None, X=None, keops=False):
    """EXTRA — outside the hot-path scope table (SURVEY.md §2.1 marks the reference's `create_multi_*` factories out of
    scope; no served spec reaches it).  Kept because it is ten lines over `CustomAdditiveKernel`.
    training_routines.py:247-258: an additive kernel over EVERY feature subset of size 1..max_degree (the group order
    inside one size follows the reference's `list(set(combinations(...)))`, so the same torch RNG stream initialises the
    same groups)."""
    from itertools import combinations
    if kernel_type not in ("RBF", "Matern", "InverseMQ", "Cosine"):
        raise ValueError("Unknown kernel type")
    max_degree = min(max_degree, d)
    groups = []
    for deg in range(1, max_degree + 1):
        groups.extend(list(set(combinations(list(range(d)), deg))))
    kernel = CustomAdditiveKernel(groups, d, kernel_type, weighted=weighted, ski=ski, ski_options=ski_options, X=X)
    kernel.initialize(init_mixin_range, init_lengthscale_range)
    return kernel


def create_full_kernel(d, ard=False, ski=False, grid_size=None, kernel_type="RBF", init_lengthscale_range=(1.0, 1.0),
                       keops=False):
    """Plain stationary kernel for `kind: full` (training_routines.py:275-293): dense torch ops, not the hot path."""
    if kernel_type not in ("RBF", "Matern", "InverseMQ", "Cosine"):
        raise ValueError("Unknown kernel type")
    if ski:
        raise NotImplementedError("d-dimensional grid interpolation is not built (only the 1-D per-projection SKI)")
    ard_num_dims = d if ard else None
    kernel = RBFKernel(ard_num_dims=ard_num_dims, kernel_type=kernel_type)
    kernel.initialize(lengthscale=_sample_from_range(d if ard else 1, init_lengthscale_range))
    return kernel


def create_sgpr_kernel(d, ard=False, kernel_type="RBF", inducing_points=800, init_lengthscale_range=(1.0, 1.0), X=None,
                       likelihood=None):
    """Inducing-point kernel for `kind: sgpr` (training_routines.py:296-322): a stationary base kernel around the first
    `inducing_points` rows of X (all of X when there are fewer), trainable.  Cosine is an unknown type here, as there."""
    if kernel_type not in ("RBF", "Matern", "InverseMQ"):
        raise ValueError("Unknown kernel type")
    kernel = RBFKernel(ard_num_dims=d if ard else None, kernel_type=kernel_type)
    kernel.initialize(lengthscale=_sample_from_range(d if ard else 1, init_lengthscale_range))
    if X is None:
        raise ValueError("X is required")
    if likelihood is None:
        raise ValueError("Likelihood is required")
    return InducingPointKernel(kernel, X[:inducing_points], likelihood)


def create_exact_gp(trainX, trainY, kind, devices=("cpu",), **kwargs):
    """Create an exact GP model with a specified kernel (training_routines.py:325-410).
    Under a torch.distributed process group (one process per GPU) the exact additive_rp kernel is pair- / J-sharded
    (distributed.JShard) and the SKI variants are row-sharded (distributed.RowShard)."""
    [n, d] = trainX.shape
    if kind not in EXACT_GP_KINDS + REFERENCE_ONLY_KINDS:
        raise ValueError("Unknown kernel structure type {}".format(kind))
    if kind in REFERENCE_ONLY_KINDS:
        raise NotImplementedError("kernel kind '%s' is outside the MI355X hot path (SURVEY.md §2.1, §8(f))" % kind)

    if kwargs.pop("noise_prior"):
        noise_prior_ = SmoothedBoxPrior(1e-4, 10, sigma=0.01)
    else:
        noise_prior_ = None
    likelihood = GaussianLikelihood(noise_prior=noise_prior_)
    likelihood.noise = _sample_from_range(1, kwargs.pop("init_noise_range", [1.0, 1.0]))
    grid_size = kwargs.pop("grid_size", None)
    kwargs.pop("grid_ratio", None)
    if kind == "full":
        kernel = create_full_kernel(d, grid_size=grid_size, **kwargs)
    elif kind == "strictly_additive":
        kernel = create_strictly_additive_kernel(d, X=trainX, **kwargs)
    elif kind == "additive":
        kernel = create_additive_kernel(d, X=trainX, **kwargs)
    elif kind == "rp_poly":
        kernel = create_rp_poly_kernel(d, X=trainX, **kwargs)
    elif kind == "general_rp_poly":
        kernel = create_general_rp_poly_kernel(d, X=trainX, **kwargs)
    elif kind == "sgpr":
        kernel = create_sgpr_kernel(d, X=trainX, likelihood=likelihood, **kwargs)
    else:
        kernel = create_additive_rp_kernel(d, **kwargs)
    kernel = ScaleKernel(kernel)
    if is_distributed() and kwargs.get("ski", False) and kind != "full":
        # the SKI variants (BASELINE config 5: additive_spread_prescale_Jd_ski on 8 GPUs; the reference wraps the kernel in
        # MultiDeviceKernel, training_routines.py:407-408 with :157-158): the N training rows are split over the ranks
        kernel.shard = RowShard(n)
    elif kind == "additive_rp" and is_distributed() and kwargs.get("kernel_type", "RBF") == "RBF" and kwargs.get("k", 1) == 1:
        kernel.shard = JShard(kwargs["J"])
    elif len(devices) > 1:
        raise RuntimeError("multi-device runs are one process per GPU: launch with `python -m torch.distributed.run "
                           "--nproc-per-node %d ...` (J terms are sharded over ranks, RCCL all-reduce per MVM)"
                           % len(devices))
    model = ExactGPModel(trainX, trainY, likelihood, kernel)
    return model, likelihood


def train_to_convergence(model, xs, ys, optimizer=None, lr=0.1, objective=None, max_iter=100, verbose=0, patience=20,
                         conv_tol=1e-4, check_conv=True, smooth=True, isloss=False, batch_size=None, checkpoint=False,
                         print_freq=1, loss_log=None):
    """Full-batch optimisation loop with moving-average early stopping (fitting/optimizing.py:14-108).

    Returns the epoch index at which convergence was declared, or max_iter.  As in the reference the moving average
    over `patience` epochs is undefined (NaN) for the first patience-1 epochs, so the earliest stop is epoch
    2*patience-1.  Mini-batching (`batch_size`) is not meaningful for an exact GP and is rejected."""
    if optimizer is None:
        optimizer = torch.optim.LBFGS
    verbose = int(verbose)
    if batch_size is not None and batch_size != xs.shape[0]:
        raise NotImplementedError("mini-batches are not supported for exact GPs (train inputs must be the full set)")
    model.train()
    optimizer_ = make_optimizer(optimizer, [p for p in model.parameters() if p.requires_grad], lr)

    best_model, best_loss = None, np.inf
    losses = np.zeros((max_iter,))
    ma = np.zeros((max_iter,))
    for i in range(max_iter):
        def closure():
            with trace_range("rpgp:objective+backward"):
                optimizer_.zero_grad()
                output = model(xs)
                if isloss:
                    loss = objective(output, ys)
                    loss.backward()
                else:                     # (an objective that can form the loss and its gradients itself does:
                    nb = getattr(objective, "negative_and_backward", None)     #  models.ExactMarginalLogLikelihood)
                    if nb is not None:
                        loss = nb(output, ys)
                    else:
                        loss = -objective(output, ys)
                        loss.backward()
            return loss

        # (roctx ranges, live under `rocprofv3 --marker-trace` only: the optimiser's own update is what is left of this range
        #  behind the closure's)
        with trace_range("rpgp:optimiser_step"):
            # (`.item()` of the reference's loop; the fused objective posted its value to the host at the end of the forward
            #  pass, so this does not wait for the derivative and the update behind it)
            loss = fused_mll.loss_value(optimizer_.step(closure))
        if verbose > 1:
            print("epoch {}, iter {}, loss {}".format(i, 0, loss))
        losses[i] = loss
        if loss_log is not None:          # (not in the reference: lets callers / tests read the per-epoch losses)
            loss_log.append(loss)
        lo = i - patience + 1
        ma[i] = losses[lo:i + 1].mean() if lo >= 0 else np.nan
        if i % print_freq == 0 and verbose >= 1:
            print("epoch {}, loss {}, noise {}".format(i, loss, model.likelihood.noise.item()))
        if checkpoint and loss < best_loss:
            best_loss = loss
            best_model = copy.deepcopy(model.state_dict())
        if check_conv and i >= patience:
            delta = (ma[i - patience] - ma[i]) if smooth else (losses[i - patience] - losses[i])
            if delta < conv_tol:          # NaN compares False: no stop while the moving average is undefined
                if verbose > 0:
                    print("Reached convergence at {}, {} < {}".format(loss, delta, conv_tol))
                if checkpoint:
                    model.load_state_dict(best_model)
                return i
    if checkpoint:
        model.load_state_dict(best_model)
    return max_iter


def _save_state_dict(model):
    """training_routines.py:37-44: torch.save(state_dict) to <model_base_path>/models/model_state_dict_<hash>.pkl.
    The base path comes from the environment (RPGP_MODEL_BASE_PATH) instead of a user-made config.py; without it
    nothing is written and '' is returned.  Same file name and `torch.save(state_dict)` format as the reference, but the
    KEY LAYOUT IS THIS PACKAGE'S OWN (e.g. `likelihood.raw_noise` where GPyTorch has `likelihood.noise_covar.raw_noise`,
    float64 `weight` / `inner_lengthscale` buffers of the additive base kernel, no frozen inner RBF parameters): the
    checkpoints reload into rpgp_amd models, they are not interchangeable with GPyTorch state dicts."""
    base = os.environ.get("RPGP_MODEL_BASE_PATH")
    if not base:
        return ""
    # RPGP_STATE_DICT_LAYOUT=gpytorch writes the reference's key layout (gpytorch_state_dict above, [GPT-mem])
    d = gpytorch_state_dict(model) if os.environ.get("RPGP_STATE_DICT_LAYOUT", "") == "gpytorch" else model.state_dict()
    fname = "model_state_dict_{}.pkl".format(hash(str(d)))
    os.makedirs(os.path.join(base, "models"), exist_ok=True)
    torch.save(d, os.path.join(base, "models", fname))
    return fname


# ---- GPyTorch-layout checkpoints -------------------------------------------------------------------------------------
# [GPT-mem] (GPyTorch 1.0 - 1.2, from memory; unverifiable in this image): the reference's checkpoints
# (training_routines.py:37-44) are `model.state_dict()` of a GPyTorch ExactGP, whose keys for the `additive_rp` model are
#     likelihood.noise_covar.raw_noise                                   (1,)      <->  likelihood.raw_noise
#     mean_module.constant                                               (1,)      <->  mean_module.constant
#     covar_module.raw_outputscale                                       ()        <->  covar_module.raw_outputscale
#     covar_module.base_kernel.raw_lengthscale                           (1, ard)  <->  covar_module.base_kernel.raw_lengthscale
#     covar_module.base_kernel.projection_module.weight                  (J k, d)  <->  ...projection_module.weight
#     covar_module.base_kernel.base_kernel.base_kernel.raw_outputscale   ()        frozen inner ScaleKernel: softplus^-1(weight)
#     covar_module.base_kernel.base_kernel.base_kernel.base_kernel.raw_lengthscale (1, 1)   frozen inner RBF: softplus^-1(l_b)
# (batch `AdditiveStructureKernel(ScaleKernel(RBFKernel))`, training_routines.py:148-159; the memory-efficient GAM kernel has
# `covar_module.base_kernel.base_kernel.raw_lengthscale` on both sides).  The two functions translate between that layout and
# this package's own for the flagship structure; prior buffers are not translated.
_GPY_INNER_OS = "covar_module.base_kernel.base_kernel.base_kernel.raw_outputscale"
_GPY_INNER_LS = "covar_module.base_kernel.base_kernel.base_kernel.base_kernel.raw_lengthscale"


def gpytorch_state_dict(model):
    """`model.state_dict()` re-keyed to the GPyTorch layout above (flagship `additive_rp` structure).

    The layout is written from memory ([GPT-mem]) and carries the PARAMETERS only: GPyTorch modules also register
    their prior and constraint buffers (`...raw_noise_constraint.lower_bound`, `...noise_prior.a`, ...), which are not
    emitted here — load the result on the GPyTorch side with `model.load_state_dict(state, strict=False)`."""
    from .kernels import inv_softplus
    out = {}
    for k, v in model.state_dict().items():
        if k == "likelihood.raw_noise":
            out["likelihood.noise_covar.raw_noise"] = v
        elif k == "covar_module.base_kernel.base_kernel.weight":
            out[_GPY_INNER_OS] = inv_softplus(v.double()).to(torch.float32).reshape(())
        elif k == "covar_module.base_kernel.base_kernel.inner_lengthscale":
            out[_GPY_INNER_LS] = inv_softplus(v.double()).to(torch.float32).reshape(1, 1)
        else:
            out[k] = v
    return out


def load_gpytorch_state_dict(model, state):
    """Load a GPyTorch-layout state dict (see above) into an rpgp_amd model of the same structure; prior / unknown keys are
    ignored, the frozen inner-kernel entries are checked against the model's constants."""
    own = model.state_dict()
    mapped = {}
    for k, v in state.items():
        if k == "likelihood.noise_covar.raw_noise":
            mapped["likelihood.raw_noise"] = v.reshape(own["likelihood.raw_noise"].shape)
        elif k == _GPY_INNER_OS:
            w = torch.nn.functional.softplus(v.double()).reshape(())
            if "covar_module.base_kernel.base_kernel.weight" in own and \
                    abs(float(w) - float(own["covar_module.base_kernel.base_kernel.weight"])) > 1e-5:
                raise ValueError("inner outputscale %g differs from the model's 1/J weight" % float(w))
        elif k == _GPY_INNER_LS:
            continue
        elif k in own:
            mapped[k] = v.reshape(own[k].shape)
    missing = [k for k in own if k not in mapped and not k.endswith((".weight", ".inner_lengthscale")) or
               (k.endswith("projection_module.weight") and k not in mapped)]
    if missing:
        raise KeyError("state dict lacks %s" % missing)
    model.load_state_dict({**own, **mapped})
    return model


def locality_order(X, bits=10):
    """Row permutation that makes neighbours in input space neighbours in memory: Morton (Z-order) code of the first
    min(d, 3) principal coordinates of X, `bits` bits each (a rotation for d <= 3, i.e. for the J = d projections of the
    reference's `additive_spread_prescale_Jd_ski.json`).  Why: the cell-sorted SKI scatter (csrc/rpgp_ski.hip) walks every
    projection's points in grid-cell order and reads their right-hand-side rows; with the rows in file order those are
    random 44-byte reads of a 17 MB array at N = 391 386 (measured: 93 MB fetched for 52 MB useful); in Morton order the
    points of a cell come from a few contiguous row ranges.  A GP's training set is a set: nothing else depends on the order.
    Deterministic (ties broken by the original index)."""
    Xd = X.detach().double().cpu()
    Xc = Xd - Xd.mean(0, keepdim=True)
    k = min(Xd.shape[1], 3)
    if Xd.shape[1] > 1:
        evals, evecs = torch.linalg.eigh(Xc.t() @ Xc)
        Y = Xc @ evecs[:, -k:]
    else:
        Y = Xc
    lo, hi = Y.min(0).values, Y.max(0).values
    q = ((Y - lo) / (hi - lo).clamp_min(1e-300) * ((1 << bits) - 1)).round().to(torch.int64).clamp_(0, (1 << bits) - 1)
    code = torch.zeros(Xd.shape[0], dtype=torch.int64)
    for b in range(bits):
        for c in range(k):
            code |= ((q[:, c] >> b) & 1) << (b * k + c)
    return torch.argsort(code, stable=True)


def _check_double_supported(kind, model_kwargs):
    """`--double` (training_routines.py:481): float64 parity kernels serve the RBF hot path (rpgp_f64.hip), every member of the
    generalised family (rpgp_family_generic.hip) and the grid-interpolation operator (rpgp_ski_f64.hip) — the latter also
    row-sharded over a process group (round 6: the float64 stages as separate calls, the torch CG loop with all-reduced inner
    products; the native executor is float32).  Nothing on this path is refused any more."""
    return None


class _ExactGPFactory:
    """Builds (model, likelihood, mll) on the output device; under a process group every rank starts from rank 0's
    parameters (projection draw, lengthscale / noise initialisation)."""

    def __init__(self, trainX, trainY, kind, model_kwargs, devices, output_device, dtype):
        self.args = (trainX, trainY, kind)
        self.model_kwargs, self.devices, self.output_device, self.dtype = model_kwargs, devices, output_device, dtype

    def __call__(self):
        trainX, trainY, kind = self.args
        model, likelihood = create_exact_gp(trainX, trainY, kind, devices=self.devices, **self.model_kwargs)
        model = model.to(self.output_device, self.dtype)
        if is_distributed():
            # (after the move to the output device: RCCL ("nccl") has no backend for CPU tensors)
            for t in list(model.parameters()) + list(model.buffers()):
                dist.broadcast(t.data, src=0)
        return model, likelihood, ExactMarginalLogLikelihood(likelihood, model)


def _best_of_restarts(factory, trainX, trainY, optimizer_, n_restarts, restart_kwargs):
    """`random_restarts` short fits from fresh initialisations; the one with the lowest negative MLL is trained on
    (training_routines.py:507-528)."""
    best, best_loss = None, np.inf
    for _ in range(n_restarts):
        candidate = factory()
        model, _, mll = candidate
        train_to_convergence(model, trainX, trainY, optimizer=optimizer_, objective=mll, isloss=False, **restart_kwargs)
        model.train()
        with torch.no_grad():
            loss = -mll(model(trainX), trainY).item()
        if best is None or loss < best_loss:
            best, best_loss = candidate, loss
    return best


def _evaluate_exact_gp(model, likelihood, mll, trainX, trainY, testX, testY, skip_posterior_variances, evaluate_on_train,
                       record_pred_unc):
    """The metric block of training_routines.py:543-583: prior train NMLL (train mode), then posterior quantities in eval
    mode — train MSE / NLL when `evaluate_on_train`, test NLL, fraction of targets inside the +-2 sigma region, z-scores."""
    from . import settings
    metrics, test_warnings = {}, []
    with torch.no_grad():
        model.train()
        likelihood.train()
        metrics["prior_train_nmll"] = -mll(model(trainX), trainY).item()
        with settings.skip_posterior_variances(skip_posterior_variances):
            model.eval()
            likelihood.eval()
            train_outputs = model(trainX) if evaluate_on_train else None
            if evaluate_on_train:
                metrics["train_mse"] = mean_squared_error(train_outputs.mean, trainY)
            with warnings.catch_warnings(record=True) as test_warnings:
                warnings.simplefilter("always")
                test_outputs = model(testX)
                pred_mean = test_outputs.mean
            if not skip_posterior_variances:
                if evaluate_on_train:
                    metrics["train_nll"] = -mll(train_outputs, trainY).item()
                metrics["test_nll"] = -mll(test_outputs, testY).item()
                noisy = likelihood(test_outputs)
                lower, upper = noisy.confidence_region()
                metrics["test_pred_frac_in_cr"] = ((testY > lower) * (testY < upper)).to(torch.float).mean().item()
                if record_pred_unc:
                    metrics["test_pred_z_score"] = (testY - noisy.mean) / noisy.stddev
    return metrics, pred_mean, test_warnings


def train_exact_gp(trainX, trainY, testX, testY, kind, model_kwargs, train_kwargs, devices=("cpu",),
                   skip_posterior_variances=False, skip_random_restart=False, evaluate_on_train=True,
                   output_device=None, record_pred_unc=False, double=False):
    """Create and train an exact GP with the given options (counterpart of training_routines.py:469-585: same arguments,
    same metric names, same return triple).  Returns (model_metrics, pred_mean [cpu float32], model).

    Row order: for grid-interpolation models (`ski: true`) with N >= 4096 the TRAINING rows are stored in a
    locality-preserving order (`locality_order`: Morton code of the leading principal coordinates) — the returned
    `model.train_inputs` / `model.train_targets` are that permutation of the caller's (trainX, trainY), kept on the model as
    `model.train_row_order` (a LongTensor `order` with `model.train_inputs == trainX[order]`; None when the rows were not
    reordered).  `pred_mean` and every metric refer to the TEST rows, whose order is the caller's; a GP's posterior does
    not depend on the order of its training rows."""
    model_kwargs, train_kwargs = copy.copy(model_kwargs), copy.copy(train_kwargs)
    if double:
        _check_double_supported(kind, model_kwargs)
    dtype = torch.double if double else torch.float
    devices = [torch.device(dev) for dev in devices]
    output_device = devices[0] if output_device is None else torch.device(output_device)
    order = None
    if model_kwargs.get("ski", False) and trainX.shape[0] >= 4096:
        # grid-interpolation kernels: store the training set in a locality-preserving row order (see locality_order)
        order = locality_order(trainX)
        trainX, trainY = trainX[order.to(trainX.device)], trainY[order.to(trainY.device)]
    trainX, trainY, testX, testY = (t.to(output_device, dtype).contiguous() for t in (trainX, trainY, testX, testY))
    n_features = trainX.shape[-1]
    model_kwargs = {k: (n_features if isinstance(v, str) and v == "d" else v) for k, v in model_kwargs.items()}

    n_restarts = train_kwargs.pop("random_restarts", 1)
    restart_iters = train_kwargs.pop("init_iters", 20)
    optimizer_ = _map_to_optim(train_kwargs.pop("optimizer"))
    restart_check_conv = train_kwargs.pop("rr_check_conv", False)
    restart_kwargs = dict(train_kwargs, max_iter=restart_iters, check_conv=restart_check_conv)

    from . import lowrank_mll, settings
    served0 = lowrank_mll.served_counts()
    factory = _ExactGPFactory(trainX, trainY, kind, model_kwargs, devices, output_device, dtype)
    if skip_random_restart:
        model, likelihood, mll = factory()
    else:
        model, likelihood, mll = _best_of_restarts(factory, trainX, trainY, optimizer_, n_restarts, restart_kwargs)

    with warnings.catch_warnings(record=True) as fit_warnings:
        warnings.simplefilter("always")
        trained_epochs = train_to_convergence(model, trainX, trainY, optimizer=optimizer_, objective=mll, isloss=False,
                                              **train_kwargs)
    model.eval()
    likelihood.eval()
    mll.eval()
    model_metrics = {"trained_epochs": trained_epochs}
    if settings.lowrank_mll.on():
        # the share of the fit's objective evaluations that ran in the closed-form features mode
        served, decided = (b - a for a, b in zip(served0, lowrank_mll.served_counts()))
        model_metrics["lowrank_mll_share"] = served / decided if decided else 0.0
    evaluated, pred_mean, test_warnings = _evaluate_exact_gp(model, likelihood, mll, trainX, trainY, testX, testY,
                                                             skip_posterior_variances, evaluate_on_train, record_pred_unc)
    model_metrics.update(evaluated)
    if settings.lowrank_posterior.on():
        st = getattr(model, "prediction_strategy", None)
        model_metrics["lowrank_posterior_served"] = int(getattr(st, "lowrank", None) is not None)
    if settings.ski_posterior.on():
        st = getattr(model, "prediction_strategy", None)
        model_metrics["ski_posterior_served"] = int(getattr(st, "ski_post", None) is not None)
    model_metrics["training_warnings"] = len(fit_warnings)
    model_metrics["testing_warning"] = "" if len(test_warnings) == 0 else test_warnings[-1].message
    model_metrics["state_dict_file"] = _save_state_dict(model)
    model.train_row_order = None if order is None else order.to("cpu")
    return model_metrics, pred_mean.to("cpu", torch.float), model


class ModelAverage:
    """Mixture of the predictive distributions of several fitted models, weighted by their marginal likelihoods — what
    `train_exact_gp_model_average` (training_routines.py:631-676) builds through `fitting.sampling.ModelAverage`.  That module
    is NOT part of the reference checkout, so this class follows the call sites only (`ModelAverage(predictions, log_mlls)`,
    `.mean()`, `.sample_mean()`, `.log_prob(y)`) with the textbook meaning — **unpinned**:
      weights w_i = softmax(log_mlls)          (the routine passes -prior_train_nmll, i.e. the per-datum MLL of each fit)
      mean()        = sum_i w_i mu_i           (the mixture's mean)
      sample_mean() = (1/M) sum_i mu_i         (the unweighted average over the fitted models)
      log_prob(y)   = logsumexp_i(log w_i + log N(y; mu_i, Sigma_i))."""

    def __init__(self, predictions, log_mlls):
        if len(predictions) == 0 or len(predictions) != len(log_mlls):
            raise ValueError("one log marginal likelihood per prediction is required")
        self.predictions = list(predictions)
        lm = torch.as_tensor([float(v) for v in log_mlls], dtype=torch.float64)
        self.log_weights = lm - torch.logsumexp(lm, dim=0)

    @property
    def weights(self):
        return self.log_weights.exp()

    def mean(self):
        w = self.weights
        out = None
        for wi, pr in zip(w, self.predictions):
            term = pr.mean * float(wi)
            out = term if out is None else out + term
        return out

    def sample_mean(self):
        return sum(pr.mean for pr in self.predictions) / len(self.predictions)

    def log_prob(self, value):
        lps = torch.stack([pr.log_prob(value).double().cpu() for pr in self.predictions])
        return torch.logsumexp(self.log_weights + lps, dim=0)


def train_exact_gp_model_average(trainX, trainY, testX, testY, kind, model_kwargs, train_kwargs, devices=("cpu",),
                                 skip_posterior_variances=False, evaluate_on_train=True, output_device=None,
                                 record_pred_unc=False, **fit_options):
    """training_routines.py:631-676 (model_specs/ma_dpa_gp_ard.json): fit one exact GP per value of the varying parameters
    (lists of equal length under `model_kwargs["varying_params"]`, e.g. J = 1, 2, 3, 5, ...), each without random restarts,
    and average their test predictions with marginal-likelihood weights.  Returns (metrics, mean, None)."""
    from . import settings
    model_kwargs = copy.deepcopy(model_kwargs)
    train_kwargs = copy.deepcopy(train_kwargs)
    if len(devices) > 1:
        raise ValueError("CGP not implemented for multi GPUs (yet?)")
    varying_params = model_kwargs.pop("varying_params")
    first = list(varying_params.keys())[0]
    predictions, log_mlls = [], []
    dev = torch.device(output_device if output_device is not None else devices[0])
    for i in range(len(varying_params[first])):
        for key, values in varying_params.items():
            model_kwargs[key] = values[i]
        metrics, _, model = train_exact_gp(trainX, trainY, testX, testY, kind, copy.deepcopy(model_kwargs),
                                           copy.deepcopy(train_kwargs), devices=devices,
                                           skip_posterior_variances=skip_posterior_variances, skip_random_restart=True,
                                           evaluate_on_train=False, output_device=output_device, **fit_options)
        log_mlls.append(-metrics["prior_train_nmll"])
        model.eval()
        model.likelihood.eval()
        with torch.no_grad(), settings.skip_posterior_variances(skip_posterior_variances):
            tx = testX.to(dev, next(model.parameters()).dtype).contiguous()
            # The reference appends the LATENT predictive `model(testX)` and scores the noisy targets under it; for a small J
            # that covariance is numerically singular and the density meaningless (3e5 nats on a kin8nm-shaped problem).
            # The averaged components here are the predictive distributions of the TARGETS (likelihood noise included),
            # the quantity `train_exact_gp` reports as test_nll; the means are the same.
            predictions.append(model.likelihood(model(tx)))
    test_outputs = ModelAverage(predictions, log_mlls)
    testY = testY.to(predictions[0].mean)
    model_metrics = dict()
    with torch.no_grad():
        if not skip_posterior_variances:
            model_metrics["test_nll"] = -test_outputs.log_prob(testY).item()
        model_metrics["sampled_mean_mse"] = mean_squared_error(test_outputs.sample_mean(), testY)
        model_metrics["normal_mean_mse"] = mean_squared_error(test_outputs.mean(), testY)
    return model_metrics, test_outputs.mean().to("cpu"), None
