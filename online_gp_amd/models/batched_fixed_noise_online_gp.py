"""FixedNoiseOnlineSKIGP -- the WISKI model core, MI355X-native.

Host-side mirror of the reference's
online_gp/models/batched_fixed_noise_online_gp.py (same constructor, methods,
cache keys and output shapes) with the arithmetic moved to the HIP kernels of
libwiski_hip.so:

  reference (dense torch/gpytorch)                    here
  ------------------------------------------------    ---------------------------------------------
  W^T densified m x n            (:22-28)             never formed; taps recomputed from x in-kernel
  W^T D^-1 W dense m x m         (:50-53, URLT:58)    block stencil [7^d, m], atomically scattered
  root L, Q = I + L^T Kuu L, chol(Q)   (:343-383)     preconditioned CG in inducing space (wiski_pcg)
  pred_cov dense m x m           (:385-404)           lazy operator M = (Kt^-1 + A)^-1
  left_interp / W* pred_cov W*^T (:206-228)           fused gather kernels

The posterior it returns is the exact one, mean = w*^T (Kt^-1+A)^-1 b and
cov = sigma2 W* (Kt^-1+A)^-1 W*^T, to the CG tolerance.
"""
import math

import torch

from .. import grid_ops, settings
from ..distributions import MultivariateNormal, ZeroLazyTensor, DenseLazyTensor
from ..kernels import GridInterpolationKernel, RBFKernel, ScaleKernel
from ..lazy.operators import (InducingPosterior, InterpolatedKernel, KroneckerToeplitz, PredictiveCovariance, with_input_grad)
from ..lazy.dense_woodbury import DenseInducingPosterior
from ..likelihoods import FNMGLikelihood
from . import kernel_cache as kc
from .kernel_cache import BatchOperator, _wtw_ops
from .step_pacing import PollPacing, basis_kept, basis_slow, density_profiles, profiles_moved


def _default_tol(dtype):
    v = settings.cg_tolerance.value()
    if v is not None:
        return v
    return 1e-6 if dtype == torch.float32 else 1e-10


def interval_from_labels(labels):
    """(lower, upper) of binary labels for the probit use of interval observations: a label in {0, 1} or {-1, +1}
    says f(x) + eps > 0 (positive) or < 0, eps of unit noise -- a one-sided interval at 0.  Pass them to
    ``condition_on_observations(X, None, noise=torch.ones(n), lower=lower, upper=upper)``."""
    labels = torch.as_tensor(labels)
    pos = labels > 0
    dtype = labels.dtype if labels.is_floating_point() else torch.get_default_dtype()
    zero = torch.zeros(labels.shape, dtype=dtype, device=labels.device)
    return torch.where(pos, zero, zero - float("inf")), torch.where(pos, zero + float("inf"), zero)


def monotone_bounds(n, d, dims, sign=+1):
    """(grad_lower, grad_upper [n, d] float64, grad_mask bool [n, d]) of "f increases (``sign`` < 0: decreases) in the dims ``dims``"
    (an int or a sequence), for ``condition_on_observations(..., grad_lower=, grad_upper=, grad_mask=)``: the partials of those dims
    are bounded by 0 from below (above), the other dims are not observed."""
    dims = [int(dims)] if isinstance(dims, int) else [int(q) for q in dims]
    if sign == 0 or any(not 0 <= q < d for q in dims):
        raise ValueError(f"monotone_bounds: dims must lie in 0..{d - 1} and sign must not be 0, got {dims}, {sign}")
    inf = float("inf")
    lo, hi = torch.full((n, d), -inf, dtype=torch.float64), torch.full((n, d), inf, dtype=torch.float64)
    mask = torch.zeros((n, d), dtype=torch.bool)
    mask[:, dims] = True
    (lo if sign > 0 else hi)[:, dims] = 0.0
    return lo, hi, mask


class FixedNoiseOnlineSKIGP(torch.nn.Module):
    def __init__(
        self,
        train_inputs=None,
        train_targets=None,
        train_noise_term=None,
        covar_module=None,
        kernel_cache=None,
        grid_bounds=None,
        grid_size=30,
        likelihood=None,
        learn_additional_noise=False,
        num_data=None,
        num_path_probes=0,
        path_seed=0,
        forgetting_factor=None,
        grow_grid=False,
        max_grid_size=None,
        robust_c=None,
        robust_scale="noise",
        window=None,
        window_rebuild_every=None,
        trend=None,
        trend_prior_var=None,
        input_var=None,
        input_noise_slope="posterior",
        heteroscedastic=False,
        noise_kernel=None,
        log_noise_mean=0.0,
        noise_model=None,
        site_memory=None,
        site_refine_sweeps=0,
        site_refine_damping=1.0,
    ):
        super().__init__()
        object.__setattr__(self, "noise_model", None)    # (set at the end: the initial data is absorbed plainly)
        assert train_inputs is not None or kernel_cache is not None
        # following the stream (grow_to_cover_): every update first grows the grid by whole nodes until its batch is interior
        self.grow_grid = bool(grow_grid)
        self.max_grid_size = max_grid_size
        # exponential forgetting (forget_): every update scales the statistics by this factor before it absorbs its batch
        if forgetting_factor is not None:
            forgetting_factor = float(forgetting_factor)
            if not (0.0 < forgetting_factor <= 1.0):
                raise ValueError(f"forgetting_factor must lie in (0, 1], got {forgetting_factor}")
        self.forgetting_factor = forgetting_factor
        # outlier-robust streaming (_absorb_robust): every streamed batch is Huber-weighted at this threshold against
        # the posterior before it.  None: every path is what it is without the feature
        if robust_c is not None:
            robust_c = float(robust_c)
            if not (robust_c > 0.0 and math.isfinite(robust_c)):
                raise ValueError(f"robust_c must be a finite positive number, got {robust_c}")
        if robust_scale not in ("noise", "predictive"):
            raise ValueError(f"robust_scale must be 'noise' or 'predictive', got {robust_scale!r}")
        self.robust_c = robust_c
        self.robust_scale = robust_scale
        self.last_robust_weights = None              # omega [q] of the last robustly absorbed batch, on the device
        # interval observations (_absorb_interval): (ytilde, omega, log_z) [q] of the last batch given as bounds
        self.last_interval_sites = None
        # interval observations of gradients (_absorb_grad_interval): (ytilde, omega, log_z) [q, d + 1] of the last such batch
        self.last_grad_interval_sites = None
        # count observations (_absorb_count): (ytilde, omega, log_z) [q] of the last batch given as counts
        self.last_count_sites = None
        # categorical observations (_absorb_labels): (ytilde [C, q], omega [C, q], log_z [q]) of the last batch of labels
        self.last_label_sites = None
        # noisy-input observations (_absorb_input_noise): the variance of the error of the recorded locations -- a scalar
        # or [d] -- that every unbatched update not given its own `input_var` is absorbed with; None: every path is what it is without
        # the feature.  input_noise_slope: the noise of a point is inflated by input_var E[(d f)^2] under the posterior before its batch
        # ("posterior": squared mean slope plus slope variance) or by the squared slope of the posterior mean alone ("mean", the textbook
        # rule, which lets the first batches of a stream in at almost no extra noise)
        if input_noise_slope not in ("posterior", "mean"):
            raise ValueError(f"input_noise_slope must be 'posterior' or 'mean', got {input_noise_slope!r}")
        if input_var is not None:
            input_var = torch.as_tensor(input_var, dtype=torch.float64).detach().cpu()
            if input_var.dim() > 1 or not bool((input_var >= 0).all()) or not bool(torch.isfinite(input_var).all()):
                raise ValueError("input_var of a model must be a finite non-negative scalar or one value per input dimension [d] "
                                 "(a batch passes its own [n] or [n, d] to condition_on_observations)")
        self.input_var = input_var
        self.input_noise_slope = input_noise_slope
        self.last_input_noise_sites = None           # (omega, log_z, grad_mean) of the last batch absorbed with an input variance
        # sliding window (_absorb_window): the model is the GP of exactly the last `window` points; every update absorbs
        # its batch, stores it in a device-resident ring and takes out what the ring's slots held, in one launch
        if window is not None:
            if isinstance(window, bool) or int(window) != window or int(window) < 1:
                raise ValueError(f"window must be an integer >= 1, got {window!r}")
            window = int(window)
            if forgetting_factor is not None:
                raise NotImplementedError("window and forgetting_factor are alternatives: a hard window lets a point go after `window` points, "
                                          "forgetting inflates its noise for ever -- build the model with one of them")
            if robust_c is not None:
                raise NotImplementedError("window does not combine with robust_c: the ring stores the weights a point entered with, and no "
                                          "kernel both weighs and retires in one launch")
        if window_rebuild_every is not None:
            if window is None:
                raise ValueError("window_rebuild_every needs window")
            if isinstance(window_rebuild_every, bool) or int(window_rebuild_every) != window_rebuild_every or int(window_rebuild_every) < 1:
                raise ValueError(f"window_rebuild_every must be an integer >= 1, got {window_rebuild_every!r}")
            window_rebuild_every = int(window_rebuild_every)
        self.window = window
        self.window_rebuild_every = window_rebuild_every
        self._win_voids = 0                          # void slots of the ring, as far as check_bounds() has been told
        self._win_updates = 0
        # site memory (refine_sites_): the last `site_memory` interval and count observations are kept, with their sites,
        # in a device-resident ring, and expectation-propagation sweeps re-match them against their cavities; site_refine_sweeps of them
        # follow every interval or count update.  None: every path is what it is without the feature
        if site_memory is not None:
            if isinstance(site_memory, bool) or int(site_memory) != site_memory or int(site_memory) < 1:
                raise ValueError(f"site_memory must be an integer >= 1, got {site_memory!r}")
            site_memory = int(site_memory)
            if forgetting_factor is not None:
                raise NotImplementedError("site_memory does not combine with forgetting_factor: a decayed site is no longer the stored one, "
                                          "and a sweep would take out more than is still in the statistics")
            if window is not None:
                raise NotImplementedError("site_memory does not combine with window: the window's ring stores targets, and the moment-matched "
                                          "forms do not pass through it")
            if robust_c is not None:
                raise NotImplementedError("site_memory does not combine with robust_c: a site is a weight already, and no kernel applies both")
            if trend is not None or (kernel_cache is not None and "trend_C" in kernel_cache):
                raise NotImplementedError("site_memory does not combine with a trend: a site is matched against the grid mean alone, which "
                                          "under a trend is not the predictive mean")
            if heteroscedastic or noise_model is not None:
                raise NotImplementedError("site_memory does not combine with heteroscedastic: the ring stores the sites of one model, and a "
                                          "noise site moves with the f site it was deflated by")
            if int(num_path_probes) > 0 or (kernel_cache is not None and "path_probes" in kernel_cache):
                raise NotImplementedError("site_memory does not combine with path probes (num_path_probes > 0): a probe increment is random "
                                          "and cannot follow a site whose weight shrinks")
        if isinstance(site_refine_sweeps, bool) or int(site_refine_sweeps) != site_refine_sweeps or int(site_refine_sweeps) < 0:
            raise ValueError(f"site_refine_sweeps must be an integer >= 0, got {site_refine_sweeps!r}")
        site_refine_damping = float(site_refine_damping)
        if not (0.0 <= site_refine_damping <= 1.0):
            raise ValueError(f"site_refine_damping must lie in [0, 1], got {site_refine_damping}")
        if site_memory is None and (int(site_refine_sweeps) != 0 or site_refine_damping != 1.0):
            raise ValueError("site_refine_sweeps / site_refine_damping describe the sweeps of site_memory, which was not given")
        self.site_memory = site_memory
        self.site_refine_sweeps = int(site_refine_sweeps)
        self.site_refine_damping = site_refine_damping
        self.last_refined_sites = None               # (ytilde, omega, log_z) over the filled slots, oldest first, after the last sweep

        if train_targets is not None:
            if train_targets.dim() == 1:
                train_targets = train_targets[:, None]
            num_outputs = train_targets.shape[-1]
            self.num_data = train_inputs.shape[-2]
            device, dtype = train_inputs.device, train_inputs.dtype
            num_dims = train_inputs.shape[-1]
        else:
            ic = kernel_cache["interpolation_cache"]
            num_outputs = ic.shape[0]
            self.num_data = num_data
            device, dtype = ic.device, ic.dtype
            num_dims = None
        self.num_outputs = num_outputs
        if robust_c is not None and num_outputs > 1:
            raise NotImplementedError("robust_c is implemented for a single output (the robust absorb weights one target per point)")
        if window is not None and num_outputs > 1:
            raise NotImplementedError("window is implemented for a single output (the ring stores one target per point)")
        if site_memory is not None and num_outputs > 1:
            raise NotImplementedError("site_memory is implemented for a single output (the interval and count forms it stores are)")
        if window is not None and (int(num_path_probes) > 0 or (kernel_cache is not None and "path_probes" in kernel_cache)):
            raise NotImplementedError("window does not combine with path probes (num_path_probes > 0): a probe increment is random and "
                                      "cannot be taken out again from the ring")
        _batch_shape = torch.Size([num_outputs]) if num_outputs > 1 else torch.Size()
        # probe vectors of the posterior sample paths (sample_paths): S of them, rounded up to even (the generator
        # makes Box-Muller pairs); they live in the kernel cache beside b and follow it through every hand-over
        num_path_probes = int(num_path_probes) + (int(num_path_probes) & 1)
        if kernel_cache is not None and num_path_probes > 0 and "path_probes" not in kernel_cache:
            raise ValueError("num_path_probes > 0, but the kernel cache handed over carries no path probes: they can only be accumulated "
                             "while the points stream by (build the first model of the chain from data with num_path_probes)")
        if kernel_cache is not None and num_path_probes > 0 and kernel_cache["path_probes"].shape[1] != num_path_probes:
            raise ValueError(f"num_path_probes={num_path_probes}, but the kernel cache handed over carries {kernel_cache['path_probes'].shape[1]} "
                             "probes (their number is fixed when the first model of the chain is built; num_path_probes=0 takes the cache's)")
        if num_path_probes > 0 and num_outputs > 1:
            raise NotImplementedError("path probes (num_path_probes > 0) are implemented for a single output")
        self._path_probes_init = (num_path_probes, int(path_seed))
        # polynomial trend with marginalised coefficients: y = h(x)^T beta + f(x) + eps, beta ~ N(0, trend_prior_var I)
        # (None: the flat prior).  Its statistics C, G, g live in the kernel cache beside b and follow it through every hand-over; the
        # degree is fixed when the first model of a chain is built.  None: every path is what it is without the feature
        if trend is not None and trend not in grid_ops.TREND_DEGREES:
            raise ValueError(f"trend must be None, 'constant', 'linear' or 'quadratic', got {trend!r}")
        if trend_prior_var is not None:
            trend_prior_var = float(trend_prior_var)
            if not (trend_prior_var > 0.0 and math.isfinite(trend_prior_var)):
                raise ValueError(f"trend_prior_var must be a finite positive number or None (the flat prior), got {trend_prior_var}")
        deg = None if trend is None else grid_ops.TREND_DEGREES[trend]
        if kernel_cache is not None and "trend_C" in kernel_cache:
            if deg is not None and deg != kernel_cache["trend_deg"]:
                raise ValueError(f"trend={trend!r}, but the kernel cache handed over carries the statistics of a trend of degree "
                                 f"{kernel_cache['trend_deg']} (the degree is fixed when the first model of the chain is built; trend=None takes the cache's)")
            deg = kernel_cache["trend_deg"]
        elif kernel_cache is not None and deg is not None:
            raise ValueError(f"trend={trend!r}, but the kernel cache handed over carries no trend statistics: they can only be accumulated "
                             "while the points stream by (build the first model of the chain from data with trend)")
        if deg is None and trend_prior_var is not None:
            raise ValueError("trend_prior_var needs trend")
        if deg is not None:
            if num_outputs > 1:
                raise NotImplementedError("trend is implemented for a single output (one coefficient vector, one set of p solve columns)")
            if robust_c is not None:
                raise NotImplementedError("trend does not combine with robust_c: the Huber weights are taken against the grid mean alone, "
                                          "which under a trend is not the predictive mean")
            if window is not None:
                raise NotImplementedError("trend does not combine with window: the ring's kernel takes a point out of A and b only, "
                                          "and the trend statistics would keep it")
            if num_path_probes > 0 or (kernel_cache is not None and "path_probes" in kernel_cache):
                raise NotImplementedError("trend does not combine with path probes (num_path_probes > 0): a sample path would need a "
                                          "joint draw of the coefficients, which sample_paths does not make")
        self._trend_deg = deg
        self.trend_prior_var = trend_prior_var

        if covar_module is None:
            if grid_bounds is None:
                grid_bounds = torch.stack((train_inputs.min(dim=-2)[0] - 0.1, train_inputs.max(dim=-2)[0] + 0.1)).transpose(-1, -2)
            covar_module = ScaleKernel(RBFKernel(batch_shape=_batch_shape, ard_num_dims=train_inputs.size(-1)), batch_shape=_batch_shape)
        if not isinstance(covar_module, GridInterpolationKernel):
            covar_module = GridInterpolationKernel(base_kernel=covar_module, grid_size=grid_size, num_dims=train_inputs.shape[-1],
                                                   grid_bounds=grid_bounds)
        self._batch_shape = _batch_shape
        self.train_inputs = [None]
        self.train_targets = None
        self.covar_module = covar_module.to(device)
        self._grid = self.covar_module.grid_spec
        if self.input_var is not None and self.input_var.dim() == 1 and self.input_var.shape[0] != self._grid.d:
            raise ValueError(f"input_var of a model must be a scalar or one value per input dimension [{self._grid.d}], got {tuple(self.input_var.shape)}")
        self._dtype = dtype
        self._device = device
        if num_dims is not None and num_dims != self._grid.d:
            raise RuntimeError(f"inputs have {num_dims} dims but the grid has {self._grid.d}")

        if likelihood is None:
            if train_noise_term is None:
                train_noise_term = torch.ones_like(train_targets)
            train_noise_term = self._canon_noise(train_noise_term, train_targets)
            self.likelihood = FNMGLikelihood(noise=train_noise_term.transpose(-1, -2), learn_additional_noise=learn_additional_noise,
                                             batch_shape=_batch_shape).to(device)
        else:
            self.likelihood = likelihood
            if train_noise_term is not None and train_targets is not None:
                train_noise_term = self._canon_noise(train_noise_term, train_targets)
        self.has_learnable_noise = learn_additional_noise

        self._err = grid_ops.new_err_flag(device)
        # sum_p 1/noise_p per output: host part (unit-noise updates, exact) + device part (explicit noise tensors)
        self._wsum_host = [0.0] * num_outputs
        self._wsum_dev = torch.zeros(num_outputs, dtype=torch.float64, device=device)
        self._wsum_dev_host = [0.0] * num_outputs
        self._wsum_dirty = False
        self._pcg_ws = grid_ops.PCGWorkspace()
        self._memo = {}
        self._mean_state = None  # warm-start state of the posterior-mean solve
        # the streaming step's own state, None while idle
        self._last_iters = None                      # CG iterations of the last mean solve, per output
        self._pending_step = None                    # the StreamStep whose deferred refresh is in flight (_finish_pending)
        self._stream_step_cache = None               # (key, prepared StreamStep) of _stream_fast_state
        self._profile_look = None                    # the density-profile look in flight (_density_profile_still_fits)
        self._profile_look_host = None               # its pinned host buffer, allocated once
        self._pacing = PollPacing(1e-7 if dtype == torch.float32 else 1e-11)     # where the mean solve polls first, refresh count

        if kernel_cache is None:
            self._kernel_cache = kc.fresh(self._grid, num_outputs, dtype, device, self._path_probes_init, self._trend_deg)
            if site_memory is not None:                  # (the initial data are values: they take their usual path and are not stored)
                self._kernel_cache["_site_ring"] = grid_ops.SiteRing(site_memory, self._grid.d, dtype, device)
            if window is not None:
                self._kernel_cache["_ring"] = grid_ops.WindowRing(window, self._grid.d, dtype, device)
                self._window_restart(train_inputs, train_targets, train_noise_term)
            else:
                self._absorb(self._kernel_cache, train_inputs, train_targets, train_noise_term, init=True)
        else:
            if site_memory is not None and (kernel_cache.get("_site_ring") is None or kernel_cache["_site_ring"].cap != site_memory):
                raise ValueError(f"site_memory={site_memory}, but the kernel cache handed over carries "
                                 + ("no site ring: statistics do not remember their points" if kernel_cache.get("_site_ring") is None
                                    else f"a site ring of {kernel_cache['_site_ring'].cap} slots"))
            if window is not None and (kernel_cache.get("_ring") is None or kernel_cache["_ring"].cap != window):
                raise ValueError(f"window={window}, but the kernel cache handed over carries "
                                 + ("no ring: statistics do not remember their points" if kernel_cache.get("_ring") is None
                                    else f"a ring of {kernel_cache['_ring'].cap} slots"))
            self._kernel_cache = kernel_cache
            facs = kernel_cache.get("_spectral")
            if facs:
                # the spectral factor(s) follow the statistics they describe (bayesopt.py:86-96 re-initialises the model from the
                # previous model's cache at every step: a factor kept on the model object would be rebuilt from the stencil each time)
                for fac in facs.values():
                    fac.err = self._err
                self.__dict__["_spectral"] = facs
            if "_cnt" in kernel_cache:
                # hand-over path (bayesopt.py:86-96): recover sum_p 1/noise_p from the row sums (rows of W sum to one)
                self._wsum_dev = kernel_cache["_cnt"].sum(dim=1, dtype=torch.float64)
                self._wsum_dirty = True
        # heteroscedastic streaming (_absorb_hetero): the noise of a point is sigma2 noise_p exp g(x_p), with g a second
        # single-output model on the SAME grid object -- `noise_model`, prior mean `log_noise_mean`, its kernel fixed by the caller --
        # learned from the stream's own residuals in the launch that absorbs the batch.  The initial data is absorbed plainly (at
        # multiplier 1).  None: every path is what it is without the feature.  The noise model is NOT a registered submodule: its
        # kernel's hyper-parameters are not among parameters() and no MLL step or zero_grad() touches them; state_dict() /
        # load_state_dict() do not carry them either (save model.noise_model.covar_module.state_dict() beside the model's); to(),
        # train() and eval() are passed on by hand.  `noise_model=` hands an existing noise model over instead of building one, as
        # `kernel_cache=` hands statistics over: it is how the functional form gives a sibling its clone, and it must be a single-output
        # model on this model's grid object
        self.log_noise_mean = float(log_noise_mean)
        self.last_hetero_sites = None                # (e, ytilde_g, tau_g, log_z_g, log_z_y) [q] of the last batch absorbed heteroscedastically
        if not math.isfinite(self.log_noise_mean):
            raise ValueError(f"log_noise_mean must be finite, got {log_noise_mean}")
        if noise_model is None and not heteroscedastic and (noise_kernel is not None or self.log_noise_mean != 0.0):
            raise ValueError("noise_kernel / log_noise_mean describe the noise model of heteroscedastic=True")
        if heteroscedastic or noise_model is not None:
            self._refuse_for_hetero_model()
            if noise_model is None:
                noise_model = self._new_noise_model(noise_kernel)
            if noise_model.num_outputs != 1 or noise_model._grid is not self._grid:
                raise ValueError("noise_model must be a single-output model on this model's grid object (build it on covar_module.grid_spec)")
        object.__setattr__(self, "noise_model", noise_model)

    # ------------------------------------------------------------ helpers --
    @staticmethod
    def _canon_noise(noise, targets):
        """-> [n, out] like the targets."""
        if noise.dim() == 1:
            noise = noise[:, None]
        if noise.shape != targets.shape and noise.transpose(-1, -2).shape == targets.shape:
            noise = noise.transpose(-1, -2)
        return noise.expand_as(targets) if noise.shape != targets.shape else noise

    def _clone_cache(self, cache):
        return kc.clone(cache, self._grid)

    def _stencil_pack(self, ops):
        return kc.stencil_pack(self._grid, ops)

    def _half_buffers(self):
        """Per-output symmetric half-stencil delta buffers [(R+1)/2, m] for the data-parallel
        path (rank-local increment -> all-reduce -> add; zero between uses)."""
        if getattr(self, "_half_delta", None) is None:
            H = (self._grid.R + 1) // 2
            self._half_delta = [torch.zeros((H, self._grid.m), dtype=self._dtype, device=self._device) for _ in range(self.num_outputs)]
        return self._half_delta

    def _absorb(self, cache, X, Y, noise, init, half_delta=None, res_delta=None):
        """_initialize_caches (:31-60) / _update_cache_dicts (:155-171) fused into
        one scatter launch per output; mutates `cache` in place.

        W^T D^-1 W accumulates straight into the symmetric half stencil (T(T+1)/2 atomics
        per point).  With `half_delta` given (data-parallel path) the increments go to those
        buffers instead, for the caller to all-reduce and add; `res_delta` ([out, m], zeroed) then receives this shard's
        innovation W^T (wb y - wa (W U)) of the carried residual, to be all-reduced and added to R alongside."""
        if "path_probes" in cache and half_delta is not None:
            raise NotImplementedError("path probes do not follow the data-parallel statistics exchange")
        if self.robust_c is not None and half_delta is not None:
            raise NotImplementedError("robust_c does not follow the data-parallel statistics exchange (half_delta): the Huber weights of a "
                                      "shard would be taken on one rank and the other ranks' followers never see them")
        if self.window is not None and half_delta is not None:
            raise NotImplementedError("window does not follow the data-parallel statistics exchange (half_delta): the ring of a replica "
                                      "would hold its own shard only, and what leaves must leave every replica")
        if self.site_memory is not None and half_delta is not None:
            raise NotImplementedError("site_memory does not follow the data-parallel statistics exchange (half_delta): the ring of a replica "
                                      "would hold its own shard only, and a sweep must move every replica's statistics")
        if self._trend_deg is not None and half_delta is not None:
            # (keyed on the model, as robust_c and window are: the updater absorbs into a delta dict of its own, which carries no trend entries)
            raise NotImplementedError("trend does not follow the data-parallel statistics exchange (half_delta): the deltas that are "
                                      "all-reduced carry A, b and cnt only, and C, G, g of the other ranks' points would never arrive")
        mine = self._before_launch(cache)            # the generic absorb writes every group
        X = X.reshape(-1, self._grid.d).to(self._device, self._dtype).contiguous()
        Y = Y.to(self._device, self._dtype)
        if Y.dim() == 1:
            Y = Y[:, None]
        n = X.shape[0]
        unit = noise is None            # unit noise (OnlineSKIRegression, OSR:25,122): no per-point weight tensors at all
        if not unit:
            noise = noise.to(self._device, self._dtype)
        b = cache["interpolation_cache"]
        stats = cache["_stats"]
        ops = _wtw_ops(cache["WtW"])
        dst = half_delta if half_delta is not None else [op.stencil for op in ops]
        # residual carry-over: while the posterior-mean state (U, Z, R = b - Z - A U) is current, the scatter
        # keeps R exact under the increment, and the next refresh starts without an A U product
        ms = self._mean_state
        if (mine or half_delta is not None) and self.num_outputs == 1:
            if half_delta is not None:
                # the increment arrives by all-reduce: other ranks' points never pass here.  The updater hands the gathered coordinates over
                # (_stats_points).  Failing that (callers with only an ncclComm_t, nothing to gather through) the block is given up: noting
                # this rank's own shard instead would leave every replica with a DIFFERENT preconditioner, hence different CG iterates and
                # iteration counts -- and the collective decisions of the path (carried residual, poll hints) assume replicated state
                pts = self.__dict__.pop("_stats_points", None)
                if pts is not None and not init:
                    self._two_level_note(pts[0], pts[1])            # every rank's points, gathered beside the all-reduce (distributed.py)
                else:
                    self._two_level_lose()
            else:
                self._two_level_note(X, None if unit else self._weight_a(noise[:, 0], init), init=init)
        carry_delta = (half_delta is not None and res_delta is not None and not init and ms is not None and ms.get("R_ok", False)
                       and settings.residual_carry_over.on())
        carry = self._carried(mine, init or half_delta is not None) is not None
        if getattr(self, "_scratch_stats", None) is None:
            self._scratch_stats = torch.zeros(2, dtype=torch.float64, device=self._device)
        if half_delta is None and self._absorb_all_outputs(cache, X, Y, noise, init, ops, ms if carry else None):
            return carry_delta
        for o in range(self.num_outputs):
            yo = Y[:, o].contiguous()
            no, wa, wb = self._batch_weights(None if unit else noise[:, o].contiguous(), init, n)
            cnt_o = cache["_cnt"][o] if "_cnt" in cache else None     # row sums W^T wa ride on the same launch
            half = grid_ops.is_half_stencil(self._grid, dst[o])      # a handed-over cache may carry a full stencil
            if carry and not half:
                carry = ms["R_ok"] = False
            if carry_delta and not half:
                carry_delta = False
            grid_ops.scatter_stats_cnt(self._grid, X, yo, wa, wb, no, b[o, :, 0], dst[o], half, cnt_o, stats[o], self._err,
                                       u=ms["U"][o] if (carry or carry_delta) else None,
                                       res=ms["R"][o] if carry else (res_delta[o] if carry_delta else None))
            if (init or half_delta is not None) and getattr(ops[o], "root", None) is not None:
                # the stencil is being rebuilt (set_train_data) or receives its increment later, after an all-reduce
                # (data-parallel path): a carried root pair would describe the OLD matrix -- drop it, it is re-derived on demand
                ops[o].root = ops[o].inv_root = None
            self._follow(cache, o, X, None if unit else wa, yo if unit else yo * wb, init=init, bypass=half_delta is not None)
        return carry_delta

    # ---- what an absorb owes the things that follow the statistics: stated once, used by every observation form ----
    def _before_launch(self, cache):
        """Before a launch writes into `cache`: nothing is in flight, and the model's own stencil is whole (the launches of the
        absorb forms write every group).  Returns whether `cache` is the model's own."""
        self._finish_pending()
        mine = cache is self._kernel_cache
        if mine:
            self.leave_stencil_shard()
        return mine

    def _native_half_op(self, cache, form, half_delta=None):
        """The half-stencil operator of `cache` for a form whose launch writes the statistics themselves: a single output, the
        native half-stencil cache with its row sums, no data-parallel exchange -- refused otherwise, in the form's name."""
        if half_delta is not None:
            raise NotImplementedError(f"{form}: no data-parallel statistics exchange (half_delta) -- the launch takes its weights on one rank "
                                      "and writes the statistics themselves: there is no increment to all-reduce, and the other ranks' "
                                      "followers would never see the weights")
        if self.num_outputs > 1:
            raise NotImplementedError(f"{form}: implemented for a single output")
        op = _wtw_ops(cache["WtW"])[0]
        if not grid_ops.is_half_stencil(self._grid, op.stencil) or "_cnt" not in cache:
            raise NotImplementedError(f"{form}: the native half-stencil cache is needed (a full stencil was handed over)")
        return op

    def _canon_batch(self, X, y, noise, init=False):
        """A single-output batch as the absorb kernels take it: (X [n, d], y [n] or None, noise, wa, wb) on the model's device, in its
        dtype, contiguous; noise None: unit noise (_batch_weights)."""
        X = X.reshape(-1, self._grid.d).to(self._device, self._dtype).contiguous()
        if y is not None:
            y = y.to(self._device, self._dtype).reshape(-1).contiguous()
        if noise is not None:
            noise = noise.to(self._device, self._dtype).reshape(-1).contiguous()
        return (X, y) + self._batch_weights(noise, init, X.shape[0])

    def _carried(self, mine, init=False, u=None):
        """The carried-residual decision of a launch into the model's own cache (`mine`): the mean state whose R = b - Z - A U the
        launch keeps exact under its increment -- it is current, the statistics are not being rebuilt (`init`), and, where the
        launch reads a grid mean `u` of its own, that is this state's U itself -- or None, and then the state's residual is marked
        as no longer carried (the next refresh recomputes it)."""
        ms = self._mean_state
        if ms is None:
            return None
        if (mine and not init and ms.get("R_ok", False) and settings.residual_carry_over.on()
                and (u is None or ms["U"][0].data_ptr() == u.data_ptr())):
            return ms
        if mine:
            ms["R_ok"] = False
        return None

    def _follow(self, cache, o, X, wa, wby, init=False, bypass=False):
        """Follower policy "follow": every point of X has entered A of output o with the effective weight wa (None: unit) and b with
        wby = wb_eff * y_eff.  Everything that follows the stream point by point receives the same: a carried root pair, the
        spectral factor, the noise-weight sum, the path probes.  bypass: the increment reaches the stencil later, by all-reduce."""
        n, mine = X.shape[0], cache is self._kernel_cache
        op = _wtw_ops(cache["WtW"])[o]
        if not bypass and getattr(op, "root", None) is not None and n > 0:
            # the reference's root pair, once somebody asked for it: L L^T follows A by a rank-n root update (URLT:62-119)
            Wd = grid_ops.wt_columns(self._grid, X, self._err)                                       # [n, m]
            op.update_roots_((Wd if wa is None else Wd * wa.sqrt()[:, None]).t().contiguous())       # V = W^T diag(wa)^(1/2), BFN:163-168
        if mine and n > 0:
            self._spectral_absorb(o, X, wa, wby, init=init, bypass=bypass)
        if mine or init:
            self._wsum_add(o, n, wa)
        if "path_probes" in cache:                   # (single output)
            self._absorb_probes(cache, X, wa, init)
        if "trend_C" in cache:                       # (single output)
            self._absorb_trend(cache, X, wa, wby)

    def _give_up(self, cache):
        """Follower policy "give up": the launch changed A by something that cannot be followed point by point (a derivative row, a
        point that left, a scaling).  A carried root pair is dropped (L L^T described the matrix before), and for the model's own
        cache the two-level block is lost and the spectral factors are marked stale: each is rebuilt from the stencil, exactly,
        where it is wanted again.  (On the factor, not the model: it travels with the kernel cache.)"""
        for op in _wtw_ops(cache["WtW"]):
            op.root = op.inv_root = None
        if cache is self._kernel_cache:
            self._two_level_lose()
            for fac in self.__dict__.get("_spectral", {}).values():
                fac.stale = True

    def _absorb_probes(self, cache, X, wa, init=False):
        """Every point that enters A enters the probes P with the same weight wa (None: unit) and its global index, so that
        cov(P_s) = A whatever the hyper-parameters (one launch, wiski_scatter_probes).  init: the statistics restart at index 0."""
        P = cache["path_probes"]
        if init:
            P.zero_()
            cache["path_count"] = 0
        n = X.shape[0]
        if n:
            grid_ops.scatter_probes(self._grid, X, wa, cache["path_count"], cache["path_seed"], P, self._err)
            cache["path_count"] += n

    def _absorb_trend(self, cache, X, wa, wby):
        """Every point that enters A with the weight wa (None: unit) and b with wby enters the trend statistics C, G, g with the same
        (one launch, wiski_scatter_trend).  A restart finds them zero: a fresh cache, or set_train_data, which zeroes them with b."""
        if X.shape[0]:
            grid_ops.scatter_trend(self._grid, X, wa, wby, cache["trend_deg"], cache["trend_center"], cache["trend_scale"], cache["trend_C"],
                                   cache["trend_G"], cache["trend_g"], self._err)

    def _absorb_all_outputs(self, cache, X, Y, noise, init, ops, ms):
        """Several outputs, native packed half stencils, no root pairs to carry: ONE scatter launch for all of them
        (wiski_scatter_stats_multi) instead of one per output.  The arguments are what _absorb has prepared (noise None: unit;
        ms: the mean state whose residual is carried, or None).  False: not applicable, the caller loops."""
        out, n = self.num_outputs, X.shape[0]
        if out == 1 or n == 0 or "_cnt" not in cache or any(getattr(op, "root", None) is not None for op in ops):
            return False
        pack = self._stencil_pack(ops)
        if pack is None:
            return False
        unit = noise is None
        Yt = Y.t().contiguous()                                   # [out, n]
        no, wa, wb = self._batch_weights(None if unit else noise.t().contiguous(), init, n)
        b = cache["interpolation_cache"][:, :, 0]
        if not b.is_contiguous():
            return False
        grid_ops.scatter_stats_multi(self._grid, X, Yt, wa, wb, no, b, pack, cache["_cnt"], cache["_stats"], self._err,
                                     u=ms["U"] if ms else None, res=ms["R"] if ms else None)
        for o in range(out):                                       # (no root pair, no probes: the spectral factor and the weight sum)
            self._follow(cache, o, X, None if unit else wa[o], Yt[o] if unit else Yt[o] * wb[o], init=init)
        return True

    def _ones(self, n):
        """[n] ones, a view of one cached vector (unit noise: weights and noise of every point)."""
        if getattr(self, "_ones_cache", None) is None or self._ones_cache.shape[0] < n:
            self._ones_cache = torch.ones(max(n, 4096), dtype=self._dtype, device=self._device)
        return self._ones_cache[:n]

    @staticmethod
    def _weight_a(noise, init):
        """The weight a point enters A with: 1 / noise, the noise floored at 1e-7 in an update (clamp_min(1e-7)**0.5 of :163, squared)."""
        return 1.0 / noise if init else 1.0 / noise.clamp_min(1e-7)

    def _batch_weights(self, noise, init, n):
        """(noise, wa, wb) of a batch of n points, as the absorb kernels take them; noise None: unit noise, three times _ones(n)."""
        if noise is None:
            ones = self._ones(n)
            return ones, ones, ones
        wb = 1.0 / noise
        return noise, wb if init else self._weight_a(noise, init), wb

    def _wsum_add(self, o, n, wa):
        """Output o's noise-weight sum grows by the weights wa of n absorbed points: on the host for unit noise (wa None), else on the device."""
        if wa is None:
            self._wsum_host[o] += float(n)
        else:
            self._wsum_dev[o] += wa.sum(dtype=torch.float64)
            self._wsum_dirty = True

    # (the return value of _absorb tells the data-parallel caller whether res_delta was filled)
    @property
    def _wsum(self):
        if self._wsum_dirty:
            self._wsum_dev_host = self._wsum_dev.tolist()
            self._wsum_dirty = False
        if self.window is not None:                  # (a sum that points have left is zero up to rounding only)
            return [max(0.0, h + d) for h, d in zip(self._wsum_host, self._wsum_dev_host)]
        return [h + d for h, d in zip(self._wsum_host, self._wsum_dev_host)]

    def check_bounds(self):
        """Raise like gpytorch's grid check if any point seen so far was outside the
        grid (the kernels only set a device flag; this is the one host sync; the
        device part of the noise-weight sum rides on the same transfer)."""
        self._finish_pending()
        if self.window is not None:
            # the number of void slots that were overwritten rides on the same transfer: num_data is the ring's occupancy less the
            # voids still in it (dropped at entry, not yet left)
            ring = self._kernel_cache["_ring"]
            vals = torch.cat([self._err.double(), ring.void_left.double(), self._wsum_dev]).tolist()
            if self._wsum_dirty:
                self._wsum_dev_host, self._wsum_dirty = vals[2:], False
            flag, left = int(vals[0]), int(vals[1])
            if left:
                ring.void_left.zero_()
                self._win_voids -= left
                self.num_data = ring.fill - self._win_voids
        elif self._wsum_dirty:
            vals = torch.cat([self._err.double(), self._wsum_dev]).tolist()
            self._wsum_dev_host, self._wsum_dirty = vals[1:], False
            flag = int(vals[0])
        else:
            flag = int(self._err.item())
        if flag:
            self._raise_out_of_bounds(flag)

    def _raise_out_of_bounds(self, flag):
        """`flag` is the raw device word: bit 0 = some point (query or training) was outside the grid, bits 1.. = number
        of *training* points the scatter dropped.  Dropped points contributed nothing to A, b, y^T D^-1 y or log|D|
        (scatter_stats.hip), so taking them out of `num_data` and of the noise-weight sum leaves statistics that
        describe exactly the points that were absorbed -- a caller may catch the error and carry on."""
        dropped = flag >> 1
        self._err.zero_()
        self._stream_step_cache = None
        self._drop_spectral()          # rows of out-of-grid points were zero for the factor too, but a prepared state may be half-updated
        if dropped and self.window is not None:
            ring = self._kernel_cache["_ring"]
            self._win_voids += dropped
            self.num_data = ring.fill - self._win_voids
            # the noise-weight sum is that of the ring (a void holds wa = 0): from now on the device keeps all of it
            ring.unit[:] = False
            ring.explicit.fill_(1)
            ring.explicit_host[:] = True
            self._wsum_host = [0.0]
            self._wsum_dev = ring.wa.sum(dtype=torch.float64).reshape(1)
            self._wsum_dirty = True
            self._dump_caches()
        elif dropped:
            self.num_data = self.num_data - dropped
            cnt = self._kernel_cache.get("_cnt")
            if cnt is not None:                       # row sums of W^T D^-1 W: sum_i cnt_i = sum over absorbed points of 1/noise
                self._wsum_dev = cnt.sum(dim=1, dtype=torch.float64)
                self._wsum_host = [0.0] * self.num_outputs
                self._wsum_dirty = True
            self._dump_caches()
        raise RuntimeError("Received data that was out of bounds for the specified grid. "
                           f"Grid bounds were {self.covar_module.grid_bounds}.")

    def _sigma2(self, o=0):
        if not self.has_learnable_noise:
            return 1.0
        n = self.likelihood.second_noise_covar.noise.detach().reshape(-1)
        return float(n[o] if n.numel() > 1 else n[0])

    def _hyper_version(self):
        ps = self.__dict__.get("_hyper_params")
        if ps is None:
            ps = list(self.covar_module.parameters()) + (list(self.likelihood.second_noise_covar.parameters()) if self.has_learnable_noise else [])
            self.__dict__["_hyper_params"] = ps
        return (self.__dict__.get("_hyper_epoch", 0),) + tuple(p._version for p in ps)

    def _hyper(self):
        """Per-output (tcol on device in the data dtype, sigma2 float); memoised on
        the parameters' version counters."""
        ver = self._hyper_version()
        h = self._memo.get("hyper")
        if h is None or h[0] != ver:
            vals = []
            with torch.no_grad():
                for o in range(self.num_outputs):
                    bi = o if self.num_outputs > 1 else None
                    tcol64 = self.covar_module.toeplitz_columns(batch_index=bi, device=self._device).contiguous()
                    vals.append((tcol64.to(self._dtype).contiguous(), self._sigma2(o), tcol64))
            h = (ver, vals)
            self._memo["hyper"] = h
        return h[1]

    def _use_dense(self):
        return settings.dense_small_grids.on() and self._grid.m <= settings.max_cholesky_size.value()

    def _spectral_allowed(self):
        """May a request go to the spectral factor (lazy/spectral_woodbury.py)?  Beyond the dense regime always; inside it only for
        the reference's per-batch loop, whose owner (a streaming wrapper) has said so -- direct users of the model, BO posteriors
        and fantasies keep the nodal dense factor with its cached M and rank-q updates."""
        if settings.spectral_factor.off() or self._trend_deg is not None:    # (a trend's moments always come through the prediction cache)
            return False
        if not self._use_dense():
            return True
        return settings.spectral_dense_regime.on() and bool(self.__dict__.get("_stream_owner")) and not self._kernel_families().periodic

    def _kernel_families(self):
        """kernels.KernelFamilies(periodic, any) of the covariance module, looked up once per covariance module object (the per-step
        path reads the memo; assigning another module looks again)."""
        cm = self.covar_module
        memo = self.__dict__.get("_families_memo")
        if memo is None or memo[0] is not cm:
            from ..kernels import kernel_families

            memo = self.__dict__["_families_memo"] = (cm, kernel_families(cm))
        return memo[1]

    def _mll_spectral_state(self, o):
        """The spectral factor's state for the MLL terms of output o and their gradient, or None where the MLL has to come from the
        nodal dense factor or the PCG terms: wherever the factor does not serve at all, and for a covariance with a PeriodicKernel, whose
        period gradient from the truncated factor is not the MLL's.  Predictions may still use the factor."""
        if not self._spectral_allowed() or self._kernel_families().periodic:
            return None
        return self._spectral_state(o)

    def _precond(self, o, tcol):
        """(eigen tuple, shift) of wiski_pcg's preconditioner (Kt^-1 + a kron_q diag(t_q))^-1.
        t_q = per-dim marginal of the row sums of W^T D^-1 W (the data-density profile: the
        grid nodes outside the data box carry no data), a = total mass / prod_q sum(t_q).
        The d small generalized eigenproblems are re-solved when the hyper-parameters change,
        or when the normalised density profile has moved by more than
        settings.precond_profile_drift (a stationary stream keeps its eigenbasis).  The profile is
        looked at (3 small reductions + one host read, ~0.15 ms) each time the data volume has
        doubled, or as soon as a warm refresh needs 2 more CG iterations than the first one after
        the last re-solve did -- the symptom of a stale basis; `a` follows the stream exactly."""
        if settings.spectral_preconditioner.off():
            return None, 0.0
        # (the eigenbasis must belong to the CURRENT hyper-parameters exactly: the fused solver kernels take the u = Kt z image of every
        # search direction from it, so a basis kept across even a 1 % lengthscale step changes the converged mean at the 1e-4 level --
        # tried and reverted in round 3, tests/test_model_gpu.py::test_preconditioner_eigenbasis_is_resolved_for_every_hyperparameter_change)
        ver = self._hyper_version()
        st = self._memo.setdefault("precond", {}).get(o)
        wsum = float(self._wsum[o])
        stale = st is None or st["ver"] != ver
        slow = not stale and basis_slow(st, (self._last_iters or [0] * (o + 1))[o], wsum)
        if stale or wsum > 2.0 * st["wsum"] or wsum < 0.5 * st["wsum"] or slow:
            profiles, norm = None, float(self._grid.m)
            if settings.density_profile_preconditioner.on() and self._kernel_cache.get("_cnt") is not None and wsum > 0:
                profiles, norm = density_profiles(self._cnt_marginals(o).cpu().numpy(), self._grid.g, self._grid.m)
            old = None if stale else st.get("profiles")
            if old is not None and profiles is not None and not profiles_moved(profiles, old):
                basis_kept(st, wsum)
            else:
                host = {}
                # where the truncated preconditioner can engage (_keep_for_step: one output, d = 3, fp32) decompose the fp64 columns:
                # the tables are fp32 either way and reproduce the prior factor as closely as before
                # (tests/test_precond_keep_host.py::test_tables_from_fp64_columns_reproduce_the_factor_as_closely).  Columns rounded to fp32
                # first carry ~1e-9 of rounding noise in their spectrum, which the truncation rule would have to keep as if it were
                # prior (grid_ops.kron_eigen).  Everything else decomposes what it always did
                fine = settings.truncated_preconditioner.on() and tcol.dtype == torch.float32 and self.num_outputs == 1 and self._grid.d == 3
                src = self._hyper()[o][2] if fine else tcol
                eig = grid_ops.kron_eigen(self._grid, src, profiles=profiles, host_out=host, dtype=tcol.dtype)
                st = {"ver": ver, "wsum": wsum, "eig": eig, "norm": norm, "profiles": profiles, "it0": None, "eig_host": host}
                self._memo["precond"][o] = st
        return st["eig"], wsum / st["norm"]

    def _cnt_marginals(self, o):
        """Per-dim marginals of the row sums of W^T D^-1 W of output o, [d, max g] in fp64 on the device (rows padded with zeros)."""
        g, d = self._grid.g, self._grid.d
        c3 = self._kernel_cache["_cnt"][o].reshape(g).double()
        margs = [c3.sum(dim=[r for r in range(d) if r != q]) if d > 1 else c3 for q in range(d)]
        # (cnt of a cell whose points have all left a sliding window is zero up to rounding only: no negative density)
        return torch.stack([torch.nn.functional.pad(mg, (0, max(g) - mg.numel())) for mg in margs]).clamp_min(0)

    def _posterior_op(self, o):
        self.leave_stencil_shard()                   # solves outside the sharded streaming step need the whole stencil
        tcol, s2, _ = self._hyper()[o]
        if self._use_dense():
            return DenseInducingPosterior(self._grid, _wtw_ops(self._kernel_cache["WtW"])[o], tcol, 1.0 / s2, grid_ops.kron_eigen(self._grid, tcol))
        eig, shift = self._precond(o, tcol)
        post = InducingPosterior(self._grid, _wtw_ops(self._kernel_cache["WtW"])[o], tcol, 1.0 / s2, _default_tol(self._dtype),
                                 settings.max_cg_iterations.value(), workspace=self._pcg_ws, check_every=settings.cg_check_every.value(),
                                 eigen=eig, shift=shift, err=self._err)
        # the exact block of the two-level preconditioner, where the stream keeps one for this eigenbasis: every solve through this
        # operator that names no block of its own asks for it when it runs (the operator outlives many streaming steps)
        if o == 0:
            import weakref

            ref = weakref.ref(self)
            post.two_level_provider = lambda op, k: (ref()._two_level_for_solve(op, k) if ref() is not None else None)
        return post

    def _two_level_for_solve(self, post, k):
        """The stream's two-level block for a solve of k columns through `post` (variances, probes, fantasies: 15 -> 4-5 iterations
        per 64-column solve on the road-like stream): the tracker's block if it belongs to the operator's
        eigenbasis; where it was lost (hyper-parameter step, profile re-solve, points behind the tracker's back) and the solve is
        wide, a block rebuilt from the statistics (settings.two_level_rebuild)."""
        tr = self.__dict__.get("_two_level") if self._two_level_applies() else None
        if tr is None:
            return None
        pst = self._memo.get("precond", {}).get(0)
        if pst is None or pst.get("eig") is not post.eigen:
            return None
        tl = tr.current(pst, post.kscale, cols=k)
        warming = tr.block is not None and tr.covered and not tr.block.failed and tr.block.active < 0 and tr.block.in_flight is not None
        if tl is None and k >= 16 and tr.wanted and not warming:   # (a block whose first refresh is in flight is not thrown away for a ~1.5 ms rebuild; 8 or 1 columns: the q = 1 reference step on the PCG path 5.0 -> 5.2 / 6.4 ms: the rebuild costs more than narrow solves save)
            tl = tr.rebuild(self._grid, self._device, pst, post.kscale, post.wtw.stencil, float(self._wsum[0]), self._err)
            if tl is not None:
                tr.block.ensure_cols(k)
                self._pacing.new_block()
        return tl

    # ------------------------------------------------------- stencil shard --
    def enter_stencil_shard(self, rank, world, allreduce, allreduce_full=None, comm=None):
        """Multi-GPU step that divides the work (include/wiski.h: wiski_shard): from now on this replica keeps
        only ITS groups of the half stencil current -- the streaming step scatters 1 / world of the tap pairs per point and
        computes 1 / world of A p, one all-reduce of an m-vector per CG iteration makes the product whole.  Every rank must
        see every point (the caller all-gathers the shards) and must make the same calls.  `allreduce(vec, dots)`: in-place
        SUM over the ranks of the two tensors (dots may be None); `allreduce_full(t)`: the same for one large tensor, used
        when a consumer needs the whole stencil again (leave_stencil_shard).  `comm`: an ncclComm_t (wiski_comm_*) -- the per-product
        all-reduce is then issued from C on the solve's stream (one grouped RCCL launch, no re-entry into Python); a single rank
        with a communicator owns every group and still takes that path (both precisions).  Returns False
        where the sharded step does not apply (then nothing changes): one output, native half stencil, m % 4 == 0, a grid beyond the
        dense regime.  Any d and both precisions: the d = 3 fp32 products run on the LDS-DMA kernel's part table, all others on
        the LDS-window kernel restricted to the replica's group range."""
        if self.window is not None:
            raise NotImplementedError("window does not combine with enter_stencil_shard: the window absorb writes every stencil group")
        if self.site_memory is not None:
            raise NotImplementedError("site_memory does not combine with enter_stencil_shard: a sweep of refine_sites_ writes every stencil group")
        self._refuse_trend("enter_stencil_shard", "the trend's solve columns S = M C need the whole stencil at every refresh")
        if self.noise_model is not None:
            raise NotImplementedError("heteroscedastic does not combine with enter_stencil_shard: its launch writes every stencil group of both models")
        op = _wtw_ops(self._kernel_cache["WtW"])[0]
        if (world <= 1 and not comm) or self.num_outputs != 1 or self._use_dense() or not op.is_half or self._grid.m % 4 or op.root is not None:
            return False
        if self.forgetting_factor is not None:
            return False                             # (a decay touches the whole stencil: forgetting replicas are not sharded)
        if self.__dict__.get("_stencil_shard") is not None:
            return True
        self._finish_pending()
        lo, hi = grid_ops.shard_groups(self._grid.d, rank, world)
        ng = (self._grid.R // 7 + 1) // 2
        flat = op.stencil.reshape(-1)
        for a, b in grid_ops.half_stencil_group_slices(self._grid, 0, lo) + grid_ops.half_stencil_group_slices(self._grid, hi, ng):
            flat[a:b].zero_()
        self.__dict__["_stencil_shard"] = {"rank": rank, "world": world, "allreduce": allreduce, "allreduce_full": allreduce_full or (lambda t: allreduce(t, None)),
                                           "comm": comm}
        self._stream_step_cache = None
        self._drop_spectral()
        return True

    def leave_stencil_shard(self):
        """Collective: sum the disjoint stencil shards back into a full replica on every rank (one all-reduce of the half
        stencil).  Called automatically by every consumer that reads the stencil outside the sharded streaming step."""
        sh = self.__dict__.get("_stencil_shard")
        if sh is None:
            return
        self._finish_pending()
        self.__dict__["_stencil_shard"] = None
        self._stream_step_cache = None
        sh["allreduce_full"](_wtw_ops(self._kernel_cache["WtW"])[0].stencil)

    # ------------------------------------------------------ spectral factor --
    def _spectral_state(self, o=0):
        """(factor, state, fp64 Toeplitz columns on the device) of the reduced-eigenbasis Woodbury factor
        (lazy/spectral_woodbury.py) for the current hyper-parameters and statistics, or None where it does not apply:
        dense regime, switched off, or a prior whose numerical rank exceeds settings.spectral_max_rank."""
        if not self._spectral_allowed():
            return None
        from ..lazy import spectral_woodbury as sw

        self._finish_pending()
        self.leave_stencil_shard()
        ver = self._hyper_version()
        key = (ver, sw.default_tail(self._dtype), settings.spectral_max_rank.value(), settings.fast_pred_var.on(),
               settings.max_root_decomposition_size.value())
        memo = self._memo.setdefault("spectral", {})
        ent = memo.get(o)
        if ent is None or ent[0] != key:
            tcol64 = self._hyper()[o][2]                 # fp64 Toeplitz columns, computed once per hyper-parameter version
            ent = (key, tcol64)
            memo[o] = ent
        if ent[1] is None:
            return None                                  # not applicable at these hyper-parameters (remembered)
        _, tcol64 = ent
        facs = self.__dict__.setdefault("_spectral", {})
        self._kernel_cache["_spectral"] = facs           # (travels with the statistics: kernel_cache hand-over, functional conditioning)
        fac = facs.get(o)
        if fac is None:
            fac = facs[o] = sw.SpectralWoodburyFactor(self._grid, self._dtype, self._device, self._err)
        kscale = 1.0 / self._hyper()[o][1]
        if fac.stale:
            fac.stale = False
            # statistics changed behind the factor's back: rebuild from the stencil (and forget the state derived from the old ones)
            fac.ref = fac.cur = None
            fac.data_version += 1
        # the columns go in as a device tensor: after a hyper-parameter step the factor refreshes its eigenvectors on the
        # device (no host copy, no synchronisation) unless it has to re-select its index set
        st = fac.state(key, tcol64, kscale)
        if st is None:
            memo[o] = (key, None)
            return None
        if st.get("need_reference"):
            tc_host = tcol64.detach().cpu().numpy()
            # reference basis with a margin, so that the eigenbasis may drift with the hyper-parameters before the
            # reference has to be rebuilt; if the margin does not fit the rank cap, the basis itself
            refb = None if settings.fast_pred_var.on() else sw.select_basis(self._grid, tc_host, st["tail"] * 1e-2, 2 * settings.spectral_max_rank.value(),
                                                                            self._device)
            op = _wtw_ops(self._kernel_cache["WtW"])[o]
            fac.build_reference(refb if refb is not None else st["basis"], op.stencil, self._kernel_cache["interpolation_cache"][o, :, 0])
            st = fac.state(key, tcol64, kscale)
            if st is None or st.get("need_reference"):
                memo[o] = (key, None)
                return None
        return fac, st, tcol64

    def _measure_factor_means(self, sps):
        """Factors whose mean monitor can no longer decide by its bound (SpectralWoodburyFactor.measure_due): measure the factor's mean
        against the PCG mean at the current hyper-parameters on the factor's probe set (one PCG solve, rare: every few hundred steps at
        most), which either keeps the factor serving the mean or switches it off."""
        due = [o for o, sp in enumerate(sps) if sp[0].measure_due]
        if not due:
            return
        pc = self.prediction_cache
        for o in due:
            fac, st, tc = sps[o]
            fac.measure_mean(st, tc, lambda pts, o=o: grid_ops.gather(self._grid, pts, pc["pred_mean"][..., 0], self._err)[:, o])

    def _spectral_in_use(self):
        """Every output has a spectral factor that follows the stream and has been asked for a state recently."""
        if not self._spectral_allowed():
            return False
        facs = self.__dict__.get("_spectral", {})
        return all((f := facs.get(o)) is not None and f.ref is not None and f.cur is not None and not f.stale and f.idle_absorbs < 8
                   for o in range(self.num_outputs))

    def _spectral_absorb(self, o, X, wa, wby, init=False, bypass=False):
        """Keep the spectral factor of output o (if one exists) in step with the statistics."""
        fac = self.__dict__.get("_spectral", {}).get(o)
        if fac is None or fac.ref is None:
            return
        if init or bypass or X.shape[0] > 2048 or fac.idle_absorbs >= 8:
            # rebuilt from scratch / changed by an all-reduce / a batch large enough that re-projecting the stencil on
            # demand (r SpMV columns) is cheaper than following it / nobody has asked the factor anything for 8 batches (a
            # streaming loop that only wants means must not pay a projection + GEMM per step): mark, rebuild when next asked
            fac.stale = True                             # (on the factor, not the model: it travels with the kernel cache)
            return
        fac.absorb(X, wa, wby)

    def _drop_spectral(self):
        self.__dict__.pop("_spectral", None)
        if self._kernel_cache is not None:
            self._kernel_cache.pop("_spectral", None)
        self._memo.pop("spectral", None)

    # --------------------------------------------------------------- caches --
    @property
    def Kuu(self):
        """Lazy Kuu (/ sigma2 when the second noise is learnable), :334-341."""
        ops = [KroneckerToeplitz(self._grid, tcol, 1.0 / s2) for tcol, s2, _ in self._hyper()]
        return ops[0] if self.num_outputs == 1 else BatchOperator(ops)

    @property
    def Kuu_response(self):
        """Kuu @ W^T D^-1 y, :363-366; [out, m, 1]."""
        b = self._kernel_cache["interpolation_cache"]
        outs = [grid_ops.kron_toeplitz_mm(self._grid, tcol, b[o, :, 0], 1.0 / s2) for o, (tcol, s2, _) in enumerate(self._hyper())]
        return torch.stack(outs)[..., None]

    @property
    def prediction_cache(self):
        """pred_mean = (Kt^-1 + A)^-1 W^T D^-1 y  [out, m, 1]   (:368-383), and the
        lazy pred_cov operator(s).  The mean solve is warm-started from the
        previous solution (U, Z) after every streaming update."""
        self._finish_pending()
        self.leave_stencil_shard()                   # whoever asks for the cache may go on to solve with the whole stencil
        self._apply_pending_rank_update()
        pc = self._memo.get("prediction_cache")
        if pc is not None:
            return self._with_trend(pc)
        if self._use_dense() or self._wsum_dirty:
            self.check_bounds()          # dense path has no solver poll to ride on; a dirty weight sum needs the read anyway
        out, m = self.num_outputs, self._grid.m
        b = self._kernel_cache["interpolation_cache"]
        hyper = self._hyper()
        ver = self._hyper_version()
        ms = self._mean_state
        if ms is not None and ms["U"].shape == (out, m):
            U, Z, R = ms["U"], ms["Z"], ms["R"]       # refreshed in place by the warm-started solves
        else:
            U = torch.empty((out, m), dtype=self._dtype, device=self._device)
            Z = torch.empty_like(U)
            R = torch.empty_like(U)
            ms = None
        iters = []
        posts = []
        converged = True
        for o in range(out):
            post = self._posterior_op(o)
            if isinstance(post, DenseInducingPosterior):
                Uo, _ = post.solve_columns(b[o, :, 0][None])
                U[o] = Uo[0]
                Z[o].zero_()
                iters.append(0)
                posts.append(post)
                continue
            warm = ms is not None
            Uo, Zo, Ro = U[o:o + 1], Z[o:o + 1], R[o:o + 1]   # contiguous row views: wiski_pcg updates them in place
            carried = warm and ms.get("R_ok", False)
            if warm and ms["ver"] != ver:
                tcol, s2, _ = hyper[o]
                Uo.copy_(grid_ops.kron_toeplitz_mm(self._grid, tcol, Zo, 1.0 / s2))   # keep U = Kt Z under the new hypers
                carried = False
            # the exact block of the two-level preconditioner, where one is being tracked (the streaming fast path takes it through
            # wiski_stream_step; this is the generic refresh -- e.g. after a statistics all-reduce, the north-star exchange)
            tl = None
            tr = self.__dict__.get("_two_level") if (out == 1 and warm and self._two_level_applies()) else None
            pst = self._memo.get("precond", {}).get(o) if tr is not None else None
            if pst is not None and "eig_host" in pst and pst.get("eig") is post.eigen:
                tl = tr.for_step(self._grid, self._device, pst, post.kscale, float(self._wsum[0]), self._err,
                                 lockstep=settings.two_level_lockstep.on(), last_iters=(self._last_iters or [0])[0])
                if tr.switched:
                    self._pacing.new_block()
            # warm refreshes poll convergence first where the previous one converged (streaming steps are
            # alike), every 8th one an iteration earlier, and then after every iteration
            fc, probe = 0, False
            if warm and self._last_iters:
                self._pacing.count()
                fc, probe = self._pacing.place(self._last_iters[o])
                post.check_every = 1
            # warm = 2: R was kept equal to b - Z - A U by the scatter launches since the last solve (recomputed
            # from scratch every 16th refresh so that fp rounding of the recursion cannot accumulate)
            if carried and self._pacing.recompute_due():
                carried = False
            post.solve_columns(b[o, :, 0][None], U=Uo, Z=Zo, warm=2 if carried else warm, first_check=fc, inplace=True, R=Ro, two_level=tl)
            self._pacing.solved(post.last_iters, None, fc, probe)    # this path does not keep the converged residual: timer-paced probes only
            iters.append(post.last_iters)
            posts.append(post)
            if post.last_err:            # out-of-grid flag delivered with the convergence poll (no extra sync)
                self._mean_state = None if ms is None else dict(ms, R_ok=False)
                self._raise_out_of_bounds(post.last_err)
            converged = converged and getattr(post, "last_converged", True)
        # a solve that stopped at max_cg_iterations (warned about in grid_ops.pcg) leaves a residual that is not small:
        # do not carry it into the next refresh as if it were
        self._mean_state = None if self._use_dense() else {"U": U, "Z": Z, "R": R, "R_ok": converged, "ver": ver}
        self._last_iters = list(iters)
        if ms is not None:
            self._pacing.warm()
        else:
            self._pacing.cold()
        pc = {"pred_mean": U[..., None], "pred_cov": posts[0] if out == 1 else BatchOperator(posts), "cg_iters": iters, "ver": ver}
        self._memo["prediction_cache"] = pc
        return self._with_trend(pc)

    # ---------------------------------------------------------------- trend --
    def _with_trend(self, pc):
        """On a trend model the prediction cache additionally holds ``trend = {S, Lchol, beta, ...}``: S = M C by p more
        columns of the solve the cache already makes (dense and PCG through the same call), then p x p algebra in fp64:
        Lambda0 = G - C^T S, Lambda = Lambda0 + (sigma2 / tau2) I = L L^T, v = g - S^T b, beta = Lambda^-1 v; where the solve hands its
        Z = Kt^-1 S over (PCG), Lambda0 and v are corrected by the solve's own residual, which leaves them second-order accurate in it."""
        cache = self._kernel_cache
        if "trend_C" not in cache or "trend" in pc:
            return pc
        post = pc["pred_cov"]
        C = cache["trend_C"]
        p = C.shape[1]
        Ct = C.t().contiguous()                                    # solve_columns takes [k, m]
        St = torch.empty_like(Ct)
        resid = None
        chunk = max(1, int(settings.variance_chunk.value()))
        for s in range(0, p, chunk):
            e = min(s + chunk, p)
            U, Z = post.solve_columns(Ct[s:e].contiguous())
            St[s:e] = U
            if getattr(post, "last_err", 0):
                self._raise_out_of_bounds(post.last_err)
            if Z is not None:
                # the solve's own residual C - Q S (Z = Kt^-1 S comes with the solve): corrects Lambda0 to second order in it
                if resid is None:
                    resid = torch.empty((p, self._grid.m), dtype=torch.float64, device=self._device)
                resid[s:e] = Ct[s:e].double() - Z.double() - grid_ops.stencil_spmv(self._grid, post.wtw.stencil, U).double()
        S64, C64 = St.double(), Ct.double()
        b64 = cache["interpolation_cache"][0, :, 0].double()
        G = grid_ops.trend_mirror(cache["trend_G"])
        lam0 = G - C64 @ S64.t()
        if resid is not None:
            lam0 = lam0 - S64 @ resid.t()                          # G - C^T S - S^T (C - Q S)
        lam0 = 0.5 * (lam0 + lam0.t())
        s2 = self._sigma2(0)
        tau2 = self.trend_prior_var
        lam = lam0.clone()
        if tau2 is not None:
            lam.diagonal().add_(s2 / tau2)
        # factored with the basis functions scaled to unit weighted norm (G~ = D G D with unit diagonal, D = diag(G)^-1/2), so that a
        # monomial that is small over the data -- data confined to a part of the first grid -- is judged by its own size.  An entry of
        # Lambda0~ is known to about eps of the dtype C is kept in (eps |G~| with |G~| <= 1), so under the flat prior a squared pivot at
        # or below 8 eps is not distinguishable from zero: the coefficients are not determined to that precision, and the model says so
        dsc = G.diagonal().clamp_min(torch.finfo(torch.float64).tiny).rsqrt()
        Ls, info = torch.linalg.cholesky_ex(lam * dsc[:, None] * dsc[None, :])
        L = Ls / dsc[:, None]                                      # Lambda = L L^T, lower triangular
        floor = 8.0 * torch.finfo(self._dtype).eps
        if int(info) != 0 or not bool(torch.isfinite(L).all()) or (tau2 is None and float(Ls.diagonal().min()) ** 2 <= floor):
            if tau2 is None:
                raise RuntimeError(f"trend: under the flat prior (trend_prior_var=None) the {p} coefficients are not determined by the data "
                                   f"absorbed so far -- Lambda0 = H^T Sigma^-1 H is singular to the precision of the statistics (fewer than {p} "
                                   f"informative points, or basis functions that the data cannot tell apart in {self._dtype}: a squared pivot of "
                                   "Lambda0, in the basis scaled to unit diag G, at or below 8 eps); absorb more points or give trend_prior_var")
            raise RuntimeError("trend: Lambda = Lambda0 + (sigma2 / tau2) I is not positive definite")
        v = cache["trend_g"] - S64 @ b64
        if resid is not None:
            v = v - resid @ pc["pred_mean"][0, :, 0].double()      # C^T M b = S^T b + (C - Q S)^T mu0: the same correction for v
        beta = torch.cholesky_solve(v[:, None], L)[:, 0]
        pc["trend"] = {"S": St.t().contiguous(), "Lchol": L, "beta": beta, "v": v, "Lambda0": lam0, "ver": pc.get("ver")}
        return pc

    def _trend_state(self):
        if self._trend_deg is None:
            raise RuntimeError("the model was built without trend")
        with torch.no_grad():
            return self.prediction_cache["trend"]

    def trend_coefficients(self):
        """(beta_hat [p], cov [p, p]) of the trend's coefficients given the data, in the normalised basis of ``trend_basis`` (fp64):
        beta_hat = Lambda^-1 v and cov = sigma2 Lambda^-1."""
        tr = self._trend_state()
        p = tr["beta"].shape[0]
        eye = torch.eye(p, dtype=torch.float64, device=self._device)
        return tr["beta"].clone(), self._sigma2(0) * torch.cholesky_solve(eye, tr["Lchol"])

    def trend_basis(self, X):
        """H [n, p]: the monomials of total degree <= the trend's in t_k = (x_k - c_k) / s_k at X [n, d], graded lexicographic
        (1, t_1 .. t_d, t_1^2, t_1 t_2, ...); c and s are the centre and half-extent of the grid the first model of the chain was built
        on.  Defined outside the grid as well (no bounds error is raised for such points)."""
        if self._trend_deg is None:
            raise RuntimeError("the model was built without trend")
        cache = self._kernel_cache
        Xf = X.detach().reshape(-1, self._grid.d).to(self._device, self._dtype).contiguous()
        scratch = grid_ops.new_err_flag(self._device)            # (the basis has no bounds: the model's flag stays as it is)
        return grid_ops.trend_rows(self._grid, Xf, cache["trend_deg"], cache["trend_center"], cache["trend_scale"], None, scratch)

    def trend_evidence(self):
        """log p_trend(y) - log p_0(y) (fp64 scalar): what the marginal likelihood of the data gains by the trend, at the current
        hyper-parameters -- -1/2 log|I + (tau2 / sigma2) Lambda0| + 1/2 v^T Lambda^-1 v / sigma2.  A proper prior only: under the flat
        prior the evidence is defined up to a constant, and a ValueError says so."""
        if self._trend_deg is None:
            raise RuntimeError("the model was built without trend")
        tau2 = self.trend_prior_var
        if tau2 is None:
            raise ValueError("trend_evidence needs a proper prior (trend_prior_var): under the flat prior the evidence is defined up to "
                             "an infinite constant only")
        tr = self._trend_state()
        s2 = self._sigma2(0)
        L, v = tr["Lchol"], tr["v"]
        p = v.shape[0]
        logdet = 2.0 * torch.log(L.diagonal()).sum() + p * math.log(tau2 / s2)      # log|Lambda| + p log(tau2 / sigma2)
        quad = v @ torch.cholesky_solve(v[:, None], L)[:, 0]
        return -0.5 * logdet + 0.5 * quad / s2

    def _refuse_trend(self, what, why):
        if self._trend_deg is not None:
            raise NotImplementedError(f"{what} is not implemented for a model with a trend: {why}")

    def _make_predictive_covar(self, *args, **kwargs):
        return self.prediction_cache["pred_cov"]

    def _root_space_unavailable(self, name):
        raise NotImplementedError(
            f"{name} is a root-space quantity of the reference's dense formulation (L, Q = I + L^T Kuu L); the matrix-free "
            "formulation has no root.  Use prediction_cache / Kuu / Kuu_response, or the dense path for small grids.")

    def _root_space(self):
        """Reference root-space objects (BFN:343-366) for small grids: L = chol(A + jitter),
        Kt L, Q = I + L^T Kt L, L^T Kt b -- dense, on the MFMA GEMM / Cholesky kernels."""
        if not self._use_dense():
            self._root_space_unavailable("root-space quantities")
        rs = self._memo.get("root_space")
        if rs is None:
            Ls, KLs, Qs, projs = [], [], [], []
            b = self._kernel_cache["interpolation_cache"]
            for o, (tcol, s2, _) in enumerate(self._hyper()):
                # L of the reference's UpdatedRootLazyTensor: chol(A + jitter) when first asked for, afterwards carried
                # through every streaming update by the rank-q root update (so it stops being triangular: BFN:343-366 only
                # ever use L L^T = A, which holds)
                L = _wtw_ops(self._kernel_cache["WtW"])[o].root_decomposition().root.evaluate()
                KL = grid_ops.kron_toeplitz_mm(self._grid, tcol, L.t().contiguous(), 1.0 / s2).t().contiguous()     # Kt L
                Q = grid_ops.gemm(L, KL, ta=True)
                Q.diagonal().add_(1.0)                                                                                # add_jitter(1.0), :355
                Kb = grid_ops.kron_toeplitz_mm(self._grid, tcol, b[o, :, 0], 1.0 / s2)
                Ls.append(L); KLs.append(KL); Qs.append(Q); projs.append(grid_ops.gemm(L, Kb[:, None].contiguous(), ta=True))
            st = (lambda xs: xs[0]) if self.num_outputs == 1 else torch.stack
            rs = {"L": st(Ls), "KL": st(KLs), "Q": st(Qs), "proj": st(projs)}
            self._memo["root_space"] = rs
        return rs

    @property
    def current_inducing_compression_matrix(self):
        return self._root_space()["KL"]

    @property
    def current_qmatrix(self):
        return self._root_space()["Q"]

    @property
    def root_space_projection(self):
        return self._root_space()["proj"]

    def _dump_caches(self):
        self._memo.pop("prediction_cache", None)
        self._memo.pop("pending_rank_update", None)
        self._memo.pop("root_space", None)
        # "hyper" (Toeplitz columns + Kronecker eigenbasis) is keyed on the parameters' version
        # counters and survives streaming updates: only a hyper-parameter change invalidates it

    def zero_grad(self, *args, **kwargs):
        # the reference calls gp.zero_grad() after every optimiser step (OSR:146, BFN:416-418): treat it as "the
        # hyper-parameters may have moved".  The memoisation below keys on the parameters' version counters, which a
        # *fused* optimiser (torch.optim.Adam(fused=True)) does not advance -- the epoch covers that.
        self.__dict__["_hyper_epoch"] = self.__dict__.get("_hyper_epoch", 0) + 1
        self._dump_caches()
        return super().zero_grad(*args, **kwargs)

    def hyperparameters_changed(self):
        """Tell the model that hyper-parameters were modified in a way autograd's version counters do not see (fused
        optimisers, writes through .data): every hyper-parameter-dependent cache is recomputed on next use."""
        self.__dict__["_hyper_epoch"] = self.__dict__.get("_hyper_epoch", 0) + 1
        self._dump_caches()

    # -------------------------------------------------------------- forward --
    def train(self, mode=True):
        """As torch's, and the noise model -- held outside the module tree -- follows."""
        if self.__dict__.get("noise_model") is not None:
            self.noise_model.train(mode)
        return super().train(mode)

    def forward(self, X, **kwargs):
        if self.training:
            return self._train_forward(X)
        return self._eval_forward(X)

    def __call__(self, *args, **kwargs):
        if len(args) == 0:
            args = (None,)
        return super().__call__(*args, **kwargs)

    def _train_forward(self, X):
        # dummy: the real action happens in the MLL (:173-203)
        out = self.num_outputs
        n = X.shape[-2] if X is not None else self.num_data
        mean_shape = (out, n) if out > 1 else (n,)
        mean = torch.zeros(mean_shape, dtype=self._dtype, device=self._device)
        if X is None:
            return MultivariateNormal(mean, ZeroLazyTensor(*mean_shape, n, dtype=self._dtype, device=self._device))
        Xf = X.reshape(-1, self._grid.d).to(self._device, self._dtype)
        ops = [InterpolatedKernel(self._grid, Xf, tcol, 1.0, self._err) for tcol, _, _ in self._hyper()]
        return MultivariateNormal(mean, ops[0] if out == 1 else BatchOperator(ops))

    def _eval_forward(self, X):
        grid, out = self._grid, self.num_outputs
        X = X.to(self._device, self._dtype)
        if self._trend_deg is not None:
            if X.dim() > 2:
                self._refuse_trend("a batched posterior (X [..., n, d])", "the trend's rank-p term is formed for one set of query points")
            if torch.is_grad_enabled() and X.requires_grad:
                self._refuse_trend("a posterior differentiable in X", "the trend rows R* = H* - W* S have no backward")
        block = None
        lead = X.shape[:-1]
        if X.dim() > 2:
            block = X.shape[-2]
        Xf = X.reshape(-1, grid.d).contiguous()
        # gradients w.r.t. the query points (acquisition optimisers): the values below are computed exactly as without them, the
        # backward of each moment is attached to the grad-tracking points Xg (DESIGN.md "Posterior gradients").  detach_interp_coeff
        # detaches the covariance's W* only, as BFN:22-28 does
        Xg = Xf if torch.is_grad_enabled() and Xf.requires_grad else None
        Xf = Xf.detach()
        Xg_cov = None if settings.detach_interp_coeff.on() else Xg
        n = Xf.shape[0]
        # smooth kernel on a large grid, variances wanted: the variance of the batch comes from the spectral factor (no solve at
        # all, with a per-query truncation bound).  The MEAN comes from the warm-started PCG state whenever that is current
        # (it carries its own tolerance and costs one gather).  Where it is not -- the hyper-parameters have moved since the
        # last solve, or no solve has run yet: a streaming wrapper that takes an MLL step per batch keeps a factor current for
        # that step anyway, while a PCG mean would first re-solve the preconditioner's eigenproblems and then iterate -- the
        # factor serves the mean too, but only while its mean monitor is green (sqrt(tail(w) b^T (Kt - Kt_B) b), evaluated every
        # few states: the variance bound does not control the mean).
        sq = None
        ms = self._mean_state
        pcg_current = self._memo.get("prediction_cache") is not None or (ms is not None and ms.get("ver") == self._hyper_version())
        hypers_moved = not pcg_current and ms is not None          # (means only, no PCG state at all: a cold solve, then warm ones)
        factor_mean = False
        try_spectral = settings.skip_posterior_variances.off() or (hypers_moved and self._spectral_in_use())
        if not try_spectral and self._use_dense() and self._spectral_in_use():
            try_spectral = True                      # small grid, means only (the classifier's predict): a factor in use serves them too
        if try_spectral and self._use_dense():
            # small grid: the cached nodal factor (M: two gathers per request, rank-q updates after conditioning at fixed hyper-parameters --
            # acquisition loops, fantasies) answers whenever it is current or one rank-q update away; the spectral factor serves the requests
            # that follow a hyper-parameter step (its refresh stays on the device), and only where somebody -- an MLL step, evaluate() --
            # has already built it
            pend = self._memo.get("pending_rank_update")
            dense_current = self._memo.get("prediction_cache") is not None or (pend is not None and pend[3] == self._hyper_version())
            facs = self.__dict__.get("_spectral", {})
            have_factor = all((f := facs.get(o)) is not None and f.ref is not None and not f.stale for o in range(out))
            try_spectral = have_factor and not dense_current
        if try_spectral:
            sps = [self._spectral_state(o) for o in range(out)]
            if all(sp is not None for sp in sps):
                if not pcg_current:
                    self._measure_factor_means(sps)
                    pcg_current = self._memo.get("prediction_cache") is not None      # (a measurement leaves a current PCG state behind)
                sq = [sp[0].query(sp[1], Xf, sp[2]) for sp in sps]
                factor_mean = not pcg_current and all(sp[0].mean_ok for sp in sps)
        pc = None
        if factor_mean:
            mean = torch.stack([s_.mean() for s_ in sq], dim=1)                   # [n, out] fp64
            scale = mean.abs().amax(0)
            for o, sp in enumerate(sps):
                sp[0].mean_monitor(sp[1], sq[o], self._kernel_cache["interpolation_cache"][o, :, 0], sp[2], scale[o])
            factor_mean = all(sp[0].mean_ok for sp in sps)                         # (a verdict read just now may have turned it off)
            mean = mean.to(self._dtype)
            if factor_mean:
                mean = with_input_grad(Xg, mean, lambda G: sum(q_.mean_grad(G[:, o]) for o, q_ in enumerate(sq)))
        if not factor_mean:
            pc = self.prediction_cache
            if Xg is None:
                mean = grid_ops.gather(grid, Xf, pc["pred_mean"][..., 0], self._err)  # [n, out]   left_interp, :206-210
            else:
                mean = grid_ops.Gather.apply(grid, Xg, pc["pred_mean"][..., 0], self._err)    # (the same launch, differentiable)
        trend_rows = None
        if self._trend_deg is not None:
            # mean = W* mu0 + R* beta with R* = H* - W* S (one fused gather); the covariance gains sigma2 R* Lambda^-1 R*^T below
            tr, kc = pc["trend"], self._kernel_cache
            trend_rows = grid_ops.trend_rows(grid, Xf, kc["trend_deg"], kc["trend_center"], kc["trend_scale"], tr["S"], self._err)
            mean = mean + (trend_rows.double() @ tr["beta"]).to(self._dtype)[:, None]
        if settings.deferred_bounds_check.off():
            flag = grid_ops.read_flag(self._err)       # gpytorch raises inside this call for queries outside the grid
            if flag:
                self._raise_out_of_bounds(flag)
        if settings.skip_posterior_variances.on():
            covs = None
        else:
            chunk = settings.variance_chunk.value()
            if sq is not None:
                posts = [None] * out
            else:
                posts = pc["pred_cov"].ops if out > 1 else [pc["pred_cov"]]
            covs = [PredictiveCovariance(_wtw_post, Xf, self._hyper()[o][1] if self.has_learnable_noise else 1.0, self._err, chunk=chunk,
                                         block=block if X.dim() > 2 else None, spectral=None if sq is None else (lambda o=o: sq[o]), xg=Xg_cov)
                    for o, _wtw_post in enumerate(posts)]
        if covs is not None and settings.fast_pred_samples.on():
            # BFN:229-243: hand out a root form of the covariance where a factor provides one (else the exact covariance, as always)
            covs = [(c.root_decomposition() or c) for c in covs]
        if covs is not None and trend_rows is not None:
            from ..lazy.trend import TrendCovariance

            covs = [TrendCovariance(covs[0], trend_rows, pc["trend"]["Lchol"], self._hyper()[0][1] if self.has_learnable_noise else 1.0)]
        # output shapes follow :248-252
        if out == 1:
            mean_o = mean[:, 0].reshape(lead)
            if covs is None:
                cov = ZeroLazyTensor(*lead, lead[-1], dtype=self._dtype, device=self._device)
            else:
                cov = covs[0]
            return MultivariateNormal(mean_o, cov)
        mean_o = mean.t().reshape((out,) + tuple(lead))
        if covs is None:
            cov = ZeroLazyTensor(out, *lead, lead[-1], dtype=self._dtype, device=self._device)
        else:
            cov = BatchOperator(covs)
        return MultivariateNormal(mean_o, cov)

    def posterior_jet(self, X, joint=False):
        """Joint Gaussian posterior of ``f`` and ``grad f`` at X [n, d]: a :class:`~online_gp_amd.lazy.jet.JetPosterior`
        with ``mean`` [n, d + 1] and ``covariance`` [n, d + 1, d + 1] -- or, with ``joint``, the [n (d + 1), n (d + 1)] covariance
        between all points, point-major.  Channel 0 is the value (its variance is that of ``posterior(X)``), channel 1 + q the
        partial derivative in dim q, which is identically zero in a boundary cell of dim q.  Answered through the prediction cache in
        every regime (a model inside a stencil shard leaves it, as for every solve).  Outputs are detached: the cubic interpolant is
        C^1 only, so a derivative of the jet with respect to X jumps at the cell faces.  One output, unbatched X."""
        from ..lazy.jet import JetCovariance, JetPosterior

        self._refuse_trend("posterior_jet", "the jet rows of the basis (h and its gradient) are not built")
        if self.num_outputs > 1:
            raise NotImplementedError("posterior_jet is implemented for a single output")
        if X.dim() > 2:
            raise NotImplementedError("posterior_jet takes unbatched points [n, d]")
        grid = self._grid
        Xf = X.detach().reshape(-1, grid.d).to(self._device, self._dtype).contiguous()
        with torch.no_grad():
            pc = self.prediction_cache
            mean = grid_ops.gather_jet(grid, Xf, pc["pred_mean"][0, :, 0], self._err)[:, 0, :]
            if settings.deferred_bounds_check.off():
                flag = grid_ops.read_flag(self._err)
                if flag:
                    self._raise_out_of_bounds(flag)
            sigma2 = self._hyper()[0][1] if self.has_learnable_noise else 1.0
            op = JetCovariance(pc["pred_cov"], Xf, sigma2, self._err, chunk=settings.variance_chunk.value())
            cov = op.joint() if joint else op.blocks()
        post = JetPosterior(mean, cov, joint)
        post.cg_iters = op.cg_iters
        return post

    def posterior_integral(self, lower, upper, joint=False, average=False):
        """Gaussian posterior of the integral of ``f`` over the boxes ``[lower_b, upper_b]`` ([B, d] each): an
        :class:`~online_gp_amd.lazy.quadrature.IntegralPosterior` with ``mean`` [B], ``variance`` [B], ``volume`` [B] and, with ``joint``,
        the [B, B] ``covariance`` between the boxes.  Exact under the SKI model, one solve column per box whatever its size.  A
        dimension with ``lower == upper`` is evaluated at that coordinate instead of integrated (line and plane integrals, marginal
        curves; a box degenerate in every dimension is ``posterior`` at that point).  The interpolant is zero outside the grid, so
        a box is clipped to the grid's extent -- and, as a point outside the grid does, a box not wholly inside raises unless
        ``settings.deferred_bounds_check`` is on.  ``average``: the mean is divided by the clipped volume and the covariance by the
        volumes' outer product (a box of zero clipped volume has mean 0 and variance 0).  Answered through the prediction cache in
        every regime.  Outputs are detached.  One output, unbatched bounds.  The bounds are checked in the precision they are given
        in and then cast to the model's: a box that the cast would collapse in some dimension (narrower than one ulp of the model's dtype)
        is refused with ``ValueError`` rather than silently evaluated instead of integrated."""
        from ..lazy.quadrature import BoxCovariance, IntegralPosterior, check_bounds_host, scale_by_volume

        self._refuse_trend("posterior_integral", "the box integrals of the basis are not built")
        if self.num_outputs > 1:
            raise NotImplementedError("posterior_integral is implemented for a single output")
        grid = self._grid
        lo, hi = check_bounds_host(lower, upper, grid.d, "posterior_integral", self._device, self._dtype)
        with torch.no_grad():
            pc = self.prediction_cache
            tables = grid_ops.box_tables(grid, lo, hi, self._err)
            mean = grid_ops.gather_box(grid, tables, pc["pred_mean"][0, :, 0])[:, 0]
            if settings.deferred_bounds_check.off():
                flag = grid_ops.read_flag(self._err)
                if flag:
                    self._raise_out_of_bounds(flag)
            sigma2 = self._hyper()[0][1] if self.has_learnable_noise else 1.0
            op = BoxCovariance(pc["pred_cov"], tables, sigma2, self._err, chunk=settings.variance_chunk.value())
            cov = op.joint() if joint else op.diag()
            if average:
                s = scale_by_volume(tables.vol)
                mean = mean * s
                cov = cov * s[:, None] * s[None, :] if joint else cov * s * s
        post = IntegralPosterior(mean, cov, tables.vol, joint)
        post.cg_iters = op.cg_iters
        return post

    # -------------------------------------------------------------- updates --
    def condition_on_observations(self, X, Y, noise=None, inplace=False, _decay=True, *, grad_Y=None, grad_noise=None, grad_mask=None,
                                  lower=None, upper=None, counts=None, exposure=None, trials=None, input_var=None, grad_lower=None, grad_upper=None,
                                  labels=None):
        """a7, :258-285.  inplace: the statistics buffers are updated where they
        live (O(4^{2d}) atomics per point); otherwise they are cloned first and a
        sibling model sharing covar_module / likelihood is returned.  With a ``forgetting_factor`` the statistics -- of the clone,
        in the functional form -- decay once before the batch is absorbed (not for fantasies: batched conditioning,
        ``get_fantasy_model``).

        With ``robust_c`` set on the model, an unbatched batch is Huber-weighted against the posterior before it (after growing and
        decaying) and absorbed at noise ``noise_i / omega_i`` in the same launch (``_absorb_robust``);
        ``last_robust_weights`` -- of the returned model, in the functional form -- then holds ``omega`` [q].  Batched X (fantasies)
        ignores ``robust_c``: fantasised targets come from the model itself.  ``"noise"`` scaling (1 / sqrt(sigma2 noise_i)) presumes
        a model that already tracks the signal; ``"predictive"`` adds the posterior variance at X (one more solve).

        With ``window=N`` set on the model, an unbatched batch enters the statistics and the model's ring of the last N points, and
        the points whose slots it takes leave them again, in the same launch (``_absorb_window``): afterwards the model
        is the GP of ``window_points()``, and ``num_data`` their number.  A batch larger than N is split on the host.  Fantasies
        (batched X, ``get_fantasy_model``) add hypothetical points and retire nothing.

        ``grad_Y`` [n, d]: observations of the gradient of f at X, absorbed with the values in the same launch;
        ``Y=None`` then means gradient-only.  ``grad_noise`` [n, d] or [n]: their noise (None: the value observation's, or unit
        noise); ``grad_mask`` bool [n, d]: which partials were observed (None: all).  ``num_data`` grows by the number of scalar
        observations.  Single output, unbatched X.

        ``lower`` / ``upper`` [n] with ``Y=None``: interval and censored observations, lower_i <= f(x_i) + eps_i <= upper_i -- a missing
        side is -inf / +inf, equal ends are an exact value (``_condition_interval``).  Every point is moment-matched
        against the posterior before the batch (after growing and decaying) and absorbed as the pseudo-target ytilde_i at noise
        ``noise_i / omega_i`` in the same launch; ``last_interval_sites`` -- of the returned model, in the functional form -- then
        holds ``(ytilde, omega, log_z)``.  This is parallel assumed-density filtering: an approximation of the non-Gaussian
        posterior, whose MLL is the Gaussian MLL of the pseudo-data; ``log_z.sum()`` is the prequential evidence of the batch.  A
        point with nothing to say (omega = 0) enters nothing and does not count in ``num_data``.  Single output, unbatched X.

        ``counts`` [n] with ``Y=None``: count observations (``_condition_count``) -- ``counts_i ~ Poisson(exposure_i
        exp f(x_i))`` (``exposure`` None: 1), or with ``trials`` given ``counts_i`` successes of ``trials_i`` at success probability
        sigmoid(f(x_i)).  Moment-matched and absorbed like bounds, at the effective noise variance ``1 / tau_i``;
        ``last_count_sites`` holds ``(ytilde, omega, log_z)`` with ``omega = sigma2 tau``.  Single output, unbatched X.

        ``input_var`` -- a scalar, [d], [n] or [n, d] -- with targets ``Y``: the recorded locations X are off by an error of that
        variance per dimension, in the units of X squared (``_condition_input_noise``).  To first order the error is
        extra output noise ``sum_k input_var_k E[(d_k f)^2]`` under the posterior before the batch (after growing and decaying;
        ``input_noise_slope="mean"``: the squared slope of the posterior mean alone), and the point enters as ``Y_i`` at noise
        ``noise_i / omega_i`` in the same launch; ``last_input_noise_sites`` then holds ``(omega, log_z, grad_mean)``.  A model built
        with ``input_var`` applies it to every unbatched update that passes none.  Single output, unbatched X.

        ``grad_lower`` / ``grad_upper`` -- a scalar, [d] or [n, d]; a missing side is -inf / +inf -- bound the partial derivatives:
        grad_lower_iq <= d_q f(x_i) + eps_iq <= grad_upper_iq (``_condition_grad_interval``; "increasing in dim q" is
        ``monotone_bounds``).  ``grad_noise`` and ``grad_mask`` as for ``grad_Y`` (for a sign constraint pass a small ``grad_noise``).
        The value of a point may be given as ``Y`` (exact), as ``lower`` / ``upper`` (an interval) or not at all.  Every present
        channel is moment-matched like a bound on a value, against its own mean and variance under ``posterior_jet`` before the
        batch, and all of them are absorbed in one launch; ``last_grad_interval_sites`` holds ``(ytilde, omega, log_z)``, [n, d + 1]
        each.  ``num_data`` grows by the channels that entered.  No ``grad_Y`` beside them (an exact partial is equal bounds).  Single
        output, unbatched X.

        ``labels`` [n] with ``Y=None`` on a model of ``C = num_outputs >= 2`` outputs: categorical observations, ``labels_i`` in
        {0 .. C - 1} the class of ``argmax_c (f_c(x_i) + eps_c)``, ``eps_c ~ N(0, sigma2_c noise_i)`` -- the multinomial probit
        (``_condition_labels``).  Every point is moment-matched against the C posteriors before the batch and output c
        takes it as the pseudo-target ``ytilde_ci`` at noise ``noise_i / omega_ci``, all outputs in one launch; ``last_label_sites``
        holds ``(ytilde [C, n], omega [C, n], log_z [n])``.  A class far below the label's says nothing and is skipped for its output
        alone; a label that is no class skips the point.  ``num_data`` grows by the points whose label class entered.  Unbatched X.

        On a model built with ``heteroscedastic=True`` the noise of a point is ``sigma2 noise_i exp g(x_i)``, g the field of
        ``noise_model`` (``_condition_hetero``): against the two posteriors before the batch a point enters f as ``Y_i``
        at noise ``noise_i e_i``, ``e = E[exp g]``, and its squared residual, deflated by the share that is f's own uncertainty, enters
        the noise model as a log-variance site, both in one launch; ``last_hetero_sites`` holds ``(e, ytilde_g, tau_g, log_z_g, log_z_y)``.
        Targets ``Y`` with ``noise`` at most, no other form in the same call.  Single output, unbatched X."""
        if self.noise_model is not None:
            given = dict(grad_Y=grad_Y, grad_noise=grad_noise, grad_mask=grad_mask, lower=lower, upper=upper, counts=counts, exposure=exposure,
                         trials=trials, input_var=input_var, grad_lower=grad_lower, grad_upper=grad_upper, labels=labels)
            others = [k for k, v in given.items() if v is not None]
            if others:
                raise NotImplementedError(f"a heteroscedastic model takes targets Y, with noise at most: no {', '.join(others)} (the noise "
                                          "site is that of a Gaussian residual, and no kernel applies two forms in one launch)")
            return self._condition_hetero(X, Y, noise, inplace, _decay)
        if labels is not None:
            given = dict(Y=Y, grad_Y=grad_Y, grad_noise=grad_noise, grad_mask=grad_mask, lower=lower, upper=upper, counts=counts, exposure=exposure,
                         trials=trials, input_var=input_var, grad_lower=grad_lower, grad_upper=grad_upper)
            others = [k for k, v in given.items() if v is not None]
            if others:
                raise NotImplementedError(f"a batch of labels is given as labels, with noise at most: no {', '.join(others)}")
            return self._condition_labels(X, labels, noise, inplace, _decay)
        if input_var is None and self.input_var is not None and X.dim() <= 2 and (Y is None or Y.dim() <= 2):
            input_var = self.input_var
        if input_var is not None:
            given = dict(grad_Y=grad_Y, grad_noise=grad_noise, grad_mask=grad_mask, lower=lower, upper=upper, counts=counts, exposure=exposure, trials=trials,
                         grad_lower=grad_lower, grad_upper=grad_upper)
            return self._condition_input_noise(X, Y, noise, input_var, inplace, _decay, [k for k, v in given.items() if v is not None])
        if counts is not None or exposure is not None or trials is not None:
            if self._trend_deg is not None:
                self._refuse_trend("count observations (counts)", "a site is matched against the grid mean alone, which under a trend "
                                   "is not the predictive mean")
            if (Y is not None or noise is not None or grad_Y is not None or grad_noise is not None or grad_mask is not None or lower is not None
                    or upper is not None or grad_lower is not None or grad_upper is not None):
                raise NotImplementedError("a batch of counts is given as counts with exposure or trials alone: no Y, noise, grad_* or lower / upper "
                                          "(a count has no Gaussian noise of its own)")
            return self._condition_count(X, counts, exposure, trials, inplace, _decay)
        if grad_lower is not None or grad_upper is not None:
            return self._condition_grad_interval(X, Y, noise, lower, upper, grad_Y, grad_lower, grad_upper, grad_noise, grad_mask, inplace, _decay)
        if self._trend_deg is not None:
            if lower is not None or upper is not None:
                self._refuse_trend("interval observations (lower / upper)", "a site is matched against the grid mean alone, which under a trend "
                                   "is not the predictive mean")
            if grad_Y is not None:
                self._refuse_trend("derivative observations (grad_Y)", "the trend statistics take value rows only (no gradient of the basis)")
            if X.dim() > 2 or (Y is not None and Y.dim() > 2):
                self._refuse_trend("batched conditioning (fantasies)", "a fantasy batch carries A and b only, not the trend statistics")
        if lower is not None or upper is not None:
            if grad_Y is not None or grad_noise is not None or grad_mask is not None:
                raise NotImplementedError("interval observations bound values only: lower / upper take no grad_Y")
            return self._condition_interval(X, Y, noise, lower, upper, inplace, _decay)
        if grad_Y is not None and self.robust_c is not None:
            raise NotImplementedError("robust_c weights value observations only: a model built with it takes no grad_Y")
        if grad_Y is not None and self.window is not None:
            raise NotImplementedError("window stores value observations only: a model built with it takes no grad_Y")
        if grad_Y is not None:
            return self._condition_on_gradients(X, Y, noise, inplace, _decay, grad_Y, grad_noise, grad_mask)
        if grad_noise is not None or grad_mask is not None:
            raise ValueError("grad_noise / grad_mask describe grad_Y, which was not given")
        if X.dim() > 2 or Y.dim() > 2:
            # batch-expanded conditioning (what OSB.fantasize asks for, OSB:51-61): a batch of conditioned copies
            if inplace:
                raise RuntimeError("batched conditioning returns a batch of models and cannot be done in place")
            from .fantasy import BatchedFantasyModel

            return BatchedFantasyModel(self, X, Y, noise)
        if Y.dim() == 1:
            Y = Y[:, None]
        if noise is not None:
            noise = self._canon_noise(noise, Y)
        q = X.reshape(-1, self._grid.d).shape[0]
        if self.grow_grid:
            self.grow_to_cover_(X)                   # (exact: the functional form grows this model too, its posterior does not move)
        gamma = self._gamma(_decay)
        if self.robust_c is not None:
            # weigh, absorb: the weights are taken against the posterior of the statistics the batch is added to
            return self._condition(lambda model, cache, src: model._absorb_robust(cache, X, Y, noise, src), inplace, gamma, reads_posterior=True)
        if self.window is not None and _decay:       # (_decay=False: a fantasy adds hypothetical points and retires nothing)
            # the batch enters the statistics and the ring, what the ring's slots held leaves.  The grid may grow
            # under a window (grow_grid, a growing regrid_): the ring holds coordinates, not node indices, so a stored point finds its
            # nodes on the grown grid when it leaves -- which is also why no node may be removed.  The functional form clones the ring
            # with the cache
            new_gp = self._condition(lambda model, cache, src: model._absorb_window(cache, X, Y, noise), inplace, None)
            (self if inplace else new_gp)._window_rebuild_due()
            return new_gp
        old_pc = None if gamma is not None else self._rank_update_source(q)      # (a rank-q update starts from the factor of the undecayed A)

        def absorb(model, cache, src):
            model._absorb(cache, X, Y, noise, init=False)
            return q

        new_gp = self._condition(absorb, inplace, gamma)
        self._seed_rank_updated_cache(self if inplace else new_gp, old_pc, X, noise, Y)
        return new_gp

    def _gamma(self, decay=True):
        """The factor an update decays the statistics by before it absorbs its batch, or None: no forgetting_factor, a factor of
        one, or an update that is a what-if on the current state (decay False: fantasies)."""
        gamma = self.forgetting_factor if decay else None
        return None if gamma == 1.0 else gamma

    def _condition(self, absorb, inplace, gamma, reads_posterior=False):
        """The skeleton of condition_on_observations, for every observation form.  `absorb(model, cache, src)` absorbs the form's batch
        into `cache`, the kernel cache of `model`, and returns what num_data grows by (None: the form keeps the count itself, as the
        window does from its ring).  In place: decay, absorb, count, dump the caches.  Functional: the same on a sibling model with a
        clone of the cache -- the clone's buffers decay, the parent keeps its statistics bit for bit -- which then starts its mean
        solve warm from a copy of this model's state, in this model's mode, and is returned.
        reads_posterior: the form takes weights or sites against the posterior of the statistics the batch is added to, that of `src`.
        In place that is this model.  Functional without a decay it is this model too, whose statistics the clone still equals and
        whose posterior is usually already solved; after a decay it is the sibling, which therefore gets its warm start before the
        absorb instead of after it."""
        if inplace:
            if gamma is not None:
                self.forget_(gamma)
            grown = absorb(self, self._kernel_cache, self)
            if grown is not None:
                self.num_data = self.num_data + grown
            self._dump_caches()
            return None
        new_cache = self._clone_cache(self._kernel_cache)
        new_gp = self._sibling(new_cache, self.num_data)
        if gamma is not None:
            new_gp._decay(gamma, self.num_data)          # the clone's buffers: the parent keeps its statistics bit for bit
        warm_first = reads_posterior and gamma is not None
        if warm_first:
            self._sibling_mean_state(new_gp)             # (warm start of the solve the weights / sites need)
        grown = absorb(new_gp, new_cache, new_gp if warm_first else self)
        if grown is not None:
            new_gp.num_data = self.num_data + grown
        new_gp._dump_caches()                            # (a prediction cache the weights / sites were read from predates the batch)
        if not warm_first:
            self._sibling_mean_state(new_gp)
        return new_gp

    def _sibling(self, new_cache, num_data):
        """The model the functional form returns, before its batch is absorbed: this model's modules, `new_cache` (a clone of the
        kernel cache), this model's noise-weight sums."""
        new_gp = type(self)(
            covar_module=self.covar_module,
            kernel_cache=new_cache,
            learn_additional_noise=self.has_learnable_noise,
            likelihood=self.likelihood,
            num_data=num_data,
            forgetting_factor=self.forgetting_factor,
            grow_grid=self.grow_grid,
            max_grid_size=self.max_grid_size,
            robust_c=self.robust_c,
            robust_scale=self.robust_scale,
            window=self.window,
            window_rebuild_every=self.window_rebuild_every,
            site_memory=self.site_memory,
            site_refine_sweeps=self.site_refine_sweeps,
            site_refine_damping=self.site_refine_damping,
            trend_prior_var=self.trend_prior_var,        # (the degree travels with the cache)
            input_var=self.input_var,
            input_noise_slope=self.input_noise_slope,
            log_noise_mean=self.log_noise_mean,
            noise_model=self._noise_sibling(),
        )
        new_gp._win_voids, new_gp._win_updates = self._win_voids, self._win_updates
        new_gp._wsum_dev = self._wsum_dev.clone()
        new_gp._wsum_host = list(self._wsum_host)
        new_gp._wsum_dev_host = list(self._wsum_dev_host)
        new_gp._wsum_dirty = self._wsum_dirty
        return new_gp

    def _sibling_mean_state(self, new_gp):
        """After the sibling's absorb: it starts its mean solve warm from a copy of this model's state, and in this model's mode."""
        if self._mean_state is not None:
            new_gp._mean_state = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in self._mean_state.items()}
            new_gp._mean_state["R_ok"] = False          # the copied residual predates the increment just absorbed
        if not self.training:
            new_gp.eval()

    # ---------------------------------------------- derivative observations --
    def _condition_on_gradients(self, X, Y, noise, inplace, _decay, grad_Y, grad_noise, grad_mask):
        """condition_on_observations with grad_Y: the batch becomes [n, d + 1] channel tensors -- column 0 the value,
        column 1 + q the partial in dim q, each with its noise and a presence flag -- and one launch absorbs them."""
        d = self._grid.d
        if self.num_outputs > 1:
            raise NotImplementedError("derivative observations are implemented for a single output")
        if X.dim() > 2 or grad_Y.dim() > 2 or (Y is not None and Y.dim() > 2):
            raise NotImplementedError("derivative observations cannot be fantasised: batched conditioning (X [..., n, d]) takes values only")
        if "path_probes" in self._kernel_cache:
            raise NotImplementedError("a model with path probes cannot absorb derivative observations (its probes follow value rows only)")
        X = X.reshape(-1, d).to(self._device, self._dtype).contiguous()
        n = X.shape[0]
        dev, dt = self._device, self._dtype
        if tuple(grad_Y.shape) != (n, d):
            raise ValueError(f"grad_Y must be [{n}, {d}], got {tuple(grad_Y.shape)}")
        Yc = torch.zeros((n, d + 1), dtype=dt, device=dev)
        Nc = torch.ones((n, d + 1), dtype=dt, device=dev)
        present = torch.ones((n, d + 1), dtype=torch.bool, device=dev)
        Yc[:, 1:] = grad_Y.to(dev, dt)
        if Y is None:
            present[:, 0] = False
        else:
            Yc[:, 0] = Y.to(dev, dt).reshape(n)
            if noise is not None:
                Nc[:, 0] = noise.to(dev, dt).reshape(n)
        if grad_noise is None:
            Nc[:, 1:] = Nc[:, :1]                        # the value observation's noise (unit noise without one)
        else:
            gn = grad_noise.to(dev, dt)
            Nc[:, 1:] = gn[:, None] if gn.dim() == 1 else gn
        if grad_mask is not None:
            if tuple(grad_mask.shape) != (n, d):
                raise ValueError(f"grad_mask must be [{n}, {d}], got {tuple(grad_mask.shape)}")
            present[:, 1:] = grad_mask.to(dev, torch.bool)
        q = n * (d + 1 if Y is not None else d) if grad_mask is None else int(present.sum())     # scalar observations
        if self.grow_grid:
            self.grow_to_cover_(X)

        def absorb(model, cache, src):
            model._absorb_grad(cache, X, Yc, Nc, present)
            return q

        return self._condition(absorb, inplace, self._gamma(_decay))

    def _absorb_grad(self, cache, X, Yc, Nc, present, half_delta=None):
        """_absorb for [n, d + 1] channel tensors (values Yc, noises Nc, bool present), one launch (wiski_absorb with channels = d + 1).  The
        carried residual follows when the mean state is current.  What a derivative row cannot be followed through is given up
        rather than updated: the spectral factor is marked stale (it rebuilds from the stencil, exactly), the two-level block is
        lost, a carried root pair is dropped, and no rank update is prepared."""
        op = self._native_half_op(cache, "derivative observations", half_delta)
        if "path_probes" in cache:
            raise NotImplementedError("derivative observations: no path probes (they follow value rows only)")
        mine = self._before_launch(cache)
        zero, one = torch.zeros((), dtype=self._dtype, device=self._device), torch.ones((), dtype=self._dtype, device=self._device)
        wb = torch.where(present, 1.0 / Nc, zero)
        wa = torch.where(present, self._weight_a(Nc, False), zero)
        no = torch.where(present, Nc, one)               # an absent channel: wa = wb = 0, noise = 1 -- nothing anywhere
        Yc = torch.where(present, Yc, zero)
        ms = self._carried(mine)
        grid_ops.scatter_stats_grad(self._grid, X, Yc, wa, wb, no, cache["interpolation_cache"][0, :, 0], op.stencil, cache["_cnt"][0],
                                    cache["_stats"][0], self._err, u=ms["U"][0] if ms else None, res=ms["R"][0] if ms else None)
        self._give_up(cache)                             # L L^T described the matrix without these rows
        if mine:
            # the noise-weight sum (preconditioner shift only) is the mass of cnt, to which a derivative channel adds its diagonal
            self._wsum_dev = cache["_cnt"].sum(dim=1, dtype=torch.float64)
            self._wsum_host = [0.0] * self.num_outputs
            self._wsum_dirty = True

    # ------------------------------------------------- outlier-robust absorb --
    def _robust_inputs(self, X, noise):
        """(u [m], inv_scale [n]) of a batch under THIS model's current posterior: the grid mean from the prediction cache (every
        regime keeps one), and 1 / sqrt(sigma2 noise_i) ("noise") or 1 / sqrt(var_i + sigma2 noise_i) ("predictive", var_i the
        posterior variance at x_i: one more solve on the paths every posterior call takes)."""
        u = self.prediction_cache["pred_mean"][0, :, 0]
        s2 = self._sigma2(0)
        scale2 = noise.clamp_min(1e-7) * s2                  # (the floor _weight_a gives the noise of an update)
        if self.robust_scale == "predictive":
            with torch.no_grad(), settings.skip_posterior_variances(False):
                var = self._eval_forward(X).variance.reshape(-1).to(self._dtype)
            scale2 = scale2 + var.clamp_min(0.0)
        return u, scale2.rsqrt()

    def _absorb_robust(self, cache, X, Y, noise, src):
        """_absorb of one value-only batch with Huber weights, one launch (wiski_absorb_robust).  `src`: the model whose
        posterior the weights are taken against -- this one, or in the functional form without a decay the parent, whose statistics
        the clone still equals.  Everything that follows the stream point by point receives the effective weights wa omega and
        wb omega: a carried root pair, the spectral factor, the path probes, the noise-weight sum.  The two-level block is given up
        (a model with robust_c never takes the fused streaming step that feeds it) and the dense rank-update seed is skipped: the
        next posterior is factored afresh."""
        op = self._native_half_op(cache, "robust_c")
        X, y, no, wa, wb = self._canon_batch(X, Y, noise)
        u, inv_scale = src._robust_inputs(X, no)             # (finishes whatever is pending, leaves a stencil shard)
        targets, res = self._site_targets(cache, op, u)
        omega = grid_ops.scatter_stats_robust(self._grid, X, y, wa, wb, no, inv_scale, self.robust_c, *targets, res=res)
        self.last_robust_weights = omega
        return self._follow_sites(cache, X, wa, wb, y, omega)

    def _site_targets(self, cache, op, u):
        """What a site-weighted absorb (grid_ops.scatter_stats_robust / _interval / _count) writes, as the tail of its argument
        list: (b, A_half, cnt, stats, err, u) and res, the carried residual where one is kept."""
        ms = self._carried(self._before_launch(cache), u=u)
        return (cache["interpolation_cache"][0, :, 0], op.stencil, cache["_cnt"][0], cache["_stats"][0], self._err, u), ms["R"][0] if ms else None

    def _follow_sites(self, cache, X, wa, wb, ytilde, omega):
        """After a site-weighted absorb: everything that follows the stream point by point receives the targets ytilde at the
        effective weights wa omega, wb omega.  Returns the number of points of the batch."""
        n = X.shape[0]
        if n:
            self._two_level_lose()                           # (its block is rebuilt from the stencil where one is wanted again)
            self._follow(cache, 0, X, wa * omega, ytilde * (wb * omega))     # a skipped point, a point outside the grid: omega = 0, nothing anywhere
        return n

    # ------------------------------------------------ interval observations --
    def _refuse_for_sites(self, X, form, given):
        """What a moment-matched form (`form` observations, given as `given`) does not combine with.  (A site is matched once and never
        revisited -- unless the model keeps it: site_memory and refine_sites_, DESIGN.md 3.28, which has refusals of its own.)"""
        if self.num_outputs > 1:
            raise NotImplementedError(f"{form} observations are implemented for a single output")
        if self.robust_c is not None:
            raise NotImplementedError(f"{form} observations do not combine with robust_c: a site is a weight already, and no kernel applies both")
        if self.window is not None:
            raise NotImplementedError(f"{form} observations do not combine with window: the ring stores targets, and a site depends on the "
                                      "posterior it was matched against")
        if X.dim() > 2:
            raise NotImplementedError(f"batched conditioning (fantasies) takes targets, not {given}")

    def _condition_interval(self, X, Y, noise, lower, upper, inplace, _decay):
        """condition_on_observations with lower / upper: grow, decay, moment-match, absorb.  The sites are taken
        against the posterior of the statistics the batch is added to -- the decayed ones under forgetting."""
        if Y is not None:
            raise NotImplementedError("a batch is given as targets Y or as bounds lower / upper, not both (an exact value is lower == upper)")
        self._refuse_for_sites(X, "interval", "bounds")
        d = self._grid.d
        X = X.reshape(-1, d)
        n = X.shape[0]
        inf = float("inf")
        lo = torch.full((n,), -inf, dtype=self._dtype, device=self._device) if lower is None else lower.to(self._device, self._dtype).reshape(-1)
        hi = torch.full((n,), inf, dtype=self._dtype, device=self._device) if upper is None else upper.to(self._device, self._dtype).reshape(-1)
        if lo.shape[0] != n or hi.shape[0] != n:
            raise ValueError(f"lower / upper must hold one bound per point ([{n}]), got {tuple(lo.shape)} and {tuple(hi.shape)}")
        if noise is not None:
            noise = noise.to(self._device, self._dtype).reshape(-1)
            if noise.shape[0] != n:
                raise ValueError(f"noise must hold one value per point ([{n}]), got {tuple(noise.shape)}")
        if self.grow_grid:
            self.grow_to_cover_(X)
        new_gp = self._condition(lambda model, cache, src: model._absorb_interval(cache, X, lo, hi, noise, src), inplace, self._gamma(_decay),
                                 reads_posterior=True)
        (self if inplace else new_gp)._refine_after_update()
        return new_gp

    def _absorb_matched(self, cache, X, noise, src, form, launch, half_delta=None, pvar_of=None, store=None):
        """_absorb of one batch of moment-matched observations (`form`: what _native_half_op calls them), one launch:
        ``launch(X, pvar, sigma2, wa, wb, noise, b, A_half, cnt, stats, err, u, res=)`` is grid_ops.scatter_stats_interval or
        _count with its data bound.  `src`: the model whose posterior the sites are matched against -- this one, or in the
        functional form without a decay the parent, whose statistics the clone still equals: its grid mean from the prediction
        cache and its posterior variance at X (one more solve on the paths every posterior call takes).  Everything that follows
        the stream point by point receives the effective weights wa omega, wb omega and the pseudo-targets: a carried root pair,
        the spectral factor, the path probes, the noise-weight sum.  The two-level block is given up and the dense rank-update
        seed is skipped, as in _absorb_robust.  Returns the sites and the number of points num_data grows by: those that entered,
        and those outside the grid (which _raise_out_of_bounds takes off again when the flag is read).
        `store`: (form name, d0, d1) of a form the site memory keeps.  On a model built with site_memory the batch is
        then written, with its sites, into the cache's ring behind the launch -- index copies, no further launch of the library; a
        point outside the grid is not stored."""
        op = self._native_half_op(cache, form, half_delta)
        X, _, no, wa, wb = self._canon_batch(X, None, noise)
        u = src.prediction_cache["pred_mean"][0, :, 0]       # (finishes whatever is pending, leaves a stencil shard)
        if pvar_of is not None:                              # (a form that takes more than the variance of f from that posterior)
            pvar = pvar_of(src, X)
        else:
            with torch.no_grad(), settings.skip_posterior_variances(False):
                pvar = src._eval_forward(X).variance.reshape(-1).to(self._dtype).contiguous()
        targets, res = self._site_targets(cache, op, u)
        flag0 = self._err.clone()
        sites = launch(X, pvar, self._sigma2(0), wa, wb, no, *targets, res=res)
        if not self._follow_sites(cache, X, wa, wb, *sites[:2]):
            return sites, 0
        entered, dropped = torch.stack([(sites[1] > 0).sum(), (self._err - flag0).reshape(-1)[0] >> 1]).tolist()
        if store is not None and cache.get("_site_ring") is not None:
            keep = None
            if dropped:                                      # (the kernels' own test: g0 <= x <= last node, in the working precision)
                g = self._grid
                first = torch.tensor(g.g0, dtype=self._dtype, device=self._device)
                last = torch.tensor([g0 + h * (n - 1) for g0, h, n in zip(g.g0, g.h, g.g)], dtype=self._dtype, device=self._device)
                keep = ((X >= first) & (X <= last)).all(dim=1)
            name, d0, d1 = store
            cache["_site_ring"].store(name, X, d0, d1, no, wa, wb, sites[0], sites[1], keep=keep)
        return sites, int(entered) + int(dropped)

    def _absorb_interval(self, cache, X, lo, hi, noise, src, half_delta=None):
        """_absorb_matched with the interval launch (wiski_absorb_interval)."""
        self.last_interval_sites, grown = self._absorb_matched(
            cache, X, noise, src, "interval observations", half_delta=half_delta, store=("interval", lo, hi),
            launch=lambda X, *rest, **kw: grid_ops.scatter_stats_interval(self._grid, X, lo.contiguous(), hi.contiguous(), *rest, **kw))
        return grown

    # --------------------------------------------------- count observations --
    def _count_batch(self, n, counts, exposure, trials):
        """(counts [n], t [n], family) on the model's device in its dtype: ``trials`` given means binomial, otherwise Poisson at
        ``exposure`` (None: 1)."""
        if counts is None:
            raise ValueError("exposure / trials describe counts, which were not given")
        if exposure is not None and trials is not None:
            raise ValueError("counts are Poisson at an exposure or binomial out of trials, not both")
        t = trials if trials is not None else exposure
        y = counts.to(self._device, self._dtype).reshape(-1).contiguous()
        t = torch.ones(n, dtype=self._dtype, device=self._device) if t is None else t.to(self._device, self._dtype).reshape(-1).contiguous()
        if y.shape[0] != n or t.shape[0] != n:
            raise ValueError(f"counts and exposure / trials must hold one value per point ([{n}]), got {tuple(y.shape)} and {tuple(t.shape)}")
        return y, t, "binomial" if trials is not None else "poisson"

    def _condition_count(self, X, counts, exposure, trials, inplace, _decay):
        """condition_on_observations with counts: grow, decay, moment-match, absorb -- _condition_interval with the
        count launch.  The sites are taken against the posterior of the statistics the batch is added to."""
        self._refuse_for_sites(X, "count", "counts")
        X = X.reshape(-1, self._grid.d)
        y, t, family = self._count_batch(X.shape[0], counts, exposure, trials)
        if self.grow_grid:
            self.grow_to_cover_(X)
        new_gp = self._condition(lambda model, cache, src: model._absorb_count(cache, X, y, t, family, src), inplace, self._gamma(_decay),
                                 reads_posterior=True)
        (self if inplace else new_gp)._refine_after_update()
        return new_gp

    def _absorb_count(self, cache, X, y, t, family, src, half_delta=None):
        """_absorb_matched with the count launch (wiski_absorb_count), at noise = wa = wb = 1 -- the effective noise
        variance of a point is sigma2 / omega = 1 / tau."""
        self.last_count_sites, grown = self._absorb_matched(
            cache, X, None, src, "count observations", half_delta=half_delta, store=(family, y, t),
            launch=lambda X, *rest, **kw: grid_ops.scatter_stats_count(self._grid, X, y, t, family, *rest, **kw))
        return grown

    # ------------------------------------------------------- site memory --
    def _refine_after_update(self):
        """site_refine_sweeps sweeps behind an interval or count update of a model with site memory."""
        if self.site_memory is not None and self.site_refine_sweeps > 0:
            self.refine_sites_(self.site_refine_sweeps, self.site_refine_damping)

    def _site_ring(self, what):
        if self.site_memory is None:
            raise RuntimeError(f"{what}: the model was built without site_memory")
        return self._kernel_cache["_site_ring"]

    def refine_sites_(self, sweeps=1, damping=1.0, tol=None):
        """Expectation-propagation sweeps over the stored interval and count observations, in place.  Per sweep the
        grid mean is taken from the prediction cache and the posterior variance at the stored points from the path every posterior
        call takes (one more solve); then ONE launch per form present in the ring (``wiski_absorb_revisit``) re-matches every stored
        site against its cavity, damped by ``damping`` in [0, 1], and scatters only the difference of the site -- all slots against
        the same mean and variance (parallel EP).  The carried residual follows in the launch; the noise-weight sum moves by the
        weight deltas on the device; what cannot follow a weight that shrinks is given up, as after a point has left a window: a
        carried root pair, the spectral factor (rebuilt from the stencil, exactly), the two-level block; no dense rank update is
        seeded.  ``num_data`` follows the points that entered or left -- one host read per sweep, the read that fetches
        max(change).  ``tol``: stop after the sweep whose max(change) is at most tol.  Returns the list of max(change) per sweep,
        change = |omega_new - omega_old| / max(omega_new, omega_old); ``last_refined_sites`` then holds (ytilde, omega, log_z) over
        the filled slots, oldest first (log_z against the cavity of the last sweep; NaN for a slot it left alone).  A hyper-parameter
        step needs nothing: the next sweep re-matches under the new kernel."""
        ring = self._site_ring("refine_sites_")
        if isinstance(sweeps, bool) or int(sweeps) != sweeps or int(sweeps) < 0:
            raise ValueError(f"sweeps must be an integer >= 0, got {sweeps!r}")
        damping = float(damping)
        if not (0.0 <= damping <= 1.0):
            raise ValueError(f"damping must lie in [0, 1], got {damping}")
        cache = self._kernel_cache
        op = self._native_half_op(cache, "site revisit")
        changes = []
        for _ in range(int(sweeps)):
            if ring.fill == 0:
                changes.append(0.0)
                continue
            idx = torch.as_tensor(ring.order(), dtype=torch.long, device=self._device)
            u = self.prediction_cache["pred_mean"][0, :, 0]      # (finishes whatever is pending)
            with torch.no_grad(), settings.skip_posterior_variances(False):
                pv = self._eval_forward(ring.x[idx].contiguous()).variance.reshape(-1).to(self._dtype)
            pvar = torch.zeros(ring.cap, dtype=self._dtype, device=self._device)
            pvar[idx] = pv
            targets, res = self._site_targets(cache, op, u)
            before = ring.omega.clone()
            log_z = change = None
            for form in sorted(ring.forms):                  # every launch of the sweep against the same u and pvar
                log_z, change = grid_ops.revisit_sites(self._grid, ring, form, pvar, self._sigma2(0), damping, *targets, res=res, log_z=log_z, change=change)
            self._wsum_dev[0] += (ring.wa * (ring.omega - before)).sum(dtype=torch.float64)
            self._wsum_dirty = True
            self._give_up(cache)
            top, entered, left = torch.stack([change.max().double(), ((before == 0) & (ring.omega > 0)).sum().double(),
                                              ((before > 0) & (ring.omega == 0)).sum().double()]).tolist()
            self.num_data = self.num_data + int(entered) - int(left)
            self._dump_caches()
            self.last_refined_sites = (ring.ytilde[idx], ring.omega[idx], log_z[idx])
            changes.append(float(top))
            if tol is not None and top <= tol:
                break
        return changes

    def site_memory_points(self):
        """What the ring holds, oldest first: dict of X [k, d], d0, d1 [k] (lower / upper, or count and exposure / trials), form (list
        of "interval" / "poisson" / "binomial"), noise, ytilde, omega [k]."""
        ring = self._site_ring("site_memory_points")
        idx = torch.as_tensor(ring.order(), dtype=torch.long, device=self._device)
        names = {v: k for k, v in grid_ops.SITE_FORMS.items()}
        return dict(X=ring.x[idx], d0=ring.d0[idx], d1=ring.d1[idx], form=[names[int(c)] for c in ring.form[idx].tolist()], noise=ring.noise[idx],
                    ytilde=ring.ytilde[idx], omega=ring.omega[idx])

    # ------------------------------------------------ heteroscedastic noise --
    def _refuse_for_hetero_model(self):
        """What heteroscedastic=True does not combine with, each with its reason."""
        if self.num_outputs > 1:
            raise NotImplementedError("heteroscedastic is implemented for a single output (one noise field, one residual per point)")
        if self.robust_c is not None:
            raise NotImplementedError("heteroscedastic does not combine with robust_c: a large residual is either noise to be learned or an "
                                      "outlier to be down-weighted, and no kernel decides both")
        if self.window is not None:
            raise NotImplementedError("heteroscedastic does not combine with window: the ring stores the weights of one model, and a noise "
                                      "site depends on the posteriors it was matched against")
        if self._trend_deg is not None:
            self._refuse_trend("heteroscedastic", "the residual is taken against the grid mean alone, which under a trend is not the predictive mean")
        if self.input_var is not None:
            raise NotImplementedError("heteroscedastic does not combine with input_var: no kernel applies both forms in one launch")

    def _new_noise_model(self, noise_kernel):
        """The model of g - log_noise_mean: a single output on THIS model's grid object with empty statistics, sigma2 = 1 and unit
        weights.  noise_kernel None: a deep copy of this model's base kernel -- the same class, its own parameters."""
        import copy

        g = self._grid
        if noise_kernel is None:
            noise_kernel = copy.deepcopy(self.covar_module.base_kernel)
        if not isinstance(noise_kernel, GridInterpolationKernel):
            noise_kernel = GridInterpolationKernel(base_kernel=noise_kernel, grid_size=8, num_dims=g.d, grid_bounds=[list(b) for b in g.grid_bounds])
        noise_kernel.set_grid_spec(g)
        nm = FixedNoiseOnlineSKIGP(covar_module=noise_kernel, kernel_cache=kc.fresh(g, 1, self._dtype, self._device), likelihood=self.likelihood, learn_additional_noise=False, num_data=0)
        if nm._trend_deg is not None or nm.num_outputs != 1:
            raise NotImplementedError("the noise model is a single output without a trend")
        return nm

    def _noise_sibling(self):
        """The noise model of a functional sibling: a clone of its statistics on the same kernel, with this one's mean state."""
        nm = self.noise_model
        if nm is None:
            return None
        sib = nm._sibling(nm._clone_cache(nm._kernel_cache), nm.num_data)
        nm._sibling_mean_state(sib)
        return sib

    def _log_noise_state(self, X, want_mean=False):
        """(u_g [m], v_g [n]) of g - log_noise_mean under the noise model's current posterior at X [n, d] -- the prior's while it holds
        nothing (no solve on empty statistics) -- and, with want_mean, w . u_g [n] as well."""
        nm = self.noise_model
        if not nm.num_data:
            u = torch.zeros(self._grid.m, dtype=self._dtype, device=self._device)
            var = InterpolatedKernel(self._grid, X, nm._hyper()[0][0], 1.0, nm._err).diag()
            mean = torch.zeros(X.shape[0], dtype=self._dtype, device=self._device)
        else:
            u = nm.prediction_cache["pred_mean"][0, :, 0]
            with torch.no_grad(), settings.skip_posterior_variances(False):
                mvn = nm._eval_forward(X)
                mean, var = mvn.mean.reshape(-1), mvn.variance
        var = var.reshape(-1).to(self._dtype).clamp_min(0.0).contiguous()
        return (u, var, mean.to(self._dtype)) if want_mean else (u, var)

    def _condition_hetero(self, X, Y, noise, inplace, _decay):
        """condition_on_observations of a heteroscedastic model: grow, decay, weigh and match, absorb -- both models
        together.  Everything is taken against the two posteriors of the statistics the batch is added to."""
        if Y is None:
            raise ValueError("a heteroscedastic model takes targets Y")
        if X.dim() > 2 or Y.dim() > 2:
            raise NotImplementedError("batched conditioning (fantasies) of a heteroscedastic model: a fantasy batch carries the statistics of f "
                                      "alone, and its noise would have to be fantasised with it")
        if self.__dict__.get("_stencil_shard") is not None:
            raise NotImplementedError("heteroscedastic does not follow a stencil shard: the launch writes every group of both models")
        X = X.reshape(-1, self._grid.d)
        n = X.shape[0]
        Y = Y.reshape(-1)
        if Y.shape[0] != n:
            raise ValueError(f"Y must hold one target per point ([{n}]), got {tuple(Y.shape)}")
        if noise is not None:
            noise = noise.to(self._device, self._dtype).reshape(-1)
            if noise.shape[0] != n:
                raise ValueError(f"noise must hold one value per point ([{n}]), got {tuple(noise.shape)}")
        if self.grow_grid:
            self.grow_to_cover_(X)
        return self._condition(lambda model, cache, src: model._absorb_hetero(cache, X, Y, noise, src), inplace, self._gamma(_decay), reads_posterior=True)

    def _absorb_hetero(self, cache, X, Y, noise, src):
        """_absorb of one batch into BOTH models, one launch (wiski_absorb_hetero).  `src`: the model whose posteriors -- its own
        and its noise model's -- everything is taken against: this one, or in the functional form without a decay the parent.  f is
        followed with (wa omega_f, y wb omega_f), omega_f = 1 / e; the noise model with its sites at unit weights.  Returns what
        num_data grows by: the points that entered f and those outside the grid (which _raise_out_of_bounds takes off again)."""
        form = "heteroscedastic observations"
        nm = self.noise_model
        ncache = nm._kernel_cache
        op, nop = self._native_half_op(cache, form), nm._native_half_op(ncache, form + " (the noise model)")
        X, y, no, wa, wb = self._canon_batch(X, Y, noise)
        u = src.prediction_cache["pred_mean"][0, :, 0]       # (finishes whatever is pending, leaves a stencil shard)
        with torch.no_grad(), settings.skip_posterior_variances(False):
            pvar = src._eval_forward(X).variance.reshape(-1).to(self._dtype).contiguous()
        u2, pvar2 = src._log_noise_state(X)
        (b, A, cnt, stats, err, _), res = self._site_targets(cache, op, u)
        (b2, A2, cnt2, stats2, _, _), res2 = nm._site_targets(ncache, nop, u2)
        flag0 = self._err.clone()
        g0 = self.log_noise_mean
        sites = grid_ops.scatter_stats_hetero(self._grid, X, y, pvar, pvar2, self._sigma2(0), g0, wa, wb, no, (b, A, cnt, stats, u, res),
                                              (b2, A2, cnt2, stats2, u2, res2), err)
        self.last_hetero_sites = sites
        if not X.shape[0]:
            return 0
        e, yt, tau, _, lzy = sites
        in_f = (e > 0) & torch.isfinite(lzy)
        omega_f = torch.where(in_f, 1.0 / e.clamp_min(torch.finfo(self._dtype).tiny), torch.zeros_like(e))
        self._follow_sites(cache, X, wa, wb, torch.where(in_f, y, torch.zeros_like(y)), omega_f)
        one = nm._ones(X.shape[0])
        nm._follow_sites(ncache, X, one, one, torch.where(tau > 0, yt - g0, torch.zeros_like(yt)), tau)
        entered, entered_g, dropped = torch.stack([in_f.sum(), (tau > 0).sum(), (self._err - flag0).reshape(-1)[0] >> 1]).tolist()
        nm.num_data = (nm.num_data or 0) + int(entered_g)
        nm._dump_caches()
        return int(entered) + int(dropped)

    def _require_hetero(self, what):
        if self.noise_model is None:
            raise RuntimeError(f"{what} needs a model built with heteroscedastic=True")

    def noise_posterior(self, X):
        """(mean [n], variance [n]) of g(X) = log of the noise multiplier under the noise model's posterior."""
        self._require_hetero("noise_posterior")
        X = X.reshape(-1, self._grid.d).to(self._device, self._dtype).contiguous()
        _, var, mean = self._log_noise_state(X, want_mean=True)
        return mean + self.log_noise_mean, var

    def predict_noise(self, X, noise=None):
        """E[sigma2 noise exp g(X)] [n]: the noise variance a point at X is expected to carry (``noise`` None: 1)."""
        mean, var = self.noise_posterior(X)
        e = torch.exp(mean.double() + 0.5 * var.double()) * self._sigma2(0)
        return (e if noise is None else e * noise.to(self._device).reshape(-1).double()).to(self._dtype)

    def predictive(self, X, noise=None):
        """(mean [n], variance [n]) of a target at X: the posterior of f plus the predicted noise."""
        self._require_hetero("predictive")
        Xf = X.reshape(-1, self._grid.d).to(self._device, self._dtype).contiguous()
        with torch.no_grad(), settings.skip_posterior_variances(False):
            mvn = self._eval_forward(Xf)
            mean, var = mvn.mean.reshape(-1), mvn.variance.reshape(-1).clamp_min(0.0)
        return mean, var + self.predict_noise(Xf, noise)

    def hetero_log_probability(self, X, Y, noise=None):
        """log N(Y; predictive mean, predictive variance) [n] float64 of held-out targets."""
        mean, var = self.predictive(X, noise)
        mean, var, y = mean.double(), var.double(), Y.to(self._device).reshape(-1).double()
        return -0.5 * torch.log(2.0 * math.pi * var) - 0.5 * (y - mean) ** 2 / var

    # ---------------------------------------------- categorical observations --
    def _label_noise(self, noise, n):
        """The per-point noise of a batch of labels as [n] in the model's dtype, or None: unit noise."""
        if noise is None:
            return None
        noise = noise.to(self._device, self._dtype).reshape(-1).contiguous()
        if noise.shape[0] != n:
            raise ValueError(f"noise must hold one value per point ([{n}]), got {tuple(noise.shape)}")
        return noise

    def _condition_labels(self, X, labels, noise, inplace, _decay):
        """condition_on_observations with labels: grow, decay, moment-match, absorb -- _condition_count for the one
        form that couples the outputs.  It refuses what _refuse_for_sites refuses, except several outputs, which it needs; and a
        trend, as counts do."""
        C = self.num_outputs
        if not 2 <= C <= grid_ops.LABEL_MAX_CLASSES:
            raise NotImplementedError(f"label observations need a model with 2 .. {grid_ops.LABEL_MAX_CLASSES} outputs, one per class; this one has {C}")
        if self.robust_c is not None:
            raise NotImplementedError("label observations do not combine with robust_c: a site is a weight already, and no kernel applies both")
        if self.window is not None:
            raise NotImplementedError("label observations do not combine with window: the ring stores targets, and a site depends on the "
                                      "posterior it was matched against")
        if X.dim() > 2:
            raise NotImplementedError("batched conditioning (fantasies) takes targets, not labels")
        if self.input_var is not None:
            raise NotImplementedError("label observations do not combine with input_var on the model: a label has no target whose noise "
                                      "the location error could inflate, and the sites would be matched at exact locations")
        if self._trend_deg is not None:
            self._refuse_trend("label observations (labels)", "a site is matched against the grid mean alone, which under a trend "
                               "is not the predictive mean")
        X = X.reshape(-1, self._grid.d)
        n = X.shape[0]
        y = labels.to(self._device, self._dtype).reshape(-1).contiguous()
        if y.shape[0] != n:
            raise ValueError(f"labels must hold one class per point ([{n}]), got {tuple(y.shape)}")
        noise = self._label_noise(noise, n)
        if self.grow_grid:
            self.grow_to_cover_(X)
        return self._condition(lambda model, cache, src: model._absorb_labels(cache, X, y, noise, src), inplace, self._gamma(_decay),
                               reads_posterior=True)

    def _absorb_labels(self, cache, X, y, noise, src):
        """_absorb of one batch of labels, one launch for all outputs (wiski_absorb_label): _absorb_matched for the one form
        that couples the outputs, in its order -- the source posterior is read first (`src` as there: its C grid means from the
        prediction cache, which finishes whatever is pending and leaves a stencil shard, and its C posterior variances at X), then
        the launch is prepared (_before_launch, the carried residual) as _site_targets does, then everything that follows the stream
        per output receives that output's pseudo-targets at the weights wa omega_c, wb omega_c, as _follow_sites does for one output.
        It is not _absorb_matched itself because that takes one output's operator, vector views and one sigma2 (_native_half_op,
        _site_targets) where this needs the packed [C, ...] buffers.  Returns what num_data grows by: the points whose label class
        entered, and those outside the grid."""
        C = self.num_outputs
        ops = _wtw_ops(cache["WtW"])
        pack = self._stencil_pack(ops)
        b = cache["interpolation_cache"][:, :, 0]
        if pack is None or "_cnt" not in cache or not b.is_contiguous():
            raise NotImplementedError("label observations: the native packed half-stencil cache is needed (a full stencil was handed over)")
        if "path_probes" in cache:                           # (_follow would feed them once per output)
            raise NotImplementedError("label observations: path probes follow a single output")
        X = X.to(self._device, self._dtype).contiguous()
        n = X.shape[0]
        no, wa, wb = self._batch_weights(noise, False, n)
        U = src.prediction_cache["pred_mean"][..., 0]        # [C, m]
        if not U.is_contiguous():
            U = U.contiguous()
        with torch.no_grad(), settings.skip_posterior_variances(False):
            pvar = src._eval_forward(X).variance.reshape(C, n).to(self._dtype).contiguous()
        ms = self._carried(self._before_launch(cache), u=U)  # (the state's U is [C, m]: its first row starts where U does)
        flag0 = self._err.clone()
        sites = grid_ops.scatter_stats_label(self._grid, X, y, pvar, [self._sigma2(c) for c in range(C)], wa, wb, no, b, pack, cache["_cnt"],
                                             cache["_stats"], self._err, U, res=ms["R"] if ms else None)
        self.last_label_sites = sites
        if not n:
            return 0
        ytilde, omega = sites[0], sites[1]
        self._two_level_lose()
        for c in range(C):
            self._follow(cache, c, X, wa * omega[c], ytilde[c] * (wb * omega[c]))     # a skipped site, a point outside the grid: omega = 0
        cls = y.clamp(0, C - 1).nan_to_num(0.0).long()
        entered, dropped = torch.stack([(omega.gather(0, cls[None])[0] > 0).sum(), (self._err - flag0).reshape(-1)[0] >> 1]).tolist()
        return int(entered) + int(dropped)

    def _label_moments(self, X, noise):
        """(mean, variance, noise variance) [C, n] of the C outputs at X under the current posterior, in the model's dtype."""
        C = self.num_outputs
        if not 2 <= C <= grid_ops.LABEL_MAX_CLASSES:
            raise NotImplementedError(f"class probabilities need a model with 2 .. {grid_ops.LABEL_MAX_CLASSES} outputs, one per class; this one has {C}")
        X = X.reshape(-1, self._grid.d)
        n = X.shape[0]
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad(), settings.skip_posterior_variances(False):
                mvn = self(X.to(self._device, self._dtype))
                mean, var = mvn.mean.reshape(C, n).contiguous(), mvn.variance.reshape(C, n).clamp_min(0.0).contiguous()
        finally:
            if was_training:
                self.train()
        noise = self._label_noise(noise, n)
        s2 = torch.tensor([self._sigma2(c) for c in range(C)], dtype=torch.float64, device=self._device)[:, None]
        s = (s2 * (torch.ones(n, dtype=torch.float64, device=self._device) if noise is None else noise.double())).to(self._dtype).contiguous()
        return mean, var, s

    def label_probability(self, X, noise=None):
        """P(label = k | x_i) [n, C] (float64) under the current posterior and the multinomial probit likelihood, with the model's own
        error bars inside (``wiski_label_proba``: the integral of the absorb's sites, once per class).  ``noise`` [n]: the per-point
        noise a label at x_i would be given (None: unit).  The rows sum to 1 to quadrature error and are not normalised."""
        return grid_ops.label_proba(*self._label_moments(X, noise))

    def label_log_probability(self, X, labels, noise=None):
        """log P(labels_i | x_i) [n] (float64) under the current posterior -- the log Z of the sites a batch of these labels would be
        absorbed with (``wiski_label_sites``: the device function of the absorb, no scatter); NaN for a label that is no class."""
        mean, var, s = self._label_moments(X, noise)
        y = labels.to(self._device, self._dtype).reshape(-1).contiguous()
        return grid_ops.label_sites(mean, var, s, y)[2]

    # --------------------------------------------------- noisy-input observations --
    def _canon_input_var(self, input_var, n):
        """input_var -- a scalar, [d], [n] or [n, d] (a vector of length n == d counts as [d]) -- as [n, d] on the model's device."""
        d = self._grid.d
        v = torch.as_tensor(input_var).detach().to(self._device, self._dtype)
        if v.dim() == 1 and v.shape[0] != d and v.shape[0] == n:
            v = v[:, None]
        if tuple(v.shape) not in ((), (d,), (n, 1), (n, d)):
            raise ValueError(f"input_var must be a scalar, [{d}], [{n}] or [{n}, {d}], got {tuple(v.shape)}")
        return v.expand(n, d).contiguous()

    def _condition_input_noise(self, X, Y, noise, input_var, inplace, _decay, others):
        """condition_on_observations with input_var: grow, decay, take the slope moments, absorb -- _condition_interval
        with the noisy-input launch.  The sites are taken against the posterior of the statistics the batch is added to."""
        if others:
            raise NotImplementedError(f"noisy-input observations inflate the noise of targets Y: input_var takes no {' / '.join(others)} "
                                      "(no kernel applies two sites)")
        self._refuse_trend("noisy-input observations (input_var)", "a site is matched against the grid mean alone, which under a trend "
                           "is not the predictive mean")
        self._refuse_for_sites(X, "noisy-input", "input_var")
        if Y is None:
            raise ValueError("input_var describes the locations of targets Y, which were not given")
        if Y.dim() > 2:
            raise NotImplementedError("batched conditioning (fantasies) takes targets, not input_var")
        X = X.reshape(-1, self._grid.d)
        n = X.shape[0]
        y = Y.to(self._device, self._dtype).reshape(-1)
        if y.shape[0] != n:
            raise ValueError(f"Y must hold one target per point ([{n}]), got {tuple(Y.shape)}")
        xvar = self._canon_input_var(input_var, n)
        if noise is not None:
            noise = noise.to(self._device, self._dtype).reshape(-1)
            if noise.shape[0] != n:
                raise ValueError(f"noise must hold one value per point ([{n}]), got {tuple(noise.shape)}")
        if self.grow_grid:
            self.grow_to_cover_(X)
        return self._condition(lambda model, cache, src: model._absorb_input_noise(cache, X, y, xvar, noise, src), inplace, self._gamma(_decay),
                               reads_posterior=True)

    def _absorb_input_noise(self, cache, X, y, xvar, noise, src, half_delta=None):
        """_absorb_matched with the noisy-input launch (wiski_absorb_input_noise).  "posterior": the variances of f and of its
        partial derivatives at X are the diagonal of ONE posterior_jet covariance of `src`; "mean": the variance of f as for intervals,
        no slope variance.  The pseudo-target is y itself."""
        gvar = []

        def jet_variances(src, X):
            diag = torch.diagonal(src.posterior_jet(X).covariance, dim1=-2, dim2=-1).to(self._dtype)
            gvar.append(diag[:, 1:].contiguous())
            return diag[:, 0].contiguous()

        def launch(X, *rest, **kw):
            omega, log_z, grad = grid_ops.scatter_stats_input_noise(self._grid, X, y.contiguous(), xvar, gvar[0] if gvar else None, *rest, want_grad=True, **kw)
            return y, omega, log_z, grad

        sites, grown = self._absorb_matched(cache, X, noise, src, "noisy-input observations", launch, half_delta=half_delta,
                                            pvar_of=jet_variances if self.input_noise_slope == "posterior" else None)
        self.last_input_noise_sites = sites[1:]
        return grown

    def posterior_noisy_input(self, X, input_var):
        """(mean [n], variance [n]) of f at queries whose locations are uncertain, X [n, d] with error variance ``input_var`` (a scalar,
        [d], [n] or [n, d]) per dimension: to first order the mean is that of ``posterior(X)`` and the variance gains
        ``sum_k input_var_k (E[g_k]^2 + Var g_k)`` with g the gradient under ``posterior_jet(X)``.  Plain torch on
        the jet; outputs are detached.  One output, unbatched X."""
        jet = self.posterior_jet(X)
        xvar = self._canon_input_var(input_var, jet.n).to(jet.mean.dtype)
        diag = torch.diagonal(jet.covariance, dim1=-2, dim2=-1)
        g = jet.mean[:, 1:]
        return jet.mean[:, 0], diag[:, 0] + (xvar * (g * g + diag[:, 1:].clamp_min(0.0))).sum(-1)

    def _latent_moments(self, X):
        """(mean, variance) [n] of f at X under the current posterior, in the model's dtype."""
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad(), settings.skip_posterior_variances(False):
                mvn = self(X.to(self._device, self._dtype))
                return mvn.mean.reshape(-1).contiguous(), mvn.variance.reshape(-1).clamp_min(0.0).contiguous()
        finally:
            if was_training:
                self.train()

    def count_log_probability(self, X, counts, exposure=None, trials=None):
        """log P(counts_i | x_i) [n] (float64) under the current posterior -- the log Z of the sites a batch of these counts would be
        absorbed with (``wiski_count_sites``: the device function of the absorb, no scatter)."""
        mean, var = self._latent_moments(X)
        y, t, family = self._count_batch(mean.shape[0], counts, exposure, trials)
        return grid_ops.count_sites(mean, var, y, t, family)[2]

    def predict_counts(self, X, exposure=None, trials=None):
        """(mean, variance) [n] (float64) of a future count at X.  Poisson: closed form from the log-normal rate, E = t exp(mu + v / 2),
        Var = E + E^2 (exp v - 1).  Binomial: with p = sigmoid(f), E = t E p and Var = t E[p (1 - p)] + t^2 Var p, the moments of p by
        a 64-point Gauss-Hermite rule in torch fp64."""
        if exposure is not None and trials is not None:
            raise ValueError("counts are Poisson at an exposure or binomial out of trials, not both")
        mean, var = (a.double() for a in self._latent_moments(X))
        t = trials if trials is not None else exposure
        t = torch.ones_like(mean) if t is None else t.to(mean.device, torch.float64).reshape(-1)
        if trials is None:
            e = t * torch.exp(mean + 0.5 * var)
            return e, e + e * e * torch.expm1(var)
        import numpy as np

        z, w = np.polynomial.hermite_e.hermegauss(64)
        z = torch.as_tensor(z, dtype=torch.float64, device=mean.device)
        w = torch.as_tensor(w / w.sum(), dtype=torch.float64, device=mean.device)
        p = torch.sigmoid(mean[:, None] + var.sqrt()[:, None] * z)
        ep, ep2 = p @ w, (p * p) @ w
        return t * ep, t * (ep - ep2) + t * t * (ep2 - ep * ep)

    def interval_probability(self, X, lower, upper, noise=None):
        """log P(lower_i <= f(x_i) + eps_i <= upper_i) [n] under the current posterior, eps_i ~ N(0, sigma2 noise_i) (``noise`` None:
        unit noise); either bound may be None or infinite.  Plain torch on the posterior's mean and variance: the Gaussian mass of
        the interval through ``torch.special.log_ndtr``, mirrored so that the difference is taken in the lower tail."""
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad(), settings.skip_posterior_variances(False):
                mvn = self(X.to(self._device, self._dtype))
                mean, var = mvn.mean.reshape(-1).double(), mvn.variance.reshape(-1).double()
        finally:
            if was_training:
                self.train()
        n = mean.shape[0]
        inf = float("inf")
        lo = torch.full((n,), -inf, dtype=torch.float64, device=mean.device) if lower is None else lower.to(mean.device, torch.float64).reshape(-1)
        hi = torch.full((n,), inf, dtype=torch.float64, device=mean.device) if upper is None else upper.to(mean.device, torch.float64).reshape(-1)
        dn = self._sigma2(0) * (1.0 if noise is None else noise.to(mean.device, torch.float64).reshape(-1))
        s = (var.clamp_min(0.0) + dn).sqrt()
        a, b = (lo - mean) / s, (hi - mean) / s
        flip = a + b > 0
        a, b = torch.where(flip, -b, a), torch.where(flip, -a, b)
        la, lb = torch.special.log_ndtr(a), torch.special.log_ndtr(b)
        return lb + torch.log1p(-torch.exp(la - lb))

    # ------------------------------------- interval observations of gradients --
    def _condition_grad_interval(self, X, Y, noise, lower, upper, grad_Y, grad_lower, grad_upper, grad_noise, grad_mask, inplace, _decay):
        """condition_on_observations with grad_lower / grad_upper: the batch becomes [n, d + 1] channel tensors of
        bounds -- column 0 the value (Y: equal bounds; lower / upper; or absent), column 1 + q the partial in dim q -- each with its
        noise and a presence flag; then grow, decay, moment-match, absorb, as _condition_interval."""
        if grad_Y is not None:
            raise NotImplementedError("a partial derivative is given as grad_Y or as bounds grad_lower / grad_upper, not both "
                                      "(an exact partial is grad_lower == grad_upper)")
        self._refuse_trend("interval observations of gradients (grad_lower / grad_upper)", "a site is matched against the grid mean alone, "
                           "which under a trend is not the predictive mean")
        self._refuse_for_sites(X, "gradient-interval", "grad_lower / grad_upper")
        if Y is not None and Y.dim() > 2:
            raise NotImplementedError("batched conditioning (fantasies) takes targets, not grad_lower / grad_upper")
        if Y is not None and (lower is not None or upper is not None):
            raise NotImplementedError("a batch is given as targets Y or as bounds lower / upper, not both (an exact value is lower == upper)")
        if "path_probes" in self._kernel_cache:
            raise NotImplementedError("a model with path probes cannot absorb derivative observations (its probes follow value rows only)")
        d, dev, dt = self._grid.d, self._device, self._dtype
        X = X.reshape(-1, d).to(dev, dt).contiguous()
        n = X.shape[0]
        inf = float("inf")

        def per_point(t, name, fill):
            if t is None:
                return torch.full((n,), fill, dtype=dt, device=dev)
            t = torch.as_tensor(t).detach().to(dev, dt).reshape(-1)
            if t.shape[0] != n:
                raise ValueError(f"{name} must hold one value per point ([{n}]), got {tuple(t.shape)}")
            return t

        def per_partial(t, name, fill):
            if t is None:
                return torch.full((n, d), fill, dtype=dt, device=dev)
            t = torch.as_tensor(t).detach().to(dev, dt)
            if tuple(t.shape) not in ((), (d,), (n, d)):
                raise ValueError(f"{name} must be a scalar, [{d}] or [{n}, {d}], got {tuple(t.shape)}")
            return t.expand(n, d)

        lo = torch.empty((n, d + 1), dtype=dt, device=dev)
        hi = torch.empty((n, d + 1), dtype=dt, device=dev)
        Nc = torch.ones((n, d + 1), dtype=dt, device=dev)
        present = torch.ones((n, d + 1), dtype=torch.bool, device=dev)
        lo[:, 1:], hi[:, 1:] = per_partial(grad_lower, "grad_lower", -inf), per_partial(grad_upper, "grad_upper", inf)
        if Y is not None:
            lo[:, 0] = hi[:, 0] = per_point(Y, "Y", 0.0)
        elif lower is not None or upper is not None:
            lo[:, 0], hi[:, 0] = per_point(lower, "lower", -inf), per_point(upper, "upper", inf)
        else:
            lo[:, 0], hi[:, 0] = -inf, inf
            present[:, 0] = False
        if noise is not None:
            Nc[:, 0] = per_point(noise, "noise", 1.0)
        if grad_noise is None:
            Nc[:, 1:] = Nc[:, :1]                        # the value observation's noise (unit noise without one)
        else:
            gn = torch.as_tensor(grad_noise).detach().to(dev, dt)
            if tuple(gn.shape) not in ((), (n,), (n, d)):
                raise ValueError(f"grad_noise must be a scalar, [{n}] or [{n}, {d}], got {tuple(gn.shape)}")
            Nc[:, 1:] = gn[:, None] if gn.dim() == 1 else gn
        if grad_mask is not None:
            if tuple(grad_mask.shape) != (n, d):
                raise ValueError(f"grad_mask must be [{n}, {d}], got {tuple(grad_mask.shape)}")
            present[:, 1:] = grad_mask.to(dev, torch.bool)
        if self.grow_grid:
            self.grow_to_cover_(X)
        return self._condition(lambda model, cache, src: model._absorb_grad_interval(cache, X, lo, hi, Nc, present, src), inplace, self._gamma(_decay),
                               reads_posterior=True)

    def _absorb_grad_interval(self, cache, X, lo, hi, noise, present, src):
        """_absorb for [n, d + 1] channel tensors of bounds (lo, hi, noises, bool present), one launch
        (wiski_absorb_grad_interval).  `src`: the model whose posterior the sites are matched against, as in _absorb_matched:
        its grid mean from the prediction cache, and the variances of f and of its partial derivatives at X from the diagonal of ONE
        posterior_jet covariance.  The followers are those of _absorb_grad: what a derivative row cannot be followed through is
        given up.  Returns what num_data grows by: the channels that entered, and the present channels of points outside the grid
        (which _raise_out_of_bounds takes off again when the flag is read)."""
        op = self._native_half_op(cache, "interval observations of gradients")
        if "path_probes" in cache:
            raise NotImplementedError("interval observations of gradients: no path probes (they follow value rows only)")
        u = src.prediction_cache["pred_mean"][0, :, 0]       # (finishes whatever is pending, leaves a stencil shard)
        pvar = torch.diagonal(src.posterior_jet(X).covariance, dim1=-2, dim2=-1).to(self._dtype).contiguous()
        mine = self._before_launch(cache)
        zero, one = torch.zeros((), dtype=self._dtype, device=self._device), torch.ones((), dtype=self._dtype, device=self._device)
        wb = torch.where(present, 1.0 / noise, zero)
        wa = torch.where(present, self._weight_a(noise, False), zero)
        no = torch.where(present, noise, one)            # an absent channel: wa = wb = 0, noise = 1 -- nothing anywhere
        ms = self._carried(mine, u=u)
        sites = grid_ops.scatter_stats_grad_interval(self._grid, X, torch.where(present, lo, zero), torch.where(present, hi, zero), pvar, self._sigma2(0),
                                                     wa, wb, no, cache["interpolation_cache"][0, :, 0], op.stencil, cache["_cnt"][0], cache["_stats"][0],
                                                     self._err, u, res=ms["R"][0] if ms else None)
        self.last_grad_interval_sites = sites
        if X.shape[0] == 0:
            return 0
        self._give_up(cache)                             # L L^T described the matrix without these rows
        if mine:
            # the noise-weight sum (preconditioner shift only) is the mass of cnt, to which a derivative channel adds its diagonal
            self._wsum_dev = cache["_cnt"].sum(dim=1, dtype=torch.float64)
            self._wsum_host = [0.0] * self.num_outputs
            self._wsum_dirty = True
        # a point is outside the grid where the kernel says so: x < g0 or x > g0 + h (g - 1), in the working precision
        g = self._grid
        g0 = torch.tensor(g.g0, dtype=self._dtype)
        top = (g0 + torch.tensor(g.h, dtype=self._dtype) * torch.tensor([gi - 1 for gi in g.g], dtype=self._dtype)).to(self._device)
        outside = ~((X >= g0.to(self._device)) & (X <= top)).all(1)
        return int(((sites[1] > 0).sum() + (present & outside[:, None]).sum()).item())

    def gradient_interval_probability(self, X, lower, upper, noise=None):
        """log P(lower_iq <= d_q f(x_i) + eps_iq <= upper_iq) [n, d] (float64) under the current posterior, eps_iq ~ N(0, sigma2
        noise_iq) (``noise`` None: unit noise; a scalar, [n] or [n, d]); either bound may be None, a scalar, [d] or [n, d], or
        infinite.  Plain torch on the gradient moments of ``posterior_jet``: the Gaussian mass of the interval through
        ``torch.special.log_ndtr``, mirrored so that the difference is taken in the lower tail, as in ``interval_probability``."""
        jet = self.posterior_jet(X)
        mean = jet.mean[:, 1:].double()
        var = torch.diagonal(jet.covariance, dim1=-2, dim2=-1)[:, 1:].double()
        n, d = mean.shape
        inf = float("inf")

        def bound(t, fill):
            t = torch.full((), fill, dtype=torch.float64) if t is None else torch.as_tensor(t).detach()
            return t.to(mean.device, torch.float64).expand(n, d)

        lo, hi = bound(lower, -inf), bound(upper, inf)
        nz = torch.ones((), dtype=torch.float64) if noise is None else torch.as_tensor(noise).detach()
        nz = nz.to(mean.device, torch.float64)
        dn = self._sigma2(0) * (nz[:, None] if nz.dim() == 1 else nz)
        s = (var.clamp_min(0.0) + dn).sqrt()
        a, b = (lo - mean) / s, (hi - mean) / s
        flip = a + b > 0
        a, b = torch.where(flip, -b, a), torch.where(flip, -a, b)
        la, lb = torch.special.log_ndtr(a), torch.special.log_ndtr(b)
        return lb + torch.log1p(-torch.exp(la - lb))

    # ------------------------------------------------------- sliding window --
    def _window_rebuild_due(self):
        self._win_updates += 1
        if self.window_rebuild_every is not None and self._win_updates % self.window_rebuild_every == 0:
            self.rebuild_window_()

    def _window_restart(self, X, Y, noise):
        """The statistics (zeroed by the caller) and the ring restart from the last `window` rows of (X, Y, noise), at the weights of a
        model built from data (1 / noise, unfloored)."""
        d = self._grid.d
        X = X.reshape(-1, d)
        Y = Y.reshape(X.shape[0], -1)
        ring = self._kernel_cache["_ring"]
        ring.clear()
        self._win_voids = 0
        lo = max(0, X.shape[0] - self.window)
        self._absorb_window(self._kernel_cache, X[lo:], Y[lo:], None if noise is None else noise.reshape(X.shape[0], -1)[lo:], init=True)

    def _absorb_window(self, cache, X, Y, noise, init=False):
        """_absorb of one value-only batch through the ring, one launch per `window` points (wiski_absorb_window): a batch larger
        than the window is split on the host so that the slots of a launch are distinct.  The carried residual follows when the mean
        state is current.  What cannot follow a point that leaves is given up rather than updated, as under a decay: a carried root
        pair is dropped, the spectral factor marked stale (it rebuilds from the stencil, exactly), the two-level block lost, no rank
        update prepared.  The noise-weight sum loses what left: on the host for the slots written at unit noise; for the others the
        device part moves by the ring's wa over the launch's slots, after minus before -- O(batch) work, queued, no host read or copy."""
        op = self._native_half_op(cache, "window")
        ring = cache["_ring"]
        mine = self._before_launch(cache)
        unit = noise is None
        X, y, no, wa, wb = self._canon_batch(X, Y, noise, init)
        n = X.shape[0]
        ms = self._carried(mine, init)
        if ms is not None:
            u = ms["U"][0]
        else:                                            # (the kernel takes both sweeps against some u; without res it goes nowhere)
            u = self.__dict__.get("_win_zero_u")
            if u is None or u.shape[0] != self._grid.m:
                u = self.__dict__["_win_zero_u"] = torch.zeros(self._grid.m, dtype=self._dtype, device=self._device)
        for lo in range(0, n, ring.cap):
            hi = min(n, lo + ring.cap)
            spans = ring.spans(hi - lo)
            # what leaves the noise-weight sum: counted on the host for slots written at unit noise; for the others the ring's own wa,
            # summed over the launch's slots BEFORE it overwrites them -- slices at host-known bounds, queued, never read back here
            left_unit = sum(int(ring.unit[sl].sum()) for sl in spans)
            left_dev = None
            if any(bool(ring.explicit_host[sl].any()) for sl in spans):
                left_dev = sum((ring.wa[sl] * ring.explicit[sl]).sum(dtype=torch.float64) for sl in spans)
            self._wsum_host[0] += (float(hi - lo) if unit else 0.0) - float(left_unit)
            ring.mark(spans, unit)
            grid_ops.scatter_stats_window(self._grid, X[lo:hi], y[lo:hi], wa[lo:hi], wb[lo:hi], no[lo:hi], ring, cache["interpolation_cache"][0, :, 0],
                                          op.stencil, cache["_cnt"][0], cache["_stats"][0], self._err, u, res=ms["R"][0] if ms else None)
            if left_dev is not None or not unit:
                delta = 0.0 if left_dev is None else -left_dev
                if not unit:                             # what entered, as the ring now holds it (a point dropped at entry: 0)
                    delta = delta + sum(ring.wa[sl].sum(dtype=torch.float64) for sl in spans)
                self._wsum_dev[0] += delta
                self._wsum_dirty = True
        self.num_data = ring.fill - self._win_voids
        if n > 0:
            self._give_up(cache)                         # L L^T described the matrix with the points that left

    def window_points(self):
        """(X [k, d], Y [k], noise [k]) of the points the model is the GP of, oldest first; slots whose point was dropped at entry
        (outside the grid) are omitted.  One host sync."""
        if self.window is None:
            raise RuntimeError("window_points: the model was built without window")
        ring = self._kernel_cache["_ring"]
        idx = torch.as_tensor(ring.order(), dtype=torch.long, device=self._device)
        X = ring.x[idx]
        keep = ~torch.isnan(X[:, 0])
        return X[keep], ring.y[idx][keep], ring.noise[idx][keep]

    def rebuild_window_(self):
        """Zero the statistics and absorb the ring again, through the plain absorb (one launch): cancels the rounding that many
        turnovers leave behind in fp32 (DESIGN.md 3.19 tabulates it) -- after it the statistics are those of a fresh model on
        ``window_points()``.  Everything derived from A is rebuilt on next use; the next mean solve starts from the current mean but
        recomputes its residual.  Returns the model."""
        if self.window is None:
            raise RuntimeError("rebuild_window_: the model was built without window")
        self._finish_pending()
        self.leave_stencil_shard()
        cache = self._kernel_cache
        ring = cache["_ring"]
        op = _wtw_ops(cache["WtW"])[0]
        for t in (cache["interpolation_cache"], cache["_stats"], cache["_cnt"], op.stencil):
            t.zero_()
        # an empty or void slot holds no weight and noise 1: absorbed at any point inside the grid it adds nothing anywhere
        dead = (ring.wa == 0) & (ring.wb == 0)
        centre = torch.tensor([g0 + 0.5 * h * (g - 1) for g0, h, g in zip(self._grid.g0, self._grid.h, self._grid.g)], dtype=self._dtype, device=self._device)
        X = torch.where(dead[:, None], centre[None, :], ring.x).contiguous()
        grid_ops.scatter_stats_cnt(self._grid, X, ring.y, ring.wa, ring.wb, ring.noise, cache["interpolation_cache"][0, :, 0], op.stencil, True,
                                   cache["_cnt"][0], cache["_stats"][0], self._err)
        if self._mean_state is not None:
            self._mean_state["R_ok"] = False
        self._give_up(cache)
        self._dump_caches()
        return self

    def stream_step(self, X, Y, want_mean=True):
        """evaluate -> absorb -> refresh for one streamed batch (the reference driver's online step at batch granularity,
        experiments/regression.py:48-54 with fixed hyper-parameters): predictive mean of X under the current posterior, then
        ``condition_on_observations(X, Y, inplace=True)``, then the posterior mean refreshed.  Equivalent to
        ``m = self(X).mean; self.condition_on_observations(X, Y, inplace=True); self.prediction_cache`` -- which is also the
        fallback -- but on large single-output grids the three launches go through ONE C-ABI call (``wiski_stream_step``) with
        the per-step host work reduced to bookkeeping.  Unit noise.  Returns the mean [n] (or None).  With a ``forgetting_factor``
        the statistics decay between the evaluation and the absorb (one more launch, ``wiski_decay_stats``)."""
        if self.noise_model is not None:
            raise NotImplementedError("stream_step on a heteroscedastic model: the fused step absorbs at unit noise -- use "
                                      "condition_on_observations(X, Y, inplace=True), which learns the noise in its launch")
        if self.grow_grid:
            self.grow_to_cover_(X)
        gamma = self._gamma()
        if gamma is not None:
            self._finish_pending()                   # the solve in flight belongs to the undecayed statistics
        st = self._stream_fast_state(X, Y)
        if st is None:
            self._finish_pending()
            self.leave_stencil_shard()               # the generic path below reads and writes the whole stencil
            mean = None
            if want_mean:
                with settings.skip_posterior_variances(True):
                    mean = self(X).mean
            self.condition_on_observations(X, Y, None, inplace=True)
            self.prediction_cache
            return mean
        step, ms, pst = st
        if gamma is not None:
            # the absorb below reads the mean of the batch from the solution U of the undecayed system, which the prediction cache keeps
            # pointing at; the refresh that ends this call makes it the solution of the decayed one
            self._decay(gamma, self.num_data, keep_mean_cache=True)
        q = X.shape[0]
        ones = self._ones(q)
        mean = torch.empty(q, dtype=self._dtype, device=self._device) if want_mean else None
        # bookkeeping of _absorb / prediction_cache
        self._wsum_add(0, q, None)
        self.num_data = self.num_data + q
        pacing = self._pacing
        pacing.count()
        self._two_level_step(step, pst, X, q)            # (may announce a new block: before the placement)
        last = (self._last_iters or [0])[0]
        # with a deferred-poll handle the library places the first poll itself, by the hindsight of the solve this call resumes
        # (stencil-sharded replicas keep the host's placement: their ranks must poll in lock step -- and so does a single GPU under
        # settings.two_level_lockstep, which exists to give it the replicas' iteration counts: a poll placed by hindsight reports the
        # masked iteration it costs when the stream gets easier, the host's early polls after a block switch do not)
        auto = (settings.poll_hindsight.on() and (settings.deferred_refresh.on() or step.pending)
                and self.__dict__.get("_stencil_shard") is None and settings.two_level_lockstep.off())
        fc, probe = pacing.place(last, step.pending if auto else None)
        carry = ms.get("R_ok", False) and not pacing.recompute_due()
        step.args.shift = float(self._wsum[0]) / pst["norm"]
        step.set_keep(self._keep_for_step(step, pst))
        y1 = Y.reshape(-1)
        y1 = y1 if y1.is_contiguous() else y1.contiguous()
        if "_spectral" in self.__dict__:
            self._spectral_absorb(0, X, None, y1)
        if settings.deferred_refresh.on() or step.pending:
            prev, pending = step(X, y1, ones, ones, ones, mean, carry, fc, defer=settings.deferred_refresh.on())
            if "path_probes" in self._kernel_cache and not (prev is not None and prev[2]):
                self._absorb_probes(self._kernel_cache, X, None)
            self._pending_step = step if pending else None
            if prev is not None:
                if prev[2]:                              # the PREVIOUS batch held out-of-grid points: this one was not queued at all
                    self._wsum_host[0] -= float(q)
                    self.num_data = self.num_data - q
                    pacing.uncount()
                self._note_solve(ms, prev, *pacing.queued)
            pacing.queue(fc, probe)
            if not pending:                              # deferral switched off meanwhile: this call ran to convergence
                self._note_solve(ms, (step.it.value, step.rr.value, step.herr.value, True), fc, probe)
            return mean
        res = step(X, y1, ones, ones, ones, mean, carry, fc)
        if "path_probes" in self._kernel_cache:
            self._absorb_probes(self._kernel_cache, X, None)       # one extra launch; none without probes
        self._note_solve(ms, res, fc, probe)
        return mean

    def _keep_for_step(self, step, pst):
        """The eigenmodes the step's preconditioner transforms (grid_ops.keep_counts; None: all).  The counts depend on the eigenvalues
        and on the shift only: they are kept with the interval of shifts on which they hold and recomputed when the shift leaves it.
        Host data that every replica of a sharded step holds alike, so the ranks stay in lock-step."""
        if (settings.truncated_preconditioner.off() or self._dtype != torch.float32 or self._grid.d != 3 or self.num_outputs != 1
                or "eig_host" not in pst):
            return None
        kscale, shift = float(step.args.kscale), float(step.args.shift)
        memo = pst.get("keep")
        if memo is None or memo[0] != kscale or not (memo[1] < shift <= memo[2]):
            K, lo, hi = grid_ops.keep_counts(pst["eig_host"]["D"], kscale, shift)
            if K is not None and not grid_ops.keep_accepts(self._grid, K, two_level=True):
                K = None                                   # above the cap / the cube does not fit the middle kernel
            memo = pst["keep"] = (kscale, lo, hi, K)
        K = memo[3]
        if K is not None and getattr(step, "_two_level", None) is not None:
            tr = self.__dict__.get("_two_level")
            blk = tr.block if tr is not None else None
            if blk is None:
                return None
            low = blk.__dict__.get("_idx_low")
            if low is None:
                low = blk._idx_low = tuple(int(v) for v in blk.idx_host.min(axis=1))
            if any(low[q] < self._grid.g[q] - K[q] for q in range(3)):
                return None                                # a selected mode of the exact block lies outside the box
        return K

    # ------------------------------------------------- two-level preconditioner --
    def _two_level_applies(self):
        if not (settings.two_level_preconditioner.on() and self.num_outputs == 1 and self._grid.d == 3 and self._dtype == torch.float32
                and max(self._grid.g) <= 64 and not self._use_dense()):
            return False
        # the slab kernel's coefficient exchange spins on words written by other blocks of the same launch: all 2 g0 blocks must be
        # co-resident (one per CU) -- not on a partitioned device or a part with fewer CUs (the C side refuses as well)
        cus = self.__dict__.get("_cu_count")
        if cus is None:
            cus = self.__dict__["_cu_count"] = torch.cuda.get_device_properties(self._device).multi_processor_count if self._device.type == "cuda" else 0
        return 2 * self._grid.g[0] <= cus

    def _two_level_note(self, X, wa, init=False):
        """Every point the statistics absorb is either pending for, or part of, the exact block of the two-level preconditioner
        (lazy/two_level.py); points absorbed without passing here make the tracker give up until the statistics are rebuilt."""
        if not self._two_level_applies():
            self.__dict__.pop("_two_level", None)
            return
        from ..lazy.two_level import TwoLevelTracker

        tr = self.__dict__.get("_two_level")
        if tr is None or init:
            if tr is None and not init:
                return                                 # statistics older than the tracker: never covered
            tr = self.__dict__["_two_level"] = TwoLevelTracker()
        tr.note(X.reshape(-1, self._grid.d), wa)

    def _two_level_lose(self):
        tr = self.__dict__.get("_two_level")
        if tr is not None:
            tr.lose()

    def _two_level_step(self, step, pst, X, q):
        """Before a one-call streaming step: note its batch, keep the block's refresh pipeline going, point the solve at the block."""
        tr = self.__dict__.get("_two_level") if self._two_level_applies() else None
        tl = None
        if tr is not None:
            tr.note(X, None)
            _, s2, _ = self._hyper()[0]
            sh = self.__dict__.get("_stencil_shard")
            # stencil-sharded replicas see the gathered batch of ALL ranks and each keeps its own copy of the block: every world-th
            # point (weighted) keeps a replica's refresh work at what one GPU's stream costs (the side stream must keep pace with
            # the steps, or the lock-step switch would stall them)
            sub = max(settings.two_level_subsample.value(), sh["world"]) if sh is not None and sh["world"] > 1 else None
            tl = tr.for_step(self._grid, self._device, pst, 1.0 / s2, float(self._wsum[0]), self._err,
                             lockstep=sh is not None or settings.two_level_lockstep.on(),
                             last_iters=(self._last_iters or [0])[0], subsample=sub)
            if tr.switched:
                self._pacing.new_block()
        if getattr(step, "_two_level", None) is not tl:
            step.set_two_level(tl)

    def _note_solve(self, ms, res, fc, probe=False):
        """Host bookkeeping after a refresh: iteration history for the poll placement, residual validity, out-of-grid error."""
        it, rel, flag, conv = res
        self._pacing.solved(it, rel, fc, probe)
        self._pacing.warm()
        self._last_iters = [it]
        ms["R_ok"] = bool(conv)
        pc = self._memo.get("prediction_cache")
        if pc is not None:
            pc["cg_iters"] = [it]
        if flag:
            ms["R_ok"] = False
            self._raise_out_of_bounds(flag)

    def _finish_pending(self):
        """A deferred refresh (settings.deferred_refresh) is still in flight: wait for its poll, finish the solve if needed."""
        step = self._pending_step
        if step is None:
            return
        self._pending_step = None
        if step.pending:
            prev, _ = step(None, None, None, None, None, None, 0, 0, defer=False)
            if prev is not None and self._mean_state is not None:
                self._note_solve(self._mean_state, prev, *self._pacing.queued)

    def _stream_fast_state(self, X, Y):
        """(prepared StreamStep, mean state, preconditioner state) when the one-call streaming step applies, else None."""
        if (self.robust_c is not None or self.window is not None or self.site_memory is not None or self._trend_deg is not None or self.input_var is not None or self.num_outputs != 1 or self._use_dense() or settings.spectral_preconditioner.off() or settings.residual_carry_over.off()
                or X.dim() != 2 or not X.is_cuda or X.dtype != self._dtype or not X.is_contiguous() or Y.dtype != self._dtype):
            return None
        ms = self._mean_state
        pc = self._memo.get("prediction_cache")
        ver = self._hyper_version()
        if ms is None or pc is None or ms.get("ver") != ver or "pending_rank_update" in self._memo:
            return None
        op = _wtw_ops(self._kernel_cache["WtW"])[0]
        if not op.is_half or op.root is not None or "_cnt" not in self._kernel_cache:
            return None
        pst = self._memo.get("precond", {}).get(0)
        wsum_new = float(self._wsum[0]) + X.shape[0]
        if pst is None or pst["ver"] != ver:
            return None
        if wsum_new > 2.0 * pst["wsum"] and not self._density_profile_still_fits(pst):
            return None                                   # the density profile has moved: generic path (new eigenbasis) this step
        if basis_slow(pst, (self._last_iters or [0])[0], wsum_new):
            return None
        tol = _default_tol(self._dtype)
        c = self._kernel_cache
        # raw device pointers go into the prepared call: key it on every one of them (ids of Python wrappers can be reused)
        sh = self.__dict__.get("_stencil_shard")
        key = (None if sh is None else (sh["rank"], sh["world"]), ver, ms["U"].data_ptr(), ms["Z"].data_ptr(), ms["R"].data_ptr(), op.stencil.data_ptr(), c["interpolation_cache"].data_ptr(),
               c["_cnt"].data_ptr(), c["_stats"].data_ptr(), self._err.data_ptr(), pst["eig"][0].data_ptr(), str(self._device), tol,
               settings.cg_check_every.value(), settings.max_cg_iterations.value())
        cached = self._stream_step_cache
        if cached is None or cached[0] != key:
            tcol, s2, _ = self._hyper()[0]
            step = grid_ops.StreamStep(self._grid, self._dtype, self._device, op.stencil, c["interpolation_cache"][0, :, 0], c["_cnt"][0],
                                       c["_stats"][0], self._err, ms["U"][0], ms["Z"][0], ms["R"][0], tcol, self._pcg_ws,
                                       settings.max_cg_iterations.value())
            step.set_solver(1.0 / s2, pst["eig"], 0.0, tol, 1)
            if sh is not None:
                step.set_shard(sh["rank"], sh["world"], comm=sh.get("comm"), allreduce=sh["allreduce"])
            cached = self._stream_step_cache = (key, step)
        return cached[1], ms, pst

    def _density_profile_still_fits(self, pst):
        """The data volume has doubled since the preconditioner's density profile was last looked at.  Look at it from inside
        the one-call streaming path instead of sending the step through the generic three-call one (4 looks per 3droad-sized
        pass used to cost a ~1 ms generic step each), and without draining the pipeline: the 3 small reductions and the copy
        of the marginals to pinned memory are QUEUED now, the verdict is read by whichever later step finds the copy done;
        meanwhile the stream carries on with the basis it has.  On a stationary stream the normalised profile has not moved
        (settings.precond_profile_drift): the eigenbasis stays, only the scale follows.  False: the profile moved (or there is
        none) -- the caller falls back to the generic path and `_precond` re-solves the eigenbasis."""
        old = pst.get("profiles")
        if old is None or settings.density_profile_preconditioner.off() or self._kernel_cache.get("_cnt") is None:
            return False
        look = self._profile_look
        if look is None:
            margs = self._cnt_marginals(0)
            host = self._profile_look_host                            # pinned once (a pinned allocation costs ~0.3 ms)
            if host is None or host.shape != margs.shape:
                host = self._profile_look_host = torch.empty(margs.shape, dtype=margs.dtype, pin_memory=True)
            host.copy_(margs, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._profile_look = (host, ev, float(self._wsum[0]), margs)
            return True
        host, ev, wsum_then, _ = look
        if self.__dict__.get("_stencil_shard") is not None:
            ev.synchronize()                              # sharded replicas must all read the verdict at the SAME step (control flow
        elif not ev.query():                              # that depends on copy timing would let the ranks' collectives diverge)
            return True                                   # still in flight
        self._profile_look = None
        profiles, _ = density_profiles(host.numpy(), self._grid.g, self._grid.m)
        if profiles is None or profiles_moved(profiles, old):
            return False
        basis_kept(pst, wsum_then)
        return True

    def _rank_update_source(self, q):
        """The cached dense posterior(s), if a rank-q Woodbury update of them is valid and cheaper than a fresh factor:
        dense regime, cache built for the current hyper-parameters, 0 < q <= m / 8, fewer than 64 stacked updates."""
        if q == 0 or not self._use_dense() or q > self._grid.m // 8 or settings.dense_rank_updates.off():
            return None
        self._apply_pending_rank_update()
        pc = self._memo.get("prediction_cache")
        if pc is None or pc.get("ver") != self._hyper_version():
            return None
        posts = pc["pred_cov"].ops if self.num_outputs > 1 else [pc["pred_cov"]]
        if not all(isinstance(p, DenseInducingPosterior) and p.updates < 64 for p in posts):
            return None
        return posts

    @staticmethod
    def _seed_rank_updated_cache(target, old_posts, X, noise, Y):
        """Note on `target` (self or the sibling model) that its prediction cache can be obtained from `old_posts` by a
        rank-q update.  Applied lazily by the next prediction_cache request; dropped if the caches are dumped first
        (e.g. by a hyper-parameter step), so a BO loop that refits after every update pays nothing for it."""
        if old_posts is None:
            return
        X = X.reshape(-1, target._grid.d).to(target._device, target._dtype).contiguous()
        was = []
        for o in range(target.num_outputs):
            if noise is None:
                was.append(torch.ones(X.shape[0], dtype=target._dtype, device=target._device))
            else:
                was.append(target._weight_a(noise.to(target._device, target._dtype)[:, o], False))
        target._memo["pending_rank_update"] = (old_posts, X, was, target._hyper_version())

    def _apply_pending_rank_update(self):
        pend = self._memo.pop("pending_rank_update", None)
        if pend is None or "prediction_cache" in self._memo:
            return
        old_posts, X, was, ver = pend
        if ver != self._hyper_version():
            return
        self.check_bounds()         # as a fresh dense factor would: raise for out-of-grid inputs before trusting the update
        b = self._kernel_cache["interpolation_cache"]
        out = self.num_outputs
        posts, U = [], torch.empty((out, self._grid.m), dtype=self._dtype, device=self._device)
        ops = _wtw_ops(self._kernel_cache["WtW"])
        for o in range(out):
            post = old_posts[o].rank_update(ops[o], X, was[o], self._err)
            U[o] = post.solve_columns(b[o, :, 0][None])[0][0]
            posts.append(post)
        self._last_iters = [0] * out
        self._memo["prediction_cache"] = {"pred_mean": U[..., None], "pred_cov": posts[0] if out == 1 else BatchOperator(posts),
                                          "cg_iters": [0] * out, "ver": ver}

    # --------------------------------------------------------- sample paths --
    def sample_paths(self, num_paths, seed=0, base_samples=None, tol=None):
        """`num_paths` joint draws u_s ~ N(M b, sigma2 M) of the m inducing values, as a :class:`GridSamplePaths`: each is a posterior
        FUNCTION sample f_s(x) = w(x)^T u_s (the SKI kernel is W Kuu W^T: no residual term), to be evaluated, differentiated and
        maximised at any number of points.  z [num_paths, m] standard normals: `base_samples`, or drawn from `seed`
        on the host generator.
          dense regime (a cached dense M):  u = M b + sigma chol(M + jitter) z; any num_paths, no probes needed;
          otherwise, Matheron's rule in statistics space:  u_s = eta_s + M (b - A eta_s - sigma P_s), eta_s = Kuu^(1/2) z_s, with the
          probe vectors P_s accumulated beside b while the points streamed by (``num_path_probes``): path s uses probe s, so
          num_paths <= num_path_probes.  The columns are solved by the system the mean solves, at `tol` (default: the mean's).
        Nothing is cached: two calls with the same arguments on the same state compute the same paths again (the normals come from the
        seeded host generator, the probes are fixed; beyond the dense regime the values agree to the solver's tolerance).  The paths of ONE call are independent draws; beyond
        the dense regime, paths with the same index s from calls with different seeds share probe s (the data-noise half of their
        randomness) and are therefore correlated: draw all the paths an acquisition needs in one call."""
        from ..sample_paths import GridSamplePaths

        self._refuse_trend("sample_paths", "a path would need a joint draw of the coefficients and the inducing values")
        if self.num_outputs != 1:
            raise NotImplementedError("sample_paths is implemented for a single output")
        num_paths = int(num_paths)
        if num_paths < 1:
            raise ValueError("num_paths must be positive")
        grid, m = self._grid, self._grid.m
        pc = self.prediction_cache                  # (finishes a deferred refresh, rejoins a sharded stencil)
        post = pc["pred_cov"]
        cache = self._kernel_cache
        if base_samples is None:
            gen = torch.Generator(device="cpu").manual_seed(int(seed))
            z = torch.randn((num_paths, m), generator=gen, dtype=torch.float64)
        else:
            z = base_samples
            if tuple(z.shape) != (num_paths, m):
                raise ValueError(f"base_samples must be [num_paths = {num_paths}, m = {m}], got {tuple(z.shape)}")
        z = z.to(self._device, self._dtype).contiguous()
        sigma = math.sqrt(self._sigma2(0))
        gb = self.covar_module.grid_bounds
        if hasattr(post, "dense"):
            fac = getattr(post, "_path_chol", None)
            if fac is None:
                # the sampling factor in fp64 whatever the model's precision (m <= max_cholesky_size), with rsample's jitter rule
                # (distributions.sampling_cholesky): jitter * mean(diag) on the diagonal, escalated tenfold until the factor exists
                M64 = post.dense.double()
                M64 = 0.5 * (M64 + M64.t())
                scale = float(M64.diagonal().mean().clamp_min(1e-30))
                base = 1e-6 if self._dtype == torch.float32 else 1e-8
                for i in range(6):
                    jit = base * 10 ** i * scale
                    L = M64.clone()
                    L.diagonal().add_(jit)
                    if int(grid_ops.potrf_(L).item()) == 0 and bool(torch.isfinite(L.diagonal()).all()):
                        break
                else:
                    raise RuntimeError("the posterior covariance of the inducing values is not positive definite after jitter")
                fac = post._path_chol = (L.tril().contiguous(), jit)
            L, jit = fac
            dev = grid_ops.gemm(z.double(), L, tb=True)                       # rows z_s^T L^T = (L z_s)^T
            u = (pc["pred_mean"][0, :, 0].double()[None] + sigma * dev).to(self._dtype)
            paths = GridSamplePaths(grid, u.contiguous(), gb, True, [0], jit)
        else:
            P = cache.get("path_probes")
            if P is None:
                raise RuntimeError("sample_paths beyond the dense regime needs the probe vectors that are accumulated while the data stream by: "
                                   "build the model with num_path_probes=S (S >= the number of paths wanted)")
            if num_paths > P.shape[1]:
                raise ValueError(f"{num_paths} paths asked for, but the model keeps num_path_probes={P.shape[1]} probes (path s uses probe s): "
                                 "build it with a larger num_path_probes")
            tcol = self._hyper()[0][0]
            ver = self._hyper_version()
            pe = self._memo.get("path_eig")
            if pe is None or pe[0] != ver:
                pe = self._memo["path_eig"] = (ver, grid_ops.kron_eigen(grid, tcol))
            eta = grid_ops.kron_spectral_mm(grid, pe[1], z, kscale=1.0, power=0.5)                    # Kuu^(1/2) z   [k, m]
            rhs = cache["interpolation_cache"][0, :, 0][None] - grid_ops.stencil_spmv(grid, post.wtw.stencil, eta)
            rhs -= sigma * P[:, :num_paths].t()
            u = torch.empty_like(eta)
            chunk = max(1, int(settings.variance_chunk.value()))
            tol_keep, conv, iters = post.tol, True, []
            if tol is not None:
                post.tol = float(tol)
            try:
                for s in range(0, num_paths, chunk):
                    e = min(s + chunk, num_paths)
                    U, _ = post.solve_columns(rhs[s:e].contiguous())
                    u[s:e] = eta[s:e] + U
                    iters.append(post.last_iters)
                    conv = conv and bool(getattr(post, "last_converged", True))
                    if post.last_err:
                        self._raise_out_of_bounds(post.last_err)
            finally:
                post.tol = tol_keep
            paths = GridSamplePaths(grid, u, gb, conv, iters)
        return paths

    def get_fantasy_model(self, inputs, targets, noise_term=None, **kwargs):
        """BFN:287-332.  inputs [*b, q, d], targets [*b, q] or [num_fantasies, *b, q]: a batch of conditioned copies
        (``models/fantasy.py``: specified from the maths, the reference's cache expansion is broken at HEAD);
        unbatched inputs [q, d] with targets [q] / [q, 1]: a plain functional ``condition_on_observations``."""
        plain = inputs.dim() == 2 and (targets.dim() == 1 or (targets.dim() == 2 and tuple(targets.shape) == (inputs.shape[0], self.num_outputs)))
        if not plain:
            from .fantasy import BatchedFantasyModel

            self._refuse_trend("batched conditioning (fantasies)", "a fantasy batch carries A and b only, not the trend statistics")
            if self.noise_model is not None:
                raise NotImplementedError("batched conditioning (fantasies) of a heteroscedastic model: a fantasy batch carries the statistics "
                                          "of f alone, and its noise would have to be fantasised with it")
            return BatchedFantasyModel(self, inputs, targets, noise_term)
        if targets.dim() == 1:
            targets = targets[:, None]
        if noise_term is None:
            noise_term = torch.ones_like(targets)
        return self.condition_on_observations(inputs, targets, noise_term, inplace=False, _decay=False)   # a what-if on the current state

    # ------------------------------------------------------------ regridding --
    def regrid_(self, below, above, drop="zero", _grid=None):
        """Grow, shift or trim the inducing grid by whole nodes, in place and exactly: ``below[q]`` nodes are added in
        front of dim q and ``above[q]`` behind it (ints or per-dim sequences, negative: removed) at unchanged spacing,
        ``GridSpec.shifted``.  A, b, cnt and the path probes are the old arrays at an index shift (new nodes hold zeros) and move in ONE
        launch (``wiski_regrid_stats``); y^T D^-1 y, log|D|, ``num_data``, the noise-weight sums and the probes' seed / count stay.
        Posterior, marginal likelihood and sample paths are unchanged to solver tolerance, and the model equals one built on the new grid
        from all the data, as long as every absorbed point lies in an interior cell of both grids (points inside ``grid_bounds`` do).
        Removing nodes no datum touches (A_ii = 0) is exact as well.

        ``drop="zero"`` (default): if a removed node has A_ii != 0 a ValueError names the dims and the dropped mass, and the model is left
        bit for bit as it was.  ``drop="any"`` commits anyway -- an APPROXIMATION: A becomes the principal submatrix on the kept nodes
        (still PSD), b / cnt / probes lose the removed entries, the scalar statistics keep counting the points.

        Everything derived from the grid size is dropped and rebuilt on next use (root pairs, spectral factors, two-level block,
        preconditioner, streaming-step cache, PCG workspace, the warm-start state of the mean solve); the regime (dense / PCG) is
        re-decided from the new m.  The kernel module receives the new grid: sibling models that share ``covar_module`` (functional
        ``condition_on_observations``) must not be used afterwards.  Returns the model for ``drop="zero"`` (as ``forget_`` does) and
        ``(model, dropped_mass)`` -- a float, summed over the outputs -- for ``drop="any"``.

        The noise model of a heteroscedastic model follows by the same nodes, with the same ``drop``, and is handed this model's new grid
        object (`_grid`: the hand-over).  Its sites sit where f's points do, so ``drop="zero"`` cannot fail on it once f has passed; what
        ``drop="any"`` cut from it is ``model.noise_model.last_regrid_dropped_mass`` (in the noise model's own units, not added to the
        float returned)."""
        if drop not in ("zero", "any"):
            raise ValueError(f'drop must be "zero" or "any", got {drop!r}')
        old = self._grid
        new = old.shifted(below, above) if _grid is None else _grid
        a = [int(below)] * old.d if isinstance(below, int) else [int(v) for v in below]
        bb = [gn - go - aq for gn, go, aq in zip(new.g, old.g, a)]
        if not any(a) and not any(bb):
            return self if drop == "zero" else (self, 0.0)
        if self.window is not None and (any(v < 0 for v in a) or any(v < 0 for v in bb)):
            raise NotImplementedError("window: regrid_ may only grow the grid -- a point of the ring whose nodes were removed could not "
                                      "be taken out of the statistics again")
        self._finish_pending()
        self.leave_stencil_shard()
        regions, fresh = kc.regrid_plan(self._kernel_cache, old, new)
        rows, mass = grid_ops.regrid_stats(old, new, a, regions)
        if sum(rows) > 0 and drop == "zero":
            dims = [q for q in range(old.d) if a[q] < 0 or bb[q] < 0]
            raise ValueError(f"regrid_: trimming dims {dims} (below {a}, above {bb}) would drop {sum(rows)} inducing nodes that carry data, "
                             f"dropped mass sum A_ii = {sum(mass):.6g}; pass drop=\"any\" to cut anyway (an approximation)")
        # ---- commit: swap the buffers, hand the new grid round, drop what was derived from the old size
        self._drop_spectral()
        kc.regrid_commit(self._kernel_cache, fresh, trimmed=any(v < 0 for v in a + bb))
        self.covar_module.set_grid_spec(new)
        self._grid = new
        self._memo = {}                                # Toeplitz columns, preconditioner, prediction cache, root space, ...
        self._stream_step_cache = self._profile_look = self._profile_look_host = None
        self.__dict__.pop("_two_level", None)
        self._half_delta = None
        self._pcg_ws = grid_ops.PCGWorkspace()
        self._mean_state = None                        # (Z = Kt^-1 U does not embed: the next solve starts cold)
        self._last_iters = None
        self.__dict__["_regrid_count"] = self.__dict__.get("_regrid_count", 0) + 1
        if self.noise_model is not None:
            # the noise model follows by the same nodes and the same rule, on this model's new grid object: operators, kernel and model
            # all hold `new` itself (its sites sit where f's points do: A_ii of f is zero wherever its own is)
            nm = self.noise_model
            nm.last_regrid_dropped_mass = 0.0
            if drop == "zero":
                nm.regrid_(below, above, _grid=new)
            else:
                nm.last_regrid_dropped_mass = nm.regrid_(below, above, drop="any", _grid=new)[1]
        return self if drop == "zero" else (self, float(sum(mass)))

    def grow_to_cover_(self, X, margin_nodes=1):
        """The smallest whole-node growth (``regrid_``) after which every row of X [n, d] lies in an interior cell, at least
        `margin_nodes` nodes away from the first and the last node of every dim; nothing happens (beyond one fused min / max and one host
        read) when X already does.  Rows that are not finite are ignored (the absorb flags them as out of bounds).  If a dim would
        exceed ``max_grid_size`` (an int or one per dim) the model's out-of-bounds RuntimeError is raised and nothing changes.
        Returns the model."""
        grid = self._grid
        k = max(1, int(margin_nodes))
        X = X.detach().reshape(-1, grid.d)
        if X.shape[0] == 0:
            return self
        lo, hi = torch.aminmax(X.double(), dim=0)
        ext = torch.stack((lo, hi)).tolist()
        below, above = [0] * grid.d, [0] * grid.d
        for q in range(grid.d):
            xmin, xmax = ext[0][q], ext[1][q]
            if not (math.isfinite(xmin) and math.isfinite(xmax)):
                continue
            below[q] = max(0, math.ceil((grid.g0[q] - xmin) / grid.h[q]) + k)               # xmin >= new node k
            above[q] = max(0, math.ceil((xmax - grid.g0[q]) / grid.h[q]) - grid.g[q] + 1 + k)     # xmax <= new node g' - 1 - k
        if not any(below) and not any(above):
            return self
        cap = self.max_grid_size
        if cap is not None:
            cap = [int(cap)] * grid.d if isinstance(cap, int) else [int(v) for v in cap]
            if any(g + a + b > c for g, a, b, c in zip(grid.g, below, above, cap)):
                self._raise_out_of_bounds(1)
        self.regrid_(below, above)
        return self

    # ------------------------------------------------------------ forgetting --
    def forget_(self, gamma):
        """Exponential forgetting, in place: every streamed statistic is scaled by gamma in (0, 1] -- A, b, c, cnt by
        gamma, the path probes by sqrt(gamma), log|D| moved by -n log gamma -- in ONE launch (``wiski_decay_stats``; a trend model's C rides on it,
        its p x p G and p-vector g are scaled by two small launches beside it).  The model is then
        exactly the GP in which every point absorbed so far has its noise d_i replaced by d_i / gamma (k calls: d_i gamma^-k): posterior,
        marginal likelihood and sample paths follow.  ``num_data`` counts points and stays.  The warm-start state of the mean solve is
        kept (its carried residual follows in closed form in the same launch); everything else derived from A is rebuilt on next use.
        gamma = 1 does nothing.  Returns the model.

        log|D| moves by ``num_data`` log gamma.  Points outside the grid that an absorb dropped are still counted in ``num_data`` until
        the next ``check_bounds()`` takes them out (it is the one host sync), though they never entered log|D|: a decay between the two
        moves log|D| -- the marginal likelihood only, not the posterior -- by ``dropped`` log gamma too much.  A stream that may
        leave the grid and reads the MLL calls ``check_bounds()`` before it forgets."""
        gamma = float(gamma)
        if not (0.0 < gamma <= 1.0):
            raise ValueError(f"gamma must lie in (0, 1], got {gamma}")
        if self.window is not None:
            raise NotImplementedError("forget_ on a model with window: the ring keeps the weights its points entered with, and a point that "
                                      "left after a decay would take out more than is still there -- the two are alternatives")
        if self.site_memory is not None:
            raise NotImplementedError("forget_ on a model with site_memory: a decayed site is no longer the stored one, and a sweep would "
                                      "take out more than is still in the statistics")
        if gamma != 1.0:
            if self.num_data is None:
                raise RuntimeError("forget_ needs the number of absorbed points (log|D| moves by -n log gamma): hand num_data over with the kernel cache")
            self._decay(gamma, self.num_data)
        return self

    def _decay(self, gamma, count, keep_mean_cache=False):
        """forget_ for statistics that hold `count` points per output.  keep_mean_cache (the one-call streaming step, whose refresh
        follows in the same call): the prediction cache of the PCG regime -- the operator and a view of the mean state -- stays."""
        self._finish_pending()
        self.leave_stencil_shard()
        cache = self._kernel_cache
        regions = kc.decay_regions(cache, self._grid, gamma)    # (a trend's G and g are scaled there, beside the launch below)
        # R = b - Z - A U of the mean state: Z = Kt^-1 U does not depend on the data, so gamma R - (1 - gamma) Z is the residual of the
        # same (U, Z) in the decayed system -- the next refresh starts warm and without an A U product
        ms = self._carried(True)
        # (one launch for up to 8 outputs; beyond, one per 8 -- of stats rows and of the device parts of the noise-weight sums alike)
        grid_ops.decay_stats(gamma, regions, stats=cache["_stats"], counts=[float(count)] * self.num_outputs,
                             R=ms["R"] if ms else None, Z=ms["Z"] if ms else None, side=self._wsum_dev)
        self._wsum_host = [gamma * w for w in self._wsum_host]
        self._wsum_dev_host = [gamma * w for w in self._wsum_dev_host]
        # derived from A (set_train_data's recipe, except that what is invariant under a scaling stays):
        self._give_up(cache)                         # (root pair, Gram matrix and factors belong to the undecayed statistics)
        # the preconditioner (_memo["precond"]) stays: its eigenbasis depends on the NORMALISED density profile of cnt, which a scaling
        # leaves alone, and its shift is wsum / norm at every use.  The mass the profile was taken at stays as well, so that "the data
        # volume has doubled / halved since" keeps looking at the profile of a stream whose old points fade
        # _stream_step_cache bakes pointers only (its shift is set at every step): it stays
        if keep_mean_cache and not self._use_dense():
            self._memo.pop("pending_rank_update", None)
            self._memo.pop("root_space", None)
        else:
            self._dump_caches()
        if self.noise_model is not None:             # the noise sites age with the points they were taken from
            self.noise_model._decay(gamma, self.noise_model.num_data or 0)

    def set_train_data(self, train_inputs, train_targets, train_noise_term):
        """:420-428 -- rebuild every statistic from scratch."""
        if train_targets.dim() == 1:
            train_targets = train_targets[:, None]
        noise = self._canon_noise(train_noise_term, train_targets)
        cache = self._clear_statistics()
        if self.noise_model is not None:             # (the data is absorbed plainly, as the initial data is: the noise model starts empty)
            nm = self.noise_model
            nm._clear_statistics()
            nm.num_data, nm._mean_state = 0, None
            nm._dump_caches()
        if self.window is not None:
            self._window_restart(train_inputs, train_targets, noise)     # the last `window` points only
        else:
            self._absorb(cache, train_inputs, train_targets, noise, init=True)
            self.num_data = train_inputs.reshape(-1, self._grid.d).shape[0]
        self._mean_state = None
        self._dump_caches()

    def _clear_statistics(self):
        """Zero every streamed statistic and drop what was derived from them; returns the kernel cache."""
        self._finish_pending()                      # a deferred solve must not be resumed on zeroed statistics
        self._stream_step_cache = None
        kc.zero_(self._kernel_cache)
        self._wsum_dev.zero_()
        self._wsum_host = [0.0] * self.num_outputs
        self._wsum_dev_host = [0.0] * self.num_outputs
        self._wsum_dirty = False
        self._memo.pop("precond", None)
        self._drop_spectral()
        return self._kernel_cache

    def to(self, *args, **kwargs):
        res = super().to(*args, **kwargs)
        if self.noise_model is not None:             # (not a registered submodule: it is moved by hand)
            self.noise_model.to(*args, **kwargs)
        device = None
        for a in args:
            if isinstance(a, (str, torch.device)):
                device = torch.device(a)
            elif torch.is_tensor(a):
                device = a.device
        device = kwargs.get("device", device)
        if device is not None and self._kernel_cache is not None and torch.device(device) != self._device:
            self._kernel_cache = kc.to(self._kernel_cache, self._grid, device)
            self._device = torch.device(device)
            self._err = grid_ops.new_err_flag(device)
            self._mean_state = None
            self._memo = {}
            self._stream_step_cache = None
            self._drop_spectral()
        return res

    # ------------------------------------------- checkpoint, restore and merge --
    def _refuse_rings(self, what):
        if self.window is not None or self.site_memory is not None:
            raise NotImplementedError(f"{what} on a model with {'window' if self.window is not None else 'site_memory'}: its ring holds points, "
                                      "not statistics, with host-side bookkeeping on the model beside it (the void slots, the unit / explicit "
                                      "split of the weight sum), and two rings have no union -- a state carries streamed statistics only")

    def _settle(self):
        """check_bounds()'s recipe before the statistics leave the model or are added to: nothing pending, no stencil shard, the out-of-grid
        flag read -- so that num_data counts exactly the points the statistics hold."""
        self.leave_stencil_shard()
        self.check_bounds()

    def _wsum_from_cnt(self):
        """The noise-weight sums from the row sums of W^T D^-1 W, as _raise_out_of_bounds rebuilds them (in place: the device part's address stays)."""
        cnt = self._kernel_cache.get("_cnt")
        self._wsum_host = [0.0] * self.num_outputs
        self._wsum_dev_host = [0.0] * self.num_outputs
        if cnt is not None:
            self._wsum_dev.copy_(cnt.sum(dim=1, dtype=torch.float64))
            self._wsum_dirty = True

    def stream_state(self, device="cpu"):
        """The live model as a state: ``kernel_cache.pack`` of its statistics -- every node region in compact form, only the
        nodes that hold anything, found and moved on the device -- plus ``num_data``, ``module`` (this model's ``state_dict()``) and, for
        a heteroscedastic model, ``noise_model``: the nested state of ``model.noise_model`` with its kernel's parameters, which this
        model's ``state_dict()`` does not carry.  The dict holds tensors (on `device`, default the host), ints, floats, strings, lists
        and dicts only: ``torch.save`` and ``torch.load(..., weights_only=True)`` round-trip it.  As ``check_bounds()``: pending work is
        finished, a stencil shard is left, and the out-of-grid flag is read -- a stream that left the grid raises its RuntimeError here,
        with ``num_data`` corrected, and the next call packs what was absorbed.  Spectral factors, root pairs, the warm-start state and
        the two-level block are not carried.  window / site_memory: NotImplementedError."""
        self._refuse_rings("stream_state")
        self._settle()
        state = kc.pack(self._kernel_cache, self._grid, device=device)
        state["num_data"] = None if self.num_data is None else int(self.num_data)
        state["module"] = {k: v.detach().to(device).clone() for k, v in self.state_dict().items()}
        if self.noise_model is not None:
            state["noise_model"] = self.noise_model.stream_state(device)
        return state

    def _check_stream_state(self, state, what):
        kc._check_state(state)
        kc._check_fits(self._kernel_cache, self._grid, state, what)
        if (self.noise_model is None) != (state.get("noise_model") is None):
            raise ValueError(f"{what}: 'noise_model' is {'missing from' if self.noise_model is not None else 'present in'} the state, but this model is "
                             f"{'' if self.noise_model is not None else 'not '}heteroscedastic")
        if self.noise_model is not None:
            self.noise_model._check_stream_state(state["noise_model"], what + " (noise model)")

    def load_stream_state_(self, state, load_module=True):
        """Restore a ``stream_state()`` into this model, built with the same configuration on the state's grid, in place:
        the statistics are zeroed and the state is scattered INTO the tensors the model already holds, and ``load_state_dict`` copies
        into the existing parameters (load_module=False leaves the hyper-parameters alone) -- no address changes, so a captured hyper step
        keeps replaying.  ``num_data`` is the state's, the noise-weight sums are rebuilt from cnt; everything derived (spectral factors,
        root pairs, preconditioner, two-level block, the warm-start state) is rebuilt on next use: the first solve is cold.  The state
        is checked as a whole before anything is written (ValueError names the field).  Returns the model."""
        self._refuse_rings("load_stream_state_")
        self._check_stream_state(state, "load_stream_state_")
        self.leave_stencil_shard()
        cache = self._clear_statistics()
        kc.load_into_(cache, self._grid, state)
        if load_module and state.get("module") is not None:
            self.load_state_dict(state["module"])
            self.hyperparameters_changed()
        self.num_data = state.get("num_data")
        self._wsum_from_cnt()
        self._give_up(cache)
        self._mean_state = None
        self._last_iters = None
        self._dump_caches()
        if self.noise_model is not None:
            self.noise_model.load_stream_state_(state["noise_model"], load_module=load_module)
        return self

    def merge_(self, other, weight=1.0):
        """Add the statistics of `other` -- a model, or a ``stream_state()`` -- to this model's, in place.  The statistics
        are additive and independent of the kernel, so the model is afterwards exactly the GP of both sets of points under THIS model's
        hyper-parameters, the other's points at noise d_i / weight (weight in (0, 1]; 1: as they were absorbed).  The hyper-parameters
        of `other` are ignored.  Only the nodes `other` touched are read and added (a model is not packed first).  ``num_data`` adds,
        the noise-weight sums are rebuilt from cnt.  Path probes add at sqrt(weight), and the two streams must have been built with
        different ``path_seed`` (ValueError otherwise); the receiver keeps its seed and count.  weight != 1 needs the other side's
        ``num_data`` (log|D| moves by -n log weight) and raises like ``forget_`` without it.  Refused with NotImplementedError: window /
        site_memory on either side, a heteroscedastic model on either side (the noise sites of one model were matched against its own
        posterior), different grids (``regrid_`` moves a model onto the other's grid first).  Returns the model."""
        weight = float(weight)
        if not (0.0 < weight <= 1.0):
            raise ValueError(f"weight must lie in (0, 1], got {weight}")
        self._refuse_rings("merge_")
        is_model = isinstance(other, FixedNoiseOnlineSKIGP)
        if is_model:
            other._refuse_rings("merge_")
        if self.noise_model is not None or (other.noise_model if is_model else other.get("noise_model")) is not None:
            raise NotImplementedError("merge_ on or with a heteroscedastic model: the noise sites of a model were matched against its own posterior "
                                      "of f, and the sum of two noise models is the noise model of neither stream")
        if is_model:
            other._settle()
            src, n_other, og = other._kernel_cache, other.num_data, kc._grid_dict(other._grid)
        else:
            kc._check_state(other)
            src, n_other, og = other, other.get("num_data"), other["grid"]
        mine = kc._grid_dict(self._grid)
        if any(list(og[f]) != mine[f] for f in ("size", "g0", "h")):
            raise NotImplementedError(f"merge_ across different grids (size {og['size']}, g0 {og['g0']}, h {og['h']} against this model's "
                                      f"{mine['size']}, {mine['g0']}, {mine['h']}): statistics add node by node -- regrid_ moves one model onto "
                                      "the other's grid first, by whole nodes at equal spacing")
        if weight != 1.0 and n_other is None:
            raise RuntimeError("merge_ with weight != 1 needs the number of points the other side absorbed (log|D| moves by -n log weight): "
                               "hand num_data over with the kernel cache")
        self._settle()
        cache = self._kernel_cache
        kc.merge_into_(cache, self._grid, src, weight, n_other)
        self.num_data = None if self.num_data is None or n_other is None else self.num_data + n_other
        self._wsum_from_cnt()
        self._give_up(cache)
        self._memo.pop("precond", None)
        self._stream_step_cache = None
        self._mean_state = None
        self._last_iters = None
        self._dump_caches()
        return self

    # ------------------------------------------------- distributed statistics --
    def stats_buffers(self):
        """Tensors that are additive over data shards (what RCCL all-reduces):
        b, the W^T W stencils and (y^T D^-1 y, logdet D)."""
        c = self._kernel_cache
        return [c["interpolation_cache"], c["_stats"], c["_cnt"]] + [op.stencil for op in _wtw_ops(c["WtW"])]
