"""Posterior sample paths on the inducing grid.

The SKI kernel is W Kuu W^T, so a posterior function sample IS f(x) = w(x)^T u with u one joint draw of the m inducing
values -- there is no residual term.  :class:`GridSamplePaths` holds such draws (``FixedNoiseOnlineSKIGP.sample_paths``
makes them) and evaluates them with the interpolation gathers: any number of points, differentiable w.r.t. the points,
consistent between calls.  That is what Thompson sampling, max-value sampling and pathwise acquisitions are made of
(BoTorch: ``get_matheron_path_model`` / ``MaxPosteriorSampling``)."""
import torch

from . import grid_ops, settings


class GridSamplePaths:
    """``values`` [num_paths, m]: the inducing values of each path.  ``paths(X)``: X [..., d] -> [num_paths, ...]."""

    def __init__(self, grid, values, grid_bounds=None, converged=True, iters=None, jitter=0.0):
        self.grid = grid
        self.values = values
        self.num_paths = values.shape[0]
        self.last_converged = bool(converged)      # every column of the solve behind the paths reached its tolerance
        self.iters = iters or []
        self.jitter = float(jitter)                # dense regime: what was added to diag(M) before its Cholesky factor
        self._grid_bounds = grid_bounds
        self._rows = None
        self._err = grid_ops.new_err_flag(values.device)

    def _check(self):
        # as the posterior does (models/batched_fixed_noise_online_gp.py, _eval_forward): one read of the device flag per call, which
        # settings.deferred_bounds_check turns off for loops that cannot afford the round trip (call check_bounds() after the loop)
        if settings.deferred_bounds_check.on():
            return
        self.check_bounds()

    def check_bounds(self):
        """Raise if any point evaluated so far was outside the grid (such points evaluate to zero)."""
        if grid_ops.read_flag(self._err):
            self._err.zero_()
            raise RuntimeError("Received data that was out of bounds for the specified grid. "
                               f"Grid bounds were {self._grid_bounds if self._grid_bounds is not None else self.grid.grid_bounds}.")

    def __call__(self, X):
        grid = self.grid
        lead = tuple(X.shape[:-1])
        if X.shape[-1] != grid.d:
            raise ValueError(f"expected points [..., {grid.d}], got {tuple(X.shape)}")
        Xf = X.reshape(-1, grid.d).to(self.values.device, self.values.dtype)
        if self.num_paths <= 4:
            out = grid_ops.Gather.apply(grid, Xf, self.values, self._err)           # a few columns: one gather (gradient per column)
        else:
            if self._rows is None:
                self._rows = self.values.t().contiguous()                             # [m, num_paths]: a tap reads all paths in one run
            out = grid_ops.GatherRows.apply(grid, Xf, self._rows, self._err)
        self._check()
        return out.t().reshape((self.num_paths,) + lead)

    def integrate(self, lower, upper, average=False):
        """Integral of every path over the boxes [lower_b, upper_b] ([B, d] each): [num_paths, B] -- exact for the
        path f = w^T u, so consistent with its point evaluations; ``average`` divides by the volume of the box clipped to the grid's
        extent.  A dimension with lower == upper is evaluated, not integrated.  Detached; a box not wholly inside the grid raises as a
        point outside does."""
        from .lazy.quadrature import check_bounds_host, scale_by_volume

        lo, hi = check_bounds_host(lower, upper, self.grid.d, "integrate", self.values.device, self.values.dtype)
        with torch.no_grad():
            tables = grid_ops.box_tables(self.grid, lo, hi, self._err)
            out = grid_ops.gather_box(self.grid, tables, self.values.detach())          # [B, num_paths]
            if average:
                out = out * scale_by_volume(tables.vol)[:, None]
        self._check()
        return out.t()

    def max_values(self, candidates):
        """max over the candidate points [..., d] of every path: [num_paths] (the discrete max-value sample of each path)."""
        with torch.no_grad():
            return self(candidates).reshape(self.num_paths, -1).max(dim=-1).values

    def argmax(self, candidates):
        """Index (into the flattened candidates) of every path's maximiser: [num_paths]."""
        with torch.no_grad():
            return self(candidates).reshape(self.num_paths, -1).argmax(dim=-1)
