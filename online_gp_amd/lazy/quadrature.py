"""Posterior of box integrals and averages of the function: Bayesian quadrature on the inducing grid.

With the SKI model ``f(x) = w(x)^T u`` the integral of ``f`` over a box is ``c^T u`` with ``c = int_box w(x) dx`` -- a Kronecker product
of d per-dimension rows, in closed form for the cubic interpolant -- so it is Gaussian with mean ``c^T u_bar`` and variance
``sigma2 c^T M c``, ``M`` the operator the prediction cache holds.  :class:`BoxCovariance` evaluates the (co)variances of a set of
boxes, :class:`IntegralPosterior` is what ``posterior_integral`` returns."""
import torch

from .. import grid_ops


class BoxCovariance:
    """``sigma2 C^T M C`` for B boxes: ``diag()`` [B] or ``joint()`` [B, B].

    Dense posterior (``post.dense``): ``wt_columns_box`` -> product with M -> ``gather_box``.  Matrix-free: chunks of ``chunk`` boxes,
    each ``wt_columns_box`` -> ``post.solve_columns`` -> ``gather_box``.  Those solves run at the operator's own tolerance
    (``settings.variance_cg_tolerance`` is for plain quadratic forms: the off-diagonal entries are first order in the residual)."""

    def __init__(self, post, tables, sigma2, err, chunk=64):
        # err: kept for the signature it shares with JetCovariance; the flag is raised where the tables are made (box_tables) and
        # neither wt_columns_box nor gather_box takes one
        self.post, self.tables, self.sigma2, self.err = post, tables, float(sigma2), err
        self.grid = post.grid
        self.step = max(1, int(chunk))
        self.cg_iters = []                              # per solve of the matrix-free path

    def _solved(self, tables):
        cols = grid_ops.wt_columns_box(self.grid, tables)
        if hasattr(self.post, "dense"):
            return grid_ops.gemm(cols, self.post.dense.contiguous())       # rows (M c_b)^T, M symmetric
        U, _ = self.post.solve_columns(cols)
        self.cg_iters.append(getattr(self.post, "last_iters", 0))
        return U

    def _chunks(self):
        B = self.tables.B
        step = max(B, 1) if hasattr(self.post, "dense") else self.step
        return [(s, min(s + step, B)) for s in range(0, B, step)]

    def diag(self):
        t = self.tables
        out = torch.empty((t.B,), dtype=t.tab.dtype, device=t.tab.device)
        for s, e in self._chunks():
            out[s:e] = grid_ops.gather_box(self.grid, t[s:e], self._solved(t[s:e]), rows_per_box=1)[:, 0]
        return out * self.sigma2

    def joint(self):
        t = self.tables
        full = torch.empty((t.B, t.B), dtype=t.tab.dtype, device=t.tab.device)
        for s, e in self._chunks():
            full[:, s:e] = grid_ops.gather_box(self.grid, t, self._solved(t[s:e]))
        full = full * self.sigma2
        return 0.5 * (full + full.t())


class IntegralPosterior:
    """Gaussian posterior of the integrals (or, built with ``average``, the averages) of ``f`` over B boxes.

    ``mean`` [B]; ``variance`` [B]; with ``joint`` also ``covariance`` [B, B]; ``volume`` [B] the volume of each box clipped to the
    grid's extent (a dimension with ``lower == upper`` counts as factor 1).  Everything is detached from autograd."""

    def __init__(self, mean, cov, volume, joint):
        self.mean, self.volume, self.joint = mean, volume, bool(joint)
        self._cov = cov
        self.B = mean.shape[0]
        self.cg_iters = []

    @property
    def covariance(self):
        if not self.joint:
            raise AttributeError("covariance: the posterior was built without joint=True (variance holds the diagonal)")
        return self._cov

    @property
    def variance(self):
        return self._cov.diagonal() if self.joint else self._cov

    @property
    def stddev(self):
        return self.variance.clamp_min(0.0).sqrt()

    def rsample(self, sample_shape=torch.Size(), base_samples=None):
        """Draws of the integrals, [*sample_shape, B]: from the joint covariance when the posterior was built with ``joint=True`` (a
        jitter of 1e-6 (fp32) / 1e-10 (fp64) times the mean diagonal entry is added before factorising, as ``JetPosterior.rsample``
        does), else independently per box.  ``base_samples``: standard normal draws of that shape."""
        shape = torch.Size(sample_shape) + (self.B,)
        if base_samples is None:
            base_samples = torch.randn(shape, dtype=self.mean.dtype, device=self.mean.device)
        z = base_samples.to(self.mean.dtype).to(self.mean.device).reshape(-1, self.B)
        if self.joint:
            draw = z @ self.cholesky().t()
        else:
            draw = z * self.stddev
        return self.mean + draw.reshape(shape)

    def cholesky(self):
        """Lower factor that ``rsample`` uses for the joint covariance (with its jitter)."""
        rel = 1e-6 if self.mean.dtype == torch.float32 else 1e-10
        A = self.covariance.clone()
        A.diagonal().add_(rel * A.diagonal().mean().clamp_min(0.0))
        return grid_ops.psd_safe_cholesky(A.contiguous(), jitter=float(rel * A.diagonal().mean())).tril()


def check_bounds_host(lower, upper, d, what, device, dtype):
    """The refusals of ``posterior_integral`` / ``GridSamplePaths.integrate``, on the host before any launch, and the bounds as
    contiguous ``dtype`` tensors on ``device``.  The checks run in the caller's own precision, before the cast: a box that the cast
    would collapse in some dimension (``lower < upper`` but equal after rounding to ``dtype``) is refused, because ``lower == upper``
    means "evaluate here" -- a different functional, with factor 1 of the volume instead of a width near 0."""
    lower, upper = torch.as_tensor(lower).detach(), torch.as_tensor(upper).detach()
    if lower.dim() > 2 or upper.dim() > 2:
        raise NotImplementedError(f"{what} takes unbatched bounds [B, d]")
    if lower.dim() != 2 or lower.shape[1] != d or upper.shape != lower.shape:
        raise ValueError(f"{what}: expected lower and upper of shape [B, {d}], got {tuple(lower.shape)} and {tuple(upper.shape)}")
    upper = upper.to(lower.device)
    if not bool((torch.isfinite(lower) & torch.isfinite(upper)).all()):
        raise ValueError(f"{what}: bounds must be finite (a box is clipped to the grid's extent anyway)")
    if bool((lower > upper).any()):
        raise ValueError(f"{what}: lower > upper")
    lo, hi = lower.to(device, dtype).contiguous(), upper.to(device, dtype).contiguous()
    if bool(((lo == hi) & (lower < upper).to(device)).any()):
        raise ValueError(f"{what}: a box narrower than {dtype} resolves (lower < upper, equal after the cast) would be evaluated, not integrated")
    return lo, hi


def scale_by_volume(volume):
    """1 / volume, zero where the clipped volume is zero."""
    ok = volume > 0
    return torch.where(ok, 1.0 / torch.where(ok, volume, torch.ones_like(volume)), torch.zeros_like(volume))
