"""Joint posterior of a function and its gradient at query points.

With the SKI model ``f(x) = w(x)^T u`` the jet ``(f, d_1 f, .., d_d f)(x) = J(x)^T u`` -- ``J(x)`` the ``C = d + 1`` rows
``[w(x); d_1 w(x); ..; d_d w(x)]`` of the derivative observations (3.15) -- is Gaussian with mean ``J(x)^T u_bar`` and covariance
``sigma2 J(x)^T M J(x)``, ``M`` the operator the prediction cache holds.  :class:`JetCovariance` evaluates that covariance,
:class:`JetPosterior` is what ``posterior_jet`` returns."""
import torch

from .. import grid_ops, settings


class JetCovariance:
    """``sigma2 J^T M J`` for a set of points: ``blocks()`` [n, C, C] per point, ``joint()`` [n C, n C] point-major.

    Dense posterior (``post.dense``): the blocks are one ``jet_quadform`` launch on the taps' sub-blocks of M; the joint matrix is
    ``wt_columns_jet`` -> product with M -> ``gather_jet``.  Matrix-free: chunks of ``chunk // C`` points, each
    ``wt_columns_jet`` -> ``post.solve_columns`` -> ``gather_jet``.  Those solves run at the operator's own tolerance
    (``settings.variance_cg_tolerance`` is for plain quadratic forms: the off-diagonal jet entries are first order in the residual)."""

    def __init__(self, post, x, sigma2, err, chunk=64):
        self.post, self.x, self.sigma2, self.err = post, x.detach().contiguous(), float(sigma2), err
        self.grid = post.grid
        self.C = self.grid.d + 1
        self.step = max(1, int(chunk) // self.C)
        self.cg_iters = []                              # per solve of the matrix-free path

    def _solve(self, xs):
        U, _ = self.post.solve_columns(grid_ops.wt_columns_jet(self.grid, xs, self.err))
        self.cg_iters.append(getattr(self.post, "last_iters", 0))
        return U

    def blocks(self):
        grid, x, C = self.grid, self.x, self.C
        if hasattr(self.post, "dense"):
            return grid_ops.jet_quadform(grid, x, self.post.dense, self.err) * self.sigma2
        n = x.shape[0]
        out = torch.empty((n, C, C), dtype=x.dtype, device=x.device)
        for s in range(0, n, self.step):
            xs = x[s:s + self.step]
            out[s:s + self.step] = grid_ops.gather_jet(grid, xs, self._solve(xs), self.err, rows_per_point=C)
        out = out * self.sigma2
        return 0.5 * (out + out.transpose(-1, -2))

    def joint(self):
        grid, x, C = self.grid, self.x, self.C
        n = x.shape[0]
        if hasattr(self.post, "dense"):
            U = grid_ops.gemm(grid_ops.wt_columns_jet(grid, x, self.err), self.post.dense.contiguous())     # rows (M J_c(x_p))^T, M symmetric
            full = grid_ops.gather_jet(grid, x, U, self.err).permute(0, 2, 1)                                 # [n, C, n C]
        else:
            full = torch.empty((n, C, n * C), dtype=x.dtype, device=x.device)
            for s in range(0, n, self.step):
                xs = x[s:s + self.step]
                full[:, :, s * C:(s + xs.shape[0]) * C] = grid_ops.gather_jet(grid, x, self._solve(xs), self.err).permute(0, 2, 1)
        full = full.reshape(n * C, n * C) * self.sigma2
        return 0.5 * (full + full.t())


def _batched_cholesky(A):
    """Lower Cholesky factors of [n, C, C] blocks with C <= 5, column by column over the whole batch (a library factorisation per
    point would be n launches for at most fifteen entries each).  A non-positive pivot is clamped to zero: that row is then zero."""
    C = A.shape[-1]
    L = torch.zeros_like(A)
    for j in range(C):
        d = (A[:, j, j] - (L[:, j, :j] ** 2).sum(-1)).clamp_min(0.0).sqrt()
        L[:, j, j] = d
        if j + 1 < C:
            r = (A[:, j + 1:, j] - (L[:, j + 1:, :j] * L[:, None, j, :j]).sum(-1))
            L[:, j + 1:, j] = torch.where(d[:, None] > 0, r / d[:, None].clamp_min(torch.finfo(A.dtype).tiny), torch.zeros_like(r))
    return L


class JetPosterior:
    """Gaussian posterior of the jet ``(f, d_1 f, .., d_d f)`` at n points.

    ``mean`` [n, C]; ``covariance`` [n, C, C] (per point) or, with ``joint``, [n C, n C] point-major (row ``p C + c``).  Channel 0 is
    the value, channel 1 + q the partial derivative in dim q.  Everything is detached from autograd."""

    def __init__(self, mean, covariance, joint):
        self.mean, self.covariance, self.joint = mean, covariance, bool(joint)
        self.n, self.C = mean.shape

    def _blocks(self):
        if not self.joint:
            return self.covariance
        n, C = self.n, self.C
        i = torch.arange(n, device=self.mean.device)
        return self.covariance.reshape(n, C, n, C)[i, :, i, :]

    @property
    def value_mean(self):
        return self.mean[:, 0]

    @property
    def value_variance(self):
        return self._blocks()[:, 0, 0]

    @property
    def grad_mean(self):
        return self.mean[:, 1:]

    @property
    def grad_covariance(self):
        return self._blocks()[:, 1:, 1:]

    def directional(self, V):
        """(mean [n], variance [n]) of the directional derivative ``V^T grad f`` for directions V [n, d] or [d]."""
        V = V.to(self.mean.dtype).to(self.mean.device)
        if V.dim() == 1:
            V = V[None].expand(self.n, -1)
        if V.shape != (self.n, self.C - 1):
            raise ValueError(f"expected directions of shape [{self.n}, {self.C - 1}] or [{self.C - 1}], got {tuple(V.shape)}")
        return (self.grad_mean * V).sum(-1), torch.einsum("pi,pij,pj->p", V, self.grad_covariance, V)

    def rsample(self, sample_shape=torch.Size(), base_samples=None):
        """Draws of the jet, [*sample_shape, n, C]: from the per-point blocks (points independent of each other), or from the joint
        covariance when the posterior was built with ``joint=True``.  ``base_samples``: standard normal draws of that shape.  A
        jitter of 1e-6 (fp32) / 1e-10 (fp64) times the mean diagonal entry is added before factorising: a channel whose variance is
        exactly zero (a partial derivative in a boundary cell) is otherwise a zero pivot."""
        shape = torch.Size(sample_shape) + (self.n, self.C)
        if base_samples is None:
            base_samples = torch.randn(shape, dtype=self.mean.dtype, device=self.mean.device)
        z = base_samples.to(self.mean.dtype).to(self.mean.device).reshape(-1, self.n, self.C)
        rel = 1e-6 if self.mean.dtype == torch.float32 else 1e-10
        if self.joint:
            A = self.covariance.clone()
            A.diagonal().add_(rel * A.diagonal().mean().clamp_min(0.0))
            L = grid_ops.psd_safe_cholesky(A.contiguous(), jitter=float(rel * A.diagonal().mean())).tril()
            draw = z.reshape(z.shape[0], -1) @ L.t()
        else:
            A = self.covariance.clone()
            A.diagonal(dim1=-2, dim2=-1).add_((rel * A.diagonal(dim1=-2, dim2=-1).mean(-1).clamp_min(0.0))[:, None])
            draw = torch.einsum("pij,spj->spi", _batched_cholesky(A), z)
        return self.mean + draw.reshape(shape)
