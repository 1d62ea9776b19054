"""Predictive covariance of a model with a polynomial trend.

With the trend's coefficients marginalised, the covariance of a query batch is

    sigma2 (W* M W*^T + R* Lambda^-1 R*^T),   R* = H* - W* S,   S = M C,   Lambda = G - C^T S + (sigma2 / tau2) I:

the model's own predictive covariance plus a term of rank p <= 15 -- the uncertainty of the coefficients, carried to the queries
through the basis rows as the GP has not already explained them.
"""
import torch

from ..distributions import DenseLazyTensor, LazyCovariance


class TrendCovariance(LazyCovariance):
    """base + sigma2 R* Lambda^-1 R*^T: `base` the PredictiveCovariance of the same points, `rows` R* [n, p] (from
    ``wiski_trend_rows``), `chol` the lower Cholesky factor of Lambda (fp64).  The low-rank term is formed in fp64 and rounded once."""

    def __init__(self, base, rows, chol, sigma2):
        self.base = base
        self.rows = rows
        self.chol = chol
        self.sigma2 = float(sigma2)
        self.shape = base.shape
        self.dtype = base.dtype
        self.device = base.device
        self._half = None

    def _root(self):
        """sigma L^-1 R*^T [p, n] in fp64: the low-rank term is its Gram matrix."""
        if self._half is None:
            self._half = torch.linalg.solve_triangular(self.chol, self.rows.double().t(), upper=False) * self.sigma2 ** 0.5
        return self._half

    def diag(self):
        Y = self._root()
        return self.base.diag() + (Y * Y).sum(0).to(self.dtype)

    def evaluate(self):
        Y = self._root()
        return self.base.evaluate() + (Y.t() @ Y).to(self.dtype)

    def matmul(self, rhs):
        vec = rhs.dim() == 1
        V = rhs[:, None] if vec else rhs
        Y = self._root()
        out = self.base.evaluate() @ V + (Y.t() @ (Y @ V.double())).to(V.dtype)
        return out[:, 0] if vec else out

    __matmul__ = matmul

    def root_decomposition(self):
        return None                                   # (callers factorise evaluate(), as on the PCG path)

    def __getitem__(self, item):
        return DenseLazyTensor(self.evaluate()[item])
