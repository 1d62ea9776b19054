from .operators import (InducingPosterior, InterpolatedKernel, KroneckerToeplitz, PredictiveCovariance, StencilWtW)
from .dense_woodbury import DenseInducingPosterior
from .jet import JetCovariance, JetPosterior
from .quadrature import BoxCovariance, IntegralPosterior
from .updated_root_lazy_tensor import UpdatedRootLazyTensor

__all__ = ["StencilWtW", "KroneckerToeplitz", "InducingPosterior", "InterpolatedKernel", "PredictiveCovariance", "DenseInducingPosterior",
           "UpdatedRootLazyTensor", "JetCovariance", "JetPosterior", "BoxCovariance", "IntegralPosterior"]
