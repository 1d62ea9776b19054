"""Host: the look-ahead acquisitions' interface without a GPU -- the C ABI declares the bilinear-form kernels, the acquisition
names and their arguments are checked before anything runs, and the loops' new options are validated."""
import inspect
import os

import pytest
import torch

from online_gp_amd import harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_bilinear_kernels():
    with open(os.path.join(ROOT, "include", "wiski.h")) as fh:
        h = fh.read()
    for name in ("wiski_interp_bilinear_f32", "wiski_interp_bilinear_f64", "wiski_interp_bilinear_vjp_f32", "wiski_interp_bilinear_vjp_f64"):
        assert f"int {name}(" in h
    from online_gp_amd import _hip

    assert "lookahead.hip" in _hip._SOURCES


def test_grid_ops_exposes_interp_bilinear():
    from online_gp_amd import grid_ops

    assert callable(grid_ops.interp_bilinear) and issubclass(grid_ops.InterpBilinear, torch.autograd.Function)
    assert list(inspect.signature(grid_ops.interp_bilinear).parameters)[:4] == ["grid", "A", "xL", "xR"]


class _Stub:
    _dtype = torch.float64
    _device = torch.device("cpu")

    def posterior(self, X):
        raise AssertionError("the arguments are checked before the model is asked")


BOUNDS = torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.float64)


def test_lookahead_names_and_missing_arguments_are_errors():
    X = torch.rand(2, 3, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="qnipv needs mc_points"):
        harness.acqf_values(_Stub(), X, "qnipv")
    with pytest.raises(ValueError, match="qnipv needs mc_points"):
        harness.optimize_acqf(_Stub(), "qnipv", BOUNDS, q=2, raw_samples=4, num_restarts=1, maxiter=2)
    with pytest.raises(ValueError, match="kg needs current_value"):
        harness.optimize_acqf(_Stub(), "kg", BOUNDS, q=1, raw_samples=4, num_restarts=1, maxiter=2)
    with pytest.raises(ValueError, match="kg needs base_samples"):
        harness.acqf_values(_Stub(), X, "kg", best_f=0.0)
    with pytest.raises(ValueError, match="online SKI model"):
        harness.acqf_values(_Stub(), X, "kg", base_samples=torch.randn(1, 2, dtype=torch.float64), best_f=0.0)
    with pytest.raises(ValueError, match="unknown acquisition"):
        harness.acqf_values(_Stub(), X, "qnei")


def test_loop_options():
    assert inspect.signature(harness.qnipv_active_learning).parameters["selector"].default == "random"
    assert inspect.signature(harness.bayesopt).parameters["acqf"].default == "ucb"
    assert inspect.signature(harness.bayesopt).parameters["num_fantasies"].default == 256
    assert inspect.signature(harness.optimize_acqf).parameters["num_fantasies"].default == 64
    with pytest.raises(ValueError, match="selector"):
        harness.qnipv_active_learning(_Stub(), torch.rand(4, 2), None, torch.rand(4, 2), num_steps=1, selector="best")
