"""Cost of the jet posterior: median of 200 launches between HIP events.  Not part of any test.

  dense        30^2 (m = 900) and 10^3 grids, fp64, n = 1 024 points:
               (a) jet_quadform   (b) today's value-only variance, gather_rows + gather(diag=True)
  matrix-free  50^3 grid, fp32, 64 points (a handful of repeats: each is a batched PCG solve):
               (a) jet blocks, 256 columns in chunks of settings.variance_chunk   (b) the 64 value variances
Prints one JSON line per comparison."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_gp_amd import grid_ops, settings  # noqa: E402
from online_gp_amd.models import FixedNoiseOnlineSKIGP  # noqa: E402

DEV = "cuda"


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def dense(gs):
    d, dtype = len(gs), torch.float64
    grid = grid_ops.GridSpec(torch.tensor([[-1.0, 1.0]] * d, dtype=torch.float64), list(gs))
    rng = np.random.default_rng(0)
    x = torch.as_tensor(rng.uniform(-0.8, 0.8, (1024, d)), device=DEV, dtype=dtype)
    B = torch.as_tensor(rng.standard_normal((grid.m, grid.m)), device=DEV, dtype=dtype)
    M = (B @ B.t() / grid.m).contiguous()
    err = grid_ops.new_err_flag(DEV)
    a = timed(lambda: grid_ops.jet_quadform(grid, x, M, err), 200)
    b = timed(lambda: grid_ops.gather(grid, x, grid_ops.gather_rows(grid, x, M, err), err, diag=True), 200)
    print(json.dumps({"case": "dense", "grid": list(gs), "m": grid.m, "n": 1024, "dtype": "f64", "jet_quadform_us": round(a, 1),
                      "value_variance_us": round(b, 1), "ratio": round(a / b, 3)}))


def matrix_free():
    d, dtype, g = 3, torch.float32, 50
    rng = np.random.default_rng(0)
    X = torch.as_tensor(rng.uniform(-0.9, 0.9, (4096, d)), device=DEV, dtype=dtype)
    y = (torch.sin(2 * X[:, :1]) * torch.cos(X[:, 1:2]) + 0.5 * X[:, 2:]) + 0.05 * torch.randn(4096, 1, device=DEV, dtype=dtype)
    xs = torch.as_tensor(rng.uniform(-0.8, 0.8, (64, d)), device=DEV, dtype=dtype)
    with settings.spectral_factor(False):
        m = FixedNoiseOnlineSKIGP(X, y, torch.ones_like(y), grid_bounds=torch.tensor([[-1.0, 1.0]] * d), grid_size=[g] * d,
                                  learn_additional_noise=True).eval()
        m.prediction_cache
        iters = {}

        def jet():
            iters["jet"] = m.posterior_jet(xs).cg_iters

        def var():
            m(xs).variance
            iters["var"] = m.prediction_cache["pred_cov"].last_iters

        a, b = timed(jet, 5), timed(var, 5)
    print(json.dumps({"case": "matrix-free", "grid": [g] * d, "n": 64, "dtype": "f32", "jet_blocks_us": round(a, 1), "value_variance_us": round(b, 1),
                      "ratio": round(a / b, 2), "cg_iters_jet_chunks": iters["jet"], "cg_iters_value": iters["var"]}))


if __name__ == "__main__":
    dense((30, 30))
    dense((10, 10, 10))
    matrix_free()
