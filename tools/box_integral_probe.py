"""Cost of the box-integral posterior: HIP events around calls, median of 200.  Not part of any test.

50^3 grid (m = 125 000), fp32, B = 64 boxes, once cell-sized (inside one cell: 4^3 = 64 nodes of support) and once domain-sized
(the whole grid: 125 000 nodes):
  (a) gather_box per mode -- shared rows k = 1 (the mean) and k = 64 (the joint cross-covariance), one row per box (the variance) --
      with the default split of a box's support across blocks and with nsplit = 1;
  (b) the same contraction through a materialised wt_columns_box [64, m]: torch mv (k = 1), grid_ops.gemm (k = 64), an
      elementwise product and row sum (one row per box); the writer's own time is reported next to it;
  (c) posterior_integral end to end (variances, and joint) against what a user does without it: posterior() on a cloud of
      n = 64 points per box (a 4 x 4 x 4 midpoint rule) with its n x n covariance averaged, box by box (3 repeats: every box is
      a batched PCG solve of 64 columns).
Prints one JSON line per measurement."""
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
G, D, B = 50, 3, 64


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


def boxes(grid, kind, rng, dtype):
    if kind == "cell":
        j = rng.integers(2, G - 3, (B, D))
        lo = np.array([[grid.g0[q] + grid.h[q] * (j[b, q] + 0.1) for q in range(D)] for b in range(B)])
        hi = lo + 0.8 * np.array(grid.h)[None, :]
    else:                                   # node 1 .. node g - 2, shrunk a little per box so that the 64 boxes differ
        s = rng.uniform(0.0, 0.4, (B, D))
        lo = np.array([[grid.g0[q] + grid.h[q] * (1.0 + s[b, q]) for q in range(D)] for b in range(B)])
        hi = np.array([[grid.g0[q] + grid.h[q] * (G - 2.0 - s[b, q]) for q in range(D)] for b in range(B)])
    return torch.as_tensor(lo, device=DEV, dtype=dtype), torch.as_tensor(hi, device=DEV, dtype=dtype)


def kernels(kind):
    dtype = torch.float32
    grid = grid_ops.GridSpec(torch.tensor([[-1.0, 1.0]] * D, dtype=torch.float64), [G] * D)
    rng = np.random.default_rng(0)
    lo, hi = boxes(grid, kind, rng, dtype)
    err = grid_ops.new_err_flag(DEV)
    t = grid_ops.box_tables(grid, lo, hi, err)
    V1 = torch.randn(1, grid.m, device=DEV, dtype=dtype)
    VB = torch.randn(B, grid.m, device=DEV, dtype=dtype)
    out = {"case": "kernels", "boxes": kind, "grid": [G] * D, "B": B, "dtype": "f32",
           "box_tables_us": round(timed(lambda: grid_ops.box_tables(grid, lo, hi, err), 200), 1),
           "wt_columns_box_us": round(timed(lambda: grid_ops.wt_columns_box(grid, t), 200), 1)}
    cols = grid_ops.wt_columns_box(grid, t)
    for name, V, R, via in (("shared_k1", V1, 0, lambda: torch.mv(cols, V1[0])), ("shared_k64", VB, 0, lambda: grid_ops.gemm(cols, VB, tb=True)),
                            ("perbox_R1", VB, 1, lambda: (cols * VB).sum(1))):
        k = 1 if R else V.shape[0]
        ns = grid_ops.box_gather_nsplit(grid, B * k)
        out[name] = {"nsplit": ns, "gather_box_us": round(timed(lambda: grid_ops.gather_box(grid, t, V, rows_per_box=R), 200), 1),
                     "gather_box_nsplit1_us": round(timed(lambda: grid_ops.gather_box(grid, t, V, rows_per_box=R, nsplit=1), 200), 1),
                     "materialised_contraction_us": round(timed(via, 200), 1)}
        a, b = grid_ops.gather_box(grid, t, V, rows_per_box=R), via().reshape(B, -1)
        out[name]["max_abs_difference"] = float((a - b).abs().max())
    print(json.dumps(out), flush=True)


def end_to_end(kind):
    dtype = torch.float32
    rng = np.random.default_rng(0)
    X = torch.as_tensor(rng.uniform(-0.9, 0.9, (4096, D)), device=DEV, dtype=dtype)
    y = (torch.sin(2 * X[:, :1]) * torch.cos(X[:, 1:2]) + 0.5 * X[:, 2:]) + 0.05 * torch.randn(4096, 1, device=DEV, dtype=dtype)
    with settings.spectral_factor(False):
        m = FixedNoiseOnlineSKIGP(X, y, torch.ones_like(y), grid_bounds=torch.tensor([[-1.0, 1.0]] * D), grid_size=[G] * D,
                                  learn_additional_noise=True).eval()
        m.prediction_cache
        lo, hi = boxes(m._grid, kind, rng, dtype)
        res = {}

        def integral():
            res["ip"] = m.posterior_integral(lo, hi, average=True)

        def joint():
            res["ij"] = m.posterior_integral(lo, hi, joint=True, average=True)

        u = (torch.arange(4, device=DEV, dtype=dtype) + 0.5) / 4
        cube = torch.stack(torch.meshgrid(u, u, u, indexing="ij"), -1).reshape(-1, D)

        def cloud():
            means, vars_ = [], []
            for b in range(B):
                mvn = m(lo[b] + cube * (hi[b] - lo[b]))
                means.append(mvn.mean.mean())
                vars_.append(mvn.covariance_matrix.mean())
            res["cloud"] = (torch.stack(means), torch.stack(vars_))

        a, j, c = timed(integral, 5), timed(joint, 5), timed(cloud, 3)
    ip, (cm, cv) = res["ip"], res["cloud"]
    print(json.dumps({"case": "end to end", "boxes": kind, "grid": [G] * D, "B": B, "dtype": "f32", "cloud_points_per_box": 64,
                      "posterior_integral_us": round(a, 1), "posterior_integral_joint_us": round(j, 1), "cloud_us": round(c, 1),
                      "cloud_over_integral": round(c / a, 1), "cg_iters_integral": ip.cg_iters, "cg_iters_joint": res["ij"].cg_iters,
                      "mean_cloud_minus_exact_max": float((cm - ip.mean).abs().max()), "mean_scale": float(ip.mean.abs().max()),
                      "variance_cloud_over_exact_range": [float((cv / ip.variance).min()), float((cv / ip.variance).max())]}), flush=True)


if __name__ == "__main__":
    for kind in ("cell", "domain"):
        kernels(kind)
    for kind in ("cell", "domain"):
        end_to_end(kind)
