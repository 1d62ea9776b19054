"""Cost of weighting a batch inside its absorb: one grid, one batch of q uniform points, two launches, each timed
with HIP events around single launches (median over --reps, after --warm warm-up launches, the two interleaved so that they share
whatever else the machine is doing):

  robust  wiski_absorb_robust with the carry (u, res, mean_out) and omega_out;
  plain   the value-only absorb with the same carry (wiski_scatter_stats_step without zero regions, guard or owner workspace:
          k_scatter_stats_sym with u, res and mean_out).

The targets are zeroed between launches outside the timed region (the sums otherwise grow without bound in fp32).  Prints one JSON
line with the two medians and the fastest runs in microseconds, robust / plain, and the share of down-weighted points."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_gp_amd import _hip, grid_ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--grid", type=int, default=50)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--q", type=int, default=4096)
    ap.add_argument("--c", type=float, default=2.0)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    dt = torch.float32 if a.dtype == "f32" else torch.float64
    dev, d = "cuda", a.dim
    grid = grid_ops.GridSpec([[-1.1, 1.1]] * d, a.grid)
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand((a.q, d), device=dev, dtype=dt, generator=gen) * 2 - 1
    y = torch.randn(a.q, device=dev, dtype=dt, generator=gen)
    noise = torch.rand(a.q, device=dev, dtype=dt, generator=gen) + 0.5
    u = 0.1 * torch.randn(grid.m, device=dev, dtype=dt, generator=gen)
    w, inv_scale = 1.0 / noise, noise.rsqrt()
    H = (grid.R + 1) // 2
    b, A, cnt, res = (torch.zeros(s, device=dev, dtype=dt) for s in (grid.m, (H, grid.m), grid.m, grid.m))
    mean = torch.zeros(a.q, device=dev, dtype=dt)
    stats, err = torch.zeros(2, device=dev, dtype=torch.float64), grid_ops.new_err_flag(dev)
    omega = [None]
    p, stream = _hip.dptr, _hip.stream_ptr(torch.device(dev, torch.cuda.current_device()))
    step = _hip.fn("wiski_scatter_stats_step", dt)

    def robust():
        omega[0] = grid_ops.scatter_stats_robust(grid, X, y, w, w, noise, inv_scale, a.c, b, A, cnt, stats, err, u, res=res, mean_out=mean)

    def plain():
        rc = step(grid.ref, p(X), p(y), p(w), p(w), p(noise), ctypes.c_int64(a.q), p(b), p(A), p(cnt), p(u), p(res), p(mean), p(stats), p(err),
                  None, ctypes.c_int64(0), None, ctypes.c_int64(0), None, ctypes.c_int64(0), None, ctypes.c_int64(0), stream)
        _hip.check(rc, "wiski_scatter_stats_step")

    forms = {"robust": robust, "plain": plain}
    times = {k: [] for k in forms}
    for rep in range(a.warm + a.reps):
        for k, f in forms.items():
            for t in (b, A, cnt, res, stats):
                t.zero_()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            torch.cuda.synchronize()
            if rep >= a.warm:
                times[k].append(t0.elapsed_time(t1) * 1e3)
    assert int(err.item()) == 0
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"grid": [a.grid] * d, "dtype": a.dtype, "q": a.q, "reps": a.reps, "c": a.c,
                      "down_weighted": round(float((omega[0] < 1).double().mean()), 4), "us_robust": round(med["robust"], 2),
                      "us_plain": round(med["plain"], 2), "robust_over_plain": round(med["robust"] / med["plain"], 3),
                      "us_min": {k: round(min(v), 2) for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
