"""Cost of moment-matching the value and the partial derivatives of a batch inside its absorb: one grid, one batch of
q uniform points, three launches, each timed with HIP events around single launches (median over --reps, after --warm warm-up
launches, the three interleaved so that they share whatever else the machine is doing):

  grad_interval  wiski_absorb_grad_interval with the carry (u, res, mean_out) and its three outputs: every point carries an
                 exact value and a full gradient bounded on one side (from 4 s violated to 3 s satisfied, either side), placed
                 around the channels' own predictive means;
  grad           wiski_absorb at channels = d + 1, with the same carry: the same points with values and full gradients as targets;
  interval       wiski_absorb_interval with the same carry and its three outputs: the value channel alone, bounded on one side.

The targets are zeroed between launches outside the timed region (the sums otherwise grow without bound in fp32).  Prints one JSON
line with the three medians and the fastest runs in microseconds, grad_interval / grad and grad_interval / interval, and the share
of channels that were skipped."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_gp_amd import grid_ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--grid", type=int, default=50)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--q", type=int, default=4096)
    ap.add_argument("--sigma2", type=float, default=0.7)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    dt = torch.float32 if a.dtype == "f32" else torch.float64
    dev, d = "cuda", a.dim
    C = d + 1
    grid = grid_ops.GridSpec([[-1.1, 1.1]] * d, a.grid)
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *s: torch.rand(s, device=dev, dtype=dt, generator=gen)
    X = rand(a.q, d) * 2 - 1
    Y = torch.randn((a.q, C), device=dev, dtype=dt, generator=gen)
    noise = rand(a.q, C) + 0.5
    pvar = rand(a.q, C)
    u = 0.1 * torch.randn(grid.m, device=dev, dtype=dt, generator=gen)
    w = 1.0 / noise
    H = (grid.R + 1) // 2
    b, A, cnt, res = (torch.zeros(sh, device=dev, dtype=dt) for sh in (grid.m, (H, grid.m), grid.m, grid.m))
    mean = torch.zeros((a.q, C), device=dev, dtype=dt)
    mean1 = torch.zeros(a.q, device=dev, dtype=dt)
    stats, err = torch.zeros(2, device=dev, dtype=torch.float64), grid_ops.new_err_flag(dev)
    # the channels' own predictive means: what a launch with nothing to absorb reports in mean_out
    zero = torch.zeros_like(noise)
    grid_ops.scatter_stats_grad(grid, X, zero, zero, zero, torch.ones_like(noise), b, A, cnt, stats, err, u=u, res=res, mean_out=mean)
    mu = mean.clone()
    s = (pvar + a.sigma2 * noise).sqrt()
    side = (torch.arange(a.q * C, device=dev) % 2 == 0).reshape(a.q, C)
    t = rand(a.q, C) * 7 - 4
    inf = torch.full_like(mu, float("inf"))
    lo, hi = torch.where(side, mu - t * s, -inf), torch.where(side, inf, mu + t * s)
    lo1, hi1, pv1, w1, n1 = (v[:, 0].contiguous() for v in (lo, hi, pvar, w, noise))
    lo[:, 0] = hi[:, 0] = mu[:, 0] + s[:, 0] * (rand(a.q) * 4 - 2)      # the value channel of the full form: exact
    sites = [None]

    def grad_interval():
        sites[0] = grid_ops.scatter_stats_grad_interval(grid, X, lo, hi, pvar, a.sigma2, w, w, noise, b, A, cnt, stats, err, u, res=res, mean_out=mean)

    def grad():
        grid_ops.scatter_stats_grad(grid, X, Y, w, w, noise, b, A, cnt, stats, err, u=u, res=res, mean_out=mean)

    def interval():
        grid_ops.scatter_stats_interval(grid, X, lo1, hi1, pv1, a.sigma2, w1, w1, n1, b, A, cnt, stats, err, u, res=res, mean_out=mean1)

    forms = {"grad_interval": grad_interval, "grad": grad, "interval": interval}
    times = {k: [] for k in forms}
    for rep in range(a.warm + a.reps):
        for k, f in forms.items():
            for z in (b, A, cnt, res, stats):
                z.zero_()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            torch.cuda.synchronize()
            if rep >= a.warm:
                times[k].append(t0.elapsed_time(t1) * 1e3)
    assert int(err.item()) == 0
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"grid": [a.grid] * d, "dtype": a.dtype, "q": a.q, "reps": a.reps, "skipped": round(float((sites[0][1] == 0).double().mean()), 4),
                      "us_grad_interval": round(med["grad_interval"], 2), "us_grad": round(med["grad"], 2), "us_interval": round(med["interval"], 2),
                      "grad_interval_over_grad": round(med["grad_interval"] / med["grad"], 3),
                      "grad_interval_over_interval": round(med["grad_interval"] / med["interval"], 3),
                      "us_min": {k: round(min(v), 2) for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
