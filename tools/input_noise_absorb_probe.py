"""Cost of inflating a batch's noise by the local slope inside its absorb: one grid, one batch of q uniform points,
three launches, each timed with HIP events around single launches (median over --reps, after --warm warm-up launches, the three
interleaved so that they share whatever else the machine is doing):

  input_noise  wiski_absorb_input_noise with the carry (u, res, mean_out), gvar and its three outputs (omega, log Z, the
               slopes); the input variances are drawn so that s_in / dn is log-uniform in [1e-2, 1e2];
  robust       wiski_absorb_robust with the same carry and omega_out;
  interval     wiski_absorb_interval with the same carry and its three outputs, two-sided intervals of width 0.1 s .. 3 s
               around the points' own predictive means.

The targets are zeroed between launches outside the timed region (the sums otherwise grow without bound in fp32).  Prints one JSON
line with the three medians and the fastest runs in microseconds, input_noise / robust and input_noise / interval, and the share of
skipped points."""
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
    ap.add_argument("--c", type=float, default=2.0)
    ap.add_argument("--sigma2", type=float, default=0.7)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    dt = torch.float32 if a.dtype == "f32" else torch.float64
    dev, d = "cuda", a.dim
    grid = grid_ops.GridSpec([[-1.1, 1.1]] * d, a.grid)
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *s: torch.rand(s, device=dev, dtype=dt, generator=gen)
    X = rand(a.q, d) * 2 - 1
    y = torch.randn(a.q, device=dev, dtype=dt, generator=gen)
    noise = rand(a.q) + 0.5
    pvar, gvar = rand(a.q), rand(a.q, d)
    u = 0.1 * torch.randn(grid.m, device=dev, dtype=dt, generator=gen)
    w, inv_scale = 1.0 / noise, noise.rsqrt()
    mu = grid_ops.gather(grid, X, u[None], grid_ops.new_err_flag(dev))[:, 0]
    s = (pvar + a.sigma2 * noise).sqrt()
    a0 = rand(a.q) * 5 - 4
    lo, hi = mu + s * a0, mu + s * (a0 + 0.1 + 2.9 * rand(a.q))
    ratio = 10.0 ** (rand(a.q) * 4 - 2)                             # s_in / dn up to the squared mean slope, which only adds
    xvar = ((ratio * a.sigma2 * noise / d)[:, None] / gvar.clamp_min(1e-3)).contiguous()
    H = (grid.R + 1) // 2
    b, A, cnt, res = (torch.zeros(sh, device=dev, dtype=dt) for sh in (grid.m, (H, grid.m), grid.m, grid.m))
    mean = torch.zeros(a.q, device=dev, dtype=dt)
    stats, err = torch.zeros(2, device=dev, dtype=torch.float64), grid_ops.new_err_flag(dev)
    sites = [None]

    def input_noise():
        sites[0] = grid_ops.scatter_stats_input_noise(grid, X, y, xvar, gvar, pvar, a.sigma2, w, w, noise, b, A, cnt, stats, err, u, res=res, mean_out=mean,
                                                      want_grad=True)

    def robust():
        grid_ops.scatter_stats_robust(grid, X, y, w, w, noise, inv_scale, a.c, b, A, cnt, stats, err, u, res=res, mean_out=mean)

    def interval():
        grid_ops.scatter_stats_interval(grid, X, lo, hi, pvar, a.sigma2, w, w, noise, b, A, cnt, stats, err, u, res=res, mean_out=mean)

    forms = {"input_noise": input_noise, "robust": robust, "interval": interval}
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
    om = sites[0][0]
    print(json.dumps({"grid": [a.grid] * d, "dtype": a.dtype, "q": a.q, "reps": a.reps, "skipped": round(float((om == 0).double().mean()), 4),
                      "omega_median": round(float(om.median()), 4), "us_input_noise": round(med["input_noise"], 2), "us_robust": round(med["robust"], 2),
                      "us_interval": round(med["interval"], 2), "input_noise_over_robust": round(med["input_noise"] / med["robust"], 3),
                      "input_noise_over_interval": round(med["input_noise"] / med["interval"], 3),
                      "us_min": {k: round(min(v), 2) for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
