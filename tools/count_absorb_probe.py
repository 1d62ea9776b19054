"""Cost of the quadrature site inside the absorb: one grid, one batch of q uniform points, the count absorb of either
family against the interval absorb (unchanged code, same build), each timed with HIP events around single launches (median over
--reps, after --warm warm-up launches, the forms interleaved so that they share whatever else the machine is doing):

  poisson   wiski_absorb_count, family Poisson: counts drawn at the points' own predictive means, exposures exp(U(-1, 2));
  binomial  wiski_absorb_count, family binomial: successes out of 1..40 trials drawn likewise;
  interval  wiski_absorb_interval with the same carry (u, res, mean_out) and outputs: a third of the points each one-sided,
            two-sided and exact;
  sites     wiski_count_sites alone on the same q sites (Poisson): the quadrature without a scatter.

The targets are zeroed between launches outside the timed region.  Prints one JSON line with the medians and the fastest runs in
microseconds and count / interval per family."""
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
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    dt = torch.float32 if a.dtype == "f32" else torch.float64
    dev, d = "cuda", a.dim
    grid = grid_ops.GridSpec([[-1.1, 1.1]] * d, a.grid)
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *s: torch.rand(s, device=dev, dtype=dt, generator=gen)
    X = rand(a.q, d) * 2 - 1
    noise = rand(a.q) + 0.5
    pvar = rand(a.q)
    u = torch.randn(grid.m, device=dev, dtype=dt, generator=gen)
    w = 1.0 / noise
    mu = grid_ops.gather(grid, X, u[None], grid_ops.new_err_flag(dev))[:, 0]
    f = mu + pvar.sqrt() * torch.randn(a.q, device=dev, dtype=dt, generator=gen)
    expo = torch.exp(rand(a.q) * 3 - 1)
    y_p = torch.poisson(expo * torch.exp(f), generator=gen)
    trials = torch.floor(rand(a.q) * 40) + 1
    y_b = torch.binomial(trials, torch.sigmoid(f), generator=gen)
    s = (pvar + a.sigma2 * noise).sqrt()
    kind = torch.arange(a.q, device=dev) % 3
    side = torch.arange(a.q, device=dev) % 2 == 0
    t = rand(a.q) * 7 - 4
    a0 = rand(a.q) * 5 - 4
    width = 0.1 + 2.9 * rand(a.q)
    exact = mu + s * (rand(a.q) * 4 - 2)
    inf = torch.full_like(mu, float("inf"))
    lo = torch.where(kind == 0, torch.where(side, mu - t * s, -inf), torch.where(kind == 1, mu + s * a0, exact))
    hi = torch.where(kind == 0, torch.where(side, inf, mu + t * s), torch.where(kind == 1, mu + s * (a0 + width), exact))
    H = (grid.R + 1) // 2
    b, A, cnt, res = (torch.zeros(sh, device=dev, dtype=dt) for sh in (grid.m, (H, grid.m), grid.m, grid.m))
    mean = torch.zeros(a.q, device=dev, dtype=dt)
    stats, err = torch.zeros(2, device=dev, dtype=torch.float64), grid_ops.new_err_flag(dev)
    out = {}

    def count(family, y, tt):
        def run():
            out[family] = grid_ops.scatter_stats_count(grid, X, y, tt, family, pvar, a.sigma2, w, w, noise, b, A, cnt, stats, err, u, res=res, mean_out=mean)
        return run

    def interval():
        out["interval"] = grid_ops.scatter_stats_interval(grid, X, lo, hi, pvar, a.sigma2, w, w, noise, b, A, cnt, stats, err, u, res=res, mean_out=mean)

    def sites():
        grid_ops.count_sites(mu, pvar, y_p, expo, "poisson")

    forms = {"poisson": count("poisson", y_p, expo), "binomial": count("binomial", y_b, trials), "interval": interval, "sites": sites}
    times = {k: [] for k in forms}
    for rep in range(a.warm + a.reps):
        for k, fn in forms.items():
            for z in (b, A, cnt, res, stats):
                z.zero_()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if rep >= a.warm:
                times[k].append(t0.elapsed_time(t1) * 1e3)
    assert int(err.item()) == 0
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"grid": [a.grid] * d, "dtype": a.dtype, "q": a.q, "reps": a.reps,
                      "skipped": {k: round(float((out[k][1] == 0).double().mean()), 4) for k in ("poisson", "binomial", "interval")},
                      "us": {k: round(v, 2) for k, v in med.items()}, "us_min": {k: round(min(v), 2) for k, v in times.items()},
                      "poisson_over_interval": round(med["poisson"] / med["interval"], 3),
                      "binomial_over_interval": round(med["binomial"] / med["interval"], 3)}), flush=True)


if __name__ == "__main__":
    main()
