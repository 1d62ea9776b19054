"""Cost of one revisit launch beside the interval absorb of the same points: one grid, q uniform points given as
bounds, two launches, each timed with HIP events around single launches (median over --reps, after --warm warm-up launches, the two
interleaved so that they share whatever else the machine is doing):

  interval  wiski_absorb_interval with the carry (u, res) and its three outputs: two thirds of the points are one-sided bounds
            and two-sided intervals placed around the points' own predictive means, a third exact values;
  revisit   wiski_absorb_revisit over a ring of q slots that holds those points with the sites the interval launch gave them, against
            the same u and a variance that leaves every cavity well above the threshold: every slot that is no exact value is
            re-matched and makes its delta sweep (the first sweep of a refine: every site moves).

The targets are zeroed and the ring's sites restored between launches outside the timed region.  Prints one JSON line with the two
medians and the fastest runs in microseconds, revisit / interval, and the share of slots left alone and of slots that moved."""
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
    ap.add_argument("--damping", type=float, default=1.0)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    dt = torch.float32 if a.dtype == "f32" else torch.float64
    dev, d = "cuda", a.dim
    grid = grid_ops.GridSpec([[-1.1, 1.1]] * d, a.grid)
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *s: torch.rand(s, device=dev, dtype=dt, generator=gen)
    X = rand(a.q, d) * 2 - 1
    noise = rand(a.q) + 0.5
    pvar = rand(a.q) + 0.1
    u = 0.1 * torch.randn(grid.m, device=dev, dtype=dt, generator=gen)
    w = 1.0 / noise
    mu = grid_ops.gather(grid, X, u[None], grid_ops.new_err_flag(dev))[:, 0]
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
    stats, err = torch.zeros(2, device=dev, dtype=torch.float64), grid_ops.new_err_flag(dev)
    yt0, om0, _ = grid_ops.scatter_stats_interval(grid, X, lo, hi, pvar, a.sigma2, w, w, noise, b, A, cnt, stats, err, u, res=res)
    ring = grid_ops.SiteRing(a.q, d, dt, dev)
    ring.store("interval", X, lo, hi, noise, w, w, yt0, om0)
    # the variance of a posterior that has taken the sites in: 1 / v = 1 / pvar + tau, so that the cavity is the prior the sites were
    # matched against -- scaled by 0.9, which moves every site
    pv_now = 0.9 / (1.0 / pvar + om0 / (a.sigma2 * noise))
    log_z = torch.empty(a.q, device=dev, dtype=torch.float64)
    change = torch.empty(a.q, device=dev, dtype=dt)

    def interval():
        grid_ops.scatter_stats_interval(grid, X, lo, hi, pvar, a.sigma2, w, w, noise, b, A, cnt, stats, err, u, res=res)

    def revisit():
        grid_ops.revisit_sites(grid, ring, "interval", pv_now, a.sigma2, a.damping, b, A, cnt, stats, err, u, res=res, log_z=log_z, change=change)

    forms = {"interval": interval, "revisit": revisit}
    times = {k: [] for k in forms}
    for rep in range(a.warm + a.reps):
        for k, f in forms.items():
            for z in (b, A, cnt, res, stats):
                z.zero_()
            ring.ytilde.copy_(yt0)
            ring.omega.copy_(om0)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            torch.cuda.synchronize()
            if rep >= a.warm:
                times[k].append(t0.elapsed_time(t1) * 1e3)
    assert int(err.item()) == 0
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"grid": [a.grid] * d, "dtype": a.dtype, "q": a.q, "reps": a.reps, "damping": a.damping,
                      "left_alone": round(float(torch.isnan(log_z).double().mean()), 4), "moved": round(float((change > 0).double().mean()), 4),
                      "us_interval": round(med["interval"], 2), "us_revisit": round(med["revisit"], 2),
                      "revisit_over_interval": round(med["revisit"] / med["interval"], 3), "us_min": {k: round(min(v), 2) for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
