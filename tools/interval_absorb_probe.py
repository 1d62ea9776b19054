"""Cost of moment-matching a batch inside its absorb: one grid, one batch of q uniform points, three launches, each
timed with HIP events around single launches (median over --reps, after --warm warm-up launches, the three interleaved so that they
share whatever else the machine is doing):

  interval  wiski_absorb_interval with the carry (u, res, mean_out) and its three outputs; a third of the points each are
            one-sided bounds, two-sided intervals and exact values, placed around the points' own predictive means;
  robust    wiski_absorb_robust with the same carry and omega_out;
  plain     the value-only absorb with the same carry (wiski_scatter_stats_step without zero regions, guard or owner workspace:
            k_scatter_stats_sym with u, res and mean_out).

The targets are zeroed between launches outside the timed region (the sums otherwise grow without bound in fp32).  Prints one JSON
line with the three medians and the fastest runs in microseconds, interval / robust and interval / plain, and the share of points
per kind and of skipped ones."""
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
    pvar = rand(a.q)
    u = 0.1 * torch.randn(grid.m, device=dev, dtype=dt, generator=gen)
    w, inv_scale = 1.0 / noise, noise.rsqrt()
    # bounds around the points' own predictive means, in units of s = sqrt(pvar + sigma2 noise): kind 0 one-sided (either side, from
    # 4 s violated to 3 s satisfied), kind 1 two-sided (width 0.1 s .. 3 s, within 4 s), kind 2 an exact value within 2 s
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
    mean = torch.zeros(a.q, device=dev, dtype=dt)
    stats, err = torch.zeros(2, device=dev, dtype=torch.float64), grid_ops.new_err_flag(dev)
    sites = [None]
    p, stream = _hip.dptr, _hip.stream_ptr(torch.device(dev, torch.cuda.current_device()))
    step = _hip.fn("wiski_scatter_stats_step", dt)

    def interval():
        sites[0] = grid_ops.scatter_stats_interval(grid, X, lo, hi, pvar, a.sigma2, w, w, noise, b, A, cnt, stats, err, u, res=res, mean_out=mean)

    def robust():
        grid_ops.scatter_stats_robust(grid, X, y, w, w, noise, inv_scale, a.c, b, A, cnt, stats, err, u, res=res, mean_out=mean)

    def plain():
        rc = step(grid.ref, p(X), p(y), p(w), p(w), p(noise), ctypes.c_int64(a.q), p(b), p(A), p(cnt), p(u), p(res), p(mean), p(stats), p(err),
                  None, ctypes.c_int64(0), None, ctypes.c_int64(0), None, ctypes.c_int64(0), None, ctypes.c_int64(0), stream)
        _hip.check(rc, "wiski_scatter_stats_step")

    forms = {"interval": interval, "robust": robust, "plain": plain}
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
    print(json.dumps({"grid": [a.grid] * d, "dtype": a.dtype, "q": a.q, "reps": a.reps,
                      "kinds": {"one_sided": round(float((kind == 0).double().mean()), 3), "two_sided": round(float((kind == 1).double().mean()), 3),
                                "exact": round(float((kind == 2).double().mean()), 3)},
                      "skipped": round(float((sites[0][1] == 0).double().mean()), 4), "us_interval": round(med["interval"], 2),
                      "us_robust": round(med["robust"], 2), "us_plain": round(med["plain"], 2),
                      "interval_over_robust": round(med["interval"] / med["robust"], 3), "interval_over_plain": round(med["interval"] / med["plain"], 3),
                      "us_min": {k: round(min(v), 2) for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
