"""Cost of absorbing gradients with the values: one grid, one batch of q uniform points, three ways of absorbing it,
each timed with HIP events around single launches (median over --reps, after --warm warm-up launches, the three interleaved so that
they share whatever else the machine is doing):

  fused     wiski_absorb at channels = d + 1, all of them present;
  separate  d + 1 calls of the same entry, each with one channel present (what channel-by-channel absorbing would cost);
  value     today's value-only absorb (wiski_scatter_stats_cnt on the half stencil).

The targets are zeroed between launches outside the timed region (the sums otherwise grow without bound in fp32), and every launch
writes b, A_half, cnt and the two scalars; no carry.  Prints one JSON line with the three medians in microseconds and fused / separate."""
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
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    dt = torch.float32 if a.dtype == "f32" else torch.float64
    dev, d = "cuda", a.dim
    C = d + 1
    grid = grid_ops.GridSpec([[-1.1, 1.1]] * d, a.grid)
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand((a.q, d), device=dev, dtype=dt, generator=gen) * 2 - 1
    Y = torch.randn((a.q, C), device=dev, dtype=dt, generator=gen)
    noise = torch.rand((a.q, C), device=dev, dtype=dt, generator=gen) + 0.5
    w = 1.0 / noise
    one = []                                                   # channel c alone: the others absent (wa = wb = 0, noise = 1)
    for c in range(C):
        sel = torch.zeros((1, C), dtype=torch.bool, device=dev)
        sel[0, c] = True
        one.append((torch.where(sel, Y, torch.zeros_like(Y)), torch.where(sel, w, torch.zeros_like(w)), torch.where(sel, noise, torch.ones_like(noise))))
    y0, w0, n0 = Y[:, 0].contiguous(), w[:, 0].contiguous(), noise[:, 0].contiguous()
    H = (grid.R + 1) // 2
    b, A, cnt = (torch.zeros(s, device=dev, dtype=dt) for s in (grid.m, (H, grid.m), grid.m))
    stats, err = torch.zeros(2, device=dev, dtype=torch.float64), grid_ops.new_err_flag(dev)

    def fused():
        grid_ops.scatter_stats_grad(grid, X, Y, w, w, noise, b, A, cnt, stats, err)

    def separate():
        for Yc, wc, nc in one:
            grid_ops.scatter_stats_grad(grid, X, Yc, wc, wc, nc, b, A, cnt, stats, err)

    def value():
        grid_ops.scatter_stats_cnt(grid, X, y0, w0, w0, n0, b, A, True, cnt, stats, err)

    forms = {"fused": fused, "separate": separate, "value": value}
    times = {k: [] for k in forms}
    for rep in range(a.warm + a.reps):
        for k, f in forms.items():
            for t in (b, A, cnt, stats):
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
    print(json.dumps({"grid": [a.grid] * d, "dtype": a.dtype, "q": a.q, "reps": a.reps, "us_fused": round(med["fused"], 2),
                      "us_separate": round(med["separate"], 2), "us_value": round(med["value"], 2),
                      "fused_over_separate": round(med["fused"] / med["separate"], 3), "fused_over_value": round(med["fused"] / med["value"], 3),
                      "us_min": {k: round(min(v), 2) for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
