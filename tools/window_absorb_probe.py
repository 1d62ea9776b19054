"""Cost of retiring points inside the absorb: one grid, a FULL ring, batches of q uniform points, four forms, each
timed with HIP events around its launches (median over --reps, after --warm warm-up rounds, the forms interleaved so that they share
whatever else the machine is doing):

  window    wiski_absorb_window with the carry (u, res): q points enter, q leave, one launch;
  plain_q   the plain absorb (wiski_scatter_stats_cnt, half stencil, with the carry) of q points;
  plain_2q  the same of 2 q points: the atomics of `window` without the ring traffic;
  two_step  what a caller without the fused form would do: gather the q leaving points from the ring (five index_select launches and
            two negations), the plain absorb of the q entering points, the plain absorb of the leaving ones at negated weights, and
            five index_copy launches that store the entering points.

The targets of the plain forms are zeroed between launches outside the timed region (the sums otherwise grow without bound in fp32);
the window's stay what they are, the statistics of the ring.  Prints one JSON line per q with the medians and the fastest runs in
microseconds."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_gp_amd import grid_ops  # noqa: E402


def run(a, q, dt, dev):
    d = a.dim
    grid = grid_ops.GridSpec([[-1.1, 1.1]] * d, a.grid)
    gen = torch.Generator(device=dev).manual_seed(0)
    cap = a.turns * q
    rnd = lambda *s: torch.rand(s, device=dev, dtype=dt, generator=gen)
    pool = [dict(X=rnd(2 * q, d) * 2 - 1, y=torch.randn(2 * q, device=dev, dtype=dt, generator=gen), noise=rnd(2 * q) + 0.5) for _ in range(4)]
    for pb in pool:
        pb["w"] = 1.0 / pb["noise"]
    u = 0.1 * torch.randn(grid.m, device=dev, dtype=dt, generator=gen)
    H = (grid.R + 1) // 2
    mk = lambda: [torch.zeros(s, device=dev, dtype=dt) for s in (grid.m, (H, grid.m), grid.m, grid.m)] + [torch.zeros(2, device=dev, dtype=torch.float64)]
    win, pl = mk(), mk()
    err = grid_ops.new_err_flag(dev)
    ring = grid_ops.WindowRing(cap, d, dt, dev)
    k = 0
    while ring.fill < cap:                                            # fill the ring: from here on q enter and q leave
        pb = pool[k % 4]
        grid_ops.scatter_stats_window(grid, pb["X"][:q], pb["y"][:q], pb["w"][:q], pb["w"][:q], pb["noise"][:q], ring, win[0], win[1], win[2], win[4], err, u, res=win[3])
        k += 1
    ring2 = ring.clone()
    state = {"k": 0}

    def window():
        pb = pool[state["k"] % 4]
        grid_ops.scatter_stats_window(grid, pb["X"][:q], pb["y"][:q], pb["w"][:q], pb["w"][:q], pb["noise"][:q], ring, win[0], win[1], win[2], win[4], err, u, res=win[3])

    def plain(n):
        pb = pool[state["k"] % 4]
        grid_ops.scatter_stats_cnt(grid, pb["X"][:n], pb["y"][:n], pb["w"][:n], pb["w"][:n], pb["noise"][:n], pl[0], pl[1], True, pl[2], pl[4], err, u=u, res=pl[3])

    def two_step():
        pb = pool[state["k"] % 4]
        idx = (ring2.head + torch.arange(q, device=dev)) % cap
        ox, oy, owa, owb, on = (t.index_select(0, idx) for t in ring2.tensors())
        grid_ops.scatter_stats_cnt(grid, pb["X"][:q], pb["y"][:q], pb["w"][:q], pb["w"][:q], pb["noise"][:q], pl[0], pl[1], True, pl[2], pl[4], err, u=u, res=pl[3])
        grid_ops.scatter_stats_cnt(grid, ox, oy, -owa, -owb, on, pl[0], pl[1], True, pl[2], pl[4], err, u=u, res=pl[3])
        for t, v in zip(ring2.tensors(), (pb["X"][:q], pb["y"][:q], pb["w"][:q], pb["w"][:q], pb["noise"][:q])):
            t.index_copy_(0, idx, v)
        ring2.advance(q)

    forms = {"window": window, "plain_q": lambda: plain(q), "plain_2q": lambda: plain(2 * q), "two_step": two_step}
    times = {k_: [] for k_ in forms}
    for rep in range(a.warm + a.reps):
        state["k"] = rep
        for name, f in forms.items():
            for t in pl:
                t.zero_()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            torch.cuda.synchronize()
            if rep >= a.warm:
                times[name].append(t0.elapsed_time(t1) * 1e3)
    assert int(err.item()) == 0 and int(ring.void_left.item()) == 0
    med = {k_: statistics.median(v) for k_, v in times.items()}
    print(json.dumps({"grid": [a.grid] * d, "dtype": a.dtype, "q": q, "cap": cap, "reps": a.reps, "us": {k_: round(v, 2) for k_, v in med.items()},
                      "window_over_plain_2q": round(med["window"] / med["plain_2q"], 3), "window_over_two_step": round(med["window"] / med["two_step"], 3),
                      "us_min": {k_: round(min(v), 2) for k_, v in times.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--grid", type=int, default=50)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--q", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--turns", type=int, default=4, help="ring capacity in batches")
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_absorb_probe: no GPU (timings are taken on the device or not at all)")
    dt = torch.float32 if a.dtype == "f32" else torch.float64
    for q in a.q:
        run(a, q, dt, "cuda")


if __name__ == "__main__":
    main()
