"""Time a growth of the inducing grid by 4 nodes in dim 0 (``FixedNoiseOnlineSKIGP.regrid_``) at 50^3 fp32 and at
30^4 fp64, beside two yardsticks:

  copy      a plain device copy of the same number of bytes (the source read plus the destination written, i.e. a copy of their mean);
  rebuild   the only route without regrid_: a fresh model on the new grid that re-absorbs the whole stream, at the number of points
            the benchmark's default run streams (n_init + (warmup + steps) * batch = 21743 + 25 * 4096).

Prints one line per case and one JSON line.  Usage: python tools/regrid_timing.py [--cases 50x3,30x4] [--n N] [--reps R]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CASES = {"50x3": (50, 3, torch.float32), "30x4": (30, 4, torch.float64)}


def _sync_ms(fn, reps):
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def run_case(name, n, reps, batch=4096):
    import bench
    from online_gp_amd import grid_ops
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    g, d, dtype = CASES[name]
    dev = torch.device("cuda")
    X, y = bench.synth_stream(n, d, 0, dev, dtype, "clustered")
    y = y.reshape(-1, 1)
    gb = torch.tensor([[-1.1, 1.1]] * d)

    def build(bounds, sizes):
        model = FixedNoiseOnlineSKIGP(X[:batch], y[:batch], None, grid_bounds=torch.as_tensor(bounds), grid_size=sizes, learn_additional_noise=True)
        for s in range(batch, n, batch):
            model.condition_on_observations(X[s:s + batch], y[s:s + batch], inplace=True)
        model.check_bounds()
        return model

    model = build(gb, [g] * d)
    below, above = [0] * d, [4] + [0] * (d - 1)
    es = torch.empty((), dtype=dtype).element_size()
    H = (7 ** d + 1) // 2
    m_old = model._grid.m
    m_new = model._grid.shifted(below, above).m
    moved = (H + 2) * (m_old + m_new) * es                        # stencil, b, cnt: read once, written once
    regrid_ms = []
    for _ in range(reps):                                         # grow, then trim the untouched nodes again (not timed)
        regrid_ms.append(_sync_ms(lambda: model.regrid_(below, above), 1))
        new_spec = model._grid
        model.regrid_([0] * d, [-4] + [0] * (d - 1))
    half = moved // 2 // es
    a, b = torch.empty(half, dtype=dtype, device=dev).normal_(), torch.empty(half, dtype=dtype, device=dev)
    copy_ms = _sync_ms(lambda: b.copy_(a), max(reps, 3))
    del a, b
    del model
    torch.cuda.empty_cache()
    rebuild_ms = _sync_ms(lambda: build(new_spec.grid_bounds, new_spec.g), 1)
    res = {"case": name, "dtype": str(dtype), "grid": [g] * d, "new_grid": list(new_spec.g), "bytes_moved": int(moved), "n_points": int(n),
           "regrid_ms": min(regrid_ms), "regrid_ms_all": regrid_ms, "copy_ms": copy_ms, "rebuild_ms": rebuild_ms,
           "regrid_GBps": moved / min(regrid_ms) / 1e6, "copy_GBps": moved / copy_ms / 1e6}
    print(f"{name} {dtype}: regrid_ {res['regrid_ms']:.3f} ms ({res['regrid_GBps']:.0f} GB/s, kernel + allocation + one host read), "
          f"copy of {moved / 1e6:.0f} MB {copy_ms:.3f} ms ({res['copy_GBps']:.0f} GB/s), fresh model re-absorbing {n} points {rebuild_ms:.1f} ms", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="50x3,30x4")
    ap.add_argument("--n", type=int, default=21743 + 25 * 4096)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    out = [run_case(c, args.n, args.reps) for c in args.cases.split(",")]
    print(json.dumps({"regrid_timing": out}))


if __name__ == "__main__":
    main()
