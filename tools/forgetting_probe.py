"""Cost of exponential forgetting on the streaming step: N `stream_step`s of q points with and without
``forgetting_factor`` at one grid, each run timed with HIP events around its steps.  Meant to run under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/forgetting_probe.py --grid 50 --dim 3 --dtype f32

so that the decay kernel, the half-stencil SpMV and the absorb are timed in the SAME run (tools/trace_medians.py prints their medians
from the kernel trace).  Every decay drops the exact block of the two-level preconditioner (3.5), so at the shapes that have one the
ratio holds the lost preconditioning as well as the decay; ``--two-level off`` runs both models without it and isolates the decay.
Prints one JSON line: ms per step and mean CG iterations per step of both runs, and the ratio of the times."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_gp_amd import settings  # noqa: E402
from online_gp_amd.models import FixedNoiseOnlineSKIGP  # noqa: E402


def run(a, dt, gamma):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    n = a.n0 + (a.warm + a.steps) * a.q
    X = torch.rand((n, a.dim), device=dev, dtype=dt, generator=gen) * 2 - 1
    y = torch.sin(2 * X.sum(1, keepdim=True)) + 0.1 * torch.randn((n, 1), device=dev, dtype=dt, generator=gen)
    with torch.no_grad():
        model = FixedNoiseOnlineSKIGP(X[:a.n0], y[:a.n0], None, grid_bounds=torch.tensor([[-1.1, 1.1]] * a.dim), grid_size=a.grid,
                                      learn_additional_noise=True, forgetting_factor=gamma).eval()
        lo = a.n0
        for _ in range(a.warm):
            model.stream_step(X[lo:lo + a.q], y[lo:lo + a.q])
            lo += a.q
        model._finish_pending()
        torch.cuda.synchronize()
        fast, iters = 0, 0
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            fast += int(model._stream_fast_state(X[lo:lo + a.q], y[lo:lo + a.q]) is not None)
            model.stream_step(X[lo:lo + a.q], y[lo:lo + a.q])
            lo += a.q
            iters += (getattr(model, "_last_iters", None) or [0])[0]
        model._finish_pending()
        t1.record()
        torch.cuda.synchronize()
    del model
    torch.cuda.empty_cache()
    return t0.elapsed_time(t1) / a.steps, fast, iters / a.steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--grid", type=int, default=50)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--q", type=int, default=4096)
    ap.add_argument("--n0", type=int, default=20000)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--two-level", default="on", choices=["on", "off"])
    a = ap.parse_args()
    dt = torch.float32 if a.dtype == "f32" else torch.float64
    # (a decay waits for the solve in flight: compare like with like)
    with settings.deferred_refresh(False), settings.two_level_preconditioner(a.two_level == "on"):
        plain, fast0, it0 = run(a, dt, None)
        forget, fast1, it1 = run(a, dt, a.gamma)
    print(json.dumps({"grid": [a.grid] * a.dim, "dtype": a.dtype, "q": a.q, "steps": a.steps, "gamma": a.gamma, "two_level": a.two_level,
                      "ms_per_step_plain": round(plain, 4), "ms_per_step_forgetting": round(forget, 4), "ratio": round(forget / plain, 3),
                      "cg_iters_per_step": [round(it0, 1), round(it1, 1)], "one_call_steps": [fast0, fast1]}), flush=True)


if __name__ == "__main__":
    main()
