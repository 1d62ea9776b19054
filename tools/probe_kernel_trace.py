"""Launches for a kernel trace of the probe scatter beside the absorb:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/probe_kernel_trace.py

50^3 grid, fp32, batches of 4 096 uniform points: 20 absorbs (wiski_scatter_stats_cnt into the half stencil), then 20 probe
scatters each for S = 16 and S = 64.  The S of a k_scatter_probes dispatch is read off its order in the trace (16 first)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_gp_amd import grid_ops  # noqa: E402

dev, dtype, n, reps = "cuda", torch.float32, 4096, 20
grid = grid_ops.GridSpec(torch.tensor([[-1.1, 1.1]] * 3), 50)
gen = torch.Generator().manual_seed(0)
err = grid_ops.new_err_flag(dev)
ones = torch.ones(n, dtype=dtype, device=dev)
b = torch.zeros(grid.m, dtype=dtype, device=dev)
A = torch.zeros(((grid.R + 1) // 2, grid.m), dtype=dtype, device=dev)
cnt = torch.zeros(grid.m, dtype=dtype, device=dev)
stats = torch.zeros(2, dtype=torch.float64, device=dev)
xs = [(2 * torch.rand((n, 3), generator=gen) - 1).to(dev, dtype) for _ in range(reps)]
ys = [torch.randn(n, generator=gen).to(dev, dtype) for _ in range(reps)]
for x, y in zip(xs, ys):
    grid_ops.scatter_stats_cnt(grid, x, y, ones, ones, ones, b, A, True, cnt, stats, err)
torch.cuda.synchronize()
for S in (16, 64):
    P = torch.zeros((grid.m, S), dtype=dtype, device=dev)
    for i, x in enumerate(xs):
        grid_ops.scatter_probes(grid, x, None, i * n, 1, P, err)
    torch.cuda.synchronize()
assert int(err.item()) == 0
print("done")
