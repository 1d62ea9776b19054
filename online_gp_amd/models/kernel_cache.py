"""The kernel cache of FixedNoiseOnlineSKIGP: a plain dict of streamed statistics -- ``kernel_cache=`` hands a caller's own over, which may
lack ``_cnt`` (or any optional group) or carry a full offset-major stencil.  ENTRIES names every key once with what it does under every
hand-over, and the functions below read it: a statistic added there follows without another site to edit."""
import math
from collections import namedtuple
from operator import methodcaller

import torch

from .. import grid_ops
from ..distributions import LazyCovariance
from ..lazy.operators import StencilWtW


class BatchOperator(LazyCovariance):
    """Stack of per-output operators: shape [out, n, n]."""

    def __init__(self, ops):
        self.ops = list(ops)
        self.shape = torch.Size([len(self.ops)]) + self.ops[0].shape
        self.dtype = self.ops[0].dtype
        self.device = self.ops[0].device

    def __getitem__(self, i):
        return self.ops[i]

    def __len__(self):
        return len(self.ops)

    def matmul(self, rhs):
        if rhs.dim() == 2:
            return torch.stack([op.matmul(rhs) for op in self.ops])
        return torch.stack([op.matmul(rhs[i]) for i, op in enumerate(self.ops)])

    __matmul__ = matmul

    def evaluate(self):
        return torch.stack([op.evaluate() for op in self.ops])

    def diag(self):
        return torch.stack([op.diag() for op in self.ops])

    def clone(self):
        return BatchOperator([op.clone() for op in self.ops])

    def to(self, device):
        return BatchOperator([op.to(device) for op in self.ops])


def _wtw_ops(wtw):
    return wtw.ops if isinstance(wtw, BatchOperator) else [wtw]


def _wtw(ops):
    return ops[0] if len(ops) == 1 else BatchOperator(ops)


# What an entry does under each operation (DESIGN.md 3.30 has the table in words); one that is absent, or None, is skipped by all of them.
#   move (clone, to): "copy" -- through its own .clone() / .to(device), a scalar as it is; a function -- a view, re-made from the new _stats
#   decay (decay_regions): "gamma" / "sqrt" -- a region of the launch at that factor; "mul" -- scaled here, by a launch of its own
#   regrid (regrid_plan): "rows" [out, m, ...] / "cols" [m, w] -- a node region into a new tensor; "keep" -- the same object
#   zero (zero_): "zero_" / "clear" -- that method; "stencils" -- zeroed, root pairs dropped
Entry = namedtuple("Entry", "move decay regrid zero")
_CONST = Entry("copy", None, "keep", "keep")
ENTRIES = {
    "WtW": Entry("stencils", "stencils", "stencils", "stencils"),     # W^T D^-1 W     (:50-53)
    "interpolation_cache": Entry("copy", "gamma", "rows", "zero_"),   # W^T D^-1 y     (:46)
    "_cnt": Entry("copy", "gamma", "rows", "zero_"),                  # W^T D^-1 1 = row sums of W^T D^-1 W (preconditioner density model)
    "_stats": Entry("copy", None, "keep", "zero_"),                   # (decayed by decay_stats(stats=...))
    "response_cache": Entry(lambda stats: stats[:, 0].view(-1, 1, 1), None, "keep", "keep"),     # y^T D^-1 y  (:45)  [float64 view]
    "D_logdet": Entry(lambda stats: stats[:, 1], None, "keep", "keep"),                          # logdet D    (:55)  [float64 view]
    "path_probes": Entry("copy", "sqrt", "cols", "keep"),             # P [m, S]: cov(P_s) = A stays exact; _absorb_probes(init=True) restarts them
    **dict.fromkeys(("path_seed", "path_count"), _CONST),
    "trend_C": Entry("copy", "gamma", "cols", "zero_"),               # C [m, p], G [p, p], g [p] (fp64): weighted sums, like A and b
    **dict.fromkeys(("trend_G", "trend_g"), Entry("copy", "mul", "keep", "zero_")),
    **dict.fromkeys(("trend_deg", "trend_center", "trend_scale"), _CONST),
    "_ring": _CONST,                                                  # (coordinates, not node indices; _window_restart clears it)
    "_site_ring": Entry("copy", None, "keep", "clear"),               # (regrid_commit empties it where nodes were removed)
    "_spectral": Entry("spectral", None, "drop", "drop"),
}
_DECAYED = [(k, e.decay) for k, e in ENTRIES.items() if e.decay is not None]      # (a forgetting stream asks at every step)


def _present(cache):
    return [(k, e, cache[k]) for k, e in ENTRIES.items() if cache.get(k) is not None]


def fresh(grid, num_outputs, dtype, device, probes=(0, 0), trend_deg=None):
    """Empty statistics of `num_outputs` outputs on `grid`; probes = (S, seed) adds the path probes, trend_deg the trend's entries."""
    out, m = num_outputs, grid.m
    z = lambda *shape, dtype=dtype: torch.zeros(shape, dtype=dtype, device=device)
    stats = z(out, 2, dtype=torch.float64)
    pack = z(out, (grid.R + 1) // 2, m)                  # ONE tensor, each operator holds a view: an absorb of several outputs is a single launch
    cache = {"WtW": _wtw([StencilWtW(grid, pack[o]) for o in range(out)]), "interpolation_cache": z(out, m, 1), "_cnt": z(out, m), "_stats": stats,
             "response_cache": ENTRIES["response_cache"].move(stats), "D_logdet": ENTRIES["D_logdet"].move(stats)}
    if probes[0] > 0:                                    # path_count: global index of the next point (the generator is keyed on (seed, index, s))
        cache.update(path_probes=z(m, probes[0]), path_seed=probes[1], path_count=0)
    if trend_deg is not None:                            # (the basis is normalised by the centre and half-extent of THIS grid, for good)
        p = grid_ops.trend_size(grid.d, trend_deg)
        half = [0.5 * hq * (gq - 1) for hq, gq in zip(grid.h, grid.g)]
        f64 = dict(dtype=torch.float64, device=device)
        cache.update(trend_C=z(m, p), trend_G=z(p, p, dtype=torch.float64), trend_g=z(p, dtype=torch.float64), trend_deg=trend_deg,
                     trend_center=torch.tensor([g0 + hf for g0, hf in zip(grid.g0, half)], **f64), trend_scale=torch.tensor(half, **f64))
    return cache


def stencil_pack(grid, ops):
    """The [out, H, m] tensor the outputs' half stencils are views of, if they (still) are: consecutive, same shape."""
    st = [op.stencil for op in ops]
    if not all(grid_ops.is_half_stencil(grid, t) and t.is_contiguous() for t in st):
        return None
    (H, m), es, base = st[0].shape, st[0].element_size(), st[0].data_ptr()
    if any(t.shape != (H, m) or t.data_ptr() != base + o * H * m * es for o, t in enumerate(st)):
        return None
    if len(st) == 1:
        return st[0][None]
    root = st[0]._base
    return root if root is not None and root.dim() == 3 and root.shape == (len(st), H, m) and root.data_ptr() == base else None


def clone(cache, grid, mv=methodcaller("clone"), spectral=True):
    """A copy that shares no storage with `cache`: a child's increments never reach the parent's (to(): each object through `mv`)."""
    new = {}
    for k, e, v in _present(cache):
        if callable(e.move):                             # (_stats stands before its views in the table)
            new[k] = e.move(new["_stats"])
        elif e.move == "copy":
            new[k] = mv(v) if hasattr(v, "clone") else v
        elif e.move == "stencils":
            ops = _wtw_ops(v)
            pack = stencil_pack(grid, ops)
            if pack is not None and len(ops) > 1:            # keep the outputs' stencils in one tensor (see fresh)
                pk = mv(pack)
                opt = lambda t: None if t is None else mv(t)
                ops = [StencilWtW(grid, pk[o], opt(op.root), opt(op.inv_root)) for o, op in enumerate(ops)]
            else:
                ops = [mv(op) for op in ops]
            new[k] = _wtw(ops)
        elif spectral and v:
            new[k] = {o: mv(fac) for o, fac in v.items() if fac.ref is not None and not fac.stale}
    return new


def to(cache, grid, device):
    """The cache on `device`, without the spectral factors."""
    return clone(cache, grid, methodcaller("to", device), spectral=False)


def decay_regions(cache, grid, gamma):
    """The (tensor, factor) list of grid_ops.decay_stats for a decay of `cache` by gamma; scales the "mul" entries itself."""
    regions = []
    for k, how in _DECAYED:
        v = cache.get(k)
        if v is None:
            continue
        if how == "stencils":
            ops = _wtw_ops(v)
            pack = stencil_pack(grid, ops)
            regions += [(pack, gamma)] if pack is not None else [(op.stencil, gamma) for op in ops]
        elif how == "mul":
            v.mul_(gamma)
        else:
            regions.append((v, gamma if how == "gamma" else math.sqrt(gamma)))
    return regions


def regrid_plan(cache, old, new):
    """(regions of grid_ops.regrid_stats that move `cache` from grid `old` to `new`, the cache they fill); `cache` is not touched."""
    regions, fresh = [], {}
    for k, e, v in _present(cache):
        if e.regrid == "keep":
            fresh[k] = v
        elif e.regrid in ("rows", "cols"):               # [out, m, ...]: out blocks of width 1; [m, w], probe-shaped: one block of width w
            kw = (v.shape[0], 1) if e.regrid == "rows" else (1, v.shape[1])
            fresh[k] = v.new_empty((kw[0], new.m) + v.shape[2:] if e.regrid == "rows" else (new.m, kw[1]))     # (the kernel writes every element)
            regions.append((v.contiguous(), fresh[k]) + kw)
        elif e.regrid == "stencils":
            ops = _wtw_ops(v)
            pack = stencil_pack(old, ops)
            if pack is not None:                         # the outputs' half stencils stay in one tensor
                new_pack = pack.new_empty((len(ops), pack.shape[1], new.m))
                new_st = [new_pack[o] for o in range(len(ops))]
            else:                                        # (an offset-major stencil is regridded in that layout)
                new_st = [op.stencil.new_empty((op.stencil.shape[0], new.m)) for op in ops]
            for o, op in enumerate(ops):
                regions += grid_ops.stencil_regrid_regions(old, new, op.stencil.contiguous(), new_st[o], report=o)
            fresh[k] = _wtw([StencilWtW(new, st) for st in new_st])
    return regions, fresh


def regrid_commit(cache, fresh, trimmed):
    """Put the filled `fresh` of regrid_plan into the same dict; trimmed (nodes were removed): the sites stay in, frozen, their ring is emptied."""
    cache.clear()
    cache.update(fresh)
    if trimmed and cache.get("_site_ring") is not None:
        cache["_site_ring"].clear()


def zero_(cache):
    """Zero every streamed statistic in place; root pairs (L L^T described the old matrix), spectral factors and stored sites go."""
    for k, e, v in _present(cache):
        if e.zero == "stencils":
            for op in _wtw_ops(v):
                op.stencil.zero_()
                op.root = op.inv_root = None
        elif e.zero == "drop":
            cache.pop(k)
        elif e.zero != "keep":
            getattr(v, e.zero)()
