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
#   state (pack, unpack, load_into_): "stencils" / "rows" / "cols" -- node regions, carried compact (the touched nodes only); "copy" -- as it is;
#       "view" -- not carried, re-made from _stats; "refuse" -- NotImplementedError when present; "drop" -- not carried
#   merge (merge_into_, weight w): "stencils" / "w" -- += w x; "sqrt" -- += sqrt(w) x (the seeds of the two sides must differ); "stats" -- slot 0
#       += w s0, slot 1 += s1 - n_other log w; "keep" -- the receiver's; "equal" -- must be equal; "view"; "refuse"; "drop" -- popped on the receiver
Entry = namedtuple("Entry", "move decay regrid zero state merge")
_CONST = ("copy", None, "keep", "keep")
ENTRIES = {
    "WtW": Entry("stencils", "stencils", "stencils", "stencils", "stencils", "stencils"),     # W^T D^-1 W     (:50-53)
    "interpolation_cache": Entry("copy", "gamma", "rows", "zero_", "rows", "w"),   # W^T D^-1 y     (:46)
    "_cnt": Entry("copy", "gamma", "rows", "zero_", "rows", "w"),     # W^T D^-1 1 = row sums of W^T D^-1 W (preconditioner density model)
    "_stats": Entry("copy", None, "keep", "zero_", "copy", "stats"),  # (decayed by decay_stats(stats=...))
    "response_cache": Entry(lambda stats: stats[:, 0].view(-1, 1, 1), None, "keep", "keep", "view", "view"),     # y^T D^-1 y  (:45)  [float64 view]
    "D_logdet": Entry(lambda stats: stats[:, 1], None, "keep", "keep", "view", "view"),                          # logdet D    (:55)  [float64 view]
    "path_probes": Entry("copy", "sqrt", "cols", "keep", "cols", "sqrt"),     # P [m, S]: cov(P_s) = A stays exact; _absorb_probes(init=True) restarts them
    **dict.fromkeys(("path_seed", "path_count"), Entry(*_CONST, "copy", "keep")),
    "trend_C": Entry("copy", "gamma", "cols", "zero_", "cols", "w"),  # C [m, p], G [p, p], g [p] (fp64): weighted sums, like A and b
    **dict.fromkeys(("trend_G", "trend_g"), Entry("copy", "mul", "keep", "zero_", "copy", "w")),
    **dict.fromkeys(("trend_deg", "trend_center", "trend_scale"), Entry(*_CONST, "copy", "equal")),
    "_ring": Entry(*_CONST, "refuse", "refuse"),                      # (coordinates, not node indices; _window_restart clears it)
    "_site_ring": Entry("copy", None, "keep", "clear", "refuse", "refuse"),   # (regrid_commit empties it where nodes were removed)
    "_spectral": Entry("spectral", None, "drop", "drop", "drop", "drop"),
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


# ---------------------------------------------------------------- checkpoint, restore and merge --
STATE_FORMAT, STATE_VERSION = "online_gp_amd.stream_state", 1
_NODE = ("stencils", "rows", "cols")
_DTYPES = {str(torch.float32): torch.float32, str(torch.float64): torch.float64}


def _node_items(obj):
    """(name, kind, tensor) of every tensor of a cache -- or of a state, whose "WtW" is ONE [out, rows, n_sel] tensor (_describe: the list of
    a cache's stencils) -- that is made of node regions, in the table's order; kind: the entry's `state` column."""
    for k, e in ENTRIES.items():
        v = obj.get(k)
        if v is None or e.state not in _NODE:
            continue
        if e.state == "stencils":
            for o, t in enumerate(v if torch.is_tensor(v) or isinstance(v, list) else [op.stencil for op in _wtw_ops(v)]):
                yield f"{k}[{o}]", e.state, t
        else:
            yield k, e.state, v


def _regions(grid, kind, t):
    """The (flat view, k, w) node regions of one tensor of _node_items, whatever its number of nodes (m, or n_sel for a compact one)."""
    if not t.is_contiguous():
        raise ValueError("the node regions of a kernel cache must be contiguous tensors")
    if kind == "stencils":
        return grid_ops.stencil_node_regions(grid, t)
    if kind == "rows":
        return [(t.reshape(-1), t.shape[0], max(1, math.prod(t.shape[2:])))]
    return [(t.reshape(-1), 1, t.shape[1])]


def _compact_shape(kind, t, n_sel):
    return (t.shape[0], n_sel) + tuple(t.shape[2:]) if kind != "cols" else (n_sel, t.shape[1])


def _refuse(obj, what):
    for k, e in ENTRIES.items():
        if e.state == "refuse" and obj.get(k) is not None:
            raise NotImplementedError(f"{what}: the statistics carry {k!r}, the ring of a window / site_memory model.  A ring is more than "
                                      "statistics -- its slots hold points, with host-side bookkeeping on the model beside them (the void "
                                      "slots, the unit / explicit split of the weight sum) -- and two rings have no union")


def _layout(grid, stencils):
    halves = {grid_ops.is_half_stencil(grid, t) for t in stencils}
    if len(halves) != 1:
        raise ValueError("WtW: the outputs' stencils must have one layout")
    return "half" if halves.pop() else "offset-major"


def _grid_dict(grid):
    return {"bounds": [list(map(float, b)) for b in grid.grid_bounds], "size": [int(v) for v in grid.g], "g0": [float(v) for v in grid.g0],
            "h": [float(v) for v in grid.h]}


def _describe(cache, grid):
    """A cache in the form of a state whose node regions are the cache's own full tensors ("WtW": the list of the stencils): what merge_into_
    takes from another cache without packing it."""
    _refuse(cache, "merge_into_")
    st = [op.stencil for op in _wtw_ops(cache["WtW"])]
    ic = cache["interpolation_cache"]
    desc = {"format": STATE_FORMAT, "version": STATE_VERSION, "grid": _grid_dict(grid), "dtype": str(ic.dtype), "num_outputs": ic.shape[0],
            "layout": _layout(grid, st), "nodes": None}
    for k, e, v in _present(cache):
        if e.state in _NODE or e.state == "copy":
            desc[k] = st if e.state == "stencils" else v
    return desc


def _bad(field, why):
    return ValueError(f"stream state: {field!r} {why}")


def _check_state(state):
    """Everything a state can be checked for by itself; returns (GridSpec fields, m, n_sel, dtype).  ValueError names the field."""
    if not isinstance(state, dict) or state.get("format") != STATE_FORMAT:
        raise _bad("format", f"is not {STATE_FORMAT!r}")
    if state.get("version") != STATE_VERSION:
        raise _bad("version", f"is {state.get('version')!r}, this build reads version {STATE_VERSION}")
    _refuse(state, "stream state")
    gd = state.get("grid")
    if not isinstance(gd, dict) or any(not isinstance(gd.get(f), list) for f in ("bounds", "size", "g0", "h")):
        raise _bad("grid", "needs the lists bounds, size, g0 and h")
    d = len(gd["size"])
    if not (1 <= d <= 4) or any(len(gd[f]) != d for f in ("bounds", "g0", "h")) or any(int(g) != g or g < 4 for g in gd["size"]):
        raise _bad("grid", "needs 1..4 dims of at least 4 nodes, one entry per dim in every list")
    m = math.prod(int(g) for g in gd["size"])
    dtype = _DTYPES.get(state.get("dtype"))
    if dtype is None:
        raise _bad("dtype", f"is {state.get('dtype')!r}, not one of {sorted(_DTYPES)}")
    out = state.get("num_outputs")
    if isinstance(out, bool) or not isinstance(out, int) or out < 1:
        raise _bad("num_outputs", f"is {out!r}")
    if state.get("layout") not in ("half", "offset-major"):
        raise _bad("layout", f"is {state.get('layout')!r}")
    nodes = state.get("nodes")
    n_sel = m
    if nodes is not None:
        if not torch.is_tensor(nodes) or nodes.dtype != torch.int32 or nodes.dim() != 1:
            raise _bad("nodes", "must be a 1-D int32 tensor (or None: every node)")
        n_sel = nodes.numel()
        if n_sel and not (bool((nodes[1:] > nodes[:-1]).all()) and int(nodes[0]) >= 0 and int(nodes[-1]) < m):
            raise _bad("nodes", f"must be strictly ascending within [0, {m})")
    R = 7 ** d
    rows = (R + 1) // 2 if state["layout"] == "half" else R
    f64 = torch.float64

    def tensor(key, shape, dt=dtype, need=True, t=None):
        t = state.get(key) if t is None else t
        if t is None and not need:
            return False
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != tuple(shape):
            got = f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else repr(type(t).__name__)
            raise _bad(key, f"must be a {dt} tensor of shape {tuple(shape)} ({n_sel} selected nodes), got {got}")
        return True

    W = state.get("WtW")
    if isinstance(W, list):                              # (_describe: the stencils of a cache)
        if len(W) != out:
            raise _bad("WtW", f"holds {len(W)} stencils for {out} outputs")
        for o, t in enumerate(W):
            tensor(f"WtW[{o}]", (rows, n_sel), t=t)
    else:
        tensor("WtW", (out, rows, n_sel))
    tensor("interpolation_cache", (out, n_sel, 1))
    tensor("_cnt", (out, n_sel), need=False)
    tensor("_stats", (out, 2), f64)
    if tensor("path_probes", (n_sel, state["path_probes"].shape[-1] if torch.is_tensor(state.get("path_probes")) and state["path_probes"].dim() == 2 else 0),
              need=False):
        for k in ("path_seed", "path_count"):
            if isinstance(state.get(k), bool) or not isinstance(state.get(k), int):
                raise _bad(k, f"must be an int beside path_probes, got {state.get(k)!r}")
    if state.get("trend_C") is not None:
        deg = state.get("trend_deg")
        if isinstance(deg, bool) or not isinstance(deg, int) or deg not in grid_ops.TREND_DEGREES.values():
            raise _bad("trend_deg", f"is {deg!r}")
        p = grid_ops.trend_size(d, deg)
        tensor("trend_C", (n_sel, p))
        tensor("trend_G", (p, p), f64)
        tensor("trend_g", (p,), f64)
        tensor("trend_center", (d,), f64)
        tensor("trend_scale", (d,), f64)
    return gd, m, n_sel, dtype


def _check_fits(cache, grid, state, what):
    """That `state` (checked) describes statistics of the kind `cache` on `grid` holds: ValueError names the field that differs."""
    gd = state["grid"]
    for f, mine in (("size", [int(v) for v in grid.g]), ("g0", [float(v) for v in grid.g0]), ("h", [float(v) for v in grid.h])):
        if list(gd[f]) != mine:
            raise ValueError(f"{what}: 'grid' differs in {f}: {gd[f]} against this model's {mine} (the grids must be equal node for node; "
                             "regrid_ moves a model onto another grid)")
    ic = cache["interpolation_cache"]
    mine = {"dtype": str(ic.dtype), "num_outputs": ic.shape[0], "layout": _layout(grid, [op.stencil for op in _wtw_ops(cache["WtW"])])}
    for f, v in mine.items():
        if state[f] != v:
            raise ValueError(f"{what}: {f!r} is {state[f]!r}, this model's is {v!r}")
    for k in ("_cnt", "path_probes", "trend_C"):
        if (state.get(k) is None) != (cache.get(k) is None):
            raise ValueError(f"{what}: {k!r} is {'missing from' if state.get(k) is None else 'present in'} the state but "
                             f"{'present in' if state.get(k) is None else 'missing from'} this model's statistics")
    if cache.get("path_probes") is not None and state["path_probes"].shape[1] != cache["path_probes"].shape[1]:
        raise ValueError(f"{what}: 'path_probes' holds S = {state['path_probes'].shape[1]} probes, this model's {cache['path_probes'].shape[1]}")
    if cache.get("trend_C") is not None:
        if state["trend_deg"] != cache["trend_deg"]:
            raise ValueError(f"{what}: 'trend_deg' is {state['trend_deg']}, this model's is {cache['trend_deg']}")
        for k in ("trend_center", "trend_scale"):
            if not torch.equal(state[k].cpu(), cache[k].cpu()):
                raise ValueError(f"{what}: {k!r} differs: the trend's basis is normalised by another frame")


def _state_nodes(state, m, device):
    nodes = state["nodes"]
    return torch.arange(m, dtype=torch.int32, device=device) if nodes is None else nodes.to(device).contiguous()


def _tree_to(v, device):
    if torch.is_tensor(v):
        return v.to(device)
    if isinstance(v, dict):
        return {k: _tree_to(x, device) for k, x in v.items()}
    return [_tree_to(x, device) for x in v] if isinstance(v, list) else v


def pack(cache, grid, device=None):
    """The statistics of `cache` on `grid` as a state: a dict of tensors, ints, floats, strings, lists and dicts of those only (torch.save, then
    torch.load(weights_only=True) round-trips it), every node region in its COMPACT form -- the nodes at which any region holds something
    (``state["nodes"]``, ascending int32; None: every node), found by one select and moved by one gather (grid_ops.stats_select /
    stats_gather; one host read).  Root pairs and spectral factors are not carried; a ring is refused.  device: where the state's tensors go
    (None: they stay on the cache's)."""
    _refuse(cache, "pack")
    items = list(_node_items(cache))
    st = [op.stencil for op in _wtw_ops(cache["WtW"])]
    ic, m = cache["interpolation_cache"], grid.m
    state = {"format": STATE_FORMAT, "version": STATE_VERSION, "grid": _grid_dict(grid), "dtype": str(ic.dtype), "num_outputs": ic.shape[0],
             "layout": _layout(grid, st)}
    nodes, n_sel = grid_ops.stats_select(m, [r for _, kind, t in items for r in _regions(grid, kind, t)])
    state["nodes"] = None if n_sel == m else nodes.clone()
    W = st[0].new_empty((len(st), st[0].shape[0], n_sel))
    moves = []
    for name, kind, t in items:
        c = W[int(name[4:-1])] if kind == "stencils" else t.new_empty(_compact_shape(kind, t, n_sel))
        if n_sel == m:
            c.copy_(t)
        else:
            moves += [(s[0], d[0], s[1], s[2]) for s, d in zip(_regions(grid, kind, t), _regions(grid, kind, c))]
        state[name if kind != "stencils" else "WtW"] = c if kind != "stencils" else W
    grid_ops.stats_gather(m, nodes, moves)
    for k, e, v in _present(cache):
        if e.state == "copy":
            state[k] = v.clone() if torch.is_tensor(v) else v
    return state if device is None else _tree_to(state, device)


def _grid_of(gd):
    """The GridSpec of a state's grid: built from its bounds and size, then given the state's very g0 and h (a shifted grid's differ from the
    constructor's in the last bits)."""
    grid = grid_ops.GridSpec(gd["bounds"], [int(g) for g in gd["size"]])
    grid.g0, grid.h = [float(v) for v in gd["g0"]], [float(v) for v in gd["h"]]
    for q in range(grid.d):
        grid.c.g0[q], grid.c.h[q] = grid.g0[q], grid.h[q]
    return grid


def unpack(state, device):
    """(GridSpec, cache) of a state: a fresh cache on `device`, filled by one scatter into zeros -- what FixedNoiseOnlineSKIGP(...,
    kernel_cache=, num_data=) accepts."""
    gd, m, n_sel, dtype = _check_state(state)
    grid = _grid_of(gd)
    out = state["num_outputs"]
    probes = (state["path_probes"].shape[1], state["path_seed"]) if state.get("path_probes") is not None else (0, 0)
    cache = fresh(grid, out, dtype, device, probes, state.get("trend_deg") if state.get("trend_C") is not None else None)
    if state["layout"] != "half":
        cache["WtW"] = _wtw([StencilWtW(grid, torch.zeros((grid.R, m), dtype=dtype, device=device)) for _ in range(out)])
    if state.get("_cnt") is None:
        cache.pop("_cnt")
    _fill(cache, grid, state, zero=False)
    return grid, cache


def _fill(cache, grid, state, zero):
    """cache <- state, into the cache's own tensors (both checked): node regions by one scatter-add into zeros, the rest copied."""
    if zero:
        zero_(cache)
        for k, e, v in _present(cache):
            if e.state in _NODE and e.zero == "keep":    # (the probes, which zero_ leaves to _absorb_probes(init=True))
                v.zero_()
    m = grid.m
    dev = cache["interpolation_cache"].device
    nodes = _state_nodes(state, m, dev)
    moves = []
    for (name, kind, t), (_, _, c) in zip(_node_items(cache), _node_items(state)):
        c = c.to(dev).contiguous()
        moves += [(s[0], d[0], d[1], d[2]) for s, d in zip(_regions(grid, kind, c), _regions(grid, kind, t))]
    grid_ops.stats_scatter_add(m, nodes, moves)
    for k, e, v in _present(state):
        if e.state == "copy":
            if torch.is_tensor(v):
                cache[k].copy_(v)
            else:
                cache[k] = v


def load_into_(cache, grid, state):
    """The statistics of `state` INTO the tensors `cache` (on `grid`) already holds: zeroed in place, then one scatter.  No pointer of the live
    cache changes, so a captured hyper step and a prepared streaming step keep valid addresses.  Everything is checked before anything is
    written (ValueError names the field; a ring on either side: NotImplementedError).  Root pairs and spectral factors go (zero_)."""
    _refuse(cache, "load_into_")
    _check_state(state)
    _check_fits(cache, grid, state, "load_into_")
    _fill(cache, grid, state, zero=True)
    return cache


def merge_into_(cache, grid, other, weight=1.0, n_other=None):
    """cache += weight x other, entry by entry as the table's `merge` column says: the statistics are additive, so the result describes both
    sets of points, the other's at noise d_i / weight.  `other` is a state (pack) or another cache on an equal grid; a cache is not packed
    first -- its touched nodes are selected and added straight from its full regions.  weight in (0, 1]; weight != 1 needs `n_other`, the
    number of points per output `other` holds (log|D| moves by -n_other log weight).  The probes of the two sides must come from different
    seeds (equal seeds would add the same random draws: cov(P) != A); the receiver keeps its seed and count.  Everything is checked before
    anything is written.  Root pairs and spectral factors of the receiver go."""
    weight = float(weight)
    if not (0.0 < weight <= 1.0):
        raise ValueError(f"merge_into_: weight must lie in (0, 1], got {weight}")
    if weight != 1.0 and n_other is None:
        raise ValueError("merge_into_: weight != 1 needs n_other, the number of points the other side holds (log|D| moves by -n_other log weight)")
    _refuse(cache, "merge_into_")
    is_state = isinstance(other, dict) and "format" in other
    if not is_state:
        if other is cache:
            raise ValueError("merge_into_: a cache cannot be merged into itself")
        state = _describe(other, _wtw_ops(other["WtW"])[0].grid)
    else:
        state = other
    _check_state(state)
    _check_fits(cache, grid, state, "merge_into_")
    if cache.get("path_probes") is not None and state["path_seed"] == cache["path_seed"]:
        raise ValueError(f"merge_into_: 'path_seed' is {state['path_seed']} on both sides: probes of equal seeds are the same random draws, and "
                         "their sum would no longer have covariance A -- build the two streams with different path_seed")
    m, dev = grid.m, cache["interpolation_cache"].device
    state = _tree_to(state, dev)
    factor = {"stencils": weight, "w": weight, "sqrt": math.sqrt(weight)}
    moves, select = [], []
    for (name, kind, t), (_, _, c) in zip(_node_items(cache), _node_items(state)):
        f = factor[ENTRIES[name.split("[")[0]].merge]
        src = _regions(grid, kind, c.contiguous())
        select += src
        moves += [(s[0], d[0], d[1], d[2], f) for s, d in zip(src, _regions(grid, kind, t))]
    if is_state:
        nodes = _state_nodes(state, m, dev)
    else:
        nodes, _ = grid_ops.stats_select(m, select)
    grid_ops.stats_scatter_add(m, nodes, moves, src_full=not is_state)
    for k, e, v in _present(state):
        if e.merge == "stats":                           # (a rounded product and a rounded add, as the kernel's)
            cache[k][:, 0] += v[:, 0] * weight
            cache[k][:, 1] += v[:, 1] - (0.0 if weight == 1.0 else float(n_other) * math.log(weight))
        elif e.merge == "w" and e.state == "copy":       # the trend's small fp64 sums
            cache[k] += v * weight
    for op in _wtw_ops(cache["WtW"]):
        op.root = op.inv_root = None                     # (L L^T described the receiver alone)
    cache.pop("_spectral", None)
    return cache
