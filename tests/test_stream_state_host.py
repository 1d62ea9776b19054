"""Host: checkpoint, restore and merge of a kernel cache (online_gp_amd/models/kernel_cache.py) on CPU tensors -- the two
new columns of the table, pack -> torch.save -> torch.load(weights_only=True) -> unpack, load_into_, merge_into_ against the independent
reference of tests/stream_state_reference.py, and the refusals.  An 8 x 8 grid, every tensor filled with distinct non-zero values, then
zeroed outside a chosen node set; no kernel runs (the three grid_ops.stats_* functions take their torch path)."""
import math

import numpy as np
import pytest
import torch

from online_gp_amd import grid_ops
from online_gp_amd.lazy.operators import StencilWtW
from online_gp_amd.models import kernel_cache as kc
from kernel_cache_leaves import leaves as _leaves, snapshot as _snapshot
import stream_state_reference as ref

S, SEED, CAP = 4, 11, 4
CASES = [(out, probes, trend) for out in (1, 3) for probes in (False, True) for trend in (False, True)]
IDS = [f"out{o}{'-probes' if p else ''}{'-trend' if t else ''}" for o, p, t in CASES]
NODE_SETS = ["none", "all", "ends", "last-slot", "b-only", "nan"]


def _grid():
    return grid_ops.GridSpec([[-1.0, 1.0]] * 2, [8, 8])


def _fill(cache, shift=0.0):
    for i, (_, t) in enumerate(_leaves(cache)):
        vals = torch.arange(1, t.numel() + 1, dtype=torch.float64).reshape(t.shape)
        t.copy_(vals / 7 + 1000 * (i + 1) + shift)


def _build(out=1, probes=True, trend=True, packed=True, dtype=torch.float64, layout="half", s=S, seed=SEED, deg=1, shift=0.0):
    """The cache of tests/test_kernel_cache_host.py::_build, restated, without the rings a state refuses."""
    g = _grid()
    cache = kc.fresh(g, out, dtype, "cpu", probes=(s, seed) if probes else (0, 0), trend_deg=deg if trend else None)
    if layout != "half":
        cache["WtW"] = kc._wtw([StencilWtW(g, torch.zeros((g.R, g.m), dtype=dtype)) for _ in range(out)])
    elif not packed:                                      # operators with a tensor each: no [out, H, m] pack behind them
        cache["WtW"] = kc._wtw([StencilWtW(g, op.stencil.clone()) for op in kc._wtw_ops(cache["WtW"])])
    if probes:
        cache["path_count"] = 17
    centre, scale = (cache["trend_center"].clone(), cache["trend_scale"].clone()) if trend else (None, None)
    _fill(cache, shift)
    if trend:                                             # (the frame belongs to the grid: two caches of one grid share it)
        cache["trend_center"].copy_(centre)
        cache["trend_scale"].copy_(scale)
    return g, cache


def _node_views(cache, g):
    """[k, m, w] views of every node region of the cache, by the layout rules of the issue (restated: not kernel_cache's walker)."""
    m, H = g.m, (g.R + 1) // 2
    views = []
    for op in kc._wtw_ops(cache["WtW"]):
        flat = op.stencil.reshape(-1)
        if op.stencil.shape[0] == H:
            views += [flat[:4 * m].view(1, m, 4), flat[4 * m:].view((H - 4) // 7, m, 7)]
        else:
            views.append(flat.view(g.R, m, 1))
    out = cache["interpolation_cache"].shape[0]
    views.append(cache["interpolation_cache"].view(out, m, 1))
    if "_cnt" in cache:
        views.append(cache["_cnt"].view(out, m, 1))
    for k in ("path_probes", "trend_C"):
        if k in cache:
            views.append(cache[k].view(1, m, -1))
    return views


def _restrict(cache, g, node_set):
    """Zero the cache outside the chosen node set; returns the expected node list (None: every node)."""
    m = g.m
    if node_set == "all":
        return None
    keep = {"none": [], "ends": [0, m - 1], "last-slot": [9], "b-only": [9], "nan": [9, 20]}[node_set]
    mask = torch.ones(m, dtype=torch.bool)
    mask[keep] = False
    for v in _node_views(cache, g):
        v[:, mask, :] = 0
    last = kc._wtw_ops(cache["WtW"])[-1].stencil.reshape(-1)
    if node_set == "last-slot":                           # node 17: only the last slot of the last group of the last output
        last[last.numel() - m * 7 + 17 * 7 + 6] = 3.5
        return [9, 17]
    if node_set == "b-only":
        cache["interpolation_cache"][0, 23, 0] = -2.25
        return [9, 23]
    if node_set == "nan":
        target = cache["_cnt"] if "_cnt" in cache else cache["interpolation_cache"]
        target.view(-1, m)[0, 41] = float("nan")
        return [9, 20, 41]
    return keep


def _same(a, b):
    """torch.equal, with a NaN equal to a NaN at the same place."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num())


def _assert_unchanged(cache, before):
    after = _snapshot(cache)
    assert list(after) == list(before)
    for name, t in before.items():
        assert _same(after[name], t), name


def _round_trip(state, tmp_path):
    torch.save(state, tmp_path / "state.pt")
    return torch.load(tmp_path / "state.pt", weights_only=True)


def test_the_table_has_the_two_columns():
    assert kc.Entry._fields == ("move", "decay", "regrid", "zero", "state", "merge")
    for k, e in kc.ENTRIES.items():
        assert e.state in ("stencils", "rows", "cols", "copy", "view", "refuse", "drop"), k
        assert e.merge in ("stencils", "w", "sqrt", "stats", "keep", "equal", "view", "refuse", "drop"), k
        assert (e.state in ("stencils", "rows", "cols")) == (e.regrid in ("stencils", "rows", "cols")), k     # a node region is one everywhere
        # the old columns, as tests/test_kernel_cache_host.py states them
        assert callable(e.move) or e.move in ("copy", "stencils", "spectral"), k
        assert e.decay in (None, "gamma", "sqrt", "mul", "stencils"), k
        assert e.regrid in ("keep", "rows", "cols", "stencils", "drop"), k
        assert e.zero in ("keep", "zero_", "clear", "drop", "stencils"), k
    want = {"WtW": ("stencils", "stencils"), "interpolation_cache": ("rows", "w"), "_cnt": ("rows", "w"), "_stats": ("copy", "stats"),
            "response_cache": ("view", "view"), "D_logdet": ("view", "view"), "path_probes": ("cols", "sqrt"), "path_seed": ("copy", "keep"),
            "path_count": ("copy", "keep"), "trend_C": ("cols", "w"), "trend_G": ("copy", "w"), "trend_g": ("copy", "w"),
            "trend_deg": ("copy", "equal"), "trend_center": ("copy", "equal"), "trend_scale": ("copy", "equal"), "_ring": ("refuse", "refuse"),
            "_site_ring": ("refuse", "refuse"), "_spectral": ("drop", "drop")}
    assert {k: (e.state, e.merge) for k, e in kc.ENTRIES.items()} == want
    old = {"WtW": ("stencils",) * 4, "interpolation_cache": ("copy", "gamma", "rows", "zero_"), "_cnt": ("copy", "gamma", "rows", "zero_"),
           "_stats": ("copy", None, "keep", "zero_"), "path_probes": ("copy", "sqrt", "cols", "keep"), "trend_C": ("copy", "gamma", "cols", "zero_"),
           "trend_G": ("copy", "mul", "keep", "zero_"), "trend_g": ("copy", "mul", "keep", "zero_"), "_site_ring": ("copy", None, "keep", "clear"),
           "_spectral": ("spectral", None, "drop", "drop")}
    const = ("copy", None, "keep", "keep")
    for k, e in kc.ENTRIES.items():
        if not callable(e.move):
            assert tuple(e[:4]) == old.get(k, const), k
        else:
            assert tuple(e[1:4]) == (None, "keep", "keep"), k


@pytest.mark.parametrize("node_set", NODE_SETS)
@pytest.mark.parametrize("packed", [True, False], ids=["pack", "separate"])
@pytest.mark.parametrize("out,probes,trend", CASES, ids=IDS)
def test_pack_save_load_unpack(out, probes, trend, packed, node_set, tmp_path):
    g, cache = _build(out, probes, trend, packed)
    for op in kc._wtw_ops(cache["WtW"]):                  # root pairs are not carried
        op.root = torch.ones((g.m, g.m), dtype=torch.float64)
    want_nodes = _restrict(cache, g, node_set)
    before = _snapshot(cache)
    state = kc.pack(cache, g)
    _assert_unchanged(cache, before)
    if want_nodes is None:
        assert state["nodes"] is None
    else:
        assert state["nodes"].dtype == torch.int32 and state["nodes"].tolist() == want_nodes
        # against the reference's select and gather
        regs = [(v.reshape(-1).numpy(), v.shape[0], v.shape[2]) for v in _node_views(cache, g)]
        assert ref.select(g.m, regs).tolist() == want_nodes
        b = cache["interpolation_cache"].reshape(-1).numpy()
        got = state["interpolation_cache"].reshape(-1).numpy()
        assert np.array_equal(ref.gather(g.m, want_nodes, b, out, 1), got, equal_nan=True)
    n_sel = g.m if want_nodes is None else len(want_nodes)
    assert state["WtW"].shape == (out, (g.R + 1) // 2, n_sel) and state["interpolation_cache"].shape == (out, n_sel, 1)
    assert state["layout"] == "half" and state["num_outputs"] == out and state["dtype"] == "torch.float64"
    assert state["grid"] == {"bounds": g.grid_bounds, "size": g.g, "g0": g.g0, "h": g.h}
    g2, new = kc.unpack(_round_trip(state, tmp_path), "cpu")
    assert (g2.g, g2.g0, g2.h) == (g.g, g.g0, g.h)
    after = _snapshot(new)
    assert set(after) == {n for n in before if not n.endswith("root")}
    for name, t in after.items():
        assert _same(t, before[name]), name
    assert all(op.root is None for op in kc._wtw_ops(new["WtW"]))
    assert torch.equal(new["response_cache"].reshape(-1), new["_stats"][:, 0]) and new["D_logdet"].data_ptr() == new["_stats"][:, 1].data_ptr()
    if probes:
        assert (new["path_seed"], new["path_count"]) == (SEED, 17)
    if trend:
        assert new["trend_deg"] == 1


@pytest.mark.parametrize("layout", ["half", "offset-major"])
def test_sparse_cache_round_trip(layout, tmp_path):
    """A caller's own cache: no _cnt, no probes, no trend; the native half stencil or a full offset-major one."""
    g, cache = _build(1, False, False, layout=layout)
    cache.pop("_cnt")
    _restrict(cache, g, "ends")
    before = _snapshot(cache)
    state = _round_trip(kc.pack(cache, g), tmp_path)
    assert state["layout"] == layout and "_cnt" not in state and state["nodes"].tolist() == [0, g.m - 1]
    assert state["WtW"].shape == (1, (g.R + 1) // 2 if layout == "half" else g.R, 2)
    _, new = kc.unpack(state, "cpu")
    assert "_cnt" not in new
    _assert_unchanged(new, before)


@pytest.mark.parametrize("out,probes,trend", CASES, ids=IDS)
def test_load_into_keeps_every_pointer(out, probes, trend):
    g, src = _build(out, probes, trend, shift=0.5)
    _restrict(src, g, "nan")
    state = kc.pack(src, g)
    _, live = _build(out, probes, trend, seed=SEED + 1)
    for op in kc._wtw_ops(live["WtW"]):
        op.root = op.inv_root = torch.ones((g.m, g.m), dtype=torch.float64)
    live["_spectral"] = {0: object()}
    ptrs = {name: t.data_ptr() for name, t in _leaves(live) if not name.endswith("root")}
    views = (live["response_cache"], live["D_logdet"])
    assert kc.load_into_(live, g, state) is live
    assert {name: t.data_ptr() for name, t in _leaves(live)} == ptrs
    _assert_unchanged(live, _snapshot(src))
    assert live["response_cache"] is views[0] and torch.equal(views[1], src["_stats"][:, 1])
    assert "_spectral" not in live and all(op.root is None and op.inv_root is None for op in kc._wtw_ops(live["WtW"]))
    if probes:
        assert (live["path_seed"], live["path_count"]) == (SEED, 17)


@pytest.mark.parametrize("form", ["state", "cache"])
@pytest.mark.parametrize("weight", [1.0, 0.5])
@pytest.mark.parametrize("out,probes,trend", CASES, ids=IDS)
def test_merge_into_matches_the_reference(out, probes, trend, weight, form):
    g, mine = _build(out, probes, trend)
    _, other = _build(out, probes, trend, seed=SEED + 1, shift=0.25)
    _restrict(mine, g, "ends")
    _restrict(other, g, "nan")
    n_other = 13
    a, b = _snapshot(mine), _snapshot(other)
    want = {name: ref.merge_leaf(name, t.numpy(), b[name].numpy(), weight, n_other) for name, t in a.items()}
    ptrs = {name: t.data_ptr() for name, t in _leaves(mine)}
    kc.merge_into_(mine, g, kc.pack(other, g) if form == "state" else other, weight, n_other)
    _assert_unchanged(other, b)
    assert {name: t.data_ptr() for name, t in _leaves(mine)} == ptrs
    got = _snapshot(mine)
    for name, t in want.items():
        assert np.array_equal(got[name].numpy(), t, equal_nan=True), name
    # what the rules say in numbers: log|D| moves by -n log w beyond the plain sum, the probes by sqrt(w)
    assert torch.equal(got["_stats"][:, 1], a["_stats"][:, 1] + (b["_stats"][:, 1] - (n_other * math.log(weight) if weight != 1.0 else 0.0)))
    if probes:
        assert torch.equal(got["path_probes"][9], a["path_probes"][9] + b["path_probes"][9] * math.sqrt(weight))
        assert (mine["path_seed"], mine["path_count"]) == (SEED, 17)


def test_merge_needs_the_count_for_a_weight():
    g, mine = _build()
    _, other = _build(seed=SEED + 1)
    before = _snapshot(mine)
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="weight"):
            kc.merge_into_(mine, g, other, bad, 5)
    with pytest.raises(ValueError, match="n_other"):
        kc.merge_into_(mine, g, other, 0.5)
    with pytest.raises(ValueError, match="itself"):
        kc.merge_into_(mine, g, mine)
    _assert_unchanged(mine, before)


def _other_state(**kw):
    g, other = _build(**{"seed": SEED + 1, **kw})
    _restrict(other, g, "ends")
    return kc.pack(other, g)


def _edit(state, **changes):
    state = dict(state)
    state.update(changes)
    return state


def _ulp_up(gd):
    gd = {k: list(v) for k, v in gd.items()}
    gd["h"][0] = math.nextafter(gd["h"][0], math.inf)
    return gd


REFUSALS = {
    "grid": (lambda: _edit(_other_state(), grid=_ulp_up(_other_state()["grid"])), ValueError, "grid"),
    "dtype": (lambda: _other_state(dtype=torch.float32), ValueError, "dtype"),
    "num_outputs": (lambda: _other_state(out=3, probes=False, trend=False), ValueError, "num_outputs"),
    "layout": (lambda: _other_state(layout="offset-major"), ValueError, "layout"),
    "S": (lambda: _other_state(s=6), ValueError, "path_probes"),
    "trend-degree": (lambda: _other_state(deg=2), ValueError, "trend_deg"),
    "no-trend": (lambda: _other_state(trend=False), ValueError, "trend_C"),
    "format": (lambda: _edit(_other_state(), format="something else"), ValueError, "format"),
    "version": (lambda: _edit(_other_state(), version=99), ValueError, "version"),
    "nodes-descending": (lambda: _edit(_other_state(), nodes=torch.tensor([63, 0], dtype=torch.int32)), ValueError, "nodes"),
    "nodes-duplicated": (lambda: _edit(_other_state(), nodes=torch.tensor([5, 5], dtype=torch.int32)), ValueError, "nodes"),
    "nodes-negative": (lambda: _edit(_other_state(), nodes=torch.tensor([-1, 5], dtype=torch.int32)), ValueError, "nodes"),
    "nodes-too-large": (lambda: _edit(_other_state(), nodes=torch.tensor([5, 64], dtype=torch.int32)), ValueError, "nodes"),
    "nodes-dtype": (lambda: _edit(_other_state(), nodes=torch.tensor([0, 63], dtype=torch.int64)), ValueError, "nodes"),
    "shape": (lambda: _edit(_other_state(), _cnt=_other_state()["_cnt"][:, :1].contiguous()), ValueError, "_cnt"),
    "shape-stencil": (lambda: _edit(_other_state(), WtW=_other_state()["WtW"][:, :-1].contiguous()), ValueError, "WtW"),
    "ring": (lambda: _edit(_other_state(), _ring=[1]), NotImplementedError, "_ring"),
}


@pytest.mark.parametrize("op", ["load", "merge"])
@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_leave_the_receiver_untouched(case, op):
    make, exc, field = REFUSALS[case]
    g, live = _build()
    before = _snapshot(live)
    with pytest.raises(exc, match=field):
        if op == "load":
            kc.load_into_(live, g, make())
        else:
            kc.merge_into_(live, g, make(), 1.0, 3)
    _assert_unchanged(live, before)
    assert (live["path_seed"], live["path_count"]) == (SEED, 17)


def test_refusals_of_caches_and_seeds():
    g, live = _build()
    before = _snapshot(live)
    with pytest.raises(ValueError, match="path_seed"):            # equal seeds: the same random draws
        kc.merge_into_(live, g, _other_state(seed=SEED))
    _, twin = _build()
    with pytest.raises(ValueError, match="path_seed"):
        kc.merge_into_(live, g, twin)
    _, ringed = _build(seed=SEED + 1)
    for key, ring in (("_ring", grid_ops.WindowRing(CAP, g.d, torch.float64, "cpu")), ("_site_ring", grid_ops.SiteRing(CAP, g.d, torch.float64, "cpu"))):
        ringed[key] = ring
        with pytest.raises(NotImplementedError, match=key):
            kc.merge_into_(live, g, ringed)
        with pytest.raises(NotImplementedError, match=key):
            kc.pack(ringed, g)
        ringed.pop(key)
        live[key] = ring                                          # ... and on the receiving side
        for call in (lambda: kc.merge_into_(live, g, ringed), lambda: kc.load_into_(live, g, _other_state()), lambda: kc.pack(live, g)):
            with pytest.raises(NotImplementedError, match=key):
                call()
        live.pop(key)
    _, other32 = _build(dtype=torch.float32, seed=SEED + 1)       # another cache, not a state: the same checks
    with pytest.raises(ValueError, match="dtype"):
        kc.merge_into_(live, g, other32)
    _assert_unchanged(live, before)
