"""Host: the kernel cache's table (online_gp_amd/models/kernel_cache.py) -- that it names every entry of a cache, and that
clone, decay_regions, regrid_plan and zero_ do to each entry what the table's contract says.  An 8 x 8 grid in fp64 on CPU tensors, every
group present, every tensor filled with distinct non-zero values; no kernel runs."""
import math

import pytest
import torch

from online_gp_amd import grid_ops
from online_gp_amd.lazy.operators import StencilWtW
from online_gp_amd.models import kernel_cache as kc
from kernel_cache_leaves import leaves as _leaves, snapshot as _snapshot, storages as _storages

S, SEED, CAP, GAMMA = 4, 11, 4, 0.75
F64 = dict(dtype=torch.float64, device="cpu")
CASES = [(out, probes, trend) for out in (1, 3) for probes in (False, True) for trend in (False, True)]
IDS = [f"out{o}{'-probes' if p else ''}{'-trend' if t else ''}" for o, p, t in CASES]


def _grid():
    return grid_ops.GridSpec([[-1.0, 1.0]] * 2, [8, 8])


class _Factor:
    """What clone() asks of a spectral factor."""

    def __init__(self, ref, stale):
        self.ref, self.stale = ref, stale

    def clone(self):
        return _Factor(self.ref, self.stale)


def _fill(cache):
    for i, (_, t) in enumerate(_leaves(cache)):
        vals = torch.arange(1, t.numel() + 1, dtype=torch.float64).reshape(t.shape)
        t.copy_(vals + 1000 * i if t.dtype == torch.int32 else vals / 7 + 1000 * (i + 1))


def _build(out, probes=True, trend=True, packed=True):
    g = _grid()
    cache = kc.fresh(g, out, torch.float64, "cpu", probes=(S, SEED) if probes else (0, 0), trend_deg=grid_ops.TREND_DEGREES["linear"] if trend else None)
    if not packed:                                        # operators with a tensor each: no [out, H, m] pack behind them
        cache["WtW"] = kc._wtw([StencilWtW(g, op.stencil.clone()) for op in kc._wtw_ops(cache["WtW"])])
    for op in kc._wtw_ops(cache["WtW"]):
        op.root, op.inv_root = torch.zeros((g.m, g.m), **F64), torch.zeros((g.m, g.m), **F64)
    cache["_ring"] = grid_ops.WindowRing(CAP, g.d, torch.float64, "cpu")
    cache["_site_ring"] = grid_ops.SiteRing(CAP, g.d, torch.float64, "cpu")
    cache["_site_ring"].head, cache["_site_ring"].fill, cache["_site_ring"].forms = 2, 3, {"interval"}
    cache["_ring"].head, cache["_ring"].fill = 1, 3
    if probes:
        cache["path_count"] = 17
    _fill(cache)
    return g, cache


def test_the_table_names_every_entry():
    g, cache = _build(3)
    cache["_spectral"] = {0: _Factor(1, False)}
    assert set(cache) <= set(kc.ENTRIES), f"entries without a row in kernel_cache.ENTRIES: {set(cache) - set(kc.ENTRIES)}"
    made = set(kc.fresh(g, 3, torch.float64, "cpu", probes=(S, SEED), trend_deg=1))
    assert made <= set(kc.ENTRIES)
    assert set(kc.ENTRIES) - made == {"_ring", "_site_ring", "_spectral"}       # (the model puts these in)
    for k, e in kc.ENTRIES.items():
        assert callable(e.move) or e.move in ("copy", "stencils", "spectral"), k
        assert e.decay in (None, "gamma", "sqrt", "mul", "stencils"), k
        assert e.regrid in ("keep", "rows", "cols", "stencils", "drop"), k
        assert e.zero in ("keep", "zero_", "clear", "drop", "stencils"), k


@pytest.mark.parametrize("out,probes,trend", CASES, ids=IDS)
def test_clone(out, probes, trend):
    g, cache = _build(out, probes, trend)
    cache["_spectral"] = {0: _Factor(1, False), 1: _Factor(None, False), 2: _Factor(1, True)}
    before = _snapshot(cache)
    new = kc.clone(cache, g)
    assert set(new) == set(cache)
    after = _snapshot(new)
    assert set(after) == set(before)
    for name, t in before.items():
        assert torch.equal(after[name], t), name
    assert not (_storages(new) & _storages(cache))
    ops = kc._wtw_ops(new["WtW"])
    assert len(ops) == out and all(op.root is not None and op.inv_root is not None for op in ops)
    if out == 3:
        pack = kc.stencil_pack(g, ops)
        assert pack is not None and pack.shape == (3, (g.R + 1) // 2, g.m)
    stats = new["_stats"]
    assert new["response_cache"].shape == (out, 1, 1) and new["D_logdet"].shape == (out,)
    stats += 1.0                                          # the views follow the clone's _stats, and the source does not
    assert torch.equal(new["response_cache"].reshape(-1), stats[:, 0]) and torch.equal(new["D_logdet"], stats[:, 1])
    assert torch.equal(cache["_stats"], before["_stats"]) and torch.equal(cache["response_cache"].reshape(-1), before["_stats"][:, 0])
    for k in ("_ring", "_site_ring"):
        assert new[k] is not cache[k] and type(new[k]) is type(cache[k])
        assert (new[k].head, new[k].fill, new[k].cap) == (cache[k].head, cache[k].fill, cache[k].cap)
    assert new["_site_ring"].forms == {"interval"} and new["_site_ring"].forms is not cache["_site_ring"].forms
    if probes:
        assert new["path_count"] == 17 and new["path_seed"] == SEED
    if trend:
        assert new["trend_deg"] == cache["trend_deg"] == 1
    # the spectral factors: those with a ref that are not stale, cloned; none of them -- no entry
    assert set(new["_spectral"]) == {0} and new["_spectral"][0] is not cache["_spectral"][0]
    cache["_spectral"] = {}
    assert "_spectral" not in kc.clone(cache, g)


@pytest.mark.parametrize("out,probes,trend", CASES, ids=IDS)
@pytest.mark.parametrize("packed", [True, False], ids=["pack", "separate"])
def test_decay_regions(out, probes, trend, packed):
    g, cache = _build(out, probes, trend, packed)
    before = _snapshot(cache)
    regions = kc.decay_regions(cache, g, GAMMA)
    ops = kc._wtw_ops(cache["WtW"])
    H = (g.R + 1) // 2
    if packed:                                            # the pack is ONE region
        want = [(ops[0].stencil.data_ptr(), out * H * g.m, GAMMA)]
    else:
        want = [(op.stencil.data_ptr(), H * g.m, GAMMA) for op in ops]
    want += [(cache["interpolation_cache"].data_ptr(), out * g.m, GAMMA), (cache["_cnt"].data_ptr(), out * g.m, GAMMA)]
    if probes:
        want.append((cache["path_probes"].data_ptr(), g.m * S, math.sqrt(GAMMA)))
    if trend:
        want.append((cache["trend_C"].data_ptr(), g.m * 3, GAMMA))
    assert [(t.data_ptr(), t.numel(), f) for t, f in regions] == want      # each once, in the order of the launches; no _stats, no constant
    after = _snapshot(cache)
    for name, t in before.items():
        if name in ("trend_G", "trend_g"):
            assert torch.equal(after[name], t * GAMMA), name
        else:
            assert torch.equal(after[name], t), name               # (the regions are scaled by the launch, not here)


def _region_key(reg):
    src, dst = reg[0], reg[1]
    return (src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel()) + tuple(reg[2:])


@pytest.mark.parametrize("out,probes,trend", CASES, ids=IDS)
def test_regrid_plan(out, probes, trend):
    g, cache = _build(out, probes, trend)
    cache["_spectral"] = {0: _Factor(1, False)}
    before, keys = _snapshot(cache), list(cache)
    new = g.shifted(1, 1)
    assert new.m == 100
    regions, fresh = kc.regrid_plan(cache, g, new)
    H = (g.R + 1) // 2
    ops, new_ops = kc._wtw_ops(cache["WtW"]), kc._wtw_ops(fresh["WtW"])
    assert len(new_ops) == out and all(op.grid is new and op.stencil.shape == (H, new.m) and op.root is None for op in new_ops)
    pack = kc.stencil_pack(new, new_ops)
    assert pack is not None and pack.shape == (out, H, new.m)
    want = []
    for o in range(out):
        want += grid_ops.stencil_regrid_regions(g, new, ops[o].stencil, new_ops[o].stencil, report=o)
    assert fresh["interpolation_cache"].shape == (out, new.m, 1) and fresh["_cnt"].shape == (out, new.m)
    want += [(cache["interpolation_cache"], fresh["interpolation_cache"], out, 1), (cache["_cnt"], fresh["_cnt"], out, 1)]
    if probes:
        assert fresh["path_probes"].shape == (new.m, S)
        want.append((cache["path_probes"], fresh["path_probes"], 1, S))
        assert fresh["path_seed"] == SEED and fresh["path_count"] == 17
    if trend:
        assert fresh["trend_C"].shape == (new.m, 3)
        want.append((cache["trend_C"], fresh["trend_C"], 1, 3))
        for k in ("trend_G", "trend_g", "trend_deg", "trend_center", "trend_scale"):
            assert fresh[k] is cache[k], k
    assert [_region_key(r) for r in regions] == [_region_key(r) for r in want]
    for k in ("_stats", "_ring", "_site_ring"):
        assert fresh[k] is cache[k], k
    assert fresh["response_cache"].data_ptr() == cache["_stats"].data_ptr() and fresh["D_logdet"].data_ptr() == cache["_stats"][:, 1].data_ptr()
    assert set(fresh) == set(keys) - {"_spectral"}
    # the source is untouched until the commit, which keeps the dict and empties the site ring only where nodes were removed
    assert list(cache) == keys and cache["_site_ring"].fill == 3
    after = _snapshot(cache)
    assert list(after) == list(before) and all(torch.equal(after[n], t) for n, t in before.items())
    held = cache
    kc.regrid_commit(cache, fresh, trimmed=False)
    assert cache is held and set(cache) == set(fresh) and cache["WtW"] is fresh["WtW"] and cache["_site_ring"].fill == 3
    kc.regrid_commit(cache, dict(cache), trimmed=True)
    assert cache["_site_ring"].fill == 0 and cache["_ring"].fill == 3


@pytest.mark.parametrize("out,probes,trend", CASES, ids=IDS)
def test_zero(out, probes, trend):
    g, cache = _build(out, probes, trend)
    cache["_spectral"] = {0: _Factor(1, False)}
    before = _snapshot(cache)
    kc.zero_(cache)
    after = _snapshot(cache)
    kept = ("path_probes", "trend_center", "trend_scale", "_ring.")
    for name, t in after.items():
        if name.startswith(kept):
            assert torch.equal(t, before[name]) and bool((t != 0).any()), name
        elif name == "_site_ring.3":                      # the noise of an empty slot
            assert bool((t == 1).all()), name
        else:
            assert not bool(t.any()), name
    assert not bool(cache["response_cache"].any()) and not bool(cache["D_logdet"].any())
    assert all(op.root is None and op.inv_root is None for op in kc._wtw_ops(cache["WtW"]))
    ring = cache["_site_ring"]
    assert (ring.head, ring.fill, ring.forms) == (0, 0, set())
    assert (cache["_ring"].head, cache["_ring"].fill) == (1, 3)
    assert "_spectral" not in cache
    if probes:
        assert cache["path_count"] == 17 and cache["path_seed"] == SEED
    if trend:
        assert cache["trend_deg"] == 1


@pytest.mark.parametrize("layout", ["half", "offset-major"])
def test_sparse_caches(layout):
    """What a caller may hand over: a literal dict without _cnt, probes, trend or rings; the stencil in the native half layout, or a full
    offset-major one."""
    g = _grid()
    rows = (g.R + 1) // 2 if layout == "half" else g.R
    stats = torch.zeros((1, 2), **F64)
    cache = {"interpolation_cache": torch.zeros((1, g.m, 1), **F64), "_stats": stats, "response_cache": stats[:, 0].view(1, 1, 1),
             "D_logdet": stats[:, 1], "WtW": StencilWtW(g, torch.zeros((rows, g.m), **F64))}
    _fill(cache)
    before = _snapshot(cache)
    new = kc.clone(cache, g)
    assert set(new) == set(cache) and "_cnt" not in new and not (_storages(new) & _storages(cache))
    assert all(torch.equal(t, before[n]) for n, t in _snapshot(new).items())
    regions = kc.decay_regions(cache, g, GAMMA)
    assert [(t.data_ptr(), f) for t, f in regions] == [(cache["WtW"].stencil.data_ptr(), GAMMA), (cache["interpolation_cache"].data_ptr(), GAMMA)]
    g2 = g.shifted(1, 1)
    regions, fresh = kc.regrid_plan(cache, g, g2)
    assert set(fresh) == set(cache) and "_cnt" not in fresh
    assert fresh["WtW"].stencil.shape == (rows, g2.m)                 # regridded in its own layout
    want = grid_ops.stencil_regrid_regions(g, g2, cache["WtW"].stencil, fresh["WtW"].stencil, report=0)
    want.append((cache["interpolation_cache"], fresh["interpolation_cache"], 1, 1))
    assert [_region_key(r) for r in regions] == [_region_key(r) for r in want] and len(want) == (3 if layout == "half" else 2)
    assert all(torch.equal(t, before[n]) for n, t in _snapshot(cache).items())
    kc.zero_(cache)
    assert not any(bool(t.any()) for _, t in _leaves(cache)) and "_cnt" not in cache
