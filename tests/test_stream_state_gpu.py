"""GPU: checkpoint, restore and merge of a live model through its touched nodes.

The three kernels (wiski_stats_select / _gather / _scatter_add) bit for bit against the plain loops of tests/stream_state_reference.py,
in an arena with 3-word guards that puts most regions off a 16-byte boundary and shows a write outside a region; then
``FixedNoiseOnlineSKIGP.stream_state`` / ``load_stream_state_`` / ``merge_`` and the wrappers' pair against the leaves of the source
(bit for bit: a restore is a scatter into zeros, a merge one rounded add per element) and against oracle/dataspace.py.

Tolerances of the oracle comparisons are the ones tests/test_regrid_gpu.py applies to its own model-against-oracle comparisons, which
it takes from tests/test_model_gpu.py (RTOL: mean and variance, 1e-4 in fp64 and 1e-2 in fp32) and tests/test_mll_gpu.py (MLL: 1e-6
dense in fp64, 5e-2 matrix-free; fp32 dense at RTOL as test_regrid_fp32 does).  A model that went on absorbing after a restore is
compared at a tolerance, not bit for bit: the absorb adds with atomics, in an order that differs from run to run.  Every comparison
prints its figures before it asserts.

Measured on an MI355X (run with -s): kernel cases 0 differing words; restored and merged models against the oracle at most 2.0e-8 mean /
1.5e-7 variance / 4.4e-8 MLL in fp64 and 7.2e-7 / 7.6e-7 / 1.9e-7 in fp32, both regimes; trend after a merge 4e-14 in beta; paths of a
restored model 7.5e-16 from the source's, merged probes 5.1e-8 against a mean deviation of 2.4e-8 (ratio 2.1, bound 3); the captured
hyper step: 3 replays before the restore, 9 after."""
import ctypes
import math

import numpy as np
import pytest
import torch

import stream_state_reference as ref
from kernel_cache_leaves import leaves as _leaves, snapshot as _snapshot
from oracle import dataspace

pytestmark = pytest.mark.gpu
DEV = "cuda"
NP = {torch.float32: np.float32, torch.float64: np.float64}
RTOL = {torch.float64: 1e-4, torch.float32: 1e-2}       # tests/test_regrid_gpu.py, from tests/test_model_gpu.py
MLL_DENSE, MLL_MATRIX_FREE = 1e-6, 5e-2                  # tests/test_regrid_gpu.py, from tests/test_mll_gpu.py
GUARD = 3
# the noise-weight sum rebuilt from cnt against the one the source kept (an fp64 sum of the weights): every cnt entry is a sum of at most n
# positive terms in the working precision, each add rounded once, so the total is off by at most n eps / 2 relative -- n = 128: 8e-6 in
# fp32, 1.4e-14 in fp64
WSUM_RTOL = {torch.float64: 1e-12, torch.float32: 1e-5}


# ------------------------------------------------------------------------------------------------------------ the kernels
GRIDS = {"d1_g8": [8], "8x8": [8, 8], "6x5x7": [6, 5, 7], "5x5x5x4": [5, 5, 5, 4], "40x37": [40, 37], "d1_g70001": [70001]}
KERNEL_CASES = [(name, out) for name in GRIDS for out in ((1, 3) if name in ("8x8", "6x5x7", "40x37") else (1,))]
NODE_SETS = ["none", "all", "ends", "last-slot", "b-only", "nan", "every-second", "one-per-block"]
S_PROBES, P_TREND = 4, 3


def _pack_layout(g, out):
    """(name, k, w) of the node regions of a cache of `out` outputs on a grid of sizes g, in the native half-stencil layout: per output group 0
    (k = 1, w = 4) and, for d > 1, the groups >= 1 (w = 7); b and cnt (k = out, w = 1); probes (w = S); trend_C (w = p)."""
    H = (7 ** len(g) + 1) // 2
    regs = []
    for o in range(out):
        regs.append((f"A{o}g0", 1, 4))
        if H > 4:
            regs.append((f"A{o}g1", (H - 4) // 7, 7))
    return regs + [("b", out, 1), ("cnt", out, 1), ("probes", 1, S_PROBES), ("trend_C", 1, P_TREND)]


def _host_regions(layout, m, npdt, seed):
    rng = np.random.default_rng(seed)
    return {name: (rng.standard_normal(k * m * w) * 3.0).astype(npdt) for name, k, w in layout}


def _restrict(host, layout, m, node_set):
    """Zero the host regions outside the node set (the sets of tests/test_stream_state_host.py and two more)."""
    if node_set == "all":
        return
    keep = {"none": [], "ends": [0, m - 1], "last-slot": [5], "b-only": [5], "nan": [5, 6], "every-second": list(range(0, m, 2)),
            "one-per-block": list(range(7, m, 256))}[node_set]
    mask = np.ones(m, dtype=bool)
    mask[keep] = False
    for name, k, w in layout:
        host[name].reshape(k, m, w)[:, mask, :] = 0
    stencils = [(name, k, w) for name, k, w in layout if name.startswith("A")]
    if node_set == "last-slot":                           # node 3: only the last slot of the last group of the last output
        name, k, w = stencils[-1]
        host[name].reshape(k, m, w)[k - 1, 3, w - 1] = 3.5
    elif node_set == "b-only":
        host["b"].reshape(-1, m)[0, 2] = -2.25
    elif node_set == "nan":
        host["cnt"].reshape(-1, m)[-1, 1] = np.nan


def _arena(parts, dtype, fill=None):
    """One device buffer that holds the named flat arrays, each between 3-word guards (odd lengths and the guards put most regions off a
    16-byte boundary).  -> (arena, {name: view}, host copy of the arena)"""
    off, where = GUARD, {}
    for name, a in parts:
        where[name] = (off, a.shape[0])
        off += a.shape[0] + GUARD
    host = np.full(off, -77.0, dtype=NP[dtype])
    for name, a in parts:
        o, n = where[name]
        host[o:o + n] = a if fill is None else fill
    dev = torch.as_tensor(host, device=DEV)
    return dev, {name: dev[o:o + n] for name, (o, n) in where.items()}, host


def _guards_intact(dev, host, views):
    """Everything of the arena outside the named views is what it was."""
    mask = np.ones(host.shape[0], dtype=bool)
    base = dev.data_ptr()
    for v in views.values():
        o = (v.data_ptr() - base) // dev.element_size()
        mask[o:o + v.numel()] = False
    return np.array_equal(dev.cpu().numpy()[mask], host[mask])


def _eq(got, want):
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def _run_case(g, out, dtype, node_set, seed):
    from online_gp_amd import grid_ops

    m = math.prod(g)
    layout = _pack_layout(g, out)
    host = _host_regions(layout, m, NP[dtype], seed)
    _restrict(host, layout, m, node_set)
    src_dev, src, src_host = _arena([(n, host[n]) for n, _, _ in layout], dtype)
    # ---- select
    nodes, n_sel = grid_ops.stats_select(m, [(src[n], k, w) for n, k, w in layout])
    want_nodes = ref.select(m, [(host[n], k, w) for n, k, w in layout])
    assert nodes.dtype == torch.int32 and n_sel == len(want_nodes) == nodes.numel()
    assert np.array_equal(nodes.cpu().numpy(), want_nodes)
    # ---- gather
    cmp_dev, cmp, cmp_host = _arena([(n, np.zeros(k * n_sel * w, dtype=NP[dtype])) for n, k, w in layout], dtype, fill=-5.0)
    err = grid_ops.new_err_flag(DEV)
    grid_ops.stats_gather(m, nodes, [(src[n], cmp[n], k, w) for n, k, w in layout], err=err)
    compact = {n: ref.gather(m, want_nodes, host[n], k, w) for n, k, w in layout}
    for n, _, _ in layout:
        assert _eq(cmp[n].cpu().numpy(), compact[n]), ("gather", n)
    assert _guards_intact(cmp_dev, cmp_host, cmp) and np.array_equal(src_dev.cpu().numpy(), src_host, equal_nan=True)
    # ---- scatter_add: factor 1 everywhere; factor 0.5 (0.7 on the probes: not a power of two) ; straight from the full regions
    base = _host_regions(layout, m, NP[dtype], seed + 1)
    for label, fac, full in (("f=1", lambda n: 1.0, False), ("f=0.5", lambda n: 0.7 if n == "probes" else 0.5, False), ("full", lambda n: 0.5, True)):
        dst_dev, dst, dst_host = _arena([(n, base[n]) for n, _, _ in layout], dtype)
        grid_ops.stats_scatter_add(m, nodes, [((src if full else cmp)[n], dst[n], k, w, fac(n)) for n, k, w in layout], err=err, src_full=full)
        for n, k, w in layout:
            want = ref.scatter_add(m, want_nodes, base[n], host[n] if full else compact[n], k, w, fac(n), src_full=full)
            assert _eq(dst[n].cpu().numpy(), want), ("scatter_add", label, n)
        assert _guards_intact(dst_dev, dst_host, dst)
    assert int(err.item()) == 0
    return n_sel


@pytest.mark.parametrize("node_set", NODE_SETS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("grid,out", KERNEL_CASES, ids=[f"{n}-out{o}" for n, o in KERNEL_CASES])
def test_kernels_bit_for_bit(grid, out, dtype, node_set):
    g = GRIDS[grid]
    m = math.prod(g)
    n_sel = _run_case(g, out, dtype, node_set, seed=len(grid) + out)
    want = {"none": 0, "all": m, "ends": 2, "last-slot": 2, "b-only": 2, "nan": 3, "every-second": (m + 1) // 2, "one-per-block": len(range(7, m, 256))}
    assert n_sel == want[node_set]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_offset_major_stencil_and_a_plan_beyond_16_regions(dtype):
    """An offset-major stencil [49, m] (k = 49, w = 1) and 19 more regions: 20 in all, two calls of each entry; the nodes one part alone
    would select differ from the other's, so the flags must accumulate."""
    from online_gp_amd import grid_ops

    m = 64
    layout = [("om", 49, 1)] + [(f"v{i}", 1 + i % 3, 1 + i % 5) for i in range(19)]
    host = _host_regions(layout, m, NP[dtype], 5)
    for i, (name, k, w) in enumerate(layout):             # region i holds something at nodes 3 i and 3 i + 1 only
        mask = np.ones(m, dtype=bool)
        mask[[3 * i, 3 * i + 1]] = False
        host[name].reshape(k, m, w)[:, mask, :] = 0
    _, src, _ = _arena([(n, host[n]) for n, _, _ in layout], dtype)
    nodes, n_sel = grid_ops.stats_select(m, [(src[n], k, w) for n, k, w in layout])
    want_nodes = ref.select(m, [(host[n], k, w) for n, k, w in layout])
    assert n_sel == 40 and np.array_equal(nodes.cpu().numpy(), want_nodes)
    cmp_dev, cmp, cmp_host = _arena([(n, np.zeros(k * n_sel * w, dtype=NP[dtype])) for n, k, w in layout], dtype, fill=-5.0)
    grid_ops.stats_gather(m, nodes, [(src[n], cmp[n], k, w) for n, k, w in layout])
    base = _host_regions(layout, m, NP[dtype], 6)
    dst_dev, dst, dst_host = _arena([(n, base[n]) for n, _, _ in layout], dtype)
    grid_ops.stats_scatter_add(m, nodes, [(cmp[n], dst[n], k, w, 0.5 if i % 2 else 1.0) for i, (n, k, w) in enumerate(layout)])
    for i, (n, k, w) in enumerate(layout):
        compact = ref.gather(m, want_nodes, host[n], k, w)
        assert _eq(cmp[n].cpu().numpy(), compact), n
        assert _eq(dst[n].cpu().numpy(), ref.scatter_add(m, want_nodes, base[n], compact, k, w, 0.5 if i % 2 else 1.0)), n
    assert _guards_intact(cmp_dev, cmp_host, cmp) and _guards_intact(dst_dev, dst_host, dst)


def test_a_bad_node_list_is_skipped_and_flagged():
    """Indices outside [0, m) never reach an address: their elements are skipped, bit 0 of err is set, the rest moves."""
    from online_gp_amd import grid_ops

    m, k, w = 40, 2, 4
    rng = np.random.default_rng(3)
    a = rng.standard_normal(k * m * w)
    nodes = torch.tensor([3, -1, m, 5, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    _, src, _ = _arena([("a", a)], torch.float64)
    cmp_dev, cmp, cmp_host = _arena([("a", np.zeros(k * 5 * w))], torch.float64, fill=-5.0)
    err = grid_ops.new_err_flag(DEV)
    grid_ops.stats_gather(m, nodes, [(src["a"], cmp["a"], k, w)], err=err)
    got = cmp["a"].cpu().numpy().reshape(k, 5, w)
    full = a.reshape(k, m, w)
    assert int(err.item()) == 1
    assert np.array_equal(got[:, 0], full[:, 3]) and np.array_equal(got[:, 3], full[:, 5]) and bool((got[:, [1, 2, 4]] == -5.0).all())
    assert _guards_intact(cmp_dev, cmp_host, cmp)
    err.zero_()
    base = rng.standard_normal(k * m * w)
    dst_dev, dst, dst_host = _arena([("a", base)], torch.float64)
    comp = rng.standard_normal(k * 5 * w)
    _, cv, _ = _arena([("a", comp)], torch.float64)
    grid_ops.stats_scatter_add(m, nodes, [(cv["a"], dst["a"], k, w, 0.5)], err=err)
    want = base.copy().reshape(k, m, w)
    for j, i in ((0, 3), (3, 5)):
        want[:, i] = want[:, i] + comp.reshape(k, 5, w)[:, j] * 0.5
    assert int(err.item()) == 1 and np.array_equal(dst["a"].cpu().numpy(), want.reshape(-1)) and _guards_intact(dst_dev, dst_host, dst)


def test_entries_refuse_bad_arguments():
    """WISKI_E_BADARG (-1) before anything is launched; a short workspace is WISKI_E_WORKSPACE (-3); n_sel = 0 is WISKI_OK and launches nothing."""
    from online_gp_amd import _hip

    m, n_sel = 300, 10
    z = lambda n, dt=torch.float64: torch.zeros(n, dtype=dt, device=DEV)
    a, c, d = z(2 * m * 4 + 1), z(2 * n_sel * 4 + 1), z(2 * m * 4)
    flags, nodes, count, work = z(m, torch.int32), z(m, torch.int32), z(1, torch.int32), z(2, torch.int32)
    nodes[:n_sel] = torch.arange(n_sel, dtype=torch.int32)
    st = _hip.stream_ptr(DEV)
    P = lambda t: t.data_ptr()

    def plan(src, dst, k=2, w=4, f=1.0, count=1):
        p = _hip.wiski_stats_plan()
        p.count = count
        p.src[0], p.dst[0], p.k[0], p.w[0], p.factor[0] = src, dst, k, w, f
        return ctypes.byref(p)

    i64, i32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    for sfx in ("_f64", "_f32"):
        sel = getattr(_hip.lib(), "wiski_stats_select" + sfx)
        gat = getattr(_hip.lib(), "wiski_stats_gather" + sfx)
        sca = getattr(_hip.lib(), "wiski_stats_scatter_add" + sfx)
        select = lambda p, mm=m, fl=P(flags), nd=P(nodes), ct=P(count), wk=P(work), we=2: sel(p, i64(mm), vp(fl), vp(nd), vp(ct), vp(wk), i64(we), st)
        gather = lambda p, mm=m, nd=P(nodes), ns=n_sel: gat(p, i64(mm), vp(nd), i64(ns), None, st)
        scatter = lambda p, mm=m, nd=P(nodes), ns=n_sel, full=0: sca(p, i64(mm), vp(nd), i64(ns), i32(full), None, st)
        bad = [select(None), select(plan(P(a), None, count=17)), select(plan(None, None)), select(plan(P(a) + 2, None)), select(plan(P(a), None, k=0)),
               select(plan(P(a), None, w=0)), select(plan(P(a), None, k=2 ** 20, w=8)), select(plan(P(a), None), mm=0), select(plan(P(a), None), fl=None),
               select(plan(P(a), None), ct=None), select(plan(P(a), None), wk=None),
               gather(None), gather(plan(None, P(c))), gather(plan(P(a), None)), gather(plan(P(a) + 2, P(c))), gather(plan(P(a), P(c), k=0)),
               gather(plan(P(a), P(c), w=-1)), gather(plan(P(a), P(c), k=2 ** 20, w=8)), gather(plan(P(a), P(c)), ns=m + 1), gather(plan(P(a), P(c)), ns=-1),
               gather(plan(P(a), P(a) + 64)), gather(plan(P(a), P(c)), nd=None),
               scatter(None), scatter(plan(P(c), None)), scatter(plan(P(c) + 2, P(d))), scatter(plan(P(c), P(d), w=0)), scatter(plan(P(c), P(d)), ns=m + 1),
               scatter(plan(P(d) + 16, P(d))), scatter(plan(P(d), P(d)), full=1), scatter(plan(P(c), P(d), f=float("nan")))]
        assert bad == [-1] * len(bad), (sfx, bad)
        assert select(plan(P(a), None), we=1) == -3
        assert gather(plan(P(a), P(c)), ns=0, nd=None) == 0 and scatter(plan(P(c), P(d)), ns=0) == 0
    torch.cuda.synchronize()
    assert not bool(d.any()) and not bool(c.any()) and not bool(flags.any())


# -------------------------------------------------------------------------------------------------------------- the model
OSC, S2 = 1.3, 0.7
MODEL_GRIDS = {"8x8": [8, 8], "6x5x7": [6, 5, 7]}
ELLS = {2: [0.45, 0.6], 3: [0.45, 0.6, 0.5]}


def _kernel(g, out=1):
    from online_gp_amd.kernels import GridInterpolationKernel, RBFKernel, ScaleKernel

    d = len(g)
    bs = torch.Size([out]) if out > 1 else torch.Size()
    k = GridInterpolationKernel(ScaleKernel(RBFKernel(ard_num_dims=d, batch_shape=bs), batch_shape=bs), grid_size=g, num_dims=d,
                                grid_bounds=torch.as_tensor([[-1.0, 1.0]] * d))
    k.base_kernel.outputscale = OSC
    k.base_kernel.base_kernel.lengthscale = torch.as_tensor(ELLS[d])
    return k


def _data(n, seed, d=2, out=1, lo=-0.9, hi=0.9):
    rng = np.random.default_rng(seed)
    X = rng.uniform(lo, hi, (n, d))
    y = np.stack([np.sin((3 + o) * X[:, 0]) * np.cos(2 * X[:, 1]) + 0.1 * rng.standard_normal(n) for o in range(out)], 1)
    return X, y, rng.uniform(0.5, 1.5, (n, out))


def _t(a, dtype):
    return torch.as_tensor(a, device=DEV, dtype=dtype)


def _model(batches, g, dtype, **kw):
    """A model built from the first (X, y, noise) batch that absorbs the others in place."""
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    X, y, nz = batches[0]
    model = FixedNoiseOnlineSKIGP(_t(X, dtype), _t(y, dtype), _t(nz, dtype), covar_module=_kernel(g, y.shape[1]).to(DEV), learn_additional_noise=True, **kw)
    model.likelihood.second_noise = S2
    model.eval()
    for X, y, nz in batches[1:]:
        model.condition_on_observations(_t(X, dtype), _t(y, dtype), _t(nz, dtype), inplace=True)
    return model


def _values(model, Xq, want_mll=True):
    """(mean [out, q], variance [out, q], mll or None) as fp64 numpy."""
    from online_gp_amd.mlls import BatchedWoodburyMarginalLogLikelihood

    with torch.no_grad():
        mvn = model(_t(Xq, model._dtype))
        mean = mvn.mean.double().cpu().numpy().reshape(model.num_outputs, -1)
        var = mvn.variance.double().cpu().numpy().reshape(model.num_outputs, -1)
    mll = None
    if want_mll:
        model.train()
        mll = float(BatchedWoodburyMarginalLogLikelihood(model.likelihood, model)(model(None), None).sum().detach())
        model.eval()
    return mean, var, mll


def _oracle(g, batches, Xq):
    d = len(g)
    X, y, nz = (np.concatenate([b[i] for b in batches]) for i in range(3))
    outs = [dataspace.DataSpaceGP([[-1.0, 1.0]] * d, g, "rbf", np.array(ELLS[d]), OSC, S2).fit(X, y[:, o], nz[:, o]) for o in range(y.shape[1])]
    pm = [O.predict(Xq) for O in outs]
    return np.stack([p[0] for p in pm]), np.stack([p[1] for p in pm]), float(sum(O.mll() for O in outs))


def _close(label, got, want, rtol, mll_tol):
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    dm, dv = rel(got[0], want[0]), rel(got[1], want[1])
    dl = None if got[2] is None or want[2] is None else abs(got[2] - want[2]) / abs(want[2])
    print(f"{label}: mean {dm:.3e} variance {dv:.3e} (bound {rtol:.0e}); mll {dl if dl is None else format(dl, '.3e')} (bound {mll_tol:.0e})")
    assert dm <= rtol and dv <= rtol
    assert dl is None or dl <= mll_tol


class _Regime:
    """dense: the defaults (m = 64 and 210 are far inside max_cholesky_size); pcg: max_cholesky_size(32) puts both grids beyond it, solved at
    cg_tolerance(1e-10) as tests/test_regrid_gpu.py::test_regrid_pcg_regime does."""

    def __init__(self, regime):
        self.regime = regime

    def __enter__(self):
        from online_gp_amd import settings

        self.ctx = [settings.max_cholesky_size(32), settings.cg_tolerance(1e-10)] if self.regime == "pcg" else []
        for c in self.ctx:
            c.__enter__()

    def __exit__(self, *exc):
        for c in reversed(self.ctx):
            c.__exit__(*exc)


def _mll_tol(regime, dtype):
    if regime == "pcg":
        return MLL_MATRIX_FREE
    return MLL_DENSE if dtype == torch.float64 else RTOL[dtype]


def _leaves_equal(a, b, label):
    sa, sb = _snapshot(a._kernel_cache), _snapshot(b._kernel_cache)
    assert set(sa) == set(sb), label
    for name, t in sa.items():
        assert torch.equal(t, sb[name]), (label, name)


def _save_load(state, tmp_path):
    torch.save(state, tmp_path / "state.pt")
    return torch.load(tmp_path / "state.pt", weights_only=True)


COMBOS = [(r, dt, g) for r in ("dense", "pcg") for dt in (torch.float64, torch.float32) for g in MODEL_GRIDS]
COMBO_IDS = [f"{r}-{'f64' if dt == torch.float64 else 'f32'}-{g}" for r, dt, g in COMBOS]


@pytest.mark.parametrize("regime,dtype,grid", COMBOS, ids=COMBO_IDS)
def test_restore(regime, dtype, grid, tmp_path):
    from online_gp_amd.models import FixedNoiseOnlineSKIGP
    from online_gp_amd.models import kernel_cache as kc

    g = MODEL_GRIDS[grid]
    d = len(g)
    batches = [_data(32, 40 + i, d) for i in range(4)]
    Xq = _data(16, 50, d)[0]
    with _Regime(regime):
        A = _model(batches[:3], g, dtype)
        B = _model([_data(32, 60, d)], g, dtype)               # the same configuration, other data, other hyper-parameters
        B.likelihood.second_noise = 0.3
        assert A._use_dense() == (regime == "dense")
        ptrs = {n: t.data_ptr() for n, t in _leaves(B._kernel_cache)}
        state = _save_load(A.stream_state(), tmp_path)
        assert state["num_data"] == 96 and all(t.device.type == "cpu" for t in (state["WtW"], state["_stats"], state["interpolation_cache"]))
        assert B.load_stream_state_(state) is B
        assert {n: t.data_ptr() for n, t in _leaves(B._kernel_cache)} == ptrs
        _leaves_equal(A, B, "restore")
        assert B.num_data == A.num_data == 96 and B._wsum == pytest.approx(A._wsum, rel=WSUM_RTOL[dtype])
        assert float(B.likelihood.second_noise.detach()) == pytest.approx(S2, rel=1e-6)
        rt, mt = RTOL[dtype], _mll_tol(regime, dtype)
        _close(f"{regime} {grid} restored vs oracle", _values(B, Xq), _oracle(g, batches[:3], Xq), rt, mt)
        # the same model from the state as a kernel cache
        grid2, cache = kc.unpack(state, DEV)
        cov = _kernel(g).to(DEV)
        cov.set_grid_spec(grid2)
        C = FixedNoiseOnlineSKIGP(covar_module=cov, kernel_cache=cache, num_data=state["num_data"], learn_additional_noise=True, likelihood=A.likelihood)
        C.eval()
        _leaves_equal(A, C, "unpack")
        assert C._wsum == pytest.approx(A._wsum, rel=WSUM_RTOL[dtype])
        _close(f"{regime} {grid} built from unpack vs oracle", _values(C, Xq), _oracle(g, batches[:3], Xq), rt, mt)
        # both go on streaming
        X, y, nz = batches[3]
        for M in (A, B):
            M.condition_on_observations(_t(X, dtype), _t(y, dtype), _t(nz, dtype), inplace=True)
            M.check_bounds()
        want = _oracle(g, batches, Xq)
        _close(f"{regime} {grid} source after a fourth batch", _values(A, Xq), want, rt, mt)
        _close(f"{regime} {grid} restored after a fourth batch", _values(B, Xq), want, rt, mt)
        assert A.num_data == B.num_data == 128


@pytest.mark.parametrize("regime,dtype,grid", COMBOS, ids=COMBO_IDS)
def test_merge(regime, dtype, grid):
    g = MODEL_GRIDS[grid]
    d = len(g)
    b1, b2 = [_data(48, 70, d), _data(16, 71, d, lo=-0.9, hi=0.0)], [_data(40, 72, d, lo=-0.2, hi=0.9)]
    Xq = _data(16, 73, d)[0]
    rt, mt = RTOL[dtype], _mll_tol(regime, dtype)
    with _Regime(regime):
        B = _model(b2, g, dtype)
        sb = _snapshot(B._kernel_cache)
        for form in ("model", "state"):
            A = _model(b1, g, dtype)
            sa = _snapshot(A._kernel_cache)
            ptrs = {n: t.data_ptr() for n, t in _leaves(A._kernel_cache)}
            assert A.merge_(B if form == "model" else B.stream_state()) is A
            got = _snapshot(A._kernel_cache)
            assert {n: t.data_ptr() for n, t in _leaves(A._kernel_cache)} == ptrs
            for name, t in sa.items():                         # one rounded add per element: A + B of the two snapshots
                assert torch.equal(got[name], t + sb[name]), (form, name)
            assert all(torch.equal(t, sb[n]) for n, t in _snapshot(B._kernel_cache).items())
            assert A.num_data == 104 and A._wsum == pytest.approx([float(A._kernel_cache["_cnt"].double().sum())], rel=1e-12)
            _close(f"{regime} {grid} merged ({form}) vs oracle of both", _values(A, Xq), _oracle(g, b1 + b2, Xq), rt, mt)
        A = _model(b1, g, dtype).merge_(B, weight=0.5)
        X2, y2, nz2 = b2[0]
        _close(f"{regime} {grid} merged at weight 0.5 vs oracle", _values(A, Xq), _oracle(g, b1 + [(X2, y2, nz2 / 0.5)], Xq), rt, mt)


def test_three_outputs(tmp_path):
    g, dtype = [8, 8], torch.float64
    b1, b2 = [_data(48, 80, out=3), _data(16, 81, out=3)], [_data(40, 82, out=3)]
    Xq = _data(16, 83)[0]
    A, B = _model(b1, g, dtype), _model(b2, g, dtype)
    R = _model([_data(8, 84, out=3)], g, dtype).load_stream_state_(_save_load(A.stream_state(), tmp_path))
    _leaves_equal(A, R, "three outputs restored")
    assert R._stencil_pack(list(R._kernel_cache["WtW"].ops)) is not None and R._wsum == pytest.approx(A._wsum, rel=1e-12)
    _close("three outputs restored vs oracle", _values(R, Xq), _oracle(g, b1, Xq), RTOL[dtype], MLL_DENSE)
    sa, sb = _snapshot(A._kernel_cache), _snapshot(B._kernel_cache)
    A.merge_(B)
    for name, t in _snapshot(A._kernel_cache).items():
        assert torch.equal(t, sa[name] + sb[name]), name
    _close("three outputs merged vs oracle", _values(A, Xq), _oracle(g, b1 + b2, Xq), RTOL[dtype], MLL_DENSE)


def test_trend_merge_and_restore(tmp_path):
    """Two halves of the problem of tests/test_trend_gpu.py (dense regime, fp64, 10 x 9, linear trend, tau2 = 100): after the merge, and
    after a restore of the merged model, the coefficients and the posterior against the data-space reference at that test's own bound for
    this regime (1e-6 relative to the largest reference magnitude)."""
    import trend_reference as tref
    from oracle import spec
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    rng = np.random.default_rng(22)
    gb, gs, n, tau2 = [[-1.1, 1.1]] * 2, [10, 9], 80, 100.0
    X = rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32).astype(np.float64)
    noise = rng.uniform(0.05, 0.5, n).astype(np.float32).astype(np.float64)
    y = (5.0 + 2.0 * X[:, 0] - X[:, 1] + np.sin(3 * X[:, 0]) + 0.2 * rng.standard_normal(n)).astype(np.float32).astype(np.float64)
    Xs = rng.uniform(-1.0, 1.0, (16, 2)).astype(np.float32).astype(np.float64)
    center, scale = tref.frame(*spec.make_grid(gb, gs))
    t = lambda v: _t(v, torch.float64)
    build = lambda sl, **kw: FixedNoiseOnlineSKIGP(t(X[sl]), t(y[sl])[:, None], t(noise[sl])[:, None], grid_bounds=torch.tensor(gb, dtype=torch.float64),
                                                   grid_size=gs, learn_additional_noise=True, **{"trend": "linear", "trend_prior_var": tau2, **kw}).eval()
    A, B = build(slice(0, 40)), build(slice(40, 80))
    A.merge_(B)
    R = build(slice(0, 8)).load_stream_state_(_save_load(A.stream_state(), tmp_path))
    _leaves_equal(A, R, "trend restored")
    s2 = float(A.likelihood.second_noise.detach())
    ell = A.covar_module.base_kernel.base_kernel.lengthscale.detach().cpu().numpy().reshape(-1).astype(np.float64)
    osc = float(A.covar_module.base_kernel.outputscale.detach())
    mean_o, cov_o, beta_o, covb_o = tref.posterior(gb, gs, ell, osc, s2, X, y, noise, Xs, 1, center, scale, tau2)[:4]
    rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())
    for label, M in (("merged", A), ("restored", R)):
        mvn = M(t(Xs))
        beta, covb = M.trend_coefficients()
        figs = {"mean": rel(mvn.mean.cpu().numpy(), mean_o), "var": rel(mvn.variance.cpu().numpy(), np.diag(cov_o)),
                "beta": rel(beta.cpu().numpy(), beta_o), "cov_beta": rel(covb.cpu().numpy(), covb_o)}
        print(f"trend {label}: " + "  ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        assert all(v < 1e-6 for v in figs.values()) and M.num_data == 80
    with pytest.raises(ValueError, match="trend_C"):
        A.merge_(build(slice(0, 8), trend=None, trend_prior_var=None))      # statistics without a trend's


def test_path_probes_restore_and_merge(tmp_path):
    """Restore: sample_paths(S, seed) is the same draw.  Merge of two streams with distinct seeds: path by path against Matheron's rule in
    data space with the normals of BOTH generators, by the rule of tests/test_sample_paths_gpu.py (deviation at most 3 x the model's own
    mean deviation from the oracle on the same problem); equal seeds are refused."""
    import sample_paths_reference as sref
    from oracle import spec
    from online_gp_amd import settings

    g, dtype, S = [8, 8], torch.float64, 8
    b1, b2 = [_data(60, 90), _data(30, 91)], [_data(50, 92)]
    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(1e-10), torch.no_grad():
        A = _model(b1, g, dtype, num_path_probes=S, path_seed=21)
        B = _model(b2, g, dtype, num_path_probes=S, path_seed=22)
        R = _model([_data(8, 93)], g, dtype, num_path_probes=S, path_seed=5).load_stream_state_(_save_load(A.stream_state(), tmp_path))
        _leaves_equal(A, R, "probes restored")
        assert (R._kernel_cache["path_seed"], R._kernel_cache["path_count"]) == (21, 90)
        pa, pr = A.sample_paths(S, seed=3), R.sample_paths(S, seed=3)
        dev = float((pa.values - pr.values).abs().max() / pa.values.abs().max())
        print(f"paths of the restored model against the source's: {dev:.3e}")
        # two PCG solves of one system (equal statistics, hyper-parameters and draws) at tolerance 1e-10: tests/test_sample_paths_gpu.py
        # measures such a solve at 6e-8 from the data-space oracle in fp64, two of them differ by at most the sum; 1e-6 leaves a factor 8
        assert dev <= 1e-6
        with pytest.raises(ValueError, match="path_seed"):
            A.merge_(_model(b2, g, dtype, num_path_probes=S, path_seed=21))
        sa, sb = _snapshot(A._kernel_cache), _snapshot(B._kernel_cache)
        A.merge_(B)
        assert torch.equal(A._kernel_cache["path_probes"], sa["path_probes"] + sb["path_probes"])
        assert (A._kernel_cache["path_seed"], A._kernel_cache["path_count"]) == (21, 90)
        m = A._grid.m
        z = torch.randn((S, m), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        paths = A.sample_paths(S, base_samples=z.to(DEV))
        assert paths.last_converged
        X, y, nz = (np.concatenate([b[i] for b in b1 + b2]) for i in range(3))
        gb = [[-1.0, 1.0]] * 2
        O = dataspace.DataSpaceGP(gb, g, "rbf", np.array(ELLS[2]), OSC, S2).fit(X, y[:, 0], nz[:, 0])
        g0, h, gg = spec.make_grid(gb, g)
        W, Kuu = sref.dense_w(g0, h, gg, X), sref.kuu_dense(O.cols)
        u_mean = Kuu @ (W.T @ O.alpha)
        eps = np.concatenate([sref.normals(21, np.arange(90), S), sref.normals(22, np.arange(50), S)])
        eta = (sref.sym_sqrt(Kuu) @ z.numpy().T).T
        uo = sref.path_dataspace(Kuu, W, 1.0 / nz[:, 0], y[:, 0], S2, eta, eps)
        U = A.prediction_cache["pred_mean"][0, :, 0].double().cpu().numpy()
        dev_mean = np.abs(U - u_mean).max() / np.abs(u_mean).max()
        dev_path = np.abs(paths.values.double().cpu().numpy() - uo).max() / np.abs(uo).max()
        print(f"merged probes: path deviation {dev_path:.3e}, mean deviation {dev_mean:.3e}, ratio {dev_path / dev_mean:.2f}")
        assert dev_path <= 3.0 * dev_mean


def test_forgetting_factor_and_weight(tmp_path):
    """A forgetting model restores bit for bit and goes on forgetting; merge at weight w is the oracle with the other's noise over w."""
    g, dtype, gamma = [8, 8], torch.float64, 0.9
    batches = [_data(32, 100 + i) for i in range(3)]
    Xq = _data(16, 110)[0]
    A = _model(batches[:2], g, dtype, forgetting_factor=gamma)
    R = _model([_data(8, 111)], g, dtype, forgetting_factor=gamma).load_stream_state_(_save_load(A.stream_state(), tmp_path))
    _leaves_equal(A, R, "forgetting restored")
    X, y, nz = batches[2]
    for M in (A, R):
        M.condition_on_observations(_t(X, dtype), _t(y, dtype), _t(nz, dtype), inplace=True)
    aged = [(b[0], b[1], b[2] / gamma ** (2 - i)) for i, b in enumerate(batches)]      # batch i was decayed by every later update
    want = _oracle(g, aged, Xq)
    _close("forgetting source", _values(A, Xq), want, RTOL[dtype], MLL_DENSE)
    _close("forgetting restored", _values(R, Xq), want, RTOL[dtype], MLL_DENSE)
    stale = A.stream_state()
    stale["num_data"] = None
    with pytest.raises(RuntimeError, match="num_data"):
        R.merge_(stale, weight=0.5)


def test_grown_grid_restores_onto_the_states_grid(tmp_path):
    """A grow_grid model that left its first grid: the state carries the grid it grew to, and a model built on that grid takes it."""
    from online_gp_amd.models import FixedNoiseOnlineSKIGP
    from online_gp_amd.models import kernel_cache as kc

    g, dtype = [8, 8], torch.float64
    A = _model([_data(48, 120)], g, dtype, grow_grid=True)
    X, y, nz = _data(24, 121, lo=0.8, hi=1.5)
    A.condition_on_observations(_t(X, dtype), _t(y, dtype), _t(nz, dtype), inplace=True)
    A.check_bounds()
    assert A._grid.g != g
    state = _save_load(A.stream_state(), tmp_path)
    assert state["grid"]["size"] == A._grid.g and state["grid"]["g0"] == A._grid.g0
    with pytest.raises(ValueError, match="grid"):
        _model([_data(8, 122)], g, dtype).load_stream_state_(state)
    grid2 = kc._grid_of(state["grid"])
    cov = _kernel(g).to(DEV)
    cov.set_grid_spec(grid2)
    X0, y0, nz0 = _data(8, 122)
    R = FixedNoiseOnlineSKIGP(_t(X0, dtype), _t(y0, dtype), _t(nz0, dtype), covar_module=cov, learn_additional_noise=True).eval()
    R.load_stream_state_(state)
    _leaves_equal(A, R, "grown grid restored")
    Xq = np.concatenate([_data(8, 123)[0], X[:8]])
    a, r = _values(A, Xq), _values(R, Xq)
    _close("grown grid: restored vs source", r, a, RTOL[dtype], MLL_DENSE)


def test_heteroscedastic_restore(tmp_path):
    from online_gp_amd.kernels import RBFKernel, ScaleKernel
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    dtype, g = torch.float64, [8, 8]

    def build(seed, ell_g):
        nk = ScaleKernel(RBFKernel(ard_num_dims=2))
        nk.base_kernel.lengthscale, nk.outputscale = ell_g, 2.0
        X, y, nz = _data(40, seed)
        return FixedNoiseOnlineSKIGP(_t(X, dtype), _t(y, dtype), _t(nz, dtype), grid_bounds=torch.tensor([[-1.0, 1.0]] * 2), grid_size=g,
                                     learn_additional_noise=True, heteroscedastic=True, noise_kernel=nk, log_noise_mean=-0.5).eval()

    A, R = build(130, 0.6), build(131, 0.9)
    for i in range(3):
        X, y, nz = _data(37, 132 + i)
        A.condition_on_observations(_t(X, dtype), _t(y * (1 + X[:, :1]), dtype), _t(nz, dtype), inplace=True)
    state = _save_load(A.stream_state(), tmp_path)
    assert state["noise_model"]["num_data"] == 111 and any("lengthscale" in k for k in state["noise_model"]["module"])
    R.load_stream_state_(state)
    _leaves_equal(A, R, "heteroscedastic f")
    sa, sr = _snapshot(A.noise_model._kernel_cache), _snapshot(R.noise_model._kernel_cache)
    assert all(torch.equal(t, sr[n]) for n, t in sa.items()) and R.noise_model.num_data == 111 and R.num_data == 151
    Xq = _t(_data(16, 140)[0], dtype)
    pa, pr = A.predict_noise(Xq), R.predict_noise(Xq)
    print(f"predict_noise restored against source: {float((pa - pr).abs().max() / pa.abs().max()):.3e}")
    assert torch.allclose(pa, pr, rtol=1e-10, atol=0)           # equal statistics and hyper-parameters, two dense solves
    with pytest.raises(NotImplementedError, match="heteroscedastic"):
        A.merge_(R)
    with pytest.raises(NotImplementedError, match="heteroscedastic"):
        _model([_data(8, 141)], g, dtype).merge_(state)
    with pytest.raises(ValueError, match="noise_model"):
        _model([_data(8, 141)], g, dtype).load_stream_state_(state)


def _regression(seed, dtype=torch.float64, **kw):
    from online_gp_amd.models import OnlineSKIRegression
    from online_gp_amd.models.stems import Identity

    X, y, _ = _data(160 + 20 * 4, seed, lo=-0.95, hi=0.95)
    Xg, yg = _t(X, dtype), _t(y, dtype)
    return OnlineSKIRegression(Identity(2), Xg[:160], yg[:160], 1e-2, 8, 1.0, **kw), Xg[160:], yg[160:]


def test_wrapper_round_trip(tmp_path):
    reg, Xg, yg = _regression(150)
    other, _, _ = _regression(151)
    for i in range(3):
        reg.update(Xg[4 * i:4 * i + 4], yg[4 * i:4 * i + 4])
    state = _save_load(reg.stream_state(), tmp_path)
    assert set(state) == {"format", "version", "gp", "stem"} and state["gp"]["num_data"] == 172
    assert other.load_stream_state_(state) is other
    _leaves_equal(reg.gp, other.gp, "wrapper")
    for (n, p), (_, q) in zip(reg.gp.named_parameters(), other.gp.named_parameters()):
        assert torch.equal(p, q), n
    ma, va = reg.predict(Xg[40:56])
    mb, vb = other.predict(Xg[40:56])
    assert torch.allclose(ma, mb, rtol=1e-9, atol=1e-12) and torch.allclose(va, vb, rtol=1e-9, atol=1e-12)
    with pytest.raises(ValueError, match="format"):
        other.load_stream_state_(state["gp"])


def test_a_captured_hyper_step_survives_a_restore():
    """8 x 8: the streaming loop steps until the captured hyper step replays, loads its own earlier state and steps on."""
    reg, Xg, yg = _regression(160)
    early = None
    for i in range(16):
        sl = slice(4 * i, 4 * i + 4)
        reg.evaluate(Xg[sl], yg[sl])
        reg.update(Xg[sl], yg[sl])
        if i == 1:
            early = reg.stream_state()
        gs = reg.__dict__.get("_graphed")
        if gs is not None and gs.replays > 0 and i >= 5:
            break
    assert gs is not None and gs.replays > 0 and gs.disabled is None, (gs.disabled, gs.replays)
    ptrs = {n: t.data_ptr() for n, t in _leaves(reg.gp._kernel_cache)}
    reg.load_stream_state_(early)
    assert {n: t.data_ptr() for n, t in _leaves(reg.gp._kernel_cache)} == ptrs and reg.gp.num_data == 168
    before = gs.replays
    for i in range(6):
        sl = slice(40 + 4 * i, 44 + 4 * i)
        reg.evaluate(Xg[sl], yg[sl])
        _, loss = reg.update(Xg[sl], yg[sl])
        assert math.isfinite(float(loss))
    gs2 = reg.__dict__.get("_graphed")
    print(f"captured hyper step: {before} replays before the restore, {gs2.replays} after, disabled = {gs2.disabled}")
    assert gs2 is gs and gs2.disabled is None and gs2.replays > before and reg.gp.num_data == 192


def test_refusals():
    from online_gp_amd.models import OnlineSKIRegression
    from online_gp_amd.models.stems import Identity

    g, dtype = [8, 8], torch.float64
    plain = _model([_data(32, 170)], g, dtype)
    before = _snapshot(plain._kernel_cache)
    state = plain.stream_state()
    for kw in (dict(window=64), dict(site_memory=16)):
        ringed = _model([_data(32, 171)], g, dtype, **kw)
        name = next(iter(kw))
        for call in (ringed.stream_state, lambda: ringed.load_stream_state_(state), lambda: ringed.merge_(plain), lambda: ringed.merge_(state),
                     lambda: plain.merge_(ringed)):
            with pytest.raises(NotImplementedError, match=name):
                call()
    X, y, _ = _data(64, 172)
    wrapped = OnlineSKIRegression(Identity(2), _t(X, dtype), _t(y, dtype), 1e-2, 8, 1.0, window=32)
    with pytest.raises(NotImplementedError, match="window"):
        wrapped.stream_state()
    shifted = _model([_data(32, 173)], g, dtype)
    shifted.regrid_((1, 0), (0, 0))
    for other in (shifted, shifted.stream_state()):
        with pytest.raises(NotImplementedError, match="regrid_"):
            plain.merge_(other)
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError, match="weight"):
            plain.merge_(state, weight=bad)
    with pytest.raises(ValueError, match="num_outputs"):
        plain.load_stream_state_(_model([_data(8, 174, out=3)], g, dtype).stream_state())
    with pytest.raises(ValueError, match="dtype"):
        plain.merge_(_model([_data(8, 175)], g, torch.float32))
    after = _snapshot(plain._kernel_cache)
    assert all(torch.equal(t, before[n]) for n, t in after.items()) and plain.num_data == 32
