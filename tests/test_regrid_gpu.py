"""GPU: growing, shifting and trimming the inducing grid of a live model.

The kernel (wiski_regrid_stats) bit for bit against the dense re-embedding of tests/regrid_reference.py, in an arena with 3-word
guards that puts most regions off a 16-byte boundary; then ``FixedNoiseOnlineSKIGP.regrid_`` / ``grow_to_cover_`` / ``grow_grid``
against the model's own values from before, oracle/dataspace.py on the new grid and a fresh model on the new grid.  Tolerances of the
oracle comparisons are the ones tests/test_model_gpu.py (RTOL, the north-star bars) and tests/test_mll_gpu.py (dense MLL 1e-6, matrix-
free MLL 5e-2) apply to an unregridded model; every comparison prints its figures before it asserts.

Measured on an MI355X (run with -s): kernel cases 0 differing words, drop record exact in rows, mass within 1 ulp; after vs before
2e-15 (dense) / 2e-9 (PCG) in the mean, after vs the oracle 6e-9 mean / 7e-8 variance / 4e-8 MLL (fp64), 7e-7 / 1e-6 (fp32); paths after a
regrid 5.7e-8 against a mean deviation of 2.7e-8 (ratio 2.1, bound 3); drifting stream 12x10 -> 26x10, 5.5e-9 / 8.9e-8 against the oracle.
"""
import ctypes

import numpy as np
import pytest
import torch

import regrid_reference as rr
from oracle import dataspace

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
RTOL = {torch.float64: 1e-4, torch.float32: 1e-2}       # tests/test_model_gpu.py
MLL_DENSE, MLL_MATRIX_FREE = 1e-6, 5e-2                  # tests/test_mll_gpu.py


# ------------------------------------------------------------------------------------------------------------ the kernel
KERNEL_CASES = {
    "d1_grow": ([8], (2,), (3,), 1, 0, False),
    "d2_mixed_odd": ([5, 7], (1, -1), (0, 2), 1, 0, False),
    "d3": ([6, 5, 4], (0, 1, 2), (1, 0, 0), 1, 0, False),
    "d2_two_outputs_probes": ([5, 7], (1, -1), (0, 2), 2, 4, False),
    "d1_trim_touched": ([9], (-3,), (0,), 1, 0, True),
}


def _spec(g):
    from online_gp_amd.grid_ops import GridSpec

    return GridSpec([[-1.0, 1.0]] * len(g), g)


def _stats(spec, below, above, out, touch_dropped, seed):
    """Dense (A, b, cnt) per output from points in interior cells; unless touch_dropped, no point's stencil reaches a node that the
    trim removes."""
    d, g = spec.d, spec.g
    rng = np.random.default_rng(seed)
    res = []
    for o in range(out):
        ta = [0 if touch_dropped else max(0, -below[q]) for q in range(d)]
        tb = [0 if touch_dropped else max(0, -above[q]) for q in range(d)]
        lo = np.array([spec.g0[q] + spec.h[q] * (1 + ta[q]) for q in range(d)])
        hi = np.array([spec.g0[q] + spec.h[q] * (g[q] - 2 - tb[q]) for q in range(d)])
        X = torch.as_tensor(lo + (hi - lo) * rng.uniform(0.0, 0.999, (30, d)))
        res.append(rr.dense_stats(spec, X, torch.as_tensor(rng.standard_normal(30)), torch.as_tensor(rng.uniform(0.5, 2.0, 30))))
    return res


def _arena(sizes, dtype, seed, guard=3):
    """One buffer that holds the named regions, each between guard words (as tests/test_forgetting_gpu.py lays its regions out):
    odd lengths and the 3-word guards put most regions off a 16-byte boundary.  -> (arena on the host, {name: (offset, length)})"""
    where, off = {}, guard
    for name, n in sizes:
        where[name] = (off, n)
        off += n + guard
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(off, generator=gen, dtype=torch.float64) * 3.0).to(dtype), where


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_regrid_kernel_bit_for_bit(case, dtype):
    from online_gp_amd import grid_ops

    g, below, above, out, S, touch = KERNEL_CASES[case]
    old = _spec(g)
    new = old.shifted(below, above)
    g2, m, m2, H = new.g, old.m, new.m, (old.R + 1) // 2
    assert g2 == rr.shifted_sizes(g, below, above)
    stats = _stats(old, below, above, out, touch, seed=len(g) + out)
    P = torch.randn((m, max(S, 1)), generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    sizes = [("pack", out * H * m), ("b", out * m), ("cnt", out * m), ("P", m * S),
             ("pack2", out * H * m2), ("b2", out * m2), ("cnt2", out * m2), ("P2", m2 * S)]
    host, where = _arena(sizes, dtype, seed=7)
    put = lambda name, t: host[where[name][0]:where[name][0] + where[name][1]].copy_(t.reshape(-1).to(dtype))
    put("pack", torch.stack([rr.pack_half(A, g) for A, _, _ in stats]))
    put("b", torch.stack([b for _, b, _ in stats]))
    put("cnt", torch.stack([c for _, _, c in stats]))
    if S:
        put("P", P)
    arena = host.to(DEV)
    view = lambda name: arena[where[name][0]:where[name][0] + where[name][1]]
    regions = []
    for o in range(out):
        regions += grid_ops.stencil_regrid_regions(old, new, view("pack").view(out, H, m)[o], view("pack2").view(out, H, m2)[o], report=o)
    regions += [(view("b"), view("b2"), out, 1), (view("cnt"), view("cnt2"), out, 1)]
    if S:
        regions.append((view("P").view(m, S), view("P2").view(m2, S), 1, S))
    rows, mass = grid_ops.regrid_stats(old, new, below, regions)
    torch.cuda.synchronize()
    # the reference: the dense statistics at the index shift, in the kernel's dtype (values are only moved), packed again
    want = host.clone()
    wput = lambda name, t: want[where[name][0]:where[name][0] + where[name][1]].copy_(t.reshape(-1))
    cast = lambda t: t.to(dtype)
    wput("pack2", torch.stack([rr.pack_half(rr.embed_matrix(cast(A), g, below, g2), g2) for A, _, _ in stats]))
    wput("b2", rr.embed_vectors(cast(torch.stack([b for _, b, _ in stats])), g, below, g2))
    wput("cnt2", rr.embed_vectors(cast(torch.stack([c for _, _, c in stats])), g, below, g2))
    if S:
        wput("P2", rr.embed_probes(cast(P), g, below, g2))
    got = arena.cpu()
    for name in ("pack2", "b2", "cnt2", "P2"):
        o, n = where[name]
        bad = int((got[o:o + n] != want[o:o + n]).sum())
        print(f"{case} {dtype}: {name} {n} elements, {bad} differ from the reference")
        assert torch.equal(got[o:o + n], want[o:o + n]), name
    assert torch.equal(got, want)                                    # guards and sources untouched
    # the drop record
    ref = [rr.dropped(cast(A), g, below, g2) for A, _, _ in stats]
    print(f"{case} {dtype}: dropped rows {rows} mass {mass}; reference {ref}")
    assert rows == [r for r, _ in ref]
    for got_m, (_, ref_m) in zip(mass, ref):
        assert abs(got_m - ref_m) <= 8 * EPS[torch.float64] * abs(ref_m)
    assert (sum(rows) > 0) == touch


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_regrid_kernel_offset_major_and_a_table_beyond_one_plan(dtype):
    """A full offset-major stencil [7^d][m] as one region, and 20 further vector regions: 21 regions, two launches."""
    from online_gp_amd import _hip, grid_ops

    g, below, above = [5, 7], (1, -1), (0, 2)
    old = _spec(g)
    new = old.shifted(below, above)
    g2, m, m2, R = new.g, old.m, new.m, old.R
    (A, _, _), = _stats(old, below, above, 1, False, seed=3)
    nvec = 20
    assert nvec + 1 > _hip.REGRID_MAX_REGIONS
    V = torch.randn((nvec, m), generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    sizes = [("om", R * m)] + [(f"v{i}", m) for i in range(nvec)] + [("om2", R * m2)] + [(f"w{i}", m2) for i in range(nvec)]
    host, where = _arena(sizes, dtype, seed=9)
    sl = lambda t, name: t[where[name][0]:where[name][0] + where[name][1]]
    sl(host, "om").copy_(rr.pack_offset_major(A, g).reshape(-1).to(dtype))
    for i in range(nvec):
        sl(host, f"v{i}").copy_(V[i].to(dtype))
    arena = host.to(DEV)
    regions = grid_ops.stencil_regrid_regions(old, new, sl(arena, "om").view(R, m), sl(arena, "om2").view(R, m2), report=0)
    assert len(regions) == 1 and regions[0][2:5] == (R, 1, 0)
    regions += [(sl(arena, f"v{i}"), sl(arena, f"w{i}"), 1, 1) for i in range(nvec)]
    rows, mass = grid_ops.regrid_stats(old, new, below, regions)
    torch.cuda.synchronize()
    want = host.clone()
    sl(want, "om2").copy_(rr.pack_offset_major(rr.embed_matrix(A.to(dtype), g, below, g2), g2).reshape(-1))
    for i in range(nvec):
        sl(want, f"w{i}").copy_(rr.embed_vectors(V[i:i + 1].to(dtype), g, below, g2)[0])
    got = arena.cpu()
    print(f"offset-major + {nvec} vectors {dtype}: {int((got != want).sum())} of {got.numel()} words differ; dropped {rows} {mass}")
    assert torch.equal(got, want) and rows == [0] and mass == [0.0]


def test_regrid_kernel_refuses_bad_arguments():
    from online_gp_amd import _hip, grid_ops

    old = _spec([6, 5])
    m = old.m
    src = torch.arange(m, dtype=torch.float32, device=DEV)
    dst = torch.full((64,), -7.0, dtype=torch.float32, device=DEV)
    f = _hip.fn("wiski_regrid_stats", torch.float32)
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)

    def call(below, above, g_new, s=None, d=None, k=1, w=1, r0=-1, report=-1, record=None):
        plan = _hip.wiski_regrid_plan()
        plan.count = 1
        plan.src[0] = src.data_ptr() if s is None else s
        plan.dst[0] = dst.data_ptr() if d is None else d
        plan.k[0], plan.w[0], plan.r0[0], plan.report[0] = k, w, r0, report
        return f(old.ref, i32(*below), i32(*above) if above is not None else None, i32(*g_new), ctypes.byref(plan), record, _hip.stream_ptr(src.device))

    assert call((0, 0), (1, 1), (7, 6)) == 0                                   # (the harness of this test works: 42 elements written)
    torch.cuda.synchronize()
    assert float(dst[:42].max()) >= 0 and bool((dst[42:] == -7.0).all())
    dst.fill_(-7.0)
    bad = {
        "g' < 4": call((0, -1), (0, -1), (6, 3)),
        "g' != g + below + above": call((0, 0), (1, 1), (7, 7)),
        "null src": call((0, 0), (1, 1), (7, 6), s=0),
        "null dst": call((0, 0), (1, 1), (7, 6), d=0),
        "misaligned dst": call((0, 0), (1, 1), (7, 6), d=dst.data_ptr() + 2),
        "misaligned src": call((0, 0), (1, 1), (7, 6), s=src.data_ptr() + 1),
        "w = 0": call((0, 0), (1, 1), (7, 6), w=0),
        "stencil rows beyond 7^d": call((0, 0), (1, 1), (7, 6), r0=49),
        "report without a record": call((0, 0), (1, 1), (7, 6), k=1, w=1, r0=24, report=0),
        "in place": call((0, 0), (1, 1), (7, 6), d=src.data_ptr()),
    }
    torch.cuda.synchronize()
    print(bad)
    assert all(rc == -1 for rc in bad.values()), bad
    assert bool((dst == -7.0).all()) and torch.equal(src, torch.arange(m, dtype=torch.float32, device=DEV))      # nothing was launched
    new = old.shifted((0, 0), (1, 1))
    with pytest.raises(_hip.WiskiError):
        grid_ops.regrid_stats(old, new, (0, 0), [(src, dst[:41], 1, 1)])           # a region that does not match the grids
    with pytest.raises(_hip.WiskiError):
        grid_ops.regrid_stats(old, _spec([6, 5, 4]), (0, 0), [(src, dst[:42], 1, 1)])


# ------------------------------------------------------------------------------------------------------------- the model
ELL, OSC, S2 = [0.45, 0.6], 1.3, 0.7


def _kernel(gb, g, out=1):
    from online_gp_amd.kernels import GridInterpolationKernel, RBFKernel, ScaleKernel

    bs = torch.Size([out]) if out > 1 else torch.Size()
    k = GridInterpolationKernel(ScaleKernel(RBFKernel(ard_num_dims=2, batch_shape=bs), batch_shape=bs), grid_size=g, num_dims=2, grid_bounds=gb)
    k.base_kernel.outputscale = OSC
    k.base_kernel.base_kernel.lengthscale = torch.as_tensor(ELL)
    return k


def _data(n, seed, lo=(-0.9, -0.9), hi=(0.9, 0.9), out=1):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(lo[q], hi[q], n) for q in range(2)], 1)
    y = np.stack([np.sin((3 + o) * X[:, 0]) * np.cos(2 * X[:, 1]) + 0.1 * rng.standard_normal(n) for o in range(out)], 1)
    return X, y, rng.uniform(0.5, 1.5, (n, out))


def _model(X, y, nz, gb, g, dtype=torch.float64, **kw):
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    t = lambda a: torch.as_tensor(a, device=DEV, dtype=dtype)
    out = y.shape[1]
    model = FixedNoiseOnlineSKIGP(t(X), t(y), t(nz), covar_module=_kernel(torch.as_tensor(gb), g, out).to(DEV), learn_additional_noise=True, **kw)
    model.likelihood.second_noise = S2
    model.eval()
    return model


def _values(model, Xq, want_mll=True):
    """(mean [out, q], variance [out, q], mll or None) as fp64 numpy."""
    from online_gp_amd.mlls import BatchedWoodburyMarginalLogLikelihood

    with torch.no_grad():
        mvn = model(torch.as_tensor(Xq, device=DEV, dtype=model._dtype))
        mean = mvn.mean.double().cpu().numpy().reshape(model.num_outputs, -1)
        var = mvn.variance.double().cpu().numpy().reshape(model.num_outputs, -1)
    mll = None
    if want_mll:
        model.train()
        mll = float(BatchedWoodburyMarginalLogLikelihood(model.likelihood, model)(model(None), None).sum().detach())
        model.eval()
    return mean, var, mll


def _oracle(gb, g, X, y, nz, Xq):
    outs = [dataspace.DataSpaceGP(gb, g, "rbf", np.array(ELL), OSC, S2).fit(X, y[:, o], nz[:, o]) for o in range(y.shape[1])]
    pm = [O.predict(Xq) for O in outs]
    return np.stack([p[0] for p in pm]), np.stack([p[1] for p in pm]), float(sum(O.mll() for O in outs))


def _close(label, got, want, rtol, mll_tol):
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    dm, dv = rel(got[0], want[0]), rel(got[1], want[1])
    dl = None if got[2] is None or want[2] is None else abs(got[2] - want[2]) / abs(want[2])
    print(f"{label}: mean {dm:.3e} variance {dv:.3e} (bound {rtol:.0e}); mll {dl if dl is None else format(dl, '.3e')} (bound {mll_tol:.0e})")
    assert dm <= rtol and dv <= rtol
    assert dl is None or dl <= mll_tol


GB = [[-1.0, 1.0]] * 2


def _three_comparisons(g, below, above, dtype, out, mll_tol, n=200, label=""):
    """regrid_ a model; its values against those from before, the oracle on the new grid and a fresh model on the new grid."""
    X, y, nz = _data(n, 21, out=out)
    Xq = _data(64, 22)[0]
    model = _model(X, y, nz, GB, g, dtype)
    dense0 = model._use_dense()
    before = _values(model, Xq)
    ret = model.regrid_(below, above)
    assert ret is model
    new = model._grid
    assert new.g == rr.shifted_sizes(g, below, above) and model.covar_module.grid_spec is new and model.covar_module.grid_sizes == new.g
    assert model.num_data == n and model._kernel_cache["interpolation_cache"].shape == (out, new.m, 1)
    after = _values(model, Xq)
    rt = RTOL[dtype]
    _close(f"{label} after vs before", after, before, rt, mll_tol)
    _close(f"{label} after vs oracle on the new grid", after, _oracle(new.grid_bounds, new.g, X, y, nz, Xq), rt, mll_tol)
    fresh = _model(X, y, nz, new.grid_bounds, new.g, dtype)
    _close(f"{label} after vs a fresh model on the new grid", after, _values(fresh, Xq), rt, mll_tol)
    return model, dense0, (X, y, nz, Xq)


def test_regrid_dense_regime():
    model, dense0, _ = _three_comparisons([12, 10], (2, 0), (1, 3), torch.float64, 1, MLL_DENSE, label="dense 12x10 -> 15x13")
    assert dense0 and model._use_dense()


def test_regrid_two_outputs():
    model, _, _ = _three_comparisons([12, 10], (2, 0), (1, 3), torch.float64, 2, MLL_DENSE, label="two outputs")
    assert model._stencil_pack([op for op in model._kernel_cache["WtW"].ops]) is not None      # still one [out, H, m'] pack


def test_regrid_fp32():
    _three_comparisons([12, 10], (2, 0), (1, 3), torch.float32, 1, RTOL[torch.float32], label="fp32")


def test_regrid_pcg_regime():
    from online_gp_amd import settings

    with settings.cg_tolerance(1e-10):
        model, dense0, _ = _three_comparisons([46, 46], (2, 0), (2, 2), torch.float64, 1, MLL_MATRIX_FREE, label="pcg 46x46 -> 50x48")
    assert not dense0 and not model._use_dense() and model._grid.g == [50, 48]


def test_regrid_crosses_the_regimes_both_ways():
    from online_gp_amd import settings

    assert 1936 <= settings.max_cholesky_size.value() < 2112
    with settings.cg_tolerance(1e-10):
        model, dense0, (X, y, nz, Xq) = _three_comparisons([44, 44], (2, 0), (2, 0), torch.float64, 1, MLL_MATRIX_FREE, label="44x44 -> 48x44")
        assert dense0 and not model._use_dense()
        pcg = _values(model, Xq, want_mll=False)
        model.regrid_((-2, 0), (-2, 0))                               # the way back: the added nodes are untouched
        assert model._grid.g == [44, 44] and model._use_dense()
        back = _values(model, Xq)
        _close("back to 44x44 vs the PCG values", back, pcg, RTOL[torch.float64], MLL_DENSE)
        old = _spec([44, 44])
        _close("back to 44x44 vs oracle", back, _oracle(GB, [44, 44], X, y, nz, Xq), RTOL[torch.float64], MLL_DENSE)
        assert max(abs(a - b) for a, b in zip(model._grid.g0, old.g0)) <= 4 * EPS[torch.float64] * 2


def test_streaming_goes_on_after_growth():
    X, y, nz = _data(200, 31)
    model = _model(X, y, nz, GB, [12, 10])
    old = model._grid
    model.regrid_((2, 0), (1, 3))
    new = model._grid
    # a batch wholly in the region that only the new grid covers: beyond the old grid's last node in dim 1
    lo1 = old.g0[1] + old.h[1] * (old.g[1] - 1) + 0.02
    hi1 = new.g0[1] + new.h[1] * (new.g[1] - 2) - 0.02
    assert hi1 > lo1
    X2, y2, nz2 = _data(40, 32, lo=(-0.9, lo1), hi=(0.9, hi1))
    t = lambda a: torch.as_tensor(a, device=DEV)
    model.condition_on_observations(t(X2), t(y2), t(nz2), inplace=True)
    model.check_bounds()
    Xa, ya, na = np.concatenate([X, X2]), np.concatenate([y, y2]), np.concatenate([nz, nz2])
    Xq = np.concatenate([_data(32, 33)[0], X2[:32]])
    _close("absorb after growth vs oracle", _values(model, Xq), _oracle(new.grid_bounds, new.g, Xa, ya, na, Xq), RTOL[torch.float64], MLL_DENSE)
    assert model.num_data == 240


def _buffers(model):
    c = model._kernel_cache
    return [t.clone() for t in model.stats_buffers()] + ([c["path_probes"].clone()] if "path_probes" in c else [])


def test_drop_zero_refuses_and_leaves_the_model_untouched():
    X, y, nz = _data(200, 41)
    Xq = _data(32, 42)[0]
    model = _model(X, y, nz, GB, [12, 10], num_path_probes=4, path_seed=3)
    before, vals = _buffers(model), _values(model, Xq)
    grid = model._grid
    with pytest.raises(ValueError, match=r"dims \[0\].*dropped mass") as ei:
        model.regrid_((-4, 0), (0, 0))
    print(ei.value)
    after = _buffers(model)
    assert model._grid is grid and model.covar_module.grid_spec is grid and len(after) == len(before)
    assert all(torch.equal(a, b) for a, b in zip(after, before))
    again = _values(model, Xq)
    assert np.array_equal(again[0], vals[0]) and np.array_equal(again[1], vals[1]) and again[2] == vals[2]
    with pytest.raises(ValueError):
        model.regrid_(0, 0, drop="some")
    with pytest.raises(ValueError, match="at least 4"):
        model.regrid_((-9, 0), (0, 0))


def test_drop_any_commits_the_principal_submatrix():
    X, y, nz = _data(200, 43)
    model = _model(X, y, nz, GB, [12, 10])
    g = [12, 10]
    op = model._kernel_cache["WtW"]
    A = rr.unpack_half(op.stencil.reshape(-1).cpu(), g)
    b = model._kernel_cache["interpolation_cache"][:, :, 0].cpu()
    cnt = model._kernel_cache["_cnt"].cpu()
    below, g2 = (-4, 0), [8, 10]
    rows, mass = rr.dropped(A, g, below, g2)
    ret = model.regrid_(below, (0, 0), drop="any")
    assert ret[0] is model and model._grid.g == g2
    print(f"drop='any': dropped mass {ret[1]!r}, reference {mass!r} over {rows} nodes")
    assert rows > 0 and abs(ret[1] - mass) <= 8 * EPS[torch.float64] * mass
    c = model._kernel_cache
    assert torch.equal(c["WtW"].stencil.reshape(-1).cpu(), rr.pack_half(rr.embed_matrix(A, g, below, g2), g2))
    assert torch.equal(c["interpolation_cache"][:, :, 0].cpu(), rr.embed_vectors(b, g, below, g2))
    assert torch.equal(c["_cnt"].cpu(), rr.embed_vectors(cnt, g, below, g2))
    with torch.no_grad():
        assert bool(torch.isfinite(model(torch.as_tensor(_data(8, 44, lo=(0.0, -0.9))[0], device=DEV)).variance).all())


def test_forgetting_commutes_with_regridding():
    X, y, nz = _data(200, 51)
    m1 = _model(X, y, nz, GB, [12, 10], num_path_probes=4, path_seed=3)
    m2 = _model(X, y, nz, GB, [12, 10], num_path_probes=4, path_seed=3)
    for dst, src in zip(m2.stats_buffers() + [m2._kernel_cache["path_probes"]], m1.stats_buffers() + [m1._kernel_cache["path_probes"]]):
        dst.copy_(src)                                                # (atomics: two absorbs differ in the last bits)
    m1.forget_(0.9).regrid_((2, 0), (1, 3))
    m2.regrid_((2, 0), (1, 3)).forget_(0.9)
    b1, b2 = _buffers(m1), _buffers(m2)
    same = [torch.equal(a, b) for a, b in zip(b1, b2)]
    print(f"forget then regrid vs regrid then forget: {same}")
    assert len(b1) == 5 and all(same) and b1[3].shape[1] == 15 * 13


def test_path_probes_follow_the_grid():
    """The probe buffer is the reference embed; the paths of the regridded model pass the check tests/test_sample_paths_gpu.py applies
    (path by path against Matheron's rule in data space, within 3 x the deviation of the model's own mean from the oracle)."""
    import sample_paths_reference as ref
    from online_gp_amd import settings
    from oracle import spec

    S, seed, g = 8, 21, [12, 14]
    X, y, nz = _data(300, 61)
    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(1e-10), torch.no_grad():
        model = _model(X, y, nz, GB, g, num_path_probes=S, path_seed=seed)
        P = model._kernel_cache["path_probes"].cpu()
        below, above = (1, 2), (2, 0)
        model.regrid_(below, above)
        new = model._grid
        assert torch.equal(model._kernel_cache["path_probes"].cpu(), rr.embed_probes(P, g, below, new.g))
        assert model._kernel_cache["path_count"] == 300 and model._kernel_cache["path_seed"] == seed
        m = new.m
        z = torch.randn((S, m), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        paths = model.sample_paths(S, base_samples=z.to(DEV))
        assert paths.last_converged and paths.values.shape == (S, m)
        O = dataspace.DataSpaceGP(new.grid_bounds, new.g, "rbf", np.array(ELL), OSC, S2).fit(X, y[:, 0], nz[:, 0])
        g0, h, gg = spec.make_grid(new.grid_bounds, new.g)
        W = ref.dense_w(g0, h, gg, X)
        Kuu = ref.kuu_dense(O.cols)
        u_mean = Kuu @ (W.T @ O.alpha)
        U = model.prediction_cache["pred_mean"][0, :, 0].double().cpu().numpy()
        dev_mean = np.abs(U - u_mean).max() / np.abs(u_mean).max()
        eps = ref.normals(seed, np.arange(300), S)
        eta = (ref.sym_sqrt(Kuu) @ z.numpy().T).T
        uo = ref.path_dataspace(Kuu, W, 1.0 / nz[:, 0], y[:, 0], S2, eta, eps)
        dev_path = np.abs(paths.values.double().cpu().numpy() - uo).max() / np.abs(uo).max()
        print(f"paths after regrid: path deviation {dev_path:.3e}, mean deviation {dev_mean:.3e}, ratio {dev_path / dev_mean:.2f}")
        assert dev_path <= 3.0 * dev_mean


# ---------------------------------------------------------------------------------------------------- following the stream
def _drift(seed=71):
    """32 points inside, then six batches of 32 that drift along dim 0 to 1.5 grid widths (3.0) beyond hi = 1."""
    rng = np.random.default_rng(seed)
    centres = [0.0] + list(np.linspace(0.4, 3.6, 6))
    Xs = [np.stack([c + rng.uniform(-0.4, 0.4, 32), rng.uniform(-0.8, 0.8, 32)], 1) for c in centres]
    ys = [np.sin(2 * x[:, :1]) * np.cos(2 * x[:, 1:]) + 0.1 * rng.standard_normal((32, 1)) for x in Xs]
    assert Xs[-1][:, 0].max() > 3.9
    return Xs, ys


def test_grow_grid_follows_a_drifting_stream():
    Xs, ys = _drift()
    ones = np.ones((32, 1))
    model = _model(Xs[0], ys[0], ones, GB, [12, 10], grow_grid=True)
    old = model._grid
    t = lambda a: torch.as_tensor(a, device=DEV)
    sizes = [list(model._grid.g)]
    for k in range(1, 7):
        if k % 2:
            model.condition_on_observations(t(Xs[k]), t(ys[k]), t(ones), inplace=True)
        else:
            model.stream_step(t(Xs[k]), t(ys[k]))
        sizes.append(list(model._grid.g))
    model.check_bounds()                                              # nothing was dropped
    new = model._grid
    print(f"grid sizes along the stream: {sizes}")
    assert model.num_data == 7 * 32
    assert new.g[1] == old.g[1] and new.g[0] > old.g[0] and new.g0 == old.g0 and new.h == old.h      # only dim 0, only upward
    assert all(b[0] >= a[0] for a, b in zip(sizes, sizes[1:]))
    Xa, ya = np.concatenate(Xs), np.concatenate(ys)
    assert Xa[:, 0].max() <= new.g0[0] + new.h[0] * (new.g[0] - 2)
    assert Xa[:, 0].max() > new.g0[0] + new.h[0] * (new.g[0] - 3)    # ... and not a node more than needed
    Xq = Xa[::4]
    _close("drifting stream vs oracle on the final grid", _values(model, Xq), _oracle(new.grid_bounds, new.g, Xa, ya, np.ones((224, 1)), Xq),
           RTOL[torch.float64], MLL_DENSE)
    # explicit call: nothing outside, nothing happens
    assert model.grow_to_cover_(t(Xs[0])) is model and model._grid is new


def test_max_grid_size_and_the_default_raise_out_of_bounds():
    Xs, ys = _drift()
    ones = np.ones((32, 1))
    t = lambda a: torch.as_tensor(a, device=DEV)
    capped = _model(Xs[0], ys[0], ones, GB, [12, 10], grow_grid=True, max_grid_size=16)
    with pytest.raises(RuntimeError, match="out of bounds"):
        for k in range(1, 7):
            capped.condition_on_observations(t(Xs[k]), t(ys[k]), t(ones), inplace=True)
    assert max(capped._grid.g) <= 16 and capped._grid.g[1] == 10
    plain = _model(Xs[0], ys[0], ones, GB, [12, 10])                 # grow_grid=False: as ever
    assert plain.grow_grid is False and plain.max_grid_size is None
    with pytest.raises(RuntimeError, match="out of bounds"):
        for k in range(1, 7):
            plain.condition_on_observations(t(Xs[k]), t(ys[k]), t(ones), inplace=True)
            plain.check_bounds()
    assert plain._grid.g == [12, 10]


def test_wrapper_passes_grow_grid_through():
    from online_gp_amd.models import Identity, OnlineSKIRegression

    Xs, ys = _drift()
    t = lambda a: torch.as_tensor(a, device=DEV, dtype=torch.float32)
    r = OnlineSKIRegression(Identity(2), t(Xs[0]), t(ys[0]), 1e-2, 12, 1.0, grow_grid=True)
    g0 = list(r.gp._grid.g)
    for k in range(1, 7):
        r.update(t(Xs[k]), t(ys[k]))
        pm, pv = r.predict(t(Xs[k][:5]))
        assert pm.shape == (5, 1) and bool(torch.isfinite(pm).all()) and bool((pv > 0).all())
    r.gp.check_bounds()
    print(f"wrapper: grid {g0} -> {r.gp._grid.g}")
    assert r.gp.num_data == 7 * 32 and r.gp._grid.g[0] > g0[0] and r.gp._grid.g[1] == g0[1]


def test_fantasy_models_do_not_regrid():
    X, y, nz = _data(60, 81)
    model = _model(X, y, nz, GB, [12, 10])
    t = lambda a: torch.as_tensor(a, device=DEV)
    fant = model.condition_on_observations(t(_data(6, 82)[0].reshape(2, 3, 2)), t(np.zeros((2, 3))), t(np.ones((2, 3))))
    with pytest.raises(NotImplementedError, match="regrid the base model"):
        fant.regrid_(1, 1)
