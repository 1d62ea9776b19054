"""GPU: the sliding-window absorb -- one launch absorbs the entering points, stores them in a device-resident ring and
takes out what their slots held -- against the fp64 slot-rule reference of tests/window_reference.py and the data-space oracle on
exactly the points in the ring: the kernel through the C ABI, the contract, then the model surface.

Bounds: those of tests/test_robust_gpu.py (scatter 1e-11 / 2e-4, x 10; model 1e-4 / 1e-2; MLL 1e-7 dense, 0.05 matrix-free).  The
scatter bounds are relative to the magnitude of the statistics BEFORE the points left -- what the buffers held plus what entered --
not to the result: rounding scales with what was summed, and after a removal the result can be arbitrarily smaller than that (a cell
whose points have all left holds rounding alone).  The ring arrays, err and void_left are compared exactly.
"""
import ctypes

import numpy as np
import pytest
import torch

import window_reference as wref
from oracle import dataspace, spec
from test_robust_gpu import DTYPES, KGRIDS, MLL_DENSE, MLL_FREE, RTOL, N, _buffers, _kernel_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("A", "b", "cnt", "stats", "res")
CAP = 48
RING_KEYS = ("x", "y", "wa", "wb", "noise")


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _launches(c):
    """The three launches on the 37-point layout (two points outside the grid, five colliding in one cell), cap = 48:
      1. 37 points at head 0, rolled by 9 so that the two outside points take slots 1 and 2: nothing leaves;
      2. 7 points (layout 8 .. 14: its outside points, three of the colliding ones) at head 43: five empty slots, then the ring
         wraps onto a point (slot 0) and a void (slot 1);
      3. 37 points at head 43: slots 43 .. 47 and 0 .. 31 hold a point or a void each -- the voids of launch 2 at 45 and 46, the one
         of launch 1 left at 2 -- and every one of them leaves."""
    roll = lambda a: np.roll(a, -9, axis=0)
    X, Y, wa, nz = c["X"], c["Y"], c["wa"], c["noise"]
    sl = slice(8, 15)
    return [(0, roll(X), roll(Y), roll(wa), roll(nz)), (43, X[sl], -Y[sl], wa[sl], nz[sl]), (43, X, 0.5 * Y, wa, nz)]


def _ring_arrays(ring):
    return {k: t.double().cpu().numpy() for k, t in zip(RING_KEYS, ring.tensors())}


@pytest.mark.parametrize("tdt,tol", DTYPES)
@pytest.mark.parametrize("name", list(KGRIDS))
def test_kernel_matches_the_slot_rule_reference(name, tdt, tol):
    from online_gp_amd import grid_ops

    c = _kernel_case(name)
    grid, u64 = c["grid"], c["u"]
    mk = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=tdt)
    u = mk(u64)
    launches = _launches(c)
    rring = wref.empty_ring(CAP, grid.d)
    first = wref.dense_absorb(grid, rring, 0, *launches[0][1:3], launches[0][3], launches[0][3], launches[0][4], u64)
    rng = np.random.default_rng(5)
    first_named = dict(first["before"], A=first["before"]["A_half"])
    state = {k: 0.5 * float(np.abs(first_named[k]).max()) * rng.standard_normal(np.shape(first_named[k])) for k in KEYS}   # non-zero buffers
    got = _buffers(grid, tdt, state)
    state = {k: v.double().cpu().numpy().copy() for k, v in got.items()}          # (as rounded to the working precision)
    ring, err = grid_ops.WindowRing(CAP, grid.d, tdt, DEV), grid_ops.new_err_flag(DEV)
    err_ref = void_ref = 0
    want_void = [0, 1, 3]
    for k, (head, X, Y, wa, nz) in enumerate(launches):
        n = X.shape[0]
        r = wref.dense_absorb(grid, rring, head, X, Y, wa, wa, nz, u64)
        assert r["void_left"] == want_void[k]                           # the launches are what the docstring of _launches says
        mean = torch.full((n,), float("nan"), device=DEV, dtype=tdt)
        ring.head = head
        grid_ops.scatter_stats_window(grid, mk(X), mk(Y), mk(wa), mk(wa), mk(nz), ring, got["b"], got["A"], got["cnt"], got["stats"], err, u,
                                      res=got["res"], mean_out=mean)
        assert ring.head == (head + n) % CAP
        rn, bn = dict(r, A=r["A_half"]), dict(r["before"], A=r["before"]["A_half"])
        for key in KEYS:
            mag = float(np.abs(state[key] + bn[key]).max())              # before anything left
            state[key] = state[key] + rn[key]
            e = float(np.abs(got[key].double().cpu().numpy() - state[key]).max())
            print(f"{name} {tdt} launch {k} {key}: max err {e:.3e}  bound {10 * tol * mag:.3e}")
            assert e <= 10 * tol * mag, (k, key, e, mag)
        e = float(np.abs(mean.double().cpu().numpy() - r["mean_out"]).max())
        assert e <= 10 * tol * float(np.abs(r["mean_out"]).max()), (k, "mean_out", e)
        rring = r["ring"]
        ga = _ring_arrays(ring)
        for key in RING_KEYS:
            assert np.array_equal(ga[key], rring[key], equal_nan=True), (k, key)
        err_ref, void_ref = err_ref + r["err"] - (r["err"] & 1 if err_ref & 1 else 0), void_ref + r["void_left"]
        assert int(err.item()) == err_ref and int(ring.void_left.item()) == void_ref, (k, int(err.item()), int(ring.void_left.item()))
    assert void_ref == 4 and err_ref == 1 + 2 * 6


BIG_CAP = 5000
_big = {}


def _big_case():
    """Batches large enough for SEVERAL passes of a block's loop (the 37-point launches above take one): d = 2, 5 x 7 nodes,
    cap = 5 000, fp32-exact inputs, about 2 % of the points outside the grid -- two of those with a non-finite target, which a void
    slot must not keep.  Launches (head, n) and what their slots hold:
      (0, 1 500)     256 blocks of four waves, 375 groups of four points: one or two passes per block; every slot empty;
      (1 000, 4 500) 282 blocks at 16 points each, four passes: slots 1 000 .. 1 499 hold points and voids, 1 500 .. 4 999 are empty,
                     then the ring wraps onto 0 .. 499 -- blocks meet live and empty groups in different passes, and the groups at the
                     two boundaries mix them;
      (400, 2 500)   256 blocks, two or three passes: every slot holds a point or a void.
    The references are built once and shared by both precisions."""
    if _big:
        return _big
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(77)
    grid = grid_ops.GridSpec([[-1.0, 1.0], [-1.0, 1.25]], [5, 7])
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
    u = f32(rng.standard_normal(grid.m))
    ring, state, launches = wref.empty_ring(BIG_CAP, 2), None, []
    for head, n in ((0, 1500), (1000, 4500), (400, 2500)):
        X = rng.uniform([-1.0, -1.0], [1.0, 1.25], (n, 2))
        out = rng.random(n) < 0.02
        X[out, 0] += 2.5
        X = f32(X)
        Y = f32(np.sin(2 * X[:, 0]) + 0.3 * rng.standard_normal(n))
        Y[np.flatnonzero(out)[:2]] = [np.inf, np.nan]
        nz = f32(rng.uniform(0.5, 2.0, n))
        wa = f32(1.0 / nz)
        r = wref.dense_absorb(grid, ring, head, X, Y, wa, wa, nz, u)
        launches.append(dict(head=head, X=X, Y=Y, wa=wa, nz=nz, ref=r, ring_before=ring))
        ring = r["ring"]
    _big.update(grid=grid, u=u, launches=launches)
    return _big


@pytest.mark.parametrize("tdt,tol", DTYPES)
def test_kernel_matches_the_reference_over_several_passes_of_a_block(tdt, tol):
    """The block loop's own machinery -- the votes per parity of the pass, the block-uniform skip of the second sweep, the scalars
    and the void count accumulated over passes, both launch geometries -- against the slot-rule reference (see _big_case).  Bounds
    as above: relative to the statistics before the points left."""
    from online_gp_amd import grid_ops

    c = _big_case()
    grid = c["grid"]
    mk = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=tdt)
    u = mk(c["u"])
    got = _buffers(grid, tdt)
    state = {k: v.double().cpu().numpy().copy() for k, v in got.items()}
    ring, err = grid_ops.WindowRing(BIG_CAP, 2, tdt, DEV), grid_ops.new_err_flag(DEV)
    dropped = voids = 0
    for k, L in enumerate(c["launches"]):
        r, n = L["ref"], L["X"].shape[0]
        old = L["ring_before"]
        slots = (L["head"] + np.arange(n)) % BIG_CAP
        live, void = old["wa"][slots] != 0, np.isnan(old["x"][slots, 0])
        print(f"launch {k}: {n} enter, {int(live.sum())} leave, {int(void.sum())} voids leave, {int((~live & ~void).sum())} empty slots, "
              f"{r['err'] >> 1} dropped at entry")
        assert r["void_left"] == int(void.sum()) and (k == 0 or (live.any() and void.any())) and (k == 2 or (~live & ~void).any())
        mean = torch.full((n,), float("nan"), device=DEV, dtype=tdt)
        ring.head = L["head"]
        grid_ops.scatter_stats_window(grid, mk(L["X"]), mk(L["Y"]), mk(L["wa"]), mk(L["wa"]), mk(L["nz"]), ring, got["b"], got["A"], got["cnt"],
                                      got["stats"], err, u, res=got["res"], mean_out=mean)
        rn, bn = dict(r, A=r["A_half"]), dict(r["before"], A=r["before"]["A_half"])
        for key in KEYS:
            mag = float(np.abs(state[key] + bn[key]).max())
            state[key] = state[key] + rn[key]
            e = float(np.abs(got[key].double().cpu().numpy() - state[key]).max())
            print(f"several passes {tdt} launch {k} {key}: max err {e:.3e}  bound {10 * tol * mag:.3e}")
            assert np.isfinite(state[key]).all() and e <= 10 * tol * mag, (k, key, e, mag)
        e = float(np.abs(mean.double().cpu().numpy() - r["mean_out"]).max())
        assert e <= 10 * tol * float(np.abs(r["mean_out"]).max()), (k, "mean_out", e)
        ga = _ring_arrays(ring)
        for key in RING_KEYS:
            assert np.array_equal(ga[key], r["ring"][key], equal_nan=True), (k, key)
        dropped, voids = dropped + (r["err"] >> 1), voids + r["void_left"]
        assert int(err.item()) == 1 + 2 * dropped and int(ring.void_left.item()) == voids
    assert voids > 20


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
def test_absorb_refuses_the_ring_with_what_the_kernel_does_not_do(tdt):
    """Through the full argument record plus the ring (wiski_absorb_window): every combination the contract refuses is WISKI_E_BADARG
    before any launch -- every buffer and the ring bit-identical -- n = 0 does nothing, and the record without the offending field
    runs and equals grid_ops.scatter_stats_window; res and mean_out are optional."""
    from online_gp_amd import _hip, grid_ops

    c = _kernel_case("d3")
    grid = c["grid"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, Y, wa, noise, u = (mk(c[k]) for k in ("X", "Y", "wa", "noise", "u"))
    buf, err = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    ring = grid_ops.WindowRing(CAP, grid.d, tdt, DEV)
    small = grid_ops.WindowRing(N - 1, grid.d, tdt, DEV)
    mean = torch.full((N,), float("nan"), device=DEV, dtype=tdt)
    full = torch.zeros((grid.R, grid.m), device=DEV, dtype=tdt)
    guard = torch.tensor([7], device=DEV, dtype=torch.int64)
    z1 = torch.full((2,), 0x01010101, device=DEV, dtype=torch.int32)
    bin_ws = torch.zeros(1 << 16, device=DEV, dtype=torch.uint8)
    p = lambda t: t.data_ptr()
    stream = _hip.stream_ptr(torch.device("cuda", torch.cuda.current_device()))

    def call(rg=ring, void_left=ring.void_left, ring_kw=None, null_ring=False, **kw):
        a = _hip.wiski_absorb_args(d_x=p(X), d_y=p(Y), d_wa=p(wa), d_wb=p(wa), d_noise=p(noise), n=N, d_b=p(buf["b"]), d_A=p(buf["A"]), half=1,
                                   channels=0, d_cnt=p(buf["cnt"]), d_stats=p(buf["stats"]), d_err=p(err), d_u=p(u), d_res=p(buf["res"]),
                                   d_mean_out=p(mean), nout=1)
        for k, v in kw.items():
            setattr(a, k, v)
        r = rg.ref()
        for k, v in (ring_kw or {}).items():
            setattr(r, k, v)
        return _hip.fn("wiski_absorb_window", tdt)(grid.ref, ctypes.byref(a), None if null_ring else ctypes.byref(r), _hip.dptr(void_left), stream)

    refused = [("no u", call(d_u=None, d_res=None, d_mean_out=None)), ("full stencil", call(half=0, d_A=p(full))), ("no A", call(d_A=None)),
               ("no cnt", call(d_cnt=None)), ("nout = 2", call(nout=2, d_mean_out=None)), ("channels", call(channels=4)),
               ("guard", call(d_guard=p(guard), guard_expect=7)), ("zero region", call(z1=p(z1), n1_bytes=8)), ("shard", call(g_lo=0, g_hi=3)),
               ("owner workspace", call(d_bin=p(bin_ws), bin_bytes=bin_ws.numel())), ("n > cap", call(rg=small)),
               ("head = cap", call(ring_kw=dict(head=CAP))), ("head < 0", call(ring_kw=dict(head=-1))), ("cap = 0", call(ring_kw=dict(cap=0))),
               ("no ring x", call(ring_kw=dict(d_x=None))), ("no ring noise", call(ring_kw=dict(d_noise=None))), ("no void_left", call(void_left=None)),
               ("no ring", call(null_ring=True))]
    torch.cuda.synchronize()
    assert [(what, rc) for what, rc in refused if rc != -1] == []
    assert call(n=0) == 0 and call(n=0, d_x=None, d_b=None, ring_kw=dict(d_y=None)) == 0          # n = 0: nothing is looked at
    torch.cuda.synchronize()
    fresh = grid_ops.WindowRing(CAP, grid.d, tdt, DEV)
    assert all(float(v.abs().max()) == 0.0 for v in buf.values()) and float(full.abs().max()) == 0.0 and int(err.item()) == 0
    assert bool(torch.isnan(mean).all()) and bool((z1 == 0x01010101).all())
    assert all(torch.equal(a, b) for rg in (ring, small) for a, b in zip(rg.tensors(), type(rg)(rg.cap, grid.d, tdt, DEV).tensors()))
    assert int(ring.void_left.item()) == 0 and int(small.void_left.item()) == 0
    assert call() == 0
    want, e2 = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    grid_ops.scatter_stats_window(grid, X, Y, wa, wa, noise, fresh, want["b"], want["A"], want["cnt"], want["stats"], e2, u, res=want["res"])
    tol = dict(DTYPES)[tdt]
    for k in KEYS:
        w = want[k].double().cpu().numpy()
        assert float(np.abs(buf[k].double().cpu().numpy() - w).max()) <= 10 * tol * float(np.abs(w).max()), k
    assert all(torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() and torch.equal(a.nan_to_num(), b.nan_to_num())
               for a, b in zip(ring.tensors(), fresh.tensors()))
    assert int(err.item()) == int(e2.item()) == 5
    assert call(d_res=None, d_mean_out=None, ring_kw=dict(head=N)) == 0   # u alone is a complete request: res and mean_out are optional
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- the model
from test_robust_gpu import _hyp, _mll, _t  # noqa: E402

GB = [[-1.0, 1.0], [-1.0, 1.0]]
W, Q, NUP = 40, 16, 6


def _f(X, i):
    return np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.5 * X[:, 1] + 0.02 * i          # a stream that drifts


def _stream(n=Q * (NUP + 1), seed=8):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.95, 0.95, (n, 2))
    noise = rng.uniform(0.5, 2.0, n)
    y = _f(X, np.arange(n)) + 0.05 * rng.standard_normal(n)
    return X, y, noise, rng.uniform(-0.95, 0.95, (50, 2))


def _model(X, y, nz, dtype, gs, **kw):
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    return FixedNoiseOnlineSKIGP(_t(X, dtype), _t(y, dtype)[:, None], None if nz is None else _t(nz, dtype)[:, None], grid_bounds=torch.tensor(GB),
                                 grid_size=gs, learn_additional_noise=True, **kw)


def _feed(m, X, y, nz, dtype, lo, hi, **kw):
    return m.condition_on_observations(_t(X[lo:hi], dtype), _t(y[lo:hi], dtype), None if nz is None else _t(nz[lo:hi], dtype), **kw)


def _posterior(m, Xs, dtype):
    mvn = m.eval()(_t(Xs, dtype))
    return mvn.mean.detach().double().cpu().numpy(), mvn.variance.detach().double().cpu().numpy()


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _check_window_regime(dtype, gs, unit, label, mll_bound):
    X, y, noise, Xs = _stream()
    nz = None if unit else noise
    n = X.shape[0]
    m = _model(X[:Q], y[:Q], None if unit else noise[:Q], dtype, gs, window=W).eval()
    allm = _model(X[:Q], y[:Q], None if unit else noise[:Q], dtype, gs).eval()
    for k in range(NUP):
        _feed(m, X, y, nz, dtype, Q * (k + 1), Q * (k + 2), inplace=True)
        _feed(allm, X, y, nz, dtype, Q * (k + 1), Q * (k + 2), inplace=True)
        assert m.num_data == min(W, Q * (k + 2))
    Xw, yw, nw = m.window_points()
    assert m.num_data == W and allm.num_data == n
    assert np.array_equal(Xw.double().cpu().numpy(), _t(X[n - W:], dtype).double().cpu().numpy())       # the last 40, oldest first
    assert np.array_equal(yw.double().cpu().numpy(), _t(y[n - W:], dtype).double().cpu().numpy())
    assert np.array_equal(nw.double().cpu().numpy(), np.ones(W) if unit else _t(noise[n - W:], dtype).double().cpu().numpy())
    # the noise-weight sum is that of the window: each 1 / noise is rounded once to the working precision (eps / 2 each, summed in fp64)
    want = float(W) if unit else float((1.0 / _t(noise[n - W:], dtype)).double().sum())
    print(f"{label} {dtype} unit={unit}: noise-weight sum {m._wsum[0]:.9f}  window {want:.9f}")
    assert abs(m._wsum[0] - want) <= 4 * torch.finfo(dtype).eps * want
    fresh = _model(X[:4], y[:4], None if unit else noise[:4], dtype, gs).eval()
    fresh.set_train_data(Xw, yw, nw)
    O = dataspace.DataSpaceGP(GB, gs, "rbf", *_hyp(m)).fit(X[n - W:], y[n - W:], np.ones(W) if unit else noise[n - W:])
    mo, vo = O.predict(Xs)
    mean, var = _posterior(m, Xs, dtype)
    mf, vf = _posterior(fresh, Xs, dtype)
    ma, va = _posterior(allm, Xs, dtype)
    print(f"{label} {dtype} unit={unit}: vs fresh mean {_rel(mean, mf):.3e} var {_rel(var, vf):.3e}; vs oracle mean {_rel(mean, mo):.3e} "
          f"var {_rel(var, vo):.3e}  (bound {RTOL[dtype]:.0e}); vs all points mean {_rel(mean, ma):.3e}")
    assert _rel(mean, mf) <= RTOL[dtype] and _rel(var, vf) <= RTOL[dtype]
    assert _rel(mean, mo) <= RTOL[dtype] and _rel(var, vo) <= RTOL[dtype]
    assert _rel(mean, ma) > 1e-2                                       # NOT the model that kept everything
    if dtype == torch.float64:                                         # (the MLL bounds are fp64 bounds, as in tests/test_robust_gpu.py)
        v, vfr, r = _mll(m), _mll(fresh), O.mll()
        print(f"{label}: mll {v:.10f}  fresh {vfr:.10f}  oracle {r:.10f}  (bound {mll_bound:.0e})")
        assert abs(v - r) <= mll_bound * abs(r) and abs(v - vfr) <= mll_bound * abs(vfr)
    return m


@pytest.mark.parametrize("unit", [True, False], ids=["unit", "noise"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_dense_regime_is_the_gp_of_the_last_window_points(dtype, unit):
    """8 x 8 grid, window 40, 16 initial points and six updates of 16; figures printed before the asserts."""
    _check_window_regime(dtype, [8, 8], unit, "dense", MLL_DENSE)


@pytest.mark.parametrize("unit", [True, False], ids=["unit", "noise"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_matrix_free_regime_is_the_gp_of_the_last_window_points(dtype, unit):
    from online_gp_amd import settings
    from online_gp_amd.mlls.batched_woodbury_marginal_log_likelihood import num_trace_samples

    with settings.max_cholesky_size(64), settings.spectral_factor(False), num_trace_samples(64), \
            settings.cg_tolerance(1e-10 if dtype == torch.float64 else 1e-6):
        m = _check_window_regime(dtype, [12, 12], unit, "matrix-free", MLL_FREE)
        assert not m._use_dense() and m._mean_state is not None


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 1e-6)])
def test_carried_residual_stays_valid_and_the_next_solve_starts_warm(dtype, tol):
    """PCG regime: after a converged refresh a window update keeps R_ok, R equals b - Z - A U of the updated buffers (recomputed in
    fp64; the bound of tests/test_forgetting_gpu.py: 50 tol max|b|), and the warm solve's mean equals a cold solve's within the CG
    tolerance (10 tol, relative: two solves converged to tol each)."""
    from online_gp_amd import grid_ops, settings

    X, y, noise, Xs = _stream()
    with settings.max_cholesky_size(64), settings.spectral_factor(False), settings.cg_tolerance(tol), torch.no_grad():
        m = _model(X[:Q], y[:Q], None, dtype, [12, 12], window=W).eval()
        for k in range(2):
            _feed(m, X, y, None, dtype, Q * (k + 1), Q * (k + 2), inplace=True)
        m.prediction_cache
        ms = m._mean_state
        assert ms["R_ok"]
        _feed(m, X, y, None, dtype, 3 * Q, 4 * Q, inplace=True)          # 16 enter, 8 leave
        assert m._mean_state is ms and ms["R_ok"] and m.num_data == W
        c = m._kernel_cache
        true_r = c["interpolation_cache"][0, :, 0].double() - ms["Z"][0].double() - grid_ops.stencil_spmv(m._grid, c["WtW"].stencil.double(), ms["U"][0:1].double())[0]
        scale = float(c["interpolation_cache"].abs().max())
        err = float((ms["R"][0].double() - true_r).abs().max())
        print(f"{dtype}: |R - (b - Z - A U)| = {err:.3e}, allowed {50 * tol * scale:.3e}")
        assert err <= 50 * tol * scale
        warm = m.prediction_cache["pred_mean"][0, :, 0].double().clone()
        m._mean_state = None
        m._dump_caches()
        cold = m.prediction_cache["pred_mean"][0, :, 0].double()
        dev = float((warm - cold).abs().max() / cold.abs().max())
        print(f"{dtype}: warm vs cold mean {dev:.3e}  (bound {10 * tol:.0e})")
        assert dev <= 10 * tol


def test_a_batch_larger_than_the_window_leaves_the_last_window_points():
    dtype = torch.float64
    X, y, noise, Xs = _stream(n=Q + 100)
    m = _model(X[:Q], y[:Q], noise[:Q], dtype, [8, 8], window=W).eval()
    _feed(m, X, y, noise, dtype, Q, Q + 100, inplace=True)
    Xw, yw, nw = m.window_points()
    assert m.num_data == W and np.array_equal(Xw.cpu().numpy(), X[-W:]) and np.array_equal(yw.cpu().numpy(), y[-W:])
    fresh = _model(X[-W:], y[-W:], noise[-W:], dtype, [8, 8]).eval()
    mean, var = _posterior(m, Xs, dtype)
    mf, vf = _posterior(fresh, Xs, dtype)
    print(f"batch of 100 into window 40: mean {_rel(mean, mf):.3e} var {_rel(var, vf):.3e}")
    assert _rel(mean, mf) <= RTOL[dtype] and _rel(var, vf) <= RTOL[dtype]
    # set_train_data keeps the last `window` rows as well
    m.set_train_data(_t(X[:90], dtype), _t(y[:90], dtype), _t(noise[:90], dtype))
    assert m.num_data == W and np.array_equal(m.window_points()[0].cpu().numpy(), X[50:90])
    fresh = _model(X[50:90], y[50:90], noise[50:90], dtype, [8, 8]).eval()
    assert _rel(_posterior(m, Xs, dtype)[0], _posterior(fresh, Xs, dtype)[0]) <= RTOL[dtype]


def test_functional_form_clones_the_ring_and_fantasies_retire_nothing():
    dtype = torch.float64
    X, y, noise, Xs = _stream()
    m = _model(X[:W], y[:W], noise[:W], dtype, [8, 8], window=W).eval()
    ring = m._kernel_cache["_ring"]
    before = [t.clone() for t in m.stats_buffers()] + [t.clone() for t in ring.tensors()]
    child = _feed(m, X, y, noise, dtype, W, W + Q)
    after = m.stats_buffers() + list(ring.tensors())
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and m.num_data == W and (ring.head, ring.fill) == (0, W)
    assert child.window == W and child.num_data == W and child._kernel_cache["_ring"] is not ring
    assert np.array_equal(child.window_points()[0].cpu().numpy(), X[Q:W + Q])
    fresh = _model(X[Q:W + Q], y[Q:W + Q], noise[Q:W + Q], dtype, [8, 8]).eval()
    assert _rel(_posterior(child, Xs, dtype)[0], _posterior(fresh, Xs, dtype)[0]) <= RTOL[dtype]
    # a fantasy adds its points to all 40 and retires none
    fant = m.get_fantasy_model(_t(X[W:W + Q], dtype), _t(y[W:W + Q], dtype)[:, None], _t(noise[W:W + Q], dtype)[:, None])
    assert fant.num_data == W + Q and all(torch.equal(a, b) for a, b in zip(before, after))
    both = _model(X[:W + Q], y[:W + Q], noise[:W + Q], dtype, [8, 8]).eval()
    assert _rel(_posterior(fant, Xs, dtype)[0], _posterior(both, Xs, dtype)[0]) <= RTOL[dtype]


def test_a_point_outside_the_grid_enters_and_leaves_without_a_trace():
    dtype = torch.float64
    X, y, noise, Xs = _stream()
    X = X.copy()
    X[Q + 3] = [1.5, 0.0]                                              # outside the grid, in the first update
    m = _model(X[:Q], y[:Q], noise[:Q], dtype, [8, 8], window=W).eval()
    _feed(m, X, y, noise, dtype, Q, 2 * Q, inplace=True)
    assert m.num_data == 2 * Q                                         # (not known yet: check_bounds is the one sync)
    with pytest.raises(RuntimeError, match="out of bounds"):
        m.check_bounds()
    assert m.num_data == 2 * Q - 1
    keep = np.arange(2 * Q) != Q + 3
    Xw = m.window_points()[0].cpu().numpy()
    assert np.array_equal(Xw, X[:2 * Q][keep])                         # the void slot is omitted
    fresh = _model(X[:2 * Q][keep], y[:2 * Q][keep], noise[:2 * Q][keep], dtype, [8, 8]).eval()
    assert _rel(_posterior(m, Xs, dtype)[0], _posterior(fresh, Xs, dtype)[0]) <= RTOL[dtype]
    for k in range(2, 5):                                              # the void slot comes round in the third of these updates
        _feed(m, X, y, noise, dtype, Q * k, Q * (k + 1), inplace=True)
    m.check_bounds()                                                   # nothing new outside: no error, and the void that left is taken back
    assert m.num_data == W
    want = float((1.0 / noise[5 * Q - W:5 * Q]).sum())                 # (fp64 sums of a few dozen terms, added and removed: 1e-12 is generous)
    assert abs(m._wsum[0] - want) <= 1e-12 * want
    assert np.array_equal(m.window_points()[0].cpu().numpy(), X[5 * Q - W:5 * Q])
    fresh = _model(X[5 * Q - W:5 * Q], y[5 * Q - W:5 * Q], noise[5 * Q - W:5 * Q], dtype, [8, 8]).eval()
    mean, var = _posterior(m, Xs, dtype)
    mf, vf = _posterior(fresh, Xs, dtype)
    assert _rel(mean, mf) <= RTOL[dtype] and _rel(var, vf) <= RTOL[dtype]
    v, vfr = _mll(m), _mll(fresh)
    assert abs(v - vfr) <= MLL_DENSE * abs(vfr)


def test_the_grid_may_grow_under_a_window():
    dtype = torch.float64
    X, y, noise, Xs = _stream()
    X = X.copy()
    X[2 * Q:] += [0.6, 0.0]                                            # the stream walks out of the initial grid
    m = _model(X[:Q], y[:Q], noise[:Q], dtype, [8, 8], window=W, grow_grid=True).eval()
    g0 = list(m._grid.g)
    for k in range(1, 5):
        _feed(m, X, y, noise, dtype, Q * k, Q * (k + 1), inplace=True)
    m.check_bounds()
    assert m._grid.g[0] > g0[0] and m.num_data == W
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    sl = slice(5 * Q - W, 5 * Q)
    fresh = FixedNoiseOnlineSKIGP(_t(X[sl], dtype), _t(y[sl], dtype)[:, None], _t(noise[sl], dtype)[:, None], covar_module=m.covar_module,
                                  learn_additional_noise=True).eval()
    Xq = Xs + [0.3, 0.0]
    mean, var = _posterior(m, Xq, dtype)
    mf, vf = _posterior(fresh, Xq, dtype)
    print(f"grown grid {g0} -> {m._grid.g}: mean {_rel(mean, mf):.3e} var {_rel(var, vf):.3e}")
    assert _rel(mean, mf) <= RTOL[dtype] and _rel(var, vf) <= RTOL[dtype]
    with pytest.raises(NotImplementedError):                           # but no node may be removed
        m.regrid_([-1, 0], [0, 0])


def test_window_rebuild_every_calls_the_rebuild_on_schedule(monkeypatch):
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    dtype = torch.float32
    X, y, noise, Xs = _stream()
    calls = []
    real = FixedNoiseOnlineSKIGP.rebuild_window_
    monkeypatch.setattr(FixedNoiseOnlineSKIGP, "rebuild_window_", lambda self: (calls.append(self._win_updates), real(self))[1])
    m = _model(X[:Q], y[:Q], noise[:Q], dtype, [8, 8], window=W, window_rebuild_every=2).eval()
    for k in range(1, 6):
        _feed(m, X, y, noise, dtype, Q * k, Q * (k + 1), inplace=True)
    assert calls == [2, 4] and m.num_data == W
    fresh = _model(X[6 * Q - W:6 * Q], y[6 * Q - W:6 * Q], noise[6 * Q - W:6 * Q], dtype, [8, 8]).eval()
    assert _rel(_posterior(m, Xs, dtype)[0], _posterior(fresh, Xs, dtype)[0]) <= RTOL[dtype]


def test_stream_step_takes_the_generic_path():
    from online_gp_amd import settings

    dtype = torch.float32
    X, y, noise, Xs = _stream()
    with settings.max_cholesky_size(64), settings.spectral_factor(False):
        m = _model(X[:W], y[:W], None, dtype, [12, 12], window=W).eval()
        m.prediction_cache
        assert m._stream_fast_state(_t(X[W:W + Q], dtype), _t(y[W:W + Q], dtype)) is None
        mean = m.stream_step(_t(X[W:W + Q], dtype), _t(y[W:W + Q], dtype))
        assert mean.shape == (Q,) and m.num_data == W and np.array_equal(m.window_points()[0].cpu().numpy(), _t(X[Q:W + Q], dtype).cpu().numpy())


def test_refusals():
    from online_gp_amd.distributed import ShardedStatsUpdater
    from online_gp_amd.models import FixedNoiseOnlineSKIGP, OnlineSKIBotorchModel

    dtype = torch.float64
    X, y, noise, Xs = _stream()
    Xt, yt, nt = _t(X[:12], dtype), _t(y[:12], dtype), _t(noise[:12], dtype)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            _model(X[:12], y[:12], noise[:12], dtype, [8, 8], window=bad)
    with pytest.raises(ValueError):
        _model(X[:12], y[:12], noise[:12], dtype, [8, 8], window_rebuild_every=3)
    with pytest.raises(NotImplementedError, match="alternatives"):
        _model(X[:12], y[:12], noise[:12], dtype, [8, 8], window=W, forgetting_factor=0.9)
    with pytest.raises(NotImplementedError, match="robust_c"):
        _model(X[:12], y[:12], noise[:12], dtype, [8, 8], window=W, robust_c=2.0)
    with pytest.raises(NotImplementedError, match="single output"):
        FixedNoiseOnlineSKIGP(Xt, torch.stack([yt, yt], 1), None, grid_bounds=torch.tensor(GB), grid_size=[8, 8], window=W)
    with pytest.raises(NotImplementedError, match="path probes"):
        _model(X[:12], y[:12], noise[:12], dtype, [8, 8], window=W, num_path_probes=4)
    m = _model(X[:12], y[:12], noise[:12], dtype, [8, 8], window=W)
    ring = m._kernel_cache["_ring"]
    before = [t.clone() for t in m.stats_buffers()] + [t.clone() for t in ring.tensors()]
    with pytest.raises(NotImplementedError, match="grad_Y"):
        m.condition_on_observations(Xt, yt, nt, grad_Y=torch.zeros(12, 2, device=DEV, dtype=dtype))
    with pytest.raises(NotImplementedError, match="half_delta"):
        m._absorb(m._kernel_cache, Xt, yt, nt[:, None], init=False, half_delta=m._half_buffers())
    with pytest.raises(NotImplementedError):
        ShardedStatsUpdater(m)
    with pytest.raises(NotImplementedError, match="enter_stencil_shard"):
        m.enter_stencil_shard(0, 2, lambda v, d: None)
    with pytest.raises(NotImplementedError, match="forget_"):
        m.forget_(0.9)
    with pytest.raises(NotImplementedError, match="only grow"):
        m.regrid_([0, 0], [-1, 0])
    assert all(torch.equal(a, b) for a, b in zip(before, m.stats_buffers() + list(ring.tensors()))) and m.num_data == 12
    # a handed-over full-stencil cache, and a cache that remembers no points
    cache = m._clone_cache(m._kernel_cache)
    op = cache["WtW"]
    cache["WtW"] = type(op)(m._grid, torch.zeros((m._grid.R, m._grid.m), device=DEV, dtype=dtype))
    h = FixedNoiseOnlineSKIGP(covar_module=m.covar_module, kernel_cache=cache, likelihood=m.likelihood, learn_additional_noise=True, num_data=12, window=W)
    with pytest.raises(NotImplementedError, match="full stencil"):
        h.condition_on_observations(Xt, yt, nt, inplace=True)
    plain = _model(X[:12], y[:12], noise[:12], dtype, [8, 8])
    with pytest.raises(ValueError, match="no ring"):
        FixedNoiseOnlineSKIGP(covar_module=plain.covar_module, kernel_cache=plain._clone_cache(plain._kernel_cache), likelihood=plain.likelihood,
                              learn_additional_noise=True, num_data=12, window=W)
    with pytest.raises(RuntimeError):
        plain.window_points()
    b = OnlineSKIBotorchModel(Xt, yt[:, None], nt[:, None], grid_bounds=torch.tensor(GB), grid_size=[8, 8], window=W, window_rebuild_every=5)
    assert b.window == W and b.window_rebuild_every == 5
