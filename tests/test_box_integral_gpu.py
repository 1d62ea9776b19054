"""GPU: the box kernels (wiski_box_tables, wiski_wt_columns_box, wiski_gather_box), ``posterior_integral`` and
``GridSamplePaths.integrate`` against the fp64 CPU reference of tests/quadrature_reference.py.

Tolerances, none taken from a kernel run:

* ``box_tables``, integrated dimension, per element: 16 eps64 T in fp64, T the entry with every term of its closed form by its
  absolute value (``box_rows_1d(terms=True)``).  Kernel and reference form the same cell coordinates t from the same inputs by the
  same operations, so they differ by the roundings of the closed forms alone: two quartics of about eight operations per end, each
  rounding at most eps64 / 2 of the terms, on both sides.  In fp32 the same (the kernel evaluates in fp64 from g0, h as
  GridDev<float> holds them) plus one rounding to fp32, 2^-24 |reference|.  Degenerate dimension: the point rule in the kernel's own
  precision, ``interp_reference.C_ROUND`` (8) eps of ``rows_1d(terms=True)`` against ``rows_1d`` in that precision.  Exactly zero
  where T is zero.  The node range must cover the non-zero entries and stay inside [0, g].  Volume: d + 1 roundings in fp64 and one
  to the kernel's precision, (8 eps64 + eps_real / 2) of the reference.
* ``wt_columns_box``, per element: the Kronecker product (``quadrature_reference.kron_rows``) of the tables the kernel itself made,
  d - 1 multiplications, 2 d eps of the entry; exactly zero off the support; bit-equal to ``wt_columns`` for all-degenerate boxes.
* ``gather_box`` and ``GridSamplePaths.integrate``: the jet tests' form -- fp64 per element 8 N eps64 S_abs, N the number of nodes
  in THAT box's support (the product of its node ranges: 4^d for a point box, m for a domain box, 0 for a box wholly outside); fp32
  max error 8 max(dev32, eps32 max S_abs) through ``interp_reference.check``, dev32 the deviation of the restatement with the rows
  rounded to fp32 and multiplied in fp32.  Exactly zero where S_abs is zero (a box wholly outside).
* model level: 1e-4 (fp64) and 1e-2 (fp32) of max |reference|, the bounds of tests/test_jet_gpu.py.

Measured on an MI355X (one run): see DESIGN.md 3.21."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import interp_reference as ir
import quadrature_reference as qr
from oracle import dataspace

pytestmark = pytest.mark.gpu
DEV = "cuda"
GD = [(g, dn) for g in ir.GRIDS for dn in ir.DTYPES]
GD_IDS = [f"{g}-{dn}" for g, dn in GD]
RTOL = {torch.float64: 1e-4, torch.float32: 1e-2}
EPS = {torch.float64: ir.EPS64, torch.float32: ir.EPS32}


def _flag(err):
    from online_gp_amd import grid_ops

    return grid_ops.read_flag(err)


@functools.lru_cache(maxsize=None)
def _case(gname, dname):
    """About 25 seeded boxes per grid, rounded to the case's dtype, and their reference: per-dimension rows R, terms T, volume,
    flags, ranges (with the geometry as GridDev<real> holds it) and which (box, dim) are degenerate."""
    grid, dtype = ir.make_grid(gname), ir.DTYPES[dname]
    lo, hi, kinds = qr.make_boxes(grid, np.random.default_rng(ir.seed_of("box", gname)))
    lo_t, hi_t = torch.as_tensor(lo).to(dtype), torch.as_tensor(hi).to(dtype)
    lo, hi = lo_t.double().numpy(), hi_t.double().numpy()
    R, vol, flag, rng = qr.box_rows_per_dim(grid, lo, hi, dtype)
    T = qr.box_rows_per_dim(grid, lo, hi, dtype, terms=True)[0]
    return dict(grid=grid, dtype=dtype, lo=lo_t, hi=hi_t, kinds=kinds, R=R, T=T, vol=vol, flag=flag, rng=rng, deg=lo == hi)


def _tables(c, sel=None):
    from online_gp_amd import grid_ops

    lo, hi = c["lo"], c["hi"]
    if sel is not None:
        lo, hi = lo[sel], hi[sel]
    err = grid_ops.new_err_flag(DEV)
    return grid_ops.box_tables(c["grid"], lo.to(DEV), hi.to(DEV), err), err


# -------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_box_tables(gname, dname):
    c = _case(gname, dname)
    grid, dtype = c["grid"], c["dtype"]
    t, err = _tables(c)
    assert _flag(err) != 0 and c["flag"].any()
    inside = np.flatnonzero(~c["flag"])
    t_in, err_in = _tables(c, inside)
    assert _flag(err_in) == 0 and torch.equal(t_in.tab, t.tab[inside])
    tab, rng, vol = t.tab.double().cpu().numpy(), t.range.cpu().numpy(), t.vol.double().cpu().numpy()
    assert tab.shape == (len(c["kinds"]), sum(grid.g)) and rng.shape == (len(c["kinds"]), grid.d, 2) and np.isfinite(tab).all()
    off, worst = 0, 0.0
    for q in range(grid.d):
        g = grid.g[q]
        got, ref, T, deg = tab[:, off:off + g], c["R"][q], c["T"][q], c["deg"][:, q]
        off += g
        bound = np.where(deg[:, None], ir.C_ROUND * EPS[dtype] * T, 16 * ir.EPS64 * T + (2.0 ** -24 * np.abs(ref) if dtype == torch.float32 else 0.0))
        e = np.abs(got - ref)
        assert (got[T == 0] == 0).all(), f"{gname} {dname} dim {q}: non-zero where the row is identically zero"
        worst = max(worst, float((e / np.maximum(bound, 1e-300)).max()))
        assert (e <= bound).all(), f"{gname} {dname} dim {q}: err/bound {float((e / np.maximum(bound, 1e-300)).max()):.3f}"
        for b in range(got.shape[0]):
            nz = np.flatnonzero(got[b])
            assert 0 <= rng[b, q, 0] <= rng[b, q, 1] <= g and (len(nz) == 0 or (rng[b, q, 0] <= nz[0] and nz[-1] < rng[b, q, 1])), (b, q, c["kinds"][b])
            assert not deg[b] or tuple(rng[b, q]) == tuple(c["rng"][b, q]), (b, q, c["kinds"][b])     # a point's range is its four taps
    ve = np.abs(vol - c["vol"])
    assert (ve <= (8 * ir.EPS64 + 0.5 * EPS[dtype]) * c["vol"]).all() and (vol[c["vol"] == 0] == 0).all()
    print(f"box_tables {gname} {dname}: max err/bound {worst:.3f}; volume max rel err {float((ve / np.maximum(c['vol'], 1e-300)).max()):.2e}")


@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_wt_columns_box(gname, dname):
    from online_gp_amd import grid_ops

    c = _case(gname, dname)
    grid, dtype = c["grid"], c["dtype"]
    t, _ = _tables(c)
    got = grid_ops.wt_columns_box(grid, t).double().cpu().numpy()
    tab, off, parts, mask = t.tab.double().cpu().numpy(), 0, [], []
    for q in range(grid.d):
        parts.append(tab[:, off:off + grid.g[q]])
        j = np.arange(grid.g[q])[None, :]
        mask.append(((j >= t.range[:, q, 0].cpu().numpy()[:, None]) & (j < t.range[:, q, 1].cpu().numpy()[:, None])).astype(np.float64))
        off += grid.g[q]
    want, support = qr.kron_rows(parts), qr.kron_rows(mask)
    e = np.abs(got - want)
    assert (got[support == 0] == 0).all() and (e <= 2 * grid.d * EPS[dtype] * np.abs(want)).all()
    print(f"wt_columns_box {gname} {dname}: max err / (2 d eps |entry|) {float((e / np.maximum(2 * grid.d * EPS[dtype] * np.abs(want), 1e-300)).max()):.3f}")
    # ... and against the reference's own rows: with delta_q the bound of test_box_tables on dim q's row,
    # |prod_q tab_q - prod_q R_q| <= sum_q delta_q prod_{o != q} (|R_o| + delta_o)  (every |tab_o| <= |R_o| + delta_o), plus the products' roundings
    ref = qr.kron_rows(c["R"])
    delta = [np.where(c["deg"][:, q:q + 1], ir.C_ROUND * EPS[dtype] * c["T"][q], 16 * ir.EPS64 * c["T"][q] + 0.5 * EPS[dtype] * np.abs(c["R"][q]))
             for q in range(grid.d)]
    big = [np.abs(c["R"][q]) + delta[q] for q in range(grid.d)]
    first = sum(qr.kron_rows([delta[q] if o == q else big[o] for o in range(grid.d)]) for q in range(grid.d))
    assert (np.abs(got - ref) <= 2 * grid.d * EPS[dtype] * qr.kron_rows(big) + first).all()
    if dtype == torch.float32:
        # fp32, boxes with no degenerate dimension, directly: every table entry is one rounding of its fp64 value (d eps32 / 2 in all)
        # and the d - 1 products round once each, inside 2 d eps32 of the reference's entry; what the fp64 evaluations of kernel and
        # reference themselves differ by (16 eps64 T per row, to first order as above) is kept apart
        full = ~c["deg"].any(1)
        d64 = [16 * ir.EPS64 * c["T"][q] for q in range(grid.d)]
        first64 = sum(qr.kron_rows([d64[q] if o == q else big[o] for o in range(grid.d)]) for q in range(grid.d))
        e32 = np.abs(got - ref)[full]
        b32 = (2 * grid.d * ir.EPS32 * np.abs(ref) + first64)[full]
        print(f"wt_columns_box {gname} f32 against the reference's Kronecker rows: max err / (2 d eps32 |entry| + fp64 term) {float((e32 / np.maximum(b32, 1e-300)).max()):.3f}")
        assert (e32 <= b32).all()


@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_wt_columns_box_of_points_is_wt_columns_bit_for_bit(gname, dname):
    from online_gp_amd import grid_ops

    grid, dtype = ir.make_grid(gname), ir.DTYPES[dname]
    x = ir.make_points(grid, 24, np.random.default_rng(ir.seed_of("boxpt", gname, dname)), dtype, outside=True).to(DEV)
    err = grid_ops.new_err_flag(DEV)
    t = grid_ops.box_tables(grid, x, x, err)
    assert _flag(err) != 0
    assert torch.equal(grid_ops.wt_columns_box(grid, t), grid_ops.wt_columns(grid, x, grid_ops.new_err_flag(DEV)))
    out = torch.arange(24) % 3 == 1
    assert torch.equal(t.vol.cpu(), (~out).to(dtype))


@functools.lru_cache(maxsize=None)
def _gather_ref(gname, dname, k, per_box):
    c = _case(gname, dname)
    grid, dtype = c["grid"], c["dtype"]
    B = len(c["kinds"])
    rng = np.random.default_rng(ir.seed_of("boxg", gname, dname, k, per_box))
    V = ir.normal(rng, (B * k, grid.m) if per_box else (k, grid.m), dtype)
    Vd = V.double().numpy()
    C = qr.kron_rows(c["R"])
    C32 = None
    if dtype == torch.float32:
        C32 = qr.kron_rows([r.astype(np.float32) for r in c["R"]]).astype(np.float64)

    def op(Cm, Vm):
        return np.einsum("bm,bjm->bj", Cm, Vm.reshape(B, k, grid.m)) if per_box else Cm @ Vm.T

    N = np.prod(c["rng"][:, :, 1] - c["rng"][:, :, 0], axis=1).astype(np.float64)[:, None]       # each box's own support size
    tt = torch.as_tensor
    R = dict(ref=tt(op(C, Vd)), sabs=tt(op(np.abs(C), np.abs(Vd))), N=tt(N), ref32=None if C32 is None else tt(op(C32, Vd)))
    return V, R


def _check_gather(got, R, label, sel=None):
    """See the module docstring.  sel: the boxes (rows of the reference) that `got` holds."""
    ref, sabs, N, ref32 = (None if R[key] is None else (R[key] if sel is None else R[key][sel]) for key in ("ref", "sabs", "N", "ref32"))
    if ref32 is not None:
        return ir.check(got, ir.Ref(ref, sabs, 1, ref32), label)
    got = got.detach().double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()) and float(sabs.max()) > 0, label
    assert bool((got[sabs == 0] == 0).all()), label + ": non-zero where the reference is identically zero"
    err = (got - ref).abs()
    bound = ir.C_ROUND * ir.EPS64 * N * sabs
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{label}: fp64 max err / (8 N eps64 S_abs) {ratio:.3f} (per-box N = {int(N.min())} .. {int(N.max())})")
    assert bool((err <= bound).all()), f"{label}: err/bound {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("nsplit", [1, 3, None], ids=["direct", "split3", "auto"])
@pytest.mark.parametrize("k,per_box", [(1, False), (5, False), (1, True), (3, True)], ids=["shared_k1", "shared_k5", "perbox_R1", "perbox_R3"])
@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_gather_box(gname, dname, k, per_box, nsplit):
    from online_gp_amd import grid_ops

    c = _case(gname, dname)
    V, R = _gather_ref(gname, dname, k, per_box)
    t, _ = _tables(c)
    got = grid_ops.gather_box(c["grid"], t, V.to(DEV), rows_per_box=k if per_box else 0, nsplit=nsplit)
    _check_gather(got, R, f"gather_box {gname} {dname} k={k} per_box={per_box} nsplit={nsplit}")


@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_one_box_and_no_box(gname, dname):
    from online_gp_amd import grid_ops

    c = _case(gname, dname)
    grid, dtype = c["grid"], c["dtype"]
    V, R = _gather_ref(gname, dname, 5, False)
    one, err = _tables(c, slice(0, 1))                                    # the whole domain
    assert (_flag(err) != 0) == bool(c["flag"][0]) and one.B == 1
    full, _ = _tables(c)
    assert torch.equal(one.tab, full.tab[:1]) and torch.equal(grid_ops.wt_columns_box(grid, one), grid_ops.wt_columns_box(grid, full)[:1])
    for ns in (1, 4):
        _check_gather(grid_ops.gather_box(grid, one, V.to(DEV), nsplit=ns), R, f"one box {gname} {dname} nsplit={ns}", slice(0, 1))
    none, err = _tables(c, slice(0, 0))
    assert none.tab.shape == (0, sum(grid.g)) and none.vol.shape == (0,) and _flag(err) == 0
    assert grid_ops.wt_columns_box(grid, none).shape == (0, grid.m) and grid_ops.gather_box(grid, none, V.to(DEV)).shape == (0, 5)


@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_refusals_leave_the_output_untouched(gname, dname):
    from online_gp_amd import _hip, grid_ops

    c = _case(gname, dname)
    grid, dtype = c["grid"], c["dtype"]
    t, _ = _tables(c)
    B, m = t.B, grid.m
    lo, hi = c["lo"].to(DEV), c["hi"].to(DEV)
    V = torch.ones((B * 2, m), dtype=dtype, device=DEV)
    err = grid_ops.new_err_flag(DEV)
    s = _hip.stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    p, i64, i32 = _hip.dptr, ctypes.c_int64, ctypes.c_int32
    sent = lambda *shape: torch.full(shape, 7.0, dtype=dtype, device=DEV)
    ot, ov, oc, og = sent(B, sum(grid.g)), sent(B), sent(B, m), sent(B, B * 2)
    orr = torch.full((B, grid.d, 2), 7, dtype=torch.int32, device=DEV)
    part = torch.zeros(B * B * 2 * 2, dtype=torch.float64, device=DEV)
    tabs, cols, gat = (_hip.fn(f, dtype) for f in ("wiski_box_tables", "wiski_wt_columns_box", "wiski_gather_box"))
    bad = _hip.wiski_grid()
    bad.d = 5
    gargs = lambda **kw: [kw.get(a, dflt) for a, dflt in (("grid", grid.ref), ("tab", p(t.tab)), ("range", p(t.range)), ("B", i64(B)), ("V", p(V)), ("k", i32(B * 2)),
                                                           ("R", i32(0)), ("ns", i32(1)), ("part", None), ("out", p(og)), ("s", s))]
    refused = [("tables lo", tabs(grid.ref, None, p(hi), i64(B), p(ot), p(orr), p(ov), p(err), s)),
               ("tables hi", tabs(grid.ref, p(lo), None, i64(B), p(ot), p(orr), p(ov), p(err), s)),
               ("tables tab", tabs(grid.ref, p(lo), p(hi), i64(B), None, p(orr), p(ov), p(err), s)),
               ("tables range", tabs(grid.ref, p(lo), p(hi), i64(B), p(ot), None, p(ov), p(err), s)),
               ("tables vol", tabs(grid.ref, p(lo), p(hi), i64(B), p(ot), p(orr), None, p(err), s)),
               ("tables err", tabs(grid.ref, p(lo), p(hi), i64(B), p(ot), p(orr), p(ov), None, s)),
               ("tables grid", tabs(ctypes.byref(bad), p(lo), p(hi), i64(B), p(ot), p(orr), p(ov), p(err), s)),
               ("tables B", tabs(grid.ref, p(lo), p(hi), i64(-1), p(ot), p(orr), p(ov), p(err), s)),
               ("columns tab", cols(grid.ref, None, p(t.range), i64(B), p(oc), s)),
               ("columns range", cols(grid.ref, p(t.tab), None, i64(B), p(oc), s)),
               ("columns out", cols(grid.ref, p(t.tab), p(t.range), i64(B), None, s)),
               ("columns grid", cols(ctypes.byref(bad), p(t.tab), p(t.range), i64(B), p(oc), s)),
               ("gather tab", gat(*gargs(tab=None))), ("gather range", gat(*gargs(range=None))), ("gather V", gat(*gargs(V=None))),
               ("gather out", gat(*gargs(out=None))), ("gather k", gat(*gargs(k=i32(0)))), ("gather rows_per_box", gat(*gargs(R=i32(-1)))),
               ("gather nsplit 0", gat(*gargs(ns=i32(0)))), ("gather nsplit without part", gat(*gargs(ns=i32(2)))),
               ("gather grid", gat(*gargs(grid=ctypes.byref(bad))))]
    torch.cuda.synchronize()
    assert [(what, rc) for what, rc in refused if rc != -1] == []
    assert all(bool((o == 7).all()) for o in (ot, ov, oc, og, orr)) and _flag(err) == 0
    assert gat(*gargs(ns=i32(2), part=p(part))) == 0
    empty = [tabs(grid.ref, None, None, i64(0), None, None, None, None, s), cols(grid.ref, None, None, i64(0), None, s),
             gat(*gargs(tab=None, range=None, B=i64(0), V=None, out=None))]
    assert empty == [0, 0, 0]


def test_invalid_boxes_give_zero_rows_and_raise_the_flag():
    from online_gp_amd import grid_ops

    grid = ir.make_grid("d2g9x31")
    lo = torch.tensor([[0.2, 0.0], [float("nan"), 0.0], [0.2, 1.0]], dtype=torch.float64, device=DEV)
    hi = torch.tensor([[0.6, 1.0], [0.6, 1.0], [0.6, 0.5]], dtype=torch.float64, device=DEV)
    err = grid_ops.new_err_flag(DEV)
    t = grid_ops.box_tables(grid, lo, hi, err)
    assert _flag(err) != 0
    cols = grid_ops.wt_columns_box(grid, t)
    assert float(cols[0].abs().max()) > 0 and float(cols[1:].abs().max()) == 0 and t.vol[1:].tolist() == [0.0, 0.0]
    assert float(t.tab[1, :9].abs().max()) == 0 and float(t.tab[2, 9:].abs().max()) == 0
    err2 = grid_ops.new_err_flag(DEV)
    grid_ops.box_tables(grid, lo[:1], hi[:1], err2)
    assert _flag(err2) == 0


# ---------------------------------------------------------------------------------------------------------------- the model
def _t(a, dtype):
    return torch.as_tensor(a, device=DEV, dtype=dtype)


def _f(X):
    return np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.5 * X[:, -1]


def _boxes(ref_grid, d):
    """Seven boxes in node units of the reference's grid: the interior box between node 1 and node g - 2, one inside a cell, one
    across the first boundary cell's midpoint into the interior, a line (dim 0 degenerate), a point, a box over several cells, and
    a thin slab."""
    g = ref_grid.g
    u_lo = [[1.0] * d, [2.2] * d, [0.3] * d, [2.5] + [1.4] * (d - 1), [3.3] * d, [1.6] * d, [2.0] + [1.2] * (d - 1)]
    u_hi = [[gq - 2.0 for gq in g], [2.7] * d, [2.4] * d, [2.5] + [gq - 2.6 for gq in g[1:]], [3.3] * d, [gq - 2.4 for gq in g], [2.05] + [gq - 2.2 for gq in g[1:]]]
    node = lambda U: np.array([[ref_grid.g0[q] + ref_grid.h[q] * u[q] for q in range(d)] for u in U])
    return node(u_lo), node(u_hi)


def _fit(gb, gs, dtype):
    """48 points, 32 at construction and 16 in one in-place update; the data-space reference with the model's hyper-parameters."""
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    d = len(gs)
    rng = np.random.default_rng(11)
    X = rng.uniform(-0.95, 0.95, (48, d))
    y = _f(X) + 0.05 * rng.standard_normal(48)
    nz = rng.uniform(0.5, 2.0, 48)
    m = FixedNoiseOnlineSKIGP(_t(X[:32], dtype), _t(y[:32, None], dtype), _t(nz[:32, None], dtype), grid_bounds=torch.tensor(gb), grid_size=gs,
                              learn_additional_noise=True).eval()
    m.condition_on_observations(_t(X[32:], dtype), _t(y[32:], dtype), _t(nz[32:], dtype), inplace=True)
    k = m.covar_module.base_kernel
    ell, s, s2 = k.base_kernel.lengthscale.detach().cpu().numpy().reshape(-1), float(k.outputscale), float(m.likelihood.second_noise)
    ref = qr.BoxGP(dataspace.DataSpaceGP(gb, gs, "rbf", ell, s, s2).fit(X, y, nz))
    return m, ref


def _rel(got, want):
    return float(np.abs(got.detach().double().cpu().numpy() - want).max() / np.abs(want).max())


def _check_model(m, ref, dtype, label):
    d = ref.grid.d
    lo, hi = _boxes(ref.grid, d)
    mean, cov, vol = ref.integral(lo, hi)
    ma, ca, _ = ref.integral(lo, hi, average=True)
    L, H = _t(lo, dtype), _t(hi, dtype)
    ip, ij = m.posterior_integral(L, H), m.posterior_integral(L, H, joint=True)
    ia, iaj = m.posterior_integral(L, H, average=True), m.posterior_integral(L, H, joint=True, average=True)
    pt = m(L[4:5])
    e = {"mean": _rel(ip.mean, mean), "variance": _rel(ip.variance, np.diag(cov)), "joint": _rel(ij.covariance, cov), "joint mean": _rel(ij.mean, mean),
         "variance vs joint diagonal": float((ip.variance - ij.covariance.diagonal()).abs().max() / ij.covariance.diagonal().abs().max()),
         "average mean": _rel(ia.mean, ma), "average variance": _rel(ia.variance, np.diag(ca)), "average joint": _rel(iaj.covariance, ca),
         "volume": _rel(ip.volume, vol), "stddev": _rel(ip.stddev, np.sqrt(np.diag(cov))),
         "point box mean vs posterior": float((ip.mean[4] - pt.mean[0]).abs() / pt.mean.abs().max().clamp_min(np.abs(mean).max())),
         "point box variance vs posterior": float((ip.variance[4] - pt.variance[0]).abs() / pt.variance[0].abs())}
    print(f"{label} {dtype}: " + "  ".join(f"{k} {x:.3e}" for k, x in e.items()) + f"  (bound {RTOL[dtype]:.0e})")
    B = lo.shape[0]
    assert ip.mean.shape == (B,) and ip.variance.shape == (B,) and ij.covariance.shape == (B, B) and ip.volume.shape == (B,)
    assert not ip.mean.requires_grad and not ij.covariance.requires_grad and ip.mean.dtype == dtype
    assert torch.equal(ij.covariance, ij.covariance.t()) and float(ip.volume[4]) == 1.0
    with pytest.raises(AttributeError):
        ip.covariance
    assert max(e.values()) <= RTOL[dtype]
    return ip, ij


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_posterior_integral_dense_regime(dtype):
    m, ref = _fit([[-1.0, 1.0]] * 2, [12, 10], dtype)
    ip, ij = _check_model(m, ref, dtype, "dense")
    assert hasattr(m.prediction_cache["pred_cov"], "dense") and ip.cg_iters == [] and ij.cg_iters == []


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_posterior_integral_matrix_free_regime(dtype):
    """10 x 9 x 8 grid; variance_chunk = 3 gives three solves for the seven boxes."""
    from online_gp_amd import settings

    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(1e-10 if dtype == torch.float64 else 1e-6), \
            settings.variance_chunk(3):
        m, ref = _fit([[-1.0, 1.0]] * 3, [10, 9, 8], dtype)
        ip, ij = _check_model(m, ref, dtype, "matrix-free")
        assert not hasattr(m.prediction_cache["pred_cov"], "dense") and len(ip.cg_iters) == 3 and len(ij.cg_iters) == 3


def test_rsample_is_mean_plus_factor_times_base_samples():
    dtype = torch.float64
    m, ref = _fit([[-1.0, 1.0]] * 2, [12, 10], dtype)
    lo, hi = _boxes(ref.grid, 2)
    z = _t(np.random.default_rng(3).standard_normal((6, lo.shape[0])), dtype)
    ij = m.posterior_integral(_t(lo, dtype), _t(hi, dtype), joint=True)
    A = ij.covariance.cpu().clone()
    A.diagonal().add_(1e-10 * A.diagonal().mean())
    want = ij.mean.cpu() + z.cpu() @ torch.linalg.cholesky(A).t()
    got = ij.rsample(torch.Size([6]), base_samples=z)
    assert got.shape == (6, lo.shape[0]) and float((got.cpu() - want).abs().max()) <= 1e-8 * float(want.abs().max())
    ip = m.posterior_integral(_t(lo, dtype), _t(hi, dtype))
    got = ip.rsample(torch.Size([2, 3]), base_samples=z.reshape(2, 3, -1))
    assert torch.allclose(got.reshape(6, -1), ip.mean + z * ip.variance.sqrt(), rtol=1e-12, atol=0)
    assert ip.rsample(torch.Size([4])).shape == (4, lo.shape[0])


@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_sample_paths_integrate(gname, dname):
    from online_gp_amd import settings
    from online_gp_amd.sample_paths import GridSamplePaths

    c = _case(gname, dname)
    V, R = _gather_ref(gname, dname, 5, False)
    paths = GridSamplePaths(c["grid"], V.to(DEV))
    inside = np.flatnonzero(~c["flag"])
    got = paths.integrate(c["lo"][inside], c["hi"][inside])
    assert got.shape == (5, len(inside))
    _check_gather(got.t(), R, f"integrate {gname} {dname}", inside)
    vol = torch.as_tensor(c["vol"][inside]).to(c["dtype"]).to(DEV)
    avg = paths.integrate(c["lo"][inside], c["hi"][inside], average=True)
    assert torch.allclose(avg, got / vol, rtol=4 * EPS[c["dtype"]], atol=0)
    # a path's integral is consistent with its point evaluations: a box degenerate in every dimension is the path's value there
    x = c["lo"][inside].to(DEV)
    assert torch.allclose(paths.integrate(x, x), paths(x), rtol=0, atol=64 * EPS[c["dtype"]] * float(V.abs().max()))
    with pytest.raises(RuntimeError):
        paths.integrate(c["lo"], c["hi"])
    with settings.deferred_bounds_check(True):
        out = paths.integrate(c["lo"], c["hi"])
        wholly = [i for i, kd in enumerate(c["kinds"]) if kd == "wholly_out"]
        assert float(out[:, wholly].abs().max()) == 0.0
        with pytest.raises(RuntimeError):
            paths.check_bounds()
    with pytest.raises(ValueError):
        paths.integrate(c["hi"], c["lo"])


def test_refusals_bounds_checks_and_pass_throughs():
    from online_gp_amd import settings
    from online_gp_amd.models import FixedNoiseOnlineSKIGP, Identity, LinearStem, OnlineSKIBotorchModel, OnlineSKIRegression

    dtype = torch.float64
    gb, gs = [[-1.0, 1.0]] * 2, [12, 10]
    m, ref = _fit(gb, gs, dtype)
    lo, hi = _boxes(ref.grid, 2)
    L, H = _t(lo, dtype), _t(hi, dtype)
    with pytest.raises(NotImplementedError):
        m.posterior_integral(L[None], H[None])
    for a, c in ((L[:, :1], H[:, :1]), (L[0], H[0]), (L, H[:3])):
        with pytest.raises(ValueError):
            m.posterior_integral(a, c)
    bad = H.clone()
    bad[2, 1] = float("inf")
    with pytest.raises(ValueError):
        m.posterior_integral(L, bad)
    bad[2, 1] = float("nan")
    with pytest.raises(ValueError):
        m.posterior_integral(L, bad)
    with pytest.raises(ValueError):
        m.posterior_integral(H, L)
    # bounds are checked as given, then cast: a box that fp32 would collapse to lower == upper is refused, not evaluated as a point
    m32, _ = _fit(gb, gs, torch.float32)
    with pytest.raises(ValueError):
        m32.posterior_integral(L[1:2], L[1:2] + 1e-12)
    thin = m.posterior_integral(L[1:2], L[1:2] + 1e-12)
    assert 0 < float(thin.volume[0]) < 1e-20 and float(thin.mean[0].abs()) < 1e-20
    rng = np.random.default_rng(2)
    X = _t(rng.uniform(-0.9, 0.9, (40, 2)), dtype)
    Y = _t(rng.standard_normal((40, 2)), dtype)
    two = FixedNoiseOnlineSKIGP(X, Y, None, grid_bounds=torch.tensor(gb), grid_size=gs).eval()
    with pytest.raises(NotImplementedError):
        two.posterior_integral(L, H)
    # a box partly outside the grid: raised by the call itself, or clipped and left to the next check when the check is deferred
    out_hi = H.clone()
    out_hi[0, 0] = 5.0
    with pytest.raises(RuntimeError):
        m.posterior_integral(L, out_hi)
    with settings.deferred_bounds_check(True):
        ip = m.posterior_integral(L, out_hi, average=True)
        from online_gp_amd import grid_ops
        assert grid_ops.read_flag(m._err) != 0
        m._err.zero_()
    clip_hi = hi.copy()
    clip_hi[0, 0] = ref.grid.g0[0] + ref.grid.h[0] * (ref.grid.g[0] - 1)
    mean, cov, vol = ref.integral(lo, clip_hi, average=True)
    assert _rel(ip.mean, mean) <= RTOL[dtype] and _rel(ip.variance, np.diag(cov)) <= RTOL[dtype] and _rel(ip.volume, vol) <= RTOL[dtype]
    wl = L.clone()
    wl[:, 0] = 4.0
    wh = wl + 1.0
    with settings.deferred_bounds_check(True):
        z = m.posterior_integral(wl, wh, average=True, joint=True)
        m._err.zero_()
    assert float(z.mean.abs().max()) == 0 and float(z.covariance.abs().max()) == 0 and float(z.volume.abs().max()) == 0
    bm = OnlineSKIBotorchModel(X, Y[:, :1], torch.ones_like(Y[:, :1]), grid_bounds=torch.tensor(gb), grid_size=gs)
    jb = bm.posterior_integral(L.float(), H.float(), joint=True)
    assert jb.mean.shape == (7,) and jb.covariance.shape == (7, 7) and jb.mean.dtype == dtype
    pv = bm.posterior(L[4:5]).variance.reshape(-1)
    assert float((jb.variance[4] - pv[0]).abs()) <= 1e-4 * float(pv[0])
    reg = OnlineSKIRegression(Identity(2), X, Y[:, :1], 1e-3, 10, 1.0)
    ri = reg.predict_integral(L, H, average=True)
    gi = reg.gp.posterior_integral(L, H, average=True)
    assert torch.equal(ri.mean, gi.mean) and torch.equal(ri.variance, gi.variance)
    lin = OnlineSKIRegression(LinearStem(2, 2).to(DEV).to(dtype), X, Y[:, :1], 1e-3, 10, 1.0)
    with pytest.raises(NotImplementedError):
        lin.predict_integral(L, H)
