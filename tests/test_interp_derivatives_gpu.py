"""GPU: the interpolation-derivative kernels (wiski_gather_grad, wiski_gather_rows_vjp, wiski_basis_project(_vjp),
wiski_interp_bilinear(_vjp)) against the analytic fp64 reference of tests/interp_reference.py -- dense rows W [n, m] and their
closed-form derivative dW [n, d, m], combined by fp64 matmuls on the CPU -- on anisotropic grids (pairwise different size, bounds
and spacing per dim, one dim with 4 or 5 nodes), d = 1..4, fp64 and fp32, at the launch shapes where the kernels change form, with
points on interior nodes, on the nodes where the one-hot boundary rule switches on, inside boundary cells and outside the grid.

Tolerances (interp_reference.check), none taken from a kernel run:
  fp64  |got - ref| <= 8 N eps64 S_abs per element: S_abs the reference expression with every factor replaced by its absolute
        value, N the number of accumulated terms, 8 for the roundings.  This holds as it stands for every derivative kernel and for
        the prior.  The two forwards that are single products of weights -- basis_project's F (N = 4 d) and interp_bilinear
        (N = 16^d) -- get 8 eps64 (N S_abs + S_1): the rounding inside a cubic weight is relative to the size of its polynomial's
        terms, not to the weight (the outer taps are at most 0.07 with terms up to 24, and vanish by cancellation next to a node),
        so where the outer taps carry the result no fp64 evaluation meets a bound relative to the weight; the reference's own
        weights, against exact rational arithmetic, do not (test_interp_reference_host.py).  S_1 is first order: the sum over one
        weight at a time of S_abs with that weight replaced by the sum of its terms' absolute values.  Its median over a case's
        elements is 3.7 .. 9.6 times 8 N eps64 S_abs for F and 1.0 .. 5.8 times for the bilinear form (d = 1 .. 4; least at d = 4,
        where N = 65536); it exceeds that only on elements whose S_abs itself nearly vanishes (a node hit where the eigenvector is
        zero on the node), and is there still 8 eps64 times at most 24 times the neighbouring table entries.  The ratio of the
        error to 8 N eps64 S_abs alone is printed too;
  fp32  inputs rounded to fp32 first, reference evaluated in fp64 on the rounded values; max |got - ref| <= 8 max(dev32, eps32 max
        S_abs), dev32 the deviation of the reference's own fp32 restatement (g0, h, u and the weights in fp32, sums in fp64) from
        its fp64 value.  The basis projection computes its weights in fp64 from the up-cast points in both dtypes, so its F and
        prior are held to the fp64 bound and dev32 of its gradient is the rounding of the output;
  exact zero wherever S_abs is zero (the dims in which a point sits in a boundary cell, points outside the grid), exact symmetry and
  bitwise repeatability where stated.
Cell convention shared by kernels and reference: a cell is [node j, node j + 1), so a point exactly on node 1 is in the first cubic
cell (non-zero gradient) and a point exactly on node g - 2 in the last, one-hot cell (zero gradient); the fp64 cases contain both.

Largest fp32 got/dev32 per kernel on an MI355X (head-room is 8): see the comment block below the imports.
"""
import ctypes

import numpy as np
import pytest
import torch

import interp_reference as ir

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Largest fp32 ratio max|got - ref64| / dev32 per kernel (bound: 8), on an MI355X:
#   gather_grad 1.38   gather_rows_vjp 1.56   basis_project_vjp 1.00 (output rounding)
#   interp_bilinear 4.57 (its 4^d tap sums run in fp32)   interp_bilinear_vjp left 3.58, right 2.22
# Largest fp64 ratio err / (8 N eps64 S_abs) per kernel (bound: 1), same run:
#   gather_grad 0.50   gather_rows_vjp 0.11   basis_project_vjp 0.007   prior 0.067   interp_bilinear_vjp left 0.057, right 0.46
#   the two forwards, against their bound with the first-order weight term: basis_project F 0.037, interp_bilinear 0.019
#   (against 8 N eps64 S_abs alone: interp_bilinear 8.8; F unbounded where an eigenvector is zero on a node that was hit)


def _dev(t):
    return None if t is None else t.to(DEV)


def _flag(err):
    from online_gp_amd import grid_ops

    return grid_ops.read_flag(err)


GD = [(g, dn) for g in ir.GRIDS for dn in ir.DTYPES]
GD_IDS = [f"{g}-{dn}" for g, dn in GD]


# ----------------------------------------------------------------------------------------------------------- gather_grad
@pytest.mark.parametrize("diag", [False, True], ids=["col0", "diag"])
@pytest.mark.parametrize("n", ir.GATHER_GRAD_N, ids=lambda n: f"n{n}")
@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_gather_grad(gname, dname, n, diag):
    from online_gp_amd import grid_ops

    c = ir.gather_grad_case(gname, dname, n, diag)
    got = grid_ops.gather_grad(c["grid"], _dev(c["x"]), _dev(c["V"]), diag=diag)
    ir.check(got, c["R"], f"gather_grad {gname} {dname} n={n} diag={diag}")


@pytest.mark.parametrize("diag", [False, True], ids=["col0", "diag"])
@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_gather_grad_outside_points(gname, dname, diag):
    from online_gp_amd import grid_ops

    n = 8 * len(ir.GRIDS[gname][1]) + 7
    c = ir.gather_grad_case(gname, dname, n, diag, outside=True)
    got = grid_ops.gather_grad(c["grid"], _dev(c["x"]), _dev(c["V"]), diag=diag)
    out = torch.arange(n) % 3 == 1
    assert float(got[out.to(DEV)].abs().max()) == 0.0
    ir.check(got, c["R"], f"gather_grad outside {gname} {dname} diag={diag}")


# ------------------------------------------------------------------------------------------------------- gather_rows_vjp
@pytest.mark.parametrize("ncols", ir.ROWS_VJP_NCOLS, ids=lambda c: f"ncols{c}")
@pytest.mark.parametrize("n", ir.ROWS_VJP_N, ids=lambda n: f"n{n}")
@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_gather_rows_vjp(gname, dname, n, ncols):
    from online_gp_amd import grid_ops

    c = ir.gather_rows_vjp_case(gname, dname, n, ncols)
    got = grid_ops.gather_rows_vjp(c["grid"], _dev(c["x"]), _dev(c["Vr"]), _dev(c["G"]))
    ir.check(got, c["R"], f"gather_rows_vjp {gname} {dname} n={n} ncols={ncols}")


@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_gather_rows_vjp_outside_points(gname, dname):
    from online_gp_amd import grid_ops

    n = 8 * len(ir.GRIDS[gname][1]) + 7
    c = ir.gather_rows_vjp_case(gname, dname, n, 65, outside=True)
    grid, x, Vr = c["grid"], _dev(c["x"]), _dev(c["Vr"])
    got = grid_ops.gather_rows_vjp(grid, x, Vr, _dev(c["G"]))
    out = (torch.arange(n) % 3 == 1).to(DEV)
    assert float(got[out].abs().max()) == 0.0
    ir.check(got, c["R"], f"gather_rows_vjp outside {gname} {dname}")
    # the forward of the same points: zero rows, the flag raised; without them the flag stays down
    err = grid_ops.new_err_flag(DEV)
    fwd = grid_ops.gather_rows(grid, x[~out], Vr, err)
    assert _flag(err) == 0 and bool((fwd.abs().amax(1) > 0).all())
    fwd = grid_ops.gather_rows(grid, x, Vr, err)
    assert _flag(err) != 0 and float(fwd[out].abs().max()) == 0.0


# -------------------------------------------------------------------------------------------- basis_project and its VJP
BASIS = [(g, dn) + s for g in ir.GRIDS for dn in ir.DTYPES for s in ir.basis_shapes(g)]


def _basis_id(p):
    g, dn, n, r, kmax, sc, cs, pr = p
    return f"{g}-{dn}-n{n}-r{r}-kmax{kmax}-scale{int(sc)}-colscale{int(cs)}-prior{int(pr)}"


def _basis_run(c, kmax, err=None):
    from online_gp_amd import grid_ops

    grid, x, Vtab, S = c["grid"], _dev(c["x"]), _dev(c["Vtab"]), _dev(c["S"])
    kw = dict(scale=_dev(c["scale"]), colscale=_dev(c["colscale"]), tcol=_dev(c["tcol"]))
    F, prior = grid_ops.basis_project(grid, x, Vtab, kmax, S, want_prior=True, err=err, **kw)
    gx = grid_ops.basis_project_vjp(grid, x, Vtab, kmax, S, _dev(c["GF"]), _dev(c["Gp"]), **kw)
    return F, prior, gx


@pytest.mark.parametrize("p", BASIS, ids=[_basis_id(p) for p in BASIS])
def test_basis_project_and_vjp(p):
    from online_gp_amd import grid_ops

    gname, dname, n, r, kmax, sc, cs, pr = p
    c = ir.basis_case(gname, dname, n, r, kmax, sc, cs, pr)
    err = grid_ops.new_err_flag(DEV)
    F, prior, gx = _basis_run(c, kmax, err=err)
    assert _flag(err) == 0
    label = f"basis {_basis_id(p)}"
    ir.check(F, c["F"], label + " F")
    ir.check(prior, c["prior"], label + " prior")
    ir.check(gx, c["gx"], label + " vjp")
    if (n, r) in ((3, 200), (16387, 24)):
        F2, prior2, gx2 = _basis_run(c, kmax)
        assert torch.equal(gx, gx2) and torch.equal(F, F2) and torch.equal(prior, prior2)


@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_basis_project_vjp_strided_cotangent(gname, dname):
    """ldg > r through the entry point: GF is a column slice of a wider matrix whose other columns are NaN."""
    from online_gp_amd import _hip, grid_ops

    n, r, kmax = 37, 70, 8
    c = ir.basis_case(gname, dname, n, r, kmax, True, True, True)
    grid, x, Vtab, S = c["grid"], _dev(c["x"]), _dev(c["Vtab"]), _dev(c["S"])
    wide = torch.full((n, r + 9), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, 4:4 + r] = _dev(c["GF"])
    gf = wide[:, 4:4 + r]
    gx = torch.empty((n, grid.d), dtype=x.dtype, device=DEV)
    scale, colscale, tcol, Gp = _dev(c["scale"]), _dev(c["colscale"]), _dev(c["tcol"]), _dev(c["Gp"])
    rc = _hip.fn("wiski_basis_project_vjp", x.dtype)(grid.ref, _hip.dptr(x), ctypes.c_int64(n), _hip.dptr(Vtab), ctypes.c_int32(kmax), _hip.dptr(S),
                                                     ctypes.c_int32(r), _hip.dptr(scale), _hip.dptr(colscale), _hip.dptr(tcol),
                                                     ctypes.c_void_p(gf.data_ptr()), ctypes.c_int64(wide.stride(0)), _hip.dptr(Gp), _hip.dptr(gx),
                                                     _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_basis_project_vjp")
    ir.check(gx, c["gx"], f"basis ldg {gname} {dname}")
    assert torch.equal(gx, grid_ops.basis_project_vjp(grid, x, Vtab, kmax, S, _dev(c["GF"]), Gp, scale=scale, colscale=colscale, tcol=tcol))


@pytest.mark.parametrize("n,r", [(31, 129), (70, 40)], ids=["4waves", "1wave"])
@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_basis_project_outside_points(gname, dname, n, r):
    from online_gp_amd import grid_ops

    c = ir.basis_case(gname, dname, n, r, 8, True, True, True, outside=True)
    err = grid_ops.new_err_flag(DEV)
    F, prior, gx = _basis_run(c, 8, err=err)
    assert _flag(err) != 0
    out = (torch.arange(n) % 3 == 1).to(DEV)
    assert float(F[out].abs().max()) == 0.0 and float(prior[out].abs().max()) == 0.0 and float(gx[out].abs().max()) == 0.0
    label = f"basis outside {gname} {dname} n={n} r={r}"
    ir.check(F, c["F"], label + " F")
    ir.check(prior, c["prior"], label + " prior")
    ir.check(gx, c["gx"], label + " vjp")


# ------------------------------------------------------------------------------------------ interp_bilinear and its VJP
def _bil_list():
    out = []
    for g in ir.ALL_GRIDS:
        for dn, dt in ir.DTYPES.items():
            for qL, qR, nb, sym in ir.bilinear_shapes(g):
                out.append((g, dn, qL, qR, nb, sym) + ir.bilinear_forms(g, dt, qL, qR))
    return out


BIL = _bil_list()
# collection time (arithmetic on the grid sizes only, nothing imported): every (forward, left VJP) combination of forms that exists is in the list ((pair, row) cannot occur: the VJP's
# row form needs d rows in LDS where the forward needs one, against the same number of other points), in both modes
for _sym in (False, True):
    assert {(p[6], p[7]) for p in BIL if p[5] == _sym} == {("pair", "pair"), ("row", "row"), ("row", "pair")}
assert {p[8] for p in BIL} == {"pair", "row"}


def _bil_id(p):
    g, dn, qL, qR, nb, sym, f, vl, vr = p
    return f"{g}-{dn}-qL{qL}-qR{qR}-nb{nb}-{'sym' if sym else 'gen'}-fwd_{f}-vjpL_{vl}-vjpR_{vr}"


def _bil_run(c, A):
    from online_gp_amd import grid_ops

    grid, xL, xR, G = c["grid"], _dev(c["xL"]), _dev(c["xR"]), _dev(c["G"])
    err = grid_ops.new_err_flag(DEV)
    out = grid_ops.interp_bilinear_raw(grid, A, xL, xR, err)
    gL, gR = grid_ops.interp_bilinear_vjp(grid, A, xL, xR, G)
    return out, gL, gR, err


def _bil_check(c, out, gL, gR, label):
    ir.check(out, c["fwd"], label + " fwd")
    ir.check(gL, c["gL"], label + " vjpL")
    if c["xR"] is None:
        assert gR is None
        assert torch.equal(out, out.transpose(-1, -2))
    else:
        ir.check(gR, c["gR"], label + " vjpR")


@pytest.mark.parametrize("p", BIL, ids=[_bil_id(p) for p in BIL])
def test_interp_bilinear_and_vjp(p):
    from online_gp_amd import grid_ops

    gname, dname, qL, qR, nb, sym = p[:6]
    c = ir.bilinear_case(gname, dname, qL, qR, nb, sym)
    A = _dev(c["A"])
    out, gL, gR, err = _bil_run(c, A)
    assert _flag(err) == 0
    _bil_check(c, out, gL, gR, f"bilinear {_bil_id(p)}")
    if not sym:                                                # each side alone is the same launch as in the pair
        grid, xL, xR, G = c["grid"], _dev(c["xL"]), _dev(c["xR"]), _dev(c["G"])
        a, none = grid_ops.interp_bilinear_vjp(grid, A, xL, xR, G, want_left=True, want_right=False)
        assert none is None and torch.equal(a, gL)
        none, b = grid_ops.interp_bilinear_vjp(grid, A, xL, xR, G, want_left=False, want_right=True)
        assert none is None and torch.equal(b, gR)


BIL_LDA = [p for p in BIL if p[4] == 1 and (p[0] in ir.BIG_GRIDS or p[2] == p[3] or p[2] == 2)]


@pytest.mark.parametrize("p", BIL_LDA, ids=[_bil_id(p) for p in BIL_LDA])
def test_interp_bilinear_strided_table(p):
    """lda = m + 5: A is the leading m columns of an [m, m + 5] buffer whose padding is NaN."""
    gname, dname, qL, qR, nb, sym = p[:6]
    c = ir.bilinear_case(gname, dname, qL, qR, nb, sym, lda_pad=5)
    buf = _dev(c["Abuf"])
    assert buf.stride(0) == c["grid"].m + 5 and bool(torch.isnan(buf[:, c["grid"].m:]).all())
    out, gL, gR, err = _bil_run(c, buf)
    assert _flag(err) == 0
    _bil_check(c, out, gL, gR, f"bilinear lda {_bil_id(p)}")
    out2, gL2, gR2, _ = _bil_run(c, _dev(c["A"]))
    assert torch.equal(out, out2) and torch.equal(gL, gL2) and (gR is None or torch.equal(gR, gR2))


@pytest.mark.parametrize("sym", [False, True], ids=["gen", "sym"])
@pytest.mark.parametrize("form", ["pair", "row"])
@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_interp_bilinear_outside_points(gname, dname, form, sym):
    grid = ir.make_grid(gname)
    k = grid.m // grid.T
    q = max(7, k + 2) if form == "row" else min(7, max(1, k - 1))
    nb = -(-(6 * grid.d + 2) // q)                             # nb q >= 6 d + 2 points: both sides of every dim on each side
    assert ir.bilinear_forms(gname, ir.DTYPES[dname], q, q)[0] == form
    c = ir.bilinear_case(gname, dname, q, q, nb, sym, outside=True)
    out, gL, gR, err = _bil_run(c, _dev(c["A"]))
    assert _flag(err) != 0
    gone = (torch.arange(nb * q) % 3 == 1).reshape(nb, q).to(DEV)
    assert float(out[gone].abs().max()) == 0.0 and float(out.transpose(-1, -2)[gone].abs().max()) == 0.0
    assert float(gL[gone].abs().max()) == 0.0 and (gR is None or float(gR[gone].abs().max()) == 0.0)
    _bil_check(c, out, gL, gR, f"bilinear outside {gname} {dname} {form} sym={sym}")


# ------------------------------------------------------------------------------------------------------ autograd wrappers
@pytest.mark.parametrize("dname", list(ir.DTYPES))
def test_autograd_functions_run_the_raw_vjps_on_anisotropic_grids(dname):
    from online_gp_amd import grid_ops

    dtype = ir.DTYPES[dname]
    rng = np.random.default_rng(11)
    err = grid_ops.new_err_flag(DEV)
    # Gather: diag, k <= 4 columns (wiski_gather_grad per column), k > 4 (wiski_gather_rows_vjp on V^T)
    grid = ir.make_grid("d3g20x5x11")
    n = 50
    x = _dev(ir.make_points(grid, n, rng, dtype))
    for k, diag in ((n, True), (3, False), (9, False)):
        V = _dev(ir.normal(rng, (k, grid.m), dtype))
        g = _dev(ir.normal(rng, (n,) if diag else (n, k), dtype))
        xg = x.clone().requires_grad_(True)
        (grid_ops.Gather.apply(grid, xg, V, err, diag) * g).sum().backward()
        if diag:
            raw = grid_ops.gather_grad(grid, x, V, diag=True) * g[:, None]
        elif k <= 4:
            raw = sum(grid_ops.gather_grad(grid, x, V[c]) * g[:, c, None] for c in range(k))
        else:
            raw = grid_ops.gather_rows_vjp(grid, x, V.t().contiguous(), g)
        assert torch.equal(xg.grad, raw)
    # GatherRows
    grid = ir.make_grid("d2g9x31")
    c = ir.gather_rows_vjp_case("d2g9x31", dname, 97, 65)
    x, Vr, G = _dev(c["x"]), _dev(c["Vr"]), _dev(c["G"])
    xg = x.clone().requires_grad_(True)
    (grid_ops.GatherRows.apply(grid, xg, Vr, err) * G).sum().backward()
    assert torch.equal(xg.grad, grid_ops.gather_rows_vjp(grid, x, Vr, G))
    # InterpBilinear, general and symmetric
    for sym in (False, True):
        c = ir.bilinear_case("d4g5x7x4x6", dname, 3, 3 if sym else 5, 2, sym)
        grid, A, xL, xR, G = c["grid"], _dev(c["A"]), _dev(c["xL"]), _dev(c["xR"]), _dev(c["G"])
        xLg = xL.clone().requires_grad_(True)
        xRg = None if sym else xR.clone().requires_grad_(True)
        (grid_ops.interp_bilinear(grid, A, xLg, xRg, err) * G).sum().backward()
        gL, gR = grid_ops.interp_bilinear_vjp(grid, A, xL, xR, G)
        assert torch.equal(xLg.grad, gL) and (sym or torch.equal(xRg.grad, gR))
    # BasisProject (both outputs in one launch; scale is not an argument of the Function)
    c = ir.basis_case("d3g20x5x11", dname, 65, 129, 8, False, True, True)
    grid, x, Vtab, S, cs, tcol, GF, Gp = (c["grid"], _dev(c["x"]), _dev(c["Vtab"]), _dev(c["S"]), _dev(c["colscale"]), _dev(c["tcol"]), _dev(c["GF"]),
                                          _dev(c["Gp"]))
    xg = x.clone().requires_grad_(True)
    F, prior = grid_ops.BasisProject.apply(grid, xg, Vtab, 8, S, cs, tcol, err)
    ((F * GF).sum() + (prior * Gp).sum()).backward()
    assert torch.equal(xg.grad, grid_ops.basis_project_vjp(grid, x, Vtab, 8, S, GF, Gp, colscale=cs, tcol=tcol))
    assert _flag(err) == 0
