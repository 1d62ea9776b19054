"""GPU: the jet kernels (wiski_jet_quadform, wiski_wt_columns_jet, wiski_gather_jet) and ``posterior_jet`` against the fp64 CPU
reference of tests/jet_reference.py.

Kernel tolerances are those of ``interp_reference.check``, none taken from a kernel run: fp64 per element 8 N eps64 S_abs
(N = 16^d for the quadratic form, 4^d for the gathers); fp32 max error 8 max(dev32, eps32 max S_abs); exact zero where S_abs is
zero.  The rows that wt_columns_jet writes are single products of weights (N = 1): their fp64 bound carries the first-order weight
term S_1 (``jet_reference.rows_first_order``), as the two single-product forwards of tests/test_interp_derivatives_gpu.py do.
gather_jet sums each row in fp64 over lane groups, an order different from wiski_gather's and wiski_gather_grad's, and evaluates
the weights without fused multiply-adds: its channels agree with those two kernels WITHIN ``check`` -- all three are held to the
same reference slices -- not bit for bit.  gather_jet itself meets 8 N eps64 S_abs as it stands; the two older kernels, whose
contracted weights differ from the reference's by roundings relative to the polynomial's terms, get the first-order term S_1 on
top (wiski_gather alone measured 1.36 times the bare bound on d2g9x31).
Model bounds are those of tests/test_robust_gpu.py at model level: 1e-4 (fp64) and 1e-2 (fp32) of max |reference|.

Measured on an MI355X (one run): see DESIGN.md 3.17.
"""
import ctypes

import numpy as np
import pytest
import torch

import grad_obs_reference as gr
import interp_reference as ir
import jet_reference as jr

pytestmark = pytest.mark.gpu
DEV = "cuda"
GD = [(g, dn) for g in ir.GRIDS for dn in ir.DTYPES]
GD_IDS = [f"{g}-{dn}" for g, dn in GD]
NS = [(37, False), (24, True)]
NS_IDS = ["n37", "n24outside"]
RTOL = {torch.float64: 1e-4, torch.float32: 1e-2}


def _dev(t):
    return t.to(DEV)


def _flag(err):
    from online_gp_amd import grid_ops

    return grid_ops.read_flag(err)


def _outside_rows(n, outside):
    return (torch.arange(n) % 3 == 1) if outside else torch.zeros(n, dtype=torch.bool)


# -------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("pad", [0, 5], ids=["ldm_m", "ldm_padded"])
@pytest.mark.parametrize("n,outside", NS, ids=NS_IDS)
@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_jet_quadform(gname, dname, n, outside, pad):
    from online_gp_amd import grid_ops

    c = jr.quadform_case(gname, dname, n, outside, pad)
    grid, x = c["grid"], _dev(c["x"])
    buf = _dev(c["Mbuf"])
    M = buf[:, :grid.m]
    assert M.stride(0) == grid.m + pad and (pad == 0 or bool(torch.isnan(buf[:, grid.m:]).all()))
    err = grid_ops.new_err_flag(DEV)
    got = grid_ops.jet_quadform(grid, x, M, err)
    assert (_flag(err) != 0) == outside
    assert torch.equal(got, got.transpose(-1, -2))                       # bitwise symmetric
    out = _outside_rows(n, outside)
    assert not outside or float(got[out.to(DEV)].abs().max()) == 0.0
    ir.check(got, c["R"], f"jet_quadform {gname} {dname} n={n} pad={pad}")


@pytest.mark.parametrize("k,per_point", [(1, False), (5, False), (1, True), (None, True)], ids=["shared_k1", "shared_k5", "perpoint_B1", "perpoint_BC"])
@pytest.mark.parametrize("n,outside", NS, ids=NS_IDS)
@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_gather_jet(gname, dname, n, outside, k, per_point):
    from online_gp_amd import grid_ops

    d = len(ir.GRIDS[gname][1])
    k = d + 1 if k is None else k
    c = jr.gather_case(gname, dname, n, k, per_point, outside)
    grid, x, V, R = c["grid"], _dev(c["x"]), _dev(c["V"]), c["R"]
    err = grid_ops.new_err_flag(DEV)
    got = grid_ops.gather_jet(grid, x, V, err, rows_per_point=k if per_point else 0)
    assert (_flag(err) != 0) == outside
    label = f"gather_jet {gname} {dname} n={n} k={k} per_point={per_point}"
    ir.check(got, R, label)
    out = _outside_rows(n, outside)
    assert not outside or float(got[out.to(DEV)].abs().max()) == 0.0
    # the two kernels it fuses, against the same reference slices: agreement WITHIN check, not bit for bit (other summation order,
    # and wiski_gather / wiski_gather_grad evaluate the weights with fused multiply-adds: their fp64 bound carries S_1)
    s1 = c["s1"]

    def sl(*ix):
        return ir.Ref(R.ref[ix], R.sabs[ix], R.N, None if R.ref32 is None else R.ref32[ix], None if s1 is None else s1[ix])

    if not per_point:
        val = grid_ops.gather(grid, x, V, grid_ops.new_err_flag(DEV))                                   # [n, k]
        ir.check(val, sl(..., 0), label + " wiski_gather")
        grd = torch.stack([grid_ops.gather_grad(grid, x, V[j]) for j in range(k)], 1)                   # [n, k, d]
        ir.check(grd, sl(..., slice(1, None)), label + " wiski_gather_grad")
    elif k == 1:
        val = grid_ops.gather(grid, x, V, grid_ops.new_err_flag(DEV), diag=True)                        # [n]
        ir.check(val, sl(slice(None), 0, 0), label + " wiski_gather diag")
        grd = grid_ops.gather_grad(grid, x, V, diag=True)
        ir.check(grd, sl(slice(None), 0, slice(1, None)), label + " wiski_gather_grad diag")


@pytest.mark.parametrize("n,outside", NS, ids=NS_IDS)
@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_wt_columns_jet(gname, dname, n, outside):
    from online_gp_amd import grid_ops

    c = jr.columns_case(gname, dname, n, outside)
    grid, x = c["grid"], _dev(c["x"])
    C = grid.d + 1
    err = grid_ops.new_err_flag(DEV)
    got = grid_ops.wt_columns_jet(grid, x, err)
    assert (_flag(err) != 0) == outside
    assert torch.equal(got[0::C], grid_ops.wt_columns(grid, x, grid_ops.new_err_flag(DEV)))             # rows p C: exactly wt_columns
    ir.check(got, c["R"], f"wt_columns_jet {gname} {dname} n={n}")


@pytest.mark.parametrize("gname,dname", GD, ids=GD_IDS)
def test_refusals_leave_the_output_untouched_and_empty_batches_are_ok(gname, dname):
    from online_gp_amd import _hip, grid_ops

    grid, dtype = ir.make_grid(gname), ir.DTYPES[dname]
    n, m, C = 5, grid.m, grid.d + 1
    rng = np.random.default_rng(3)
    x = _dev(ir.make_points(grid, n, rng, dtype))
    M, V = _dev(ir.normal(rng, (m, m), dtype)), _dev(ir.normal(rng, (n * C, m), dtype))
    err = grid_ops.new_err_flag(DEV)
    s = _hip.stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    p, i64, i32 = _hip.dptr, ctypes.c_int64, ctypes.c_int32
    sent = lambda *shape: torch.full(shape, 7.0, dtype=dtype, device=DEV)
    oq, oc, og = sent(n, C, C), sent(n * C, m), sent(n, n * C, C)
    quad, cols, gat = (_hip.fn(f, dtype) for f in ("wiski_jet_quadform", "wiski_wt_columns_jet", "wiski_gather_jet"))
    refused = [("quadform x", quad(grid.ref, None, i64(n), p(M), i64(m), p(oq), p(err), s)),
               ("quadform M", quad(grid.ref, p(x), i64(n), None, i64(m), p(oq), p(err), s)),
               ("quadform out", quad(grid.ref, p(x), i64(n), p(M), i64(m), None, p(err), s)),
               ("quadform err", quad(grid.ref, p(x), i64(n), p(M), i64(m), p(oq), None, s)),
               ("quadform ldm", quad(grid.ref, p(x), i64(n), p(M), i64(m - 1), p(oq), p(err), s)),
               ("columns x", cols(grid.ref, None, i64(n), p(oc), p(err), s)),
               ("columns out", cols(grid.ref, p(x), i64(n), None, p(err), s)),
               ("columns err", cols(grid.ref, p(x), i64(n), p(oc), None, s)),
               ("gather x", gat(grid.ref, None, i64(n), p(V), i32(n * C), i32(0), p(og), p(err), s)),
               ("gather V", gat(grid.ref, p(x), i64(n), None, i32(n * C), i32(0), p(og), p(err), s)),
               ("gather out", gat(grid.ref, p(x), i64(n), p(V), i32(n * C), i32(0), None, p(err), s)),
               ("gather err", gat(grid.ref, p(x), i64(n), p(V), i32(n * C), i32(0), p(og), None, s)),
               ("gather k", gat(grid.ref, p(x), i64(n), p(V), i32(0), i32(0), p(og), p(err), s)),
               ("gather rows_per_point", gat(grid.ref, p(x), i64(n), p(V), i32(C), i32(-1), p(og), p(err), s))]
    torch.cuda.synchronize()
    assert [(what, rc) for what, rc in refused if rc != -1] == []
    assert all(bool((o == 7.0).all()) for o in (oq, oc, og)) and _flag(err) == 0
    empty = [quad(grid.ref, None, i64(0), None, i64(m), None, None, s), cols(grid.ref, None, i64(0), None, None, s),
             gat(grid.ref, None, i64(0), None, i32(1), i32(0), None, None, s)]
    assert empty == [0, 0, 0]
    x0 = x[:0]
    assert grid_ops.jet_quadform(grid, x0, M, err).shape == (0, C, C) and grid_ops.wt_columns_jet(grid, x0, err).shape == (0, m)
    assert grid_ops.gather_jet(grid, x0, V[:3], err).shape == (0, 3, C)


# ---------------------------------------------------------------------------------------------------------------- the model
def _t(a, dtype):
    return torch.as_tensor(a, device=DEV, dtype=dtype)


def _fit(gb, gs, dtype):
    """40 values at construction, 16 value-and-gradient points in one in-place update; the reference of the same data."""
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    grid = gr.Grid.from_bounds(gb, gs)
    D = jr.model_data(grid)
    X, Y, nz, nv = D["X"], D["Y"], D["noise"], D["n_val"]
    m = FixedNoiseOnlineSKIGP(_t(X[:nv], dtype), _t(Y[:nv, :1], dtype), _t(nz[:nv, :1], dtype), grid_bounds=torch.tensor(gb), grid_size=gs,
                              learn_additional_noise=True).eval()
    m.condition_on_observations(_t(X[nv:], dtype), _t(Y[nv:, 0], dtype), _t(nz[nv:, 0], dtype), inplace=True,
                                grad_Y=_t(Y[nv:, 1:], dtype), grad_noise=_t(nz[nv:, 1:], dtype))
    k = m.covar_module.base_kernel
    ell, s, s2 = k.base_kernel.lengthscale.detach().cpu().numpy().reshape(-1), float(k.outputscale), float(m.likelihood.second_noise)
    ref = jr.JetGP(gr.GradObsGP(grid, gr.dense_kuu(grid, "rbf", ell, s), s2).fit(X, Y, nz, D["present"]))
    return m, ref, D


def _rel(got, want):
    return float(np.abs(got.detach().double().cpu().numpy() - want).max() / np.abs(want).max())


def _check_model(m, ref, D, dtype, label):
    Xs = D["Xs"]
    n, C = Xs.shape[0], Xs.shape[1] + 1
    mean, cov = ref.jet(Xs)
    B = jr.blocks_of(cov, n, C)
    Xq = _t(Xs, dtype)
    jp = m.posterior_jet(Xq)
    jj = m.posterior_jet(Xq, joint=True)
    var = m(Xq).variance.detach()
    v = np.random.default_rng(2).standard_normal(C - 1)
    dm, dv = jp.directional(_t(v, dtype))
    e = {"mean": _rel(jp.mean, mean), "blocks": _rel(jp.covariance, B), "joint": _rel(jj.covariance, cov),
         "joint diagonal blocks": _rel(jj.grad_covariance, B[:, 1:, 1:]), "joint mean": _rel(jj.mean, mean),
         "value variance vs posterior": float((jp.value_variance - var).abs().max() / var.abs().max()),
         "directional mean": _rel(dm, mean[:, 1:] @ v), "directional variance": _rel(dv, np.einsum("i,pij,j->p", v, B[:, 1:, 1:], v))}
    print(f"{label} {dtype}: " + "  ".join(f"{k} {x:.3e}" for k, x in e.items()) + f"  (bound {RTOL[dtype]:.0e})")
    assert jp.mean.shape == (n, C) and jp.covariance.shape == (n, C, C) and jj.covariance.shape == (n * C, n * C)
    assert jp.grad_mean.shape == (n, C - 1) and jp.grad_covariance.shape == (n, C - 1, C - 1) and jp.value_mean.shape == (n,)
    assert not jp.mean.requires_grad and not jp.covariance.requires_grad
    assert max(e.values()) <= RTOL[dtype]
    # the last query sits in a boundary cell of dim 0: that partial is identically zero, with zero (co)variance
    assert float(jp.mean[-1, 1]) == 0.0 and float(jp.covariance[-1, 1].abs().max()) == 0.0 and float(jp.covariance[-1, :, 1].abs().max()) == 0.0
    assert torch.equal(jp.covariance, jp.covariance.transpose(-1, -2)) and torch.equal(jj.covariance, jj.covariance.t())
    return jp


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_posterior_jet_dense_regime(dtype):
    m, ref, D = _fit([[-1.0, 1.0]] * 2, [12, 10], dtype)
    jp = _check_model(m, ref, D, dtype, "dense")
    assert hasattr(m.prediction_cache["pred_cov"], "dense") and jp.cg_iters == []


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_posterior_jet_matrix_free_regime(dtype):
    """10 x 9 x 8 grid; variance_chunk = 16 gives 4 points (16 columns) per solve: six chunks for the 23 queries."""
    from online_gp_amd import settings

    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(1e-10 if dtype == torch.float64 else 1e-6), \
            settings.variance_chunk(16):
        m, ref, D = _fit([[-1.0, 1.0]] * 3, [10, 9, 8], dtype)
        jp = _check_model(m, ref, D, dtype, "matrix-free")
        assert not hasattr(m.prediction_cache["pred_cov"], "dense") and len(jp.cg_iters) == 6


@pytest.mark.parametrize("joint", [False, True], ids=["blocks", "joint"])
def test_rsample_covariance(joint):
    """4 096 draws from fixed base samples.  For Gaussian draws the sample covariance S of N draws has
    var S_ij = (C_ii C_jj + C_ij^2) / (N - 1) <= 2 C_ii C_jj / (N - 1); the sample mean has var C_ii / N.  Six standard deviations
    per entry (about 13 000 entries in the joint case: a 6-sigma event has probability 2e-9 each), plus the jitter."""
    dtype, N = torch.float64, 4096
    m, ref, D = _fit([[-1.0, 1.0]] * 2, [12, 10], dtype)
    jp = m.posterior_jet(_t(D["Xs"], dtype), joint=joint)
    n, C = jp.mean.shape
    z = torch.as_tensor(np.random.default_rng(9).standard_normal((N, n, C)), device=DEV, dtype=dtype)
    draws = jp.rsample(torch.Size([N]), base_samples=z)
    assert draws.shape == (N, n, C) and torch.equal(draws, jp.rsample(torch.Size([N]), base_samples=z))
    dc = draws - draws.mean(0)
    if joint:
        cov = jp.covariance
        S = dc.reshape(N, -1).t() @ dc.reshape(N, -1) / (N - 1)
        dg = cov.diagonal()
        jit = 1e-10 * dg.mean()
    else:
        cov = jp.covariance
        S = torch.einsum("spi,spj->pij", dc, dc) / (N - 1)
        dg = cov.diagonal(dim1=-2, dim2=-1)
        jit = 1e-10 * dg.mean(-1)[:, None, None]
    dgj = dg + (1e-10 * dg.mean() if joint else 1e-10 * dg.mean(-1, keepdim=True))
    bound = 6.0 * (2.0 * dgj[..., :, None] * dgj[..., None, :] / (N - 1)).sqrt() + jit
    ratio = float(((S - cov).abs() / bound.clamp_min(1e-300)).max())
    mb = 6.0 * (dgj.reshape(n, C) / N).sqrt()
    mratio = float(((draws.mean(0) - jp.mean).abs() / mb.clamp_min(1e-300)).max())
    print(f"rsample joint={joint}: covariance deviation / bound {ratio:.3f}, mean deviation / bound {mratio:.3f}")
    assert ratio <= 1.0 and mratio <= 1.0
    assert float(draws[:, -1, 1].abs().max()) <= 1e-4 * float(dgj.max().sqrt())        # the zero-variance channel moves by the jitter only


def test_refusals_and_pass_throughs():
    from online_gp_amd.models import FixedNoiseOnlineSKIGP, Identity, LinearStem, OnlineSKIBotorchModel, OnlineSKIRegression

    dtype = torch.float64
    grid = gr.Grid.from_bounds([[-1.0, 1.0]] * 2, [12, 10])
    D = jr.model_data(grid)
    X, Y = _t(D["X"], dtype), _t(D["Y"], dtype)
    m, ref, _ = _fit([[-1.0, 1.0]] * 2, [12, 10], dtype)
    with pytest.raises(NotImplementedError):
        m.posterior_jet(X[None])
    two = FixedNoiseOnlineSKIGP(X, Y[:, :2], None, grid_bounds=torch.tensor([[-1.0, 1.0]] * 2), grid_size=[12, 10]).eval()
    with pytest.raises(NotImplementedError):
        two.posterior_jet(X)
    with pytest.raises(Exception):                                      # outside the grid: the posterior call's own error
        m.posterior_jet(_t([[5.0, 0.0]], dtype))
    bm = OnlineSKIBotorchModel(X, Y[:, :1], torch.ones_like(Y[:, :1]), grid_bounds=torch.tensor([[-1.0, 1.0]] * 2), grid_size=[12, 10])
    jb = bm.posterior_jet(X[:7].float())
    assert jb.mean.shape == (7, 3) and jb.covariance.shape == (7, 3, 3) and jb.mean.dtype == dtype
    assert float((jb.value_variance - bm.posterior(X[:7]).variance.reshape(-1)).abs().max()) <= 1e-4 * float(jb.value_variance.max())
    reg = OnlineSKIRegression(Identity(2), X, Y[:, :1], 1e-3, 10, 1.0)
    gm, gc = reg.predict_gradient(X[:7])
    jr_ = reg.gp.posterior_jet(X[:7])
    assert gm.shape == (7, 2) and gc.shape == (7, 2, 2) and torch.equal(gm, jr_.grad_mean) and torch.equal(gc, jr_.grad_covariance)
    lin = OnlineSKIRegression(LinearStem(2, 2).to(DEV).to(dtype), X, Y[:, :1], 1e-3, 10, 1.0)
    with pytest.raises(NotImplementedError):
        lin.predict_gradient(X[:7])
