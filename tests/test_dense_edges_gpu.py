"""GPU: the dense GEMM, Cholesky, triangular solves, log-determinant and root update at their edges, on every path, through the C ABI.

Every operand and output is a WINDOW of a larger parent buffer (tests/dense_reference.py): leading dimensions larger than the row, base
pointers off the 16-byte grid, NaN wherever a kernel must not read and a pattern with NaN canaries wherever it must not write -- the
parent outside the window is compared bitwise after every call.  References are fp64, from the inputs cast to the tested dtype.  The
GEMM cases are the table of dense_reference.GEMM_TABLE: each row names the kernel it reaches, and the test asserts that through
wiski_gemm_path before it runs it, so a retuned threshold moves no coverage silently.

Conditioning.  The factorisations multiply panels by explicitly inverted diagonal blocks, which is backward stable only up to the
condition of those blocks.  Measured on `graded` matrices (Q diag(lambda) Q^T, lambda log-spaced in [1, kappa], kappa = 1e4 in fp32 and
1e10 in fp64): eta = max |A - L L^T| / ((n + 1) u |Lref| |Lref^T|) of wiski_potrf and rho = max |L X - B| / (n u |Lref| |Xref|) of
wiski_trsm on that factor with 5 right-hand sides, beside the same figures of LAPACK in the same precision on the same matrix (host)
and skeel(Lref) = || |Lref^-1| |Lref| ||_inf.  The bar of test_conditioning_of_factor_and_solve is 8 x max(1, LAPACK's figure).

Measured on an MI355X (LAPACK's figures depend on the host's BLAS in their last digits; the test recomputes them where it runs):

    n    dtype  path of wiski_potrf            eta_gpu  eta_lapack   rho_gpu  rho_lapack   skeel(Lref)
    100  fp32   one launch                     0.035    0.062        0.017    0.013        9.3e2
    100  fp64   one launch                     0.11     0.12         0.020    0.021        4.8e5
    480  fp32   one launch                     0.032    0.010        0.0037   0.0054       4.0e3
    480  fp64   one launch                     0.021    0.039        0.0044   0.0047       2.2e6
    513  fp32   two-level, 2 big blocks        0.027    0.0098       0.0036   0.0054       4.3e3
    513  fp64   two-level, 2 big blocks        0.048    0.040        0.0052   0.0046       2.3e6
    897  fp32   two-level, 3 big blocks        0.015    0.0086       0.0023   0.0051       7.5e3
    897  fp64   two-level, 3 big blocks        0.025    0.035        0.0027   0.0033       4.0e6

Every figure is far below 1, the size of the textbook bounds, and within a factor of 3.2 of LAPACK's: on these matrices the explicitly
inverted 32- and 64-wide diagonal blocks cost nothing measurable, although skeel(Lref) -- what they could cost in the worst case -- is
1e3 .. 4e6.
"""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dense_reference as dr

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float64]
TRANSPOSES = [(False, False), (True, False), (False, True), (True, True)]
NAN = float("nan")


def _p(t):
    """Device address of a view's first element, also of an empty view (K = 0 operands), whose data_ptr() is NULL."""
    return ctypes.c_void_p(t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size())


def _i(v):
    return ctypes.c_int32(int(v))


def _stream():
    from online_gp_amd import _hip

    return _hip.stream_ptr(torch.device(DEV))


def _fn(name, dtype):
    from online_gp_amd import _hip

    return _hip.fn(name, dtype)


def _name(dtype):
    return "f32" if dtype == torch.float32 else "f64"


def _gemm(dtype, ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc):
    from online_gp_amd import _hip

    cr = _hip.creal(dtype)
    return _fn("wiski_gemm", dtype)(_i(ta), _i(tb), _i(M), _i(N), _i(K), cr(alpha), _p(A), _i(lda), _p(B), _i(ldb), cr(beta), _p(C), _i(ldc), _stream())


def _filled(rows, cols, ld, lead, dtype, fill, values):
    parent, view = dr.window(rows, cols, ld, lead, dtype, fill, DEV)
    if values is not None:
        view.copy_(values)
    return parent, view


# ----------------------------------------------------------------------------------------------------- GEMM ---
def _layouts(dtype):
    """(pad, lead): contiguous and aligned; a leading dimension that defeats the 16-byte loads; a leading dimension that allows them
    behind a base pointer that does not (k_gemm128::fetch tests both)."""
    return [(0, 0), (3, 0), (4 if dtype == torch.float32 else 2, 1)]


@pytest.mark.parametrize("ta,tb", TRANSPOSES, ids=["nn", "tn", "nt", "tt"])
@pytest.mark.parametrize("dtype,shape,path", dr.GEMM_CASES, ids=[f"{_name(dt)}-{s[0]}x{s[1]}x{s[2]}-k{p}" for dt, s, p in dr.GEMM_CASES])
def test_gemm_every_path_on_windows(dtype, shape, path, ta, tb):
    """Per table row, transpose pair and operand layout: alpha = 0.7, beta = -0.3 on random data within 10 tol sqrt(max(K, 1)) per element
    (tol = 2e-5 / 1e-12); beta = 0 into a C that holds NaN (what root_update_impl and potrf_two_level do into fresh scratch): every
    element finite and within the same bar; integer operands, exact in fp32, with (alpha, beta) in {(1, 0), (1, 1), (-1, 1), (0.5, 0)}:
    torch.equal with the fp64 reference.  C is a window with ldc = N + 5; its parent outside the window is bitwise unchanged."""
    from online_gp_amd import grid_ops

    M, N, K = shape
    assert grid_ops.gemm_path(M, N, K, dtype) == path                  # the kernel this row is here for
    bar = 10 * (2e-5 if dtype == torch.float32 else 1e-12) * math.sqrt(max(K, 1))
    g = torch.Generator(device="cpu").manual_seed(M * 7 + N * 3 + K + 2 * ta + tb)
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    Ash, Bsh = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
    Ar, Br, Cr = (torch.randn(s, generator=g, dtype=torch.float64).to(DEV, dtype) for s in (Ash, Bsh, (M, N)))
    Ai, Bi, Ci = (dr.int_operands(s, rng, K=max(K, 1)).to(DEV, dtype) for s in (Ash, Bsh, (M, N)))
    cases = [("random", Ar, Br, Cr, 0.7, -0.3), ("nan-C", Ar, Br, None, 0.7, 0.0)] + [("int", Ai, Bi, Ci, a, b) for a, b in dr.INT_COEFFS]
    refs = [dr.gemm_ref(a, A, ta, B, tb, b, (C if C is not None else Cr), dtype) for _, A, B, C, a, b in cases]
    for pad, lead in _layouts(dtype):
        lda, ldb, ldc = Ash[1] + pad, Bsh[1] + pad, N + 5
        wins = {}
        for key, A, B in (("r", Ar, Br), ("i", Ai, Bi)):
            wins[key] = (_filled(Ash[0], Ash[1], lda, lead, dtype, "nan", A)[1], _filled(Bsh[0], Bsh[1], ldb, lead, dtype, "nan", B)[1])
        if lead:
            assert all(_p(w).value % 16 != 0 for pair in wins.values() for w in pair)
        pc0, Cw0 = dr.window(M, N, ldc, lead, dtype, "pattern", DEV)
        for (kind, A, B, C0, alpha, beta), ref in zip(cases, refs):
            Aw, Bw = wins["i" if kind == "int" else "r"]
            pc = pc0.clone()
            Cw = pc.as_strided((M, N), (ldc, 1), Cw0.storage_offset())
            if C0 is None:
                Cw.fill_(NAN)
            elif beta == 0.0:
                Cw.fill_(-77.0)                                            # finite, and wrong everywhere if it were read
            else:
                Cw.copy_(C0)
            before = pc.clone()
            assert _gemm(dtype, ta, tb, M, N, K, alpha, Aw, lda, Bw, ldb, beta, Cw, ldc) == 0
            tag = (kind, alpha, beta, pad, lead)
            assert dr.outside_unchanged(before, pc, Cw), tag
            if kind == "int":
                assert torch.equal(Cw.double(), ref), tag
            else:
                assert bool(torch.isfinite(Cw).all()), tag
                err = float((Cw.double() - ref).abs().max())
                assert err <= bar, (tag, err, bar)
            if K == 0:                                                     # C = beta C exactly; exact zeros for beta = 0 whatever C held
                want = torch.zeros_like(Cw) if beta == 0.0 else torch.tensor(beta, dtype=dtype, device=DEV) * C0
                assert torch.equal(Cw, want), tag


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_gemm_refuses_short_leading_dimensions_and_touches_nothing(dtype):
    """lda < (ta ? M : K), ldb < (tb ? K : N), ldc < N, K < 0 and NULL operands: WISKI_E_BADARG, C bitwise as it was.  M <= 0 or
    N <= 0: WISKI_OK, nothing to do, nothing touched.  The smallest legal leading dimensions are accepted."""
    M, N, K = 40, 50, 30
    _, Aw = _filled(64, 64, 64, 0, dtype, "nan", torch.ones(64, 64, dtype=dtype))
    _, Bw = _filled(64, 64, 64, 0, dtype, "nan", torch.ones(64, 64, dtype=dtype))
    pc, Cw = dr.window(64, 64, 64, 0, dtype, "pattern", DEV)
    before = pc.clone()
    for ta, tb in TRANSPOSES:
        la, lb = (M if ta else K), (K if tb else N)
        for lda, ldb, ldc in ((la - 1, lb, N), (la, lb - 1, N), (la, lb, N - 1), (0, lb, N), (la, -5, N)):
            assert _gemm(dtype, ta, tb, M, N, K, 1.0, Aw, lda, Bw, ldb, 0.0, Cw, ldc) == -1, (ta, tb, lda, ldb, ldc)
        assert _gemm(dtype, ta, tb, M, N, -1, 1.0, Aw, la, Bw, lb, 0.0, Cw, N) == -1
        for m_, n_ in ((0, N), (M, 0), (-1, N), (M, -7)):
            assert _gemm(dtype, ta, tb, m_, n_, K, 1.0, Aw, 1, Bw, 1, 0.0, Cw, 1) == 0
    from online_gp_amd import _hip

    cr, null = _hip.creal(dtype), ctypes.c_void_p(None)
    for a_, b_, c_ in ((null, _p(Bw), _p(Cw)), (_p(Aw), null, _p(Cw)), (_p(Aw), _p(Bw), null)):
        assert _fn("wiski_gemm", dtype)(_i(0), _i(0), _i(M), _i(N), _i(K), cr(1.0), a_, _i(K), b_, _i(N), cr(0.0), c_, _i(N), _stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(dr.bits(before), dr.bits(pc))
    assert _gemm(dtype, False, False, M, N, K, 1.0, Aw, K, Bw, N, 0.0, Cw, N) == 0        # the bounds themselves are legal
    assert torch.equal(pc[Cw.storage_offset():Cw.storage_offset() + M * N], torch.full((M * N,), float(K), dtype=dtype, device=DEV))


# ----------------------------------------------------------------------------------------------------- TRSM ---
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("nrhs", [1, 5, 64, 65, 130])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_trsm_windows_ragged_blocks_and_column_tiles(dtype, trans, nrhs, n):
    """wiski_trsm with ldl = n + 3, ldb = nrhs + 5: one and several 64-blocks with a ragged last one, one and several column tiles of
    k_apply_inv with a ragged last one.  The strict upper triangle of L and all its padding hold NaN: only the lower triangle is
    referenced (k_tri_inv_blocks loads t <= r, the update GEMMs address blocks strictly below the diagonal)."""
    tol = 5e-4 if dtype == torch.float32 else 1e-10
    L = dr.chol_ref(dr.well(n).to(dtype)).to(dtype)
    B = dr.rhs(n, nrhs).to(dtype)
    Xref = dr.solve_ref(L, B, trans).to(DEV)
    _, Lw = _filled(n, n, n + 3, 0, dtype, "nan", L)
    Lw.masked_fill_(torch.triu(torch.ones(n, n, dtype=torch.bool, device=DEV), 1), NAN)
    pb, Bw = _filled(n, nrhs, nrhs + 5, 0, dtype, "pattern", B)
    before = pb.clone()
    assert _fn("wiski_trsm", dtype)(_i(trans), _i(n), _i(nrhs), _p(Lw), _i(n + 3), _p(Bw), _i(nrhs + 5), _stream()) == 0
    assert dr.outside_unchanged(before, pb, Bw)
    X = Bw.double()
    assert bool(torch.isfinite(X).all())
    Ld = L.double().to(DEV)
    res = float(((Ld.t() if trans else Ld) @ X - B.double().to(DEV)).abs().max())
    err = float((X - Xref).abs().max())
    assert res < 50 * tol, res
    assert err < 10 * tol * max(1.0, float(Xref.abs().max())), err


# ------------------------------------------------------------------------------------------------- Cholesky ---
def _potrf_inverse(dtype, n, Aw, lda, Xw, ldx, info):
    return _fn("wiski_potrf_inverse", dtype)(_i(n), _p(Aw), _i(lda), _p(Xw), _i(ldx), _p(info), _stream())


def _potrf(dtype, n, Aw, lda, info):
    return _fn("wiski_potrf", dtype)(_i(n), _p(Aw), _i(lda), _p(info), _stream())


def _check_factor_windows(dtype, n, A, tol):
    """wiski_potrf_inverse and wiski_potrf on windows (lda = n + 3 in NaN, ldx = n + 5 in a pattern) against the fp64 reference at the
    bars of test_cholesky_with_explicit_inverse; strict upper triangles exactly zero; padding bitwise unchanged."""
    Lref = dr.chol_ref(A).to(DEV)
    Xref = torch.linalg.solve_triangular(Lref, torch.eye(n, dtype=torch.float64, device=DEV), upper=False)
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool, device=DEV), 1)
    pa, Aw = _filled(n, n, n + 3, 0, dtype, "nan", A)
    px, Xw = dr.window(n, n, n + 5, 0, dtype, "pattern", DEV)
    info = torch.zeros(1, dtype=torch.int32, device=DEV)
    ba, bx = pa.clone(), px.clone()
    assert _potrf_inverse(dtype, n, Aw, n + 3, Xw, n + 5, info) == 0
    assert int(info.item()) == 0
    assert dr.outside_unchanged(ba, pa, Aw) and dr.outside_unchanged(bx, px, Xw)
    L, X = Aw.double(), Xw.double()
    assert bool((Aw[upper] == 0).all()) and bool((Xw[upper] == 0).all())
    assert float((L - Lref).abs().max()) < tol * 10
    assert float((X - Xref).abs().max()) < tol * 10 * max(1.0, float(Xref.abs().max()))
    assert float((X @ L - torch.eye(n, dtype=torch.float64, device=DEV)).abs().max()) < tol * 50
    pa2, Aw2 = _filled(n, n, n + 3, 0, dtype, "nan", A)
    ba2 = pa2.clone()
    assert _potrf(dtype, n, Aw2, n + 3, info) == 0
    assert int(info.item()) == 0
    assert dr.outside_unchanged(ba2, pa2, Aw2)
    assert bool((Aw2[upper] == 0).all())
    assert float((Aw2.double() - Lref).abs().max()) < tol * 10
    assert torch.equal(Aw2, Aw)                                           # with and without the inverse: the same factor, bit for bit


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [1, 31, 33, 100, 327, 480, 481, 512, 513, 897])
def test_cholesky_and_inverse_windows(dtype, n):
    """One launch of cooperating workgroups (n <= 480, with the inverse in the same launch), the 481..512 hand-over (one-launch factor, blocked
    solve for the inverse), two-level with 2 (513) and 3 (897) big blocks -- all with leading dimensions larger than n."""
    _check_factor_windows(dtype, n, dr.well(n).to(dtype), 5e-4 if dtype == torch.float32 else 1e-10)


def _check_info_semantics(dtype, n):
    """*d_info |= 1: preset to 4 it stays 4 on success and becomes 5 on a failing pivot -- the first of the matrix, and the last of the
    last block -- through both entries; the padding of A stays as it was either way."""
    A = dr.well(n)
    for which, M_, want in (("ok", A, 4), ("first", dr.first_pivot_fails(A), 5), ("last", dr.last_pivot_fails(A, dtype), 5)):
        for inverse in (False, True):
            pa, Aw = _filled(n, n, n + 3, 0, dtype, "nan", M_.to(dtype))
            before = pa.clone()
            info = torch.full((1,), 4, dtype=torch.int32, device=DEV)
            if inverse:
                px, Xw = dr.window(n, n, n + 5, 0, dtype, "pattern", DEV)
                bx = px.clone()
                assert _potrf_inverse(dtype, n, Aw, n + 3, Xw, n + 5, info) == 0
                assert dr.outside_unchanged(bx, px, Xw), (which, inverse)
            else:
                assert _potrf(dtype, n, Aw, n + 3, info) == 0
            assert int(info.item()) == want, (which, inverse, int(info.item()))
            assert dr.outside_unchanged(before, pa, Aw), (which, inverse)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [100, 500, 897])
def test_cholesky_info_is_ored_not_overwritten(dtype, n):
    _check_info_semantics(dtype, n)


# --------------------------------------------------------------------------------------------- conditioning ---
def _conditioning_figures(dtype, n):
    c = dr.graded_case(n, dtype)
    A, B, Lref, Xref = (c[k].to(DEV) for k in ("A", "B", "Lref", "Xref"))
    L = A.clone()
    info = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert _potrf(dtype, n, L, n, info) == 0 and int(info.item()) == 0
    X = B.clone()
    assert _fn("wiski_trsm", dtype)(_i(0), _i(n), _i(B.shape[1]), _p(L), _i(n), _p(X), _i(B.shape[1]), _stream()) == 0
    return c, dr.eta(A, L, c["u"], Lref), dr.rho(L, X, B, c["u"], Lref, Xref)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [100, 480, 513, 897])
def test_conditioning_of_factor_and_solve(dtype, n):
    """kappa = 1e4 (fp32) / 1e10 (fp64), default paths: one launch (100, 480), two-level with 2 and 3 big blocks (513, 897).  The bar is
    8 x max(1, the figure of LAPACK in the same precision on the same matrix): three bits for the other accumulation order of the MFMA
    blocks and the rsqrt-plus-Newton pivots.  Figures: the table at the top of this module."""
    c, eta_gpu, rho_gpu = _conditioning_figures(dtype, n)
    print(f"conditioning n={n} {_name(dtype)}: eta_gpu={eta_gpu:.3g} eta_ref={c['eta_ref']:.3g} rho_gpu={rho_gpu:.3g} rho_ref={c['rho_ref']:.3g} "
          f"skeel={c['skeel']:.3g}")
    assert eta_gpu <= 8.0 * max(1.0, c["eta_ref"]), (eta_gpu, c["eta_ref"])
    assert rho_gpu <= 8.0 * max(1.0, c["rho_ref"]), (rho_gpu, c["rho_ref"])


# -------------------------------------------------------------------------------------------------- logdiag ---
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_logdiag_adds_to_its_output_and_honours_lda(dtype, n):
    """*d_out += sum log a_ii with *d_out preset to 2.5, lda = n + 3, NaN everywhere off the diagonal; one and several blocks of 256.
    Reference: 2.5 + sum log(a_ii) of the cast values in extended precision.  Bar: 4 n 2^-53 sum |log a_ii| (n doubles summed in any
    order, doubled for the device log).  The bound leaves out the rounding of the sum onto the preset (half an ulp of a number near
    2.5 +- 1.8, up to 2^-52); the diagonal keeps |log a_ii| >= 0.9 with the first entry below one (n = 1: a sum in [0.7, 1.6], its
    rounding <= 2^-53), so that the stated bar covers it at every n."""
    rng = np.random.default_rng(n)
    mag = rng.uniform(2.5, 6.0, n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    sign[0] = -1.0
    d = torch.as_tensor(mag ** sign).to(dtype)
    _, Aw = dr.window(n, n, n + 3, 0, dtype, "nan", DEV)
    Aw.diagonal().copy_(d)
    out = torch.full((1,), 2.5, dtype=torch.float64, device=DEV)
    assert _fn("wiski_logdiag", dtype)(_i(n), _p(Aw), _i(n + 3), _p(out), _stream()) == 0
    logs = np.log(d.double().numpy().astype(np.longdouble))
    want = np.longdouble(2.5) + logs.sum()
    bar = 4 * n * 2.0 ** -53 * float(np.abs(logs).sum())
    err = abs(float(np.longdouble(out.item()) - want))
    print(f"logdiag n={n} {_name(dtype)}: err={err:.3g} bar={bar:.3g}")
    assert err <= bar, (err, bar)


# ---------------------------------------------------------------------------------------------- root update ---
def _root_update(dtype, m, r, q, L, R, V, short_ws=0):
    """Through the C ABI with ldl = r + 3, ldr = r + 5 (patterned parents: L and R are outputs) and ldv = q + 2 (NaN parent).
    Returns (rc, L', R', padding unchanged)."""
    from online_gp_amd import _hip

    pl, Lw = _filled(m, r, r + 3, 0, dtype, "pattern", L.to(dtype))
    pr, Rw = _filled(m, r, r + 5, 0, dtype, "pattern", R.to(dtype))
    _, Vw = _filled(m, q, q + 2, 0, dtype, "nan", V.to(dtype))
    need = int(_hip.lib().wiski_root_update_workspace_elems(_i(m), _i(r), _i(q)))
    ws = torch.full((need,), NAN, dtype=dtype, device=DEV)               # scratch: the library must not rely on what it holds
    bl, br = pl.clone(), pr.clone()
    rc = _fn("wiski_root_update", dtype)(_i(m), _i(r), _i(q), _p(Lw), _i(r + 3), _p(Rw), _i(r + 5), _p(Vw), _i(q + 2), _p(ws),
                                         ctypes.c_int64(need - short_ws), _stream())
    torch.cuda.synchronize()
    same = dr.outside_unchanged(bl, pl, Lw) and dr.outside_unchanged(br, pr, Rw)
    if short_ws:
        same = same and torch.equal(dr.bits(bl), dr.bits(pl)) and torch.equal(dr.bits(br), dr.bits(pr))
    return rc, Lw, Rw, same


def _root_pair(m, r):
    """L [m, r] and R [m, r] with R^T L = I (fp64, CPU): the Cholesky factor and its inverse transpose for r = m; its first r columns
    and their pseudo-inverse transpose for r < m."""
    L = dr.chol_ref(dr.well(m))[:, :r].contiguous()
    R = torch.linalg.inv(L).t().contiguous() if r == m else L @ torch.linalg.inv(L.t() @ L)
    return L + 0.0, R + 0.0                                                # (+ 0.0: no negative zeros, which x + 0 would not keep)


ROOT_CASES = [("full", 96, 2), ("full", 96, 31), ("full", 96, 32), ("full", 96, 33), ("range", 64, 5), ("range", 64, 33), ("scaled", 96, 7)]


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 2e-4)], ids=["f64", "f32"])
@pytest.mark.parametrize("kind,r,q", ROOT_CASES, ids=[f"{k}-r{r}-q{q}" for k, r, q in ROOT_CASES])
def test_root_update_windows_thin_roots_and_scaled_columns(dtype, tol, kind, r, q):
    """m = 96.  r = m on both sides of the device-Jacobi limit (q = 31, 32 | 33); r = 64 < m with V = L Z inside the range of L, where
    L L^T = A + V V^T holds exactly; V scaled by 1e3 with a repeated column.  Bars of test_root_update_device_and_host_eigensolve:
    tol max|A + V V^T| for the Gram matrix, 50 tol for R^T L - I."""
    m = 96
    L0, R0 = _root_pair(m, r)
    g = torch.Generator(device="cpu").manual_seed(100 * r + q)
    if kind == "range":
        V = L0 @ torch.randn(r, q, generator=g, dtype=torch.float64)
    else:
        V = torch.randn(m, q, generator=g, dtype=torch.float64)
    if kind == "scaled":
        V = 1e3 * V
        V[:, -1] = V[:, 0]
    L0, R0, V = (t.to(dtype) for t in (L0, R0, V))
    want = dr.root_update_ref(L0, V).to(DEV)
    rc, L, R, same = _root_update(dtype, m, r, q, L0, R0, V)
    assert rc == 0 and same
    gram = float(((L.double() @ L.double().t()) - want).abs().max())
    ortho = float((R.double().t() @ L.double() - torch.eye(r, dtype=torch.float64, device=DEV)).abs().max())
    print(f"root update {kind} r={r} q={q} {_name(dtype)}: gram={gram:.3g} bar={tol * float(want.abs().max()):.3g} ortho={ortho:.3g} bar={50 * tol:.3g}")
    assert gram < tol * float(want.abs().max()), gram
    assert ortho < 50 * tol, ortho


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("r,q", [(96, 5), (96, 33), (64, 5)])
def test_root_update_with_no_new_columns_changes_nothing(dtype, r, q):
    """V = 0 (a batch whose points all fell outside the grid), device and host eigensolve: L and R come back bitwise unchanged."""
    m = 96
    L0, R0 = _root_pair(m, r)
    rc, L, R, same = _root_update(dtype, m, r, q, L0, R0, torch.zeros(m, q, dtype=torch.float64))
    assert rc == 0 and same
    assert torch.equal(dr.bits(L.contiguous()), dr.bits(L0.to(DEV, dtype))) and torch.equal(dr.bits(R.contiguous()), dr.bits(R0.to(DEV, dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_root_update_refuses_a_short_workspace(dtype):
    m, r, q = 96, 96, 5
    L0, R0 = _root_pair(m, r)
    rc, _, _, same = _root_update(dtype, m, r, q, L0, R0, dr.rhs(m, q), short_ws=1)
    assert rc == -1 and same


# ------------------------------------------------------------------------------------- the 64-wide fallback ---
def _fallback_child():
    """Runs in a fresh process with WISKI_POTRF_TWO_LEVEL=0: beyond 512 rows wiski_potrf is then the 64-wide right-looking loop
    (potrf_impl: k_potrf_diag, k_apply_inv<0>, one GEMM per block) and wiski_potrf_inverse that factor plus a blocked solve.
    577 leaves a last block of one row for k_potrf_diag and a ragged k_apply_inv<0> tile."""
    assert os.environ.get("WISKI_POTRF_TWO_LEVEL") == "0"
    for dtype in DTYPES:
        tol = 5e-4 if dtype == torch.float32 else 1e-10
        for n in (513, 577, 640):
            A = dr.well(n)
            _check_factor_windows(dtype, n, A.to(dtype), tol)
            for inverse in (False, True):
                pa, Aw = _filled(n, n, n + 3, 0, dtype, "nan", dr.last_pivot_fails(A, dtype).to(dtype))
                info = torch.full((1,), 4, dtype=torch.int32, device=DEV)
                if inverse:
                    _, Xw = dr.window(n, n, n + 5, 0, dtype, "pattern", DEV)
                    assert _potrf_inverse(dtype, n, Aw, n + 3, Xw, n + 5, info) == 0
                else:
                    assert _potrf(dtype, n, Aw, n + 3, info) == 0
                assert int(info.item()) == 5, (dtype, n, inverse, int(info.item()))
    print("fallback path ok")


def test_blocked_fallback_cholesky_in_a_fresh_process():
    """WISKI_POTRF_TWO_LEVEL=0 (also what a device without the LDS opt-in gets) is read once per process: one child runs
    n = 513, 577, 640 in both dtypes with lda = n + 3 against the fp64 reference at the bars of test_cholesky_with_explicit_inverse, and
    the last-pivot failure, which must set the flag."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_dense_edges_gpu as t; t._fallback_child()"
    env = dict(os.environ, WISKI_POTRF_TWO_LEVEL="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fallback path ok" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])
