"""CPU: the kernel choice of wiski_gemm as a stated table (wiski_gemm_path launches nothing and loads without a GPU), the proof that moving
the choice into one host function changed it for no shape, and the self-checks of tests/dense_reference.py -- the windows, the exact
integer operands, the SPD families, the failing-pivot constructions and the same-precision LAPACK figures that tests/test_dense_edges_gpu.py
judges the kernels against."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dense_reference as dr

DTYPES = [torch.float32, torch.float64]


@pytest.fixture(scope="module")
def built_lib():
    from online_gp_amd import _hip

    if not os.path.exists(_hip._SO):
        _hip.build()
    lib = ctypes.CDLL(_hip._SO)
    lib.wiski_gemm_path.argtypes = [ctypes.c_int32] * 4
    lib.wiski_gemm_path.restype = ctypes.c_int
    return lib


def _eb(dtype):
    return 4 if dtype == torch.float32 else 8


def test_gemm_case_table_names_the_kernel_of_every_row(built_lib):
    got = [(dt, shape, built_lib.wiski_gemm_path(*shape, _eb(dt))) for dt, shape, _ in dr.GEMM_CASES]
    want = [(dt, shape, path) for dt, shape, path in dr.GEMM_CASES]
    assert got == want
    for dt in DTYPES:
        assert {p for d_, _, p in dr.GEMM_CASES if d_ == dt} == {0, 1, 2, 3}, dt      # each kernel is reached in each dtype
    # the thin wrapper of the package answers the same
    from online_gp_amd import grid_ops

    assert all(grid_ops.gemm_path(*shape, dt) == path for dt, shape, path in dr.GEMM_CASES)


def test_gemm_path_refuses_bad_arguments(built_lib):
    for args in ((0, 5, 5, 4), (5, 0, 5, 8), (5, 5, -1, 4), (5, 5, 5, 2), (5, 5, 5, 16), (-3, 5, 5, 8)):
        assert built_lib.wiski_gemm_path(*args) == -1, args
    assert built_lib.wiski_gemm_path(5, 5, 0, 4) == 0                                     # K = 0 is legal


def test_gemm_dispatch_is_unchanged_for_random_shapes(built_lib):
    """The selection moved out of launch_gemm into one host function: for 6000 random shapes -- uniform ones, and ones drawn around
    every threshold (tile counts 110 / 240 / 300 / 500 / 800 / 900, 32 / 128 big tiles, K = 64 / 128 / 256, M N = 8192) -- it
    answers what the old conditions, written out in dense_reference.old_gemm_dispatch, answer."""
    rng = np.random.default_rng(20)
    env = int(os.environ.get("WISKI_GEMM32_MAX_TILES", "0") or 0)              # the one switch both read
    shapes = [tuple(int(v) for v in rng.integers(1, 2600, 3)) for _ in range(3000)]
    edges_mn = [64 * t for t in (1, 2, 10, 11, 15, 16, 17, 20, 22, 23, 25, 28, 29, 30, 31, 32)] + [90, 91, 128, 1409, 2049]
    edges_k = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
    for _ in range(3000):
        M, N = (int(rng.choice(edges_mn)) + int(rng.integers(-1, 2)) for _ in range(2))
        shapes.append((max(M, 1), max(N, 1), int(rng.choice(edges_k))))
    seen = set()
    for M, N, K in shapes:
        for eb in (4, 8):
            got = built_lib.wiski_gemm_path(M, N, K, eb)
            assert got == dr.old_gemm_dispatch(M, N, K, eb, env), (M, N, K, eb)
            seen.add((eb, got))
    assert seen == {(eb, p) for eb in (4, 8) for p in range(4)}


def test_integer_cases_are_exact_in_fp32():
    rng = np.random.default_rng(0)
    for dt, (M, N, K), _ in dr.GEMM_CASES:
        assert dr.int_exact(max(K, 1))
        A = dr.int_operands((M, K), rng, K=max(K, 1))
        assert A.shape == (M, K) and torch.equal(A, A.round()) and (A.numel() == 0 or float(A.abs().max()) <= 8)
    with pytest.raises(AssertionError):
        dr.int_operands((4, 4), rng, amax=8, K=2 ** 18)
    # the claim itself, where it is cheapest to break: a long fp32 dot product of the largest entries, summed in two orders
    a = torch.full((4096,), 8.0, dtype=torch.float32)
    assert float((a * a).sum()) == float((a * a).flip(0).cumsum(0)[-1]) == 4096 * 64


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", ["nan", "pattern"])
def test_window_round_trips_and_outside_unchanged_sees_single_elements(dtype, fill):
    rows, cols, ld, lead = 5, 7, 10, 1
    parent, view = dr.window(rows, cols, ld, lead, dtype, fill)
    assert view.shape == (rows, cols) and view.stride() == (ld, 1)
    assert view.data_ptr() == parent.data_ptr() + view.storage_offset() * parent.element_size()
    assert (view.data_ptr() % 16 != 0) and dr.window(rows, cols, ld, 0, dtype, fill)[1].data_ptr() % 16 == 0
    vals = torch.arange(rows * cols, dtype=dtype).reshape(rows, cols) + 1
    before = parent.clone()
    view.copy_(vals)
    assert torch.equal(view, vals)                                               # what is written through the view is read back
    off = view.storage_offset()
    assert float(parent[off]) == 1.0 and float(parent[off + ld + 2]) == cols + 3
    assert dr.outside_unchanged(before, parent, view)                             # writes inside the window do not count
    m = dr.outside_mask(parent, view)
    assert int((~m).sum()) == rows * cols
    if fill == "nan":
        assert bool(torch.isnan(parent[m]).all())
    else:
        assert off - lead >= ld and bool(torch.isnan(parent[:off - lead]).all()) and bool(torch.isnan(parent[off + rows * ld:]).all())
        body = parent[off - lead:off + rows * ld][m[off - lead:off + rows * ld]]
        assert bool(torch.isfinite(body).all()) and float(body.max()) <= -1000.0
    # one flipped element in the row padding, before the window, and after it
    for pos in (off + cols, off - 1, off + (rows - 1) * ld + cols, parent.numel() - 1, 0):
        if lead == 0 and pos == off - 1 and fill == "nan":
            continue
        after = parent.clone()
        dr.bits(after)[pos] ^= 1
        assert not dr.outside_unchanged(parent, after, view), pos
    # a NaN overwritten by a NaN of another payload
    after = parent.clone()
    nan_pos = int(torch.nonzero(torch.isnan(parent) & m)[0])
    dr.bits(after)[nan_pos] ^= 1
    assert bool(torch.isnan(after[nan_pos])) and not dr.outside_unchanged(parent, after, view)
    # an empty window (K = 0 operands) still has a parent to point at
    p0, v0 = dr.window(4, 0, 0, 0, dtype, fill)
    assert v0.shape == (4, 0) and p0.numel() >= 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [100, 480, 513, 897])
def test_graded_family_and_the_lapack_yardstick(dtype, n, record_property):
    """cond(graded) is kappa to 1 % (also after the cast), and LAPACK's own factor / solve in the tested dtype give the eta_ref / rho_ref
    that the GPU figures are compared with (printed and recorded; both are O(1) by Higham's theorems -- asserted loosely, below 8)."""
    kappa = dr.KAPPA[dtype]
    A64 = dr.graded(n, kappa)
    assert torch.equal(A64, A64.t())
    for A in (A64, A64.to(dtype).double()):
        ev = np.linalg.eigvalsh(A.numpy())
        assert abs(ev[-1] / ev[0] / kappa - 1.0) < 1e-2
    c = dr.graded_case(n, dtype)
    print(f"graded n={n} {dtype}: eta_ref={c['eta_ref']:.3g} rho_ref={c['rho_ref']:.3g} skeel={c['skeel']:.3g}")
    for k in ("eta_ref", "rho_ref", "skeel"):
        record_property(k, c[k])
    assert 0.0 < c["eta_ref"] < 8.0 and 0.0 < c["rho_ref"] < 8.0 and c["skeel"] >= 1.0
    # the well-conditioned family for comparison: condition about 5
    ev = np.linalg.eigvalsh(dr.well(n).numpy())
    assert ev[0] >= 1.0 and ev[-1] / ev[0] < 8.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [100, 500, 513, 577, 640, 897])
def test_failing_pivot_constructions_fail_where_intended(dtype, n):
    A = dr.well(n)
    assert dr.failing_pivot(A.to(dtype)) == -1
    F = dr.first_pivot_fails(A).to(dtype)
    assert dr.failing_pivot(F) == 0
    Lst = dr.last_pivot_fails(A, dtype).to(dtype)
    assert dr.failing_pivot(Lst) == n - 1
    np.linalg.cholesky(Lst.double().numpy()[:n - 1, :n - 1])                      # the leading minor stays positive definite
    assert torch.equal(Lst[:n - 1], A.to(dtype)[:n - 1]) and float(Lst[n - 1, n - 1]) > 0
    with pytest.raises(torch.linalg.LinAlgError):
        torch.linalg.cholesky(Lst.double())


def test_error_measures_on_known_answers():
    A = dr.well(50)
    L = dr.chol_ref(A)
    assert dr.eta(A, L, dr.U[torch.float64]) < 1.0                                # the fp64 factor itself: rounding of L L^T only
    Lp = L.clone()
    Lp[7, 3] += 1e-6
    assert dr.eta(A, Lp, dr.U[torch.float64]) > 1e6                               # a perturbed entry is seen at its size over u
    B = dr.rhs(50, 5)
    X = dr.solve_ref(L, B, False)
    assert dr.rho(L, X, B, dr.U[torch.float64], L, X) < 1.0
    assert abs(dr.skeel(torch.eye(9, dtype=torch.float64)) - 1.0) < 1e-15
    T = torch.tensor([[1.0, 0.0], [1e3, 1.0]], dtype=torch.float64)               # |T^-1| |T| = [[1, 0], [2e3, 1]]
    assert abs(dr.skeel(T) - 2001.0) < 1e-9
    Xt = dr.solve_ref(L, B, True)
    assert (L.t() @ Xt - B).abs().max() < 1e-12
    V = dr.rhs(50, 3)
    assert torch.equal(dr.root_update_ref(L, V), L @ L.t() + V @ V.t())
