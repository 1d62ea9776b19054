"""CPU: tests/stencil_reference.py checked against itself and against independent routes, without a GPU -- the reference product
against an explicitly assembled dense matrix, the packers, the symmetric expansion, the integer bound, the dispatch mirror against a
hand-written list, the derived hand-over values, every seeded defect caught at its named case, and the measurement that motivated
the per-element tests: with interpolation statistics the outermost stencil groups sit below the older tests' fp32 tolerance."""
import numpy as np
import pytest

import stencil_reference as sr

SMALL = [(4,), (7,), (4, 4), (7, 9), (4, 4, 4), (7, 5, 9), (4, 4, 4, 4)]


def _id(gs):
    return "x".join(map(str, gs))


@pytest.mark.parametrize("gs", SMALL, ids=_id)
def test_reference_equals_the_dense_matrix(gs):
    for symmetric in (True, False):
        D = sr.make_data(gs, 3, "int", sr.F64, symmetric)
        M = sr.dense_matrix(gs, D["full"])
        ref, absref = sr.product(gs, D["full"], D["V"], D["add"], D["beta"])
        assert np.array_equal(ref, D["ref"]) and np.array_equal(absref, D["absref"])      # what the data maker hands out
        assert np.array_equal(ref, D["beta"] * D["add"] + D["V"] @ M.T)            # integers: exact in any order
        assert np.array_equal(absref, abs(D["beta"]) * np.abs(D["add"]) + np.abs(D["V"]) @ np.abs(M).T)
        assert np.array_equal(M, M.T) == symmetric
        G = sr.geometry(gs)
        assert (D["full"][G.mask] != 0).all() and not D["full"][~G.mask].any() and not np.signbit(D["full"][~G.mask]).any()


@pytest.mark.parametrize("gs", SMALL + [(5, 7, 64)], ids=_id)
def test_packers_round_trip_and_place_every_entry(gs):
    G = sr.geometry(gs)
    om = np.arange(G.H * G.m, dtype=np.float64).reshape(G.H, G.m)
    flat = sr.pack_half(gs, om)
    assert np.array_equal(np.sort(flat), np.arange(G.H * G.m))                       # a permutation
    assert np.array_equal(sr.unpack_half(gs, flat), om)
    for oh, i in [(0, 0), (3, G.m - 1), (G.H - 1, 0), (G.H - 1, G.m - 1), (min(4, G.H - 1), 1), (min(11, G.H - 1), 2)]:
        g = 0 if oh < 4 else (oh - 4) // 7 + 1
        at = 4 * i + oh if oh < 4 else (7 * g - 3) * G.m + 7 * i + (oh - 4) % 7     # the formula of csrc/solve.hip, k_stencil_spmv_sym
        assert flat[at] == om[oh, i]


@pytest.mark.parametrize("gs", SMALL, ids=_id)
def test_expansion_is_symmetric_and_keeps_the_half(gs):
    D = sr.make_data(gs, 1, "real", sr.F32)
    M = sr.dense_matrix(gs, D["full"])
    assert np.array_equal(M, M.T)
    assert np.array_equal(sr.pack_half(gs, sr.half_om_from_full(gs, D["full"])), D["half"])
    assert D["full"].dtype == np.float32 and D["half"].dtype == np.float32


def test_integer_partial_sums_stay_exact_at_the_largest_cases():
    assert sr.INT_BOUND == 153680 < 2 ** 24
    for gs, k in [max(sr.CASES, key=lambda c: 7 ** len(c[0]) * 1000000 + int(np.prod(c[0]))), ((20, 24, 50), 1), ((4, 4, 1001), 1)]:
        D = sr.make_data(gs, k, "int", sr.F32)
        for key in ("half", "full", "V", "add"):
            assert np.array_equal(D[key], np.rint(D[key])) and np.abs(D[key]).max() <= 8
        _, absref = sr.product(gs, D["full"], D["V"], D["add"], D["beta"])
        assert absref.max() <= 7 ** len(gs) * 64 + 16 <= sr.INT_BOUND          # absref bounds every partial sum of every order


def test_case_tables_hold_what_the_issue_lists():
    grids = {gs for gs, _ in sr.CASES}
    for gs in [(4,), (7,), (64,), (255,), (256,), (1000,), (4, 4), (7, 9), (30, 10), (5, 64), (4, 4, 4), (8, 5, 9), (6, 10, 14), (5, 7, 64),
               (7, 5, 9), (20, 24, 50), (4, 4, 4, 4), (4, 5, 4, 6)]:
        assert gs in grids
    assert any(len(gs) == 4 and np.prod(gs) % 4 for gs in grids)
    for gs in sr.ALL_COLS_GRIDS:
        assert [k for g, k in sr.CASES if g == gs] == sr.COLS_ALL
    assert len(sr.ALL_COLS_GRIDS) == 4 and sr.COLS_ALL == [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 23, 24, 25, 31, 32, 33, 63, 64, 65, 100]


def test_handover_and_shrink_values_are_the_derived_ones():
    assert sr.HANDOVER["dma"] == sr.lds_handover(sr.symdma_lds_bytes)
    assert sr.HANDOVER["mc2"] == sr.lds_handover(lambda g: sr.symdma_mc_lds_bytes(g, 2))
    assert sr.HANDOVER["mc4"] == sr.lds_handover(lambda g: sr.symdma_mc_lds_bytes(g, 4))
    for name, code in (("dma", 4), ("mc2", 5), ("mc4", 5)):
        g, k = sr.HANDOVER[name], sr.HANDOVER_K[name]
        assert ((4, 4, g), k) in sr.CASES and ((4, 4, g + 1), k) in sr.CASES
        assert sr.expected_path((4, 4, g), k, 4, True)[0] == code and sr.expected_path((4, 4, g + 1), k, 4, True)[0] == 3
    for es, kc, g in sr.SHRINK.values():
        assert 6 * g <= sr.window_cap(es, kc) < 6 * (g + 1)
        assert ((4, g), kc) in sr.CASES and ((4, g + 1), kc) in sr.CASES


# (grid, k, element bytes, half) -> (code, columns per pass), written by hand from the dispatch table of the two products
HAND = [
    ((7, 9), 1, 4, 0, (0, 1)), ((7, 9), 3, 8, 0, (0, 2)), ((4, 4, 4), 5, 8, 0, (1, 4)), ((4, 4, 4), 16, 4, 0, (1, 16)), ((4, 4, 4, 4), 9, 4, 0, (1, 8)),
    ((7, 5, 9), 7, 4, 1, (2, 4)), ((4, 4, 4), 1, 8, 1, (3, 1)), ((4, 4), 2, 4, 1, (3, 2)), ((4, 4, 4), 1, 4, 1, (4, 1)), ((8, 5, 9), 3, 4, 1, (5, 2)),
    ((8, 5, 9), 15, 4, 1, (5, 4)), ((8, 5, 9), 16, 4, 1, (6, 64)), ((8, 5, 9), 23, 8, 1, (3, 4)), ((8, 5, 9), 24, 8, 1, (6, 64)),
    ((4, 4, 1001), 1, 4, 1, (3, 1)), ((1000,), 16, 4, 1, (6, 64)),
]


def test_dispatch_mirror_agrees_with_the_hand_written_list():
    for gs, k, es, half, want in HAND:
        assert sr.expected_path(gs, k, es, bool(half)) == want, (gs, k, es, half)
    # the switches: WISKI_SYM_DMA=0 sends kernels 4 and 5 to 3, WISKI_SPMM_BCAST=0 moves the many-column threshold to 32 and to kernel 7
    assert sr.expected_path((4, 4, 4), 1, 4, True, sym_dma=False) == (3, 1)
    assert sr.expected_path((8, 5, 9), 5, 4, True, sym_dma=False) == (3, 4)
    assert sr.expected_path((8, 5, 9), 31, 4, True, spmm_bcast=False) == (5, 4)
    assert sr.expected_path((8, 5, 9), 31, 4, True, sym_dma=False, spmm_bcast=False) == (3, 4)
    assert sr.expected_path((8, 5, 9), 33, 8, True, spmm_bcast=False) == (7, 48)
    assert sr.expected_path((8, 5, 9), 64, 4, True, spmm_bcast=False) == (7, 64)
    codes = {sr.expected_path(gs, k, es, True)[0] for gs, k in sr.CASES for es in (4, 8)} | {sr.expected_path(gs, k, 4, False)[0] for gs, k in sr.CASES}
    assert codes == {0, 1, 2, 3, 4, 5, 6}


@pytest.mark.parametrize("defect", sr.DEFECTS)
def test_every_seeded_defect_is_caught_at_its_named_case(defect):
    gs, k = sr.DEFECT_CASE[defect]
    assert (gs, k) in sr.CASES
    D = sr.make_data(gs, k, "int", sr.F32)
    ref, _ = sr.product(gs, D["full"], D["V"], D["add"], D["beta"])
    assert np.array_equal(sr.emulate_half(gs, D["half"], D["V"], D["add"], D["beta"]), ref)            # the emulation itself is right
    assert not np.array_equal(sr.emulate_half(gs, D["half"], D["V"], D["add"], D["beta"], defect), ref)
    for real in (sr.F32, sr.F64):
        D = sr.make_data(gs, k, "real", real)
        ref, absref = sr.product(gs, D["full"], D["V"], D["add"], D["beta"])
        bnd = sr.bound(gs, 2, absref, real)                                    # the tightest count of the half-stencil paths
        assert sr.ratio(sr.emulate_half(gs, D["half"], D["V"], D["add"], D["beta"]), ref, bnd) <= 1.0
        r = sr.ratio(sr.emulate_half(gs, D["half"], D["V"], D["add"], D["beta"], defect), ref, bnd)
        print(f"{defect} at {sr.case_id((gs, k))} {np.dtype(real).name}: error / bound {r:.3g}")
        assert r > 1.0


@pytest.mark.parametrize("case", [c for c in sr.CASES if int(np.prod(c[0])) * 7 ** len(c[0]) * c[1] <= 4000000], ids=sr.case_id)
def test_emulation_without_a_defect_is_the_reference_at_the_table(case):
    gs, k = case
    D = sr.make_data(gs, k, "int", sr.F32)
    ref, _ = sr.product(gs, D["full"], D["V"], D["add"], D["beta"])
    assert np.array_equal(sr.emulate_half(gs, D["half"], D["V"], D["add"], D["beta"]), ref)
    assert np.array_equal(sr.emulate_half(gs, D["half"], D["V"]), sr.product(gs, D["full"], D["V"])[0])


def test_outer_groups_hide_below_the_old_tolerance_with_interpolation_statistics():
    """Why max-norm tests on W^T W statistics cannot see the far offsets: 500 interior points on 20 x 24 x 50, cubic weights.  Dropping
    the corner groups (|d0| = |d1| = 3), and even every offset with +-3 in two or more dimensions, moves the product by less than the
    2e-5 max|ref| those tests allow in fp32."""
    gs = (20, 24, 50)
    G = sr.geometry(gs)
    A = sr.interpolation_stencil(gs, 500)
    assert np.allclose(sr.expand_half(gs, sr.half_om_from_full(gs, A)), A, rtol=1e-12, atol=0)      # symmetric, up to the order of its sums
    V = np.random.default_rng(1).standard_normal((1, G.m))
    ref, _ = sr.product(gs, A, V)
    far = np.abs(G.shifts) == 3
    corner = far[:, 0] & far[:, 1]
    two = far.sum(1) >= 2
    three = far.sum(1) == 3
    amax = np.abs(A).max()
    out = {}
    for name, sel in (("corner groups", corner), ("+-3 in >= 2 dimensions", two), ("+-3 in 3 dimensions", three)):
        B = A.copy()
        B[sel] = 0.0
        out[name] = np.abs(sr.product(gs, B, V)[0] - ref).max() / np.abs(ref).max()
        print(f"{name}: largest coefficient {np.abs(A[sel]).max() / amax:.2e} of the largest, dropping them moves the product by {out[name]:.2e} max|ref|")
    half = sr.pack_half(gs, sr.half_om_from_full(gs, A))
    emu = np.abs(sr.emulate_half(gs, half, V, defect="corner_groups") - ref).max() / np.abs(ref).max()
    print(f"corner_groups defect of the half-stencil emulation: {emu:.2e} max|ref|")
    assert 0 < emu < sr.OLD_FP32_TOL and 0 < out["corner groups"] < sr.OLD_FP32_TOL
    assert out["+-3 in >= 2 dimensions"] < sr.OLD_FP32_TOL and out["+-3 in 3 dimensions"] < 1e-6
    # ... while the integer data of this table puts the same defect at full scale
    D = sr.make_data((4, 4, 4), 1, "int", sr.F32)
    ref, _ = sr.product((4, 4, 4), D["full"], D["V"])
    assert np.abs(sr.emulate_half((4, 4, 4), D["half"], D["V"], defect="corner_groups") - ref).max() >= 1
