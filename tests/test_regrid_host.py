"""Host: the grid arithmetic of ``GridSpec.shifted`` and the exactness claim of DESIGN.md 3.14 -- a grid changed by whole nodes at
unchanged spacing is the same GP as long as every datum stays in an interior cell -- on the data-space oracle, before any kernel; plus
checks of the dense re-embedding reference (tests/regrid_reference.py) that tests/test_regrid_gpu.py holds the kernel against."""
import numpy as np
import pytest
import torch

import interp_reference as ir
import regrid_reference as rr
from oracle import dataspace


def _nodes(spec, q):
    return spec.g0[q] + spec.h[q] * np.arange(spec.g[q])


def test_shifted_sizes_bounds_and_nodes():
    from online_gp_amd.grid_ops import GridSpec

    old = GridSpec([[-1.0, 1.0], [-1.0, 1.0], [0.25, 3.0]], [12, 10, 7])
    below, above = (2, 0, -1), (1, 3, 2)
    new = old.shifted(below, above)
    assert new.g == [15, 13, 8] and new.m == 15 * 13 * 8 and new.d == 3 and new.T == old.T and new.R == old.R
    assert [new.c.g[q] for q in range(3)] == new.g and [new.c.g0[q] for q in range(3)] == new.g0 and [new.c.h[q] for q in range(3)] == new.h
    assert new.h == old.h                                             # the spacing is the same number, not a recomputed one
    for q in range(3):
        a = below[q]
        no, nn = _nodes(old, q), _nodes(new, q)
        lo, hi = max(0, -a), min(old.g[q], new.g[q] - a)              # old nodes that the new grid has
        err = np.abs(nn[lo + a:hi + a] - no[lo:hi]).max()
        bound = 4 * np.finfo(np.float64).eps * max(np.abs(no).max(), np.abs(nn).max())
        print(f"dim {q}: common nodes differ by {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        # the bounds are the ones the constructor's recipe maps to this very grid, and the interior box lies inside them
        assert new.grid_bounds[q][0] <= nn[1] and new.grid_bounds[q][1] >= nn[-2]
    again = GridSpec(new.grid_bounds, new.g)
    for q in range(3):
        err = np.abs(_nodes(again, q) - _nodes(new, q)).max()
        print(f"dim {q}: grid rebuilt from the shifted bounds differs by {err:.3e}")
        assert err <= 8 * np.finfo(np.float64).eps * np.abs(_nodes(new, q)).max()
    same = old.shifted(0, 0)
    assert same.g == old.g and np.allclose(same.grid_bounds, old.grid_bounds, rtol=0, atol=1e-15)
    assert old.shifted(1, 1).g == [14, 12, 9]                         # ints apply to every dim


def test_shifted_refuses_small_and_disjoint_grids():
    from online_gp_amd.grid_ops import GridSpec

    old = GridSpec([[-1.0, 1.0]] * 2, [6, 5])
    with pytest.raises(ValueError, match="at least 4"):
        old.shifted((0, -1), (0, -1))
    with pytest.raises(ValueError, match="at least 4"):
        old.shifted((-3, 0), (0, 0))
    with pytest.raises(ValueError):
        old.shifted((-6, 0), (6, 0))                                  # same size, but no common node
    with pytest.raises(ValueError):
        old.shifted((1,), (1,))
    assert old.shifted((-2, 0), (0, -1)).g == [4, 4]


def test_shifted_honours_float32_grid():
    from online_gp_amd import settings
    from online_gp_amd.grid_ops import GridSpec

    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    with settings.float32_grid(True):
        old = GridSpec([[-1.0, 1.0], [0.1, 0.7]], [12, 9])
        new = old.shifted((3, -1), (0, 2))
    assert new.g == [15, 10]
    for q in range(2):
        assert old.g0[q] == f32(old.g0[q]) and old.h[q] == f32(old.h[q])         # what the constructor does
        assert new.g0[q] == f32(new.g0[q]) and new.h[q] == old.h[q]               # ... and the shifted grid keeps
        a = (3, -1)[q]
        no, nn = _nodes(old, q), _nodes(new, q)
        lo, hi = max(0, -a), min(old.g[q], new.g[q] - a)
        err = np.abs(nn[lo + a:hi + a] - no[lo:hi]).max()
        bound = 4 * 2.0 ** -23 * max(np.abs(no).max(), np.abs(nn).max())
        print(f"float32 grid, dim {q}: common nodes differ by {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    new64 = GridSpec([[-1.0, 1.0], [0.1, 0.7]], [12, 9]).shifted((3, -1), (0, 2))
    assert any(new64.g0[q] != f32(new64.g0[q]) for q in range(2))                 # (the setting made a difference)


# ------------------------------------------------------------------------------------- the exactness claim, in data space
def _oracle_triplet(bounds, g, X, y, Xq):
    O = dataspace.DataSpaceGP(bounds, g, "rbf", 0.45, 1.3, 0.7).fit(X, y, np.full(X.shape[0], 0.5))
    mean, var = O.predict(Xq)
    return mean, var, O.mll()


def _agree(label, got, want, tol=1e-9):
    for name, a, b in zip(("mean", "variance", "mll"), got, want):
        err = np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()
        print(f"{label}: {name} relative difference {err:.3e} (bound {tol:.0e})")
        assert err <= tol


def test_growth_is_exact_in_data_space():
    from online_gp_amd.grid_ops import GridSpec

    rng = np.random.default_rng(11)
    X = rng.uniform(-0.9, 0.9, (200, 2))
    y = np.sin(3 * X[:, 0]) * np.cos(2 * X[:, 1]) + 0.1 * rng.standard_normal(200)
    Xq = rng.uniform(-0.9, 0.9, (64, 2))
    old = GridSpec([[-1.0, 1.0]] * 2, [12, 10])
    new = old.shifted((2, 0), (1, 3))
    assert new.g == [15, 13]
    _agree("growth 12x10 -> 15x13", _oracle_triplet(new.grid_bounds, new.g, X, y, Xq), _oracle_triplet(old.grid_bounds, old.g, X, y, Xq))


def test_trim_of_untouched_nodes_is_exact_in_data_space():
    from online_gp_amd.grid_ops import GridSpec

    rng = np.random.default_rng(12)
    X = np.stack([rng.uniform(-0.4, 0.9, 200), rng.uniform(-0.9, 0.9, 200)], 1)
    y = np.sin(3 * X[:, 0]) * np.cos(2 * X[:, 1]) + 0.1 * rng.standard_normal(200)
    Xq = np.stack([rng.uniform(-0.4, 0.9, 64), rng.uniform(-0.9, 0.9, 64)], 1)
    old = GridSpec([[-1.0, 1.0]] * 2, [12, 10])
    # the admissible trim below in dim 0, from the reference rows: the nodes of dim 0 in front of the first one any datum touches
    W = ir.dense_rows(old, torch.as_tensor(X)).reshape(200, 12, 10)
    touched = (W != 0).any(0).any(1)
    trim = int(np.argmax(touched.numpy()))
    print(f"dim 0: first touched node {trim} of 12")
    assert trim >= 1                                                  # (the case must trim something)
    new = old.shifted((-trim, 0), (0, 0))
    assert new.g == [12 - trim, 10]
    # ... every datum is then in an interior cell of the new grid as well: its rows are the old ones at the index shift
    W2 = ir.dense_rows(new, torch.as_tensor(X)).reshape(200, 12 - trim, 10)
    assert float((W2 - W[:, trim:]).abs().max()) <= 64 * 2.0 ** -52
    _agree(f"trim of {trim} untouched nodes", _oracle_triplet(new.grid_bounds, new.g, X, y, Xq), _oracle_triplet(old.grid_bounds, old.g, X, y, Xq))


# ------------------------------------------------------------------------------------------------ the dense reference itself
@pytest.mark.parametrize("g", [[8], [5, 7], [6, 5, 4]], ids=["d1", "d2", "d3"])
def test_half_stencil_pack_round_trips(g):
    from online_gp_amd.grid_ops import GridSpec

    d, m = len(g), int(np.prod(g))
    spec = GridSpec([[-1.0, 1.0]] * d, g)
    rng = np.random.default_rng(d)
    lo = np.array([spec.g0[q] + spec.h[q] for q in range(d)])
    hi = np.array([spec.g0[q] + spec.h[q] * (g[q] - 2) for q in range(d)])
    X = torch.as_tensor(lo + (hi - lo) * rng.uniform(0, 1, (40, d)))
    A, b, cnt = rr.dense_stats(spec, X, torch.as_tensor(rng.standard_normal(40)), torch.as_tensor(rng.uniform(0.5, 2, 40)))
    flat = rr.pack_half(A, g)
    assert flat.numel() == (7 ** d + 1) // 2 * m
    assert torch.equal(rr.unpack_half(flat, g), A)                   # W^T D^-1 W lives inside the 7^d stencil, and A is symmetric to the bit
    assert torch.equal(flat[0:4 * m:4], torch.diagonal(A))           # group 0, slot 0: the diagonal
    # the layout conversion the package documents (a pure permutation) agrees with the offset-major rows
    from online_gp_amd.grid_ops import half_stencil_from_offset_major

    om = rr.pack_offset_major(A, g, (7 ** d - 1) // 2, 7 ** d)
    assert torch.equal(half_stencil_from_offset_major(spec, om).reshape(-1), flat)
    # embed, then trim back: the identity; a trim that cuts data drops what the reference says it drops
    below, above = [1] * d, [2] * d
    g2 = rr.shifted_sizes(g, below, above)
    A2 = rr.embed_matrix(A, g, below, g2)
    assert A2.shape == (int(np.prod(g2)),) * 2 and float(A2.sum()) == pytest.approx(float(A.sum()), rel=1e-12)
    assert torch.equal(rr.embed_matrix(A2, g2, [-1] * d, g), A)
    assert torch.equal(rr.embed_vectors(rr.embed_vectors(b[None], g, below, g2), g2, [-1] * d, g)[0], b)
    P = torch.as_tensor(rng.standard_normal((m, 4)))
    assert torch.equal(rr.embed_probes(rr.embed_probes(P, g, below, g2), g2, [-1] * d, g), P)
    assert rr.dropped(A2, g2, [-1] * d, g) == (0, 0.0)
    g3 = [gq - 1 for gq in g] if min(g) > 4 else None
    if g3 is not None:
        rows, mass = rr.dropped(A, g, [-1] * d, g3)
        diag = torch.diagonal(A).reshape(g)
        keep = diag[tuple(slice(1, None) for _ in g)]
        assert mass == pytest.approx(float(diag.sum() - keep.sum()), rel=1e-12) and rows > 0
