"""TEST INFRASTRUCTURE -- dense reference of the re-embedding of the streamed statistics on a grid changed by whole nodes
(DESIGN.md 3.14), shared by tests/test_regrid_host.py (no GPU) and tests/test_regrid_gpu.py.

Everything here is a restatement on the CPU of the documented rules, independent of the kernels and of grid_ops' wrappers:

* a grid is its list of sizes ``g`` (dim 0 slowest in the flat node index); the new grid has ``g' = g + below + above`` nodes per dim
  and the old node ``j`` of dim q is the new node ``j + below[q]``;
* the statistics move by that index shift: ``A'[i', j'] = A[i, j]`` where both nodes exist on both grids, zero elsewhere (growth:
  an embedding; trim: the principal submatrix), and the same for vectors ``[k][m]`` and probe-minor arrays ``[m][S]``;
* the half-stencil layout (include/wiski.h): the offset index ``r`` has the base-7 digits ``dg_q`` (dim 0 first, relative
  offset ``dg_q - 3`` in dim q); only ``r >= centre = (7^d - 1) / 2`` is stored; with ``P = r // 7``, ``s = r % 7`` and
  ``gp = P - (7^(d-1) - 1) / 2``: ``flat[4 i + (s - 3)]`` for gp = 0 and ``flat[(7 gp - 3) m + 7 i + s]`` for gp >= 1 hold
  ``A[i, i + off(r)]``, zero where the neighbour is outside the grid.

Values are only moved, never computed with, so every function is exact in any dtype.
"""
import numpy as np
import torch


def strides(g):
    return [int(np.prod(g[q + 1:])) for q in range(len(g))]


def node_multi_index(g):
    """[m, d] multi-indices of the flat nodes."""
    return np.stack(np.unravel_index(np.arange(int(np.prod(g))), g), 1)


def offset_digits(r, d):
    """Base-7 digits of the offset index r, dim 0 first."""
    dg = []
    for _ in range(d):
        dg.append(r % 7)
        r //= 7
    return dg[::-1]


def neighbours(g, r):
    """(nodes i whose neighbour i + off(r) is inside the grid, that neighbour's flat index) for the offset index r."""
    mi = node_multi_index(g)
    nb = mi + (np.array(offset_digits(r, len(g))) - 3)[None, :]
    ok = ((nb >= 0) & (nb < np.array(g)[None, :])).all(1)
    return np.nonzero(ok)[0], (nb[ok] * np.array(strides(g))[None, :]).sum(1)


def half_position(g, r):
    """(start, stride) such that ``A[i, i + off(r)]`` lives at ``flat[start + stride * i]`` in the row-interleaved half stencil."""
    d, m = len(g), int(np.prod(g))
    P, s = r // 7, r % 7
    gp = P - (7 ** (d - 1) - 1) // 2
    assert gp > 0 or (gp == 0 and s >= 3), "only offsets >= the centre are stored"
    return (s - 3, 4) if gp == 0 else ((7 * gp - 3) * m + s, 7)


def pack_half(A, g):
    """Dense m x m (torch) -> the row-interleaved half stencil, flat [H m]."""
    d, m = len(g), int(np.prod(g))
    R = 7 ** d
    flat = torch.zeros((R + 1) // 2 * m, dtype=A.dtype)
    for r in range((R - 1) // 2, R):
        i, j = neighbours(g, r)
        start, st = half_position(g, r)
        flat[torch.as_tensor(start + st * i)] = A[torch.as_tensor(i), torch.as_tensor(j)]
    return flat


def unpack_half(flat, g):
    """Inverse of :func:`pack_half` for a symmetric matrix whose entries beyond the 7^d stencil are zero."""
    d, m = len(g), int(np.prod(g))
    R = 7 ** d
    A = torch.zeros((m, m), dtype=flat.dtype)
    for r in range((R - 1) // 2, R):
        i, j = neighbours(g, r)
        start, st = half_position(g, r)
        v = flat[torch.as_tensor(start + st * i)]
        A[torch.as_tensor(i), torch.as_tensor(j)] = v
        A[torch.as_tensor(j), torch.as_tensor(i)] = v
    return A


def pack_offset_major(A, g, r_lo=0, r_hi=None):
    """Dense m x m -> the offset-major rows ``om[r - r_lo, i] = A[i, i + off(r)]``, r_lo <= r < r_hi (default: the full stencil)."""
    m = int(np.prod(g))
    r_hi = 7 ** len(g) if r_hi is None else r_hi
    om = torch.zeros((r_hi - r_lo, m), dtype=A.dtype)
    for r in range(r_lo, r_hi):
        i, j = neighbours(g, r)
        om[r - r_lo, torch.as_tensor(i)] = A[torch.as_tensor(i), torch.as_tensor(j)]
    return om


def shifted_sizes(g, below, above):
    return [int(gq + a + b) for gq, a, b in zip(g, below, above)]


def node_map(g, below, g_new):
    """(old flat indices that survive, their new flat indices, old flat indices that are dropped)."""
    mi = node_multi_index(g) + np.array(below)[None, :]
    ok = ((mi >= 0) & (mi < np.array(g_new)[None, :])).all(1)
    new = (mi[ok] * np.array(strides(g_new))[None, :]).sum(1)
    return np.nonzero(ok)[0], new, np.nonzero(~ok)[0]


def embed_matrix(A, g, below, g_new):
    old, new, _ = node_map(g, below, g_new)
    m2 = int(np.prod(g_new))
    out = torch.zeros((m2, m2), dtype=A.dtype)
    o, n = torch.as_tensor(old), torch.as_tensor(new)
    out[n[:, None], n[None, :]] = A[o[:, None], o[None, :]]
    return out


def embed_vectors(V, g, below, g_new):
    """[k, m] -> [k, m']."""
    old, new, _ = node_map(g, below, g_new)
    out = torch.zeros((V.shape[0], int(np.prod(g_new))), dtype=V.dtype)
    out[:, torch.as_tensor(new)] = V[:, torch.as_tensor(old)]
    return out


def embed_probes(P, g, below, g_new):
    """[m, S] -> [m', S]."""
    return embed_vectors(P.t(), g, below, g_new).t().contiguous()


def dropped(A, g, below, g_new):
    """(number of removed nodes with A_ii != 0, sum of those A_ii in fp64)."""
    _, _, gone = node_map(g, below, g_new)
    dg = torch.diagonal(A)[torch.as_tensor(gone, dtype=torch.int64)].double()
    return int((dg != 0).sum()), float(dg.sum())


def dense_stats(grid, X, y, noise, dtype=torch.float64):
    """Dense ``A = W^T D^-1 W`` [m, m], ``b = W^T D^-1 y`` [m] and ``cnt = W^T D^-1 1`` [m] of points X [n, d] from the analytic
    interpolation rows (tests/interp_reference.py); `grid` needs g0, h, g, d."""
    import interp_reference as ir

    W = ir.dense_rows(grid, X.to(dtype))
    wt = 1.0 / noise.to(dtype)
    A = torch.triu(W.t() @ (W * wt[:, None]))             # (a matrix product is not symmetric to the last bit: mirror one triangle)
    return A + torch.triu(A, 1).t(), W.t() @ (wt * y.to(dtype)), W.t() @ wt
