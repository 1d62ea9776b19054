"""Host: the rule that picks the eigenmodes the truncated preconditioner transforms (grid_ops.keep_counts) -- no GPU."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _eigenvalues(g, ell, dtype=torch.float64):
    from online_gp_amd import grid_ops

    grid = grid_ops.GridSpec([[-1.1, 1.1]] * 3, list(g))
    cols = [np.exp(-0.5 * (np.arange(gq) * hq / ell) ** 2) * 0.7 for gq, hq in zip(g, grid.h)]
    host = {}
    grid_ops.kron_eigen(grid, torch.as_tensor(np.concatenate(cols), dtype=dtype), host_out=host, dtype=torch.float32)
    return host["D"]


def test_counts_follow_the_rule_and_hold_on_their_interval():
    from online_gp_amd import grid_ops

    D = _eigenvalues((20, 16, 12), 0.9)
    K, lo, hi = grid_ops.keep_counts(D, 1.3, 2.5)
    assert K == (12, 12, 12) and lo < 2.5 <= hi
    # brute force: w = a lam / (1 + a lam) > 2^-30 with the other dims at their largest eigenvalue, noise floor g 2^-52
    for q in range(3):
        d = np.where(D[q] < len(D[q]) * 2.0 ** -52 * D[q][-1], 0.0, D[q])
        lam = 1.3 * d * np.prod([D[p][-1] for p in range(3) if p != q])
        w = 2.5 * lam / (1.0 + 2.5 * lam)
        assert K[q] == min(len(d), -(-int((w > 2.0 ** -30).sum()) // 4) * 4)
    # inside (lo, hi] the unrounded counts do not move; beyond hi they grow
    raw = lambda a: [int((a * 1.3 * np.where(D[q] < len(D[q]) * 2.0 ** -52 * D[q][-1], 0.0, D[q]) * np.prod([D[p][-1] for p in range(3) if p != q])
                          > 2.0 ** -30 / (1 - 2.0 ** -30)).sum()) for q in range(3)]
    assert raw(lo * (1 + 1e-9)) == raw(hi) == raw(2.5)
    assert raw(hi * (1 + 1e-6)) != raw(2.5) and raw(lo * (1 - 1e-6)) != raw(2.5)


def test_nothing_dropped_means_no_counts():
    from online_gp_amd import grid_ops

    assert grid_ops.keep_counts(_eigenvalues((12, 8, 16), 0.5), 1.3, 2.5)[0] is None
    assert grid_ops.keep_counts(_eigenvalues((20, 16, 12), 0.9), 1.3, 0.0)[0] is None      # no data yet: nothing to truncate against


def test_columns_rounded_to_fp32_bury_the_tail():
    """Why the model decomposes the fp64 columns: rounded to fp32 first, the 50-point RBF factor shows ~1e-9 of rounding noise as
    positive eigenvalues, and the rule -- which must not be widened -- would keep 28 indices per dimension instead of 16."""
    from online_gp_amd import grid_ops

    K64 = grid_ops.keep_counts(_eigenvalues((50, 50, 50), 0.6931), 1.0, 10.0)[0]
    K32 = grid_ops.keep_counts(_eigenvalues((50, 50, 50), 0.6931, torch.float32), 1.0, 10.0)[0]
    assert K64 == (16, 16, 16)
    assert K32 is not None and min(K32) > 24


def test_tables_from_fp64_columns_reproduce_the_factor_as_closely():
    """The fp32 eigen tables (X, D) define the prior factor the fused solve works with: K_hat = X diag(D) X^T.  Decomposed from the fp64
    columns or from columns rounded to fp32 first, K_hat stays within the tables' own rounding of the exact factor: each entry of X
    and D carries a relative error u = 2^-24, so ||K_hat - K|| <= 3 u D_max to first order (X orthogonal, or t-orthogonal with
    profiles in [1e-2, 1]: the bound then carries 1 / min t); columns rounded first add at most g u max|c|."""
    from online_gp_amd import grid_ops

    u = 2.0 ** -24
    for g, ell, profiled in (((50, 50, 50), 0.6931, False), ((50, 50, 50), 0.6931, True), ((20, 16, 12), 0.9, True)):
        rng = np.random.default_rng(1)
        grid = grid_ops.GridSpec([[-1.1, 1.1]] * 3, list(g))
        cols = [np.exp(-0.5 * (np.arange(gq) * hq / ell) ** 2) * 0.7 for gq, hq in zip(g, grid.h)]
        profiles = [np.clip(0.2 + rng.uniform(0, 1, gq), 1e-2, None) for gq in g] if profiled else None
        c64 = torch.as_tensor(np.concatenate(cols), dtype=torch.float64)
        rec = {}
        for name, src in (("fp32 columns", c64.float()), ("fp64 columns", c64)):
            e = grid_ops.kron_eigen(grid, src, profiles=profiles, dtype=torch.float32)
            assert e[0].dtype == torch.float32 and e[1].dtype == torch.float32
            X, D, ox, od = e[0].double().numpy(), e[1].double().numpy(), 0, 0
            rec[name] = []
            for gq in g:
                Xq, Dq = X[ox:ox + gq * gq].reshape(gq, gq), D[od:od + gq]
                rec[name].append((Xq * Dq) @ Xq.T)
                ox, od = ox + gq * gq, od + gq
        for q, gq in enumerate(g):
            K = cols[q][np.abs(np.arange(gq)[:, None] - np.arange(gq)[None, :])]
            tmin = 1.0 if profiles is None else float(profiles[q].min())
            bound = 3 * u * np.linalg.eigvalsh(K)[-1] / tmin
            first = gq * u * cols[q].max()
            e64, e32 = np.abs(rec["fp64 columns"][q] - K).max(), np.abs(rec["fp32 columns"][q] - K).max()
            assert e64 <= bound and e32 <= bound + first, (g, q, e64, e32, bound)
            assert np.abs(rec["fp64 columns"][q] - rec["fp32 columns"][q]).max() <= 2 * bound + first
