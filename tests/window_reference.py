"""TEST INFRASTRUCTURE -- fp64 reference of the sliding-window absorb, shared by tests/test_window_host.py (no GPU)
and tests/test_window_gpu.py.

A ring of ``cap`` slots holds the points of the window: x [cap, d], y, wa, wb, noise [cap].  An EMPTY slot holds wa = wb = 0,
noise = 1 (x = y = 0); a VOID slot -- its point lay outside the grid when it entered -- the same with x = NaN (and y = 0, whatever
its target was: a non-finite target of a dropped row must not reach the statistics when the slot comes round).  One launch takes an
entering batch of n <= cap points and the slot ``head`` of the first of them.  For entering point j, slot s = (head + j) mod cap:

  1. the old occupant of s is read;
  2. the entering point is written into s: inside the grid as it is, outside it as a void (y = 0) and counted in err;
  3. the entering point is absorbed with (+wa, +wb): mean_out[j] = w_j . u;
  4. the old occupant is absorbed with (-wa, -wb); an empty or void slot gives nothing back, and void_left counts the voids.

Straight from that rule, with dense rows W (``interp_reference.dense_rows``; zero for a point outside the grid) and the half-stencil
layout of ``regrid_reference.pack_half``, as ``robust_reference.dense_absorb``.  Independent of the kernel and of the model.
"""
import numpy as np
import torch

import interp_reference as ir
import regrid_reference as rr
from grad_obs_reference import Grid, inside  # noqa: F401


def empty_ring(cap, d):
    return {"x": np.zeros((cap, d)), "y": np.zeros(cap), "wa": np.zeros(cap), "wb": np.zeros(cap), "noise": np.ones(cap)}


def ring_points(ring, head, fill):
    """(X, y, wa, wb, noise) of the points in the ring, oldest first, voids omitted; `fill`: slots written so far (<= cap)."""
    cap = ring["y"].shape[0]
    first = head if fill == cap else 0
    idx = np.array([(first + i) % cap for i in range(fill)], dtype=np.int64)
    idx = idx[~np.isnan(ring["x"][idx, 0])] if idx.size else idx
    return tuple(ring[k][idx] for k in ("x", "y", "wa", "wb", "noise"))


def dense_absorb(grid, ring, head, X, y, wa, wb, noise, u):
    """What one window launch adds, densely: dict of A [m, m], A_half (flat), b, cnt, res [m], stats [2], mean_out [n], the new
    `ring`, err (bit 0 | 2 x dropped entering points) and void_left.  `before`: the same statistics of the entering points alone
    (what was summed before anything left: the magnitude rounding scales with)."""
    cap = ring["y"].shape[0]
    X = np.asarray(X, dtype=np.float64).reshape(-1, grid.d)
    n = X.shape[0]
    if n > cap:
        raise ValueError(f"{n} entering points, {cap} slots: the slots of a launch must be distinct")
    if not 0 <= head < cap:
        raise ValueError(f"head {head} outside [0, {cap})")
    y, wa, wb, noise, u = (np.asarray(t, dtype=np.float64) for t in (y, wa, wb, noise, u))
    new = {k: v.copy() for k, v in ring.items()}
    m = u.shape[0]
    A, b, cnt, res, stats = np.zeros((m, m)), np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(2)
    Ab, bb, cb, rb, sb = np.zeros((m, m)), np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(2)
    ok = inside(grid, X)
    W = ir.dense_rows(grid, torch.as_tensor(X)).numpy()
    mean = W @ u
    void_left = 0
    slots = (head + np.arange(n)) % cap
    Wold = ir.dense_rows(grid, torch.as_tensor(np.nan_to_num(ring["x"][slots]).reshape(-1, grid.d))).numpy()    # (used where the slot holds weight)
    for j in range(n):
        s = (head + j) % cap
        old = {k: ring[k][s].copy() for k in ring}                    # 1.
        if ok[j]:                                                     # 2.
            new["x"][s], new["y"][s], new["wa"][s], new["wb"][s], new["noise"][s] = X[j], y[j], wa[j], wb[j], noise[j]
            w = W[j]                                                  # 3.
            for (TA, Tb, Tc, Tr, Ts) in ((A, b, cnt, res, stats), (Ab, bb, cb, rb, sb)):
                TA += wa[j] * np.outer(w, w)
                Tb += wb[j] * y[j] * w
                Tc += wa[j] * w
                Tr += (wb[j] * y[j] - wa[j] * mean[j]) * w
                Ts += (wb[j] * y[j] * y[j], np.log(noise[j]))
        else:
            new["x"][s], new["y"][s], new["wa"][s], new["wb"][s], new["noise"][s] = np.nan, 0.0, 0.0, 0.0, 1.0
        if old["wa"] != 0 or old["wb"] != 0:                          # 4.
            w = Wold[j]
            A -= old["wa"] * np.outer(w, w)
            b -= old["wb"] * old["y"] * w
            cnt -= old["wa"] * w
            res -= (old["wb"] * old["y"] - old["wa"] * (w @ u)) * w
        elif np.isnan(old["x"][0]):
            void_left += 1
        stats -= (old["wb"] * old["y"] * old["y"], np.log(old["noise"]))
    sym = lambda M: np.triu(M) + np.triu(M, 1).T
    A, Ab = sym(A), sym(Ab)
    half = lambda M: rr.pack_half(torch.as_tensor(M), grid.g).numpy()
    return {"A": A, "A_half": half(A), "b": b, "cnt": cnt, "res": res, "stats": stats, "mean_out": mean, "ring": new,
            "err": int((~ok).any()) + 2 * int((~ok).sum()), "void_left": void_left,
            "before": {"A": Ab, "A_half": half(Ab), "b": bb, "cnt": cb, "res": rb, "stats": sb}}
