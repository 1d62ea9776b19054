"""No GPU: the identity behind the sliding-window absorb, in numpy fp64 on a 6 x 6 grid.  The statistics are sums
over the points, so the slot rule of tests/window_reference.py -- absorb what enters, take out what the slot held -- leaves A, b,
c = y^T D^-1 y and log|D| of exactly the points in the ring: they give the posterior mean, the posterior covariance and the marginal
likelihood of the data-space GP (oracle/dataspace.py, which never forms a statistic) fitted to those points alone.  Bound: that of
tests/test_forgetting_host.py.  Independent of the kernel and of the model."""
import ctypes
import os

import numpy as np
import pytest

import sample_paths_reference as ref
import window_reference as wref
from oracle import dataspace, spec
from test_forgetting_host import ELL, G, GB, OSC, S2, _close, _from_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP, Q, NB = 30, 12, 5


def _problem(seed=11):
    rng = np.random.default_rng(seed)
    n = NB * Q
    X = rng.uniform(-1.05, 1.05, (n, 2))
    noise = rng.uniform(0.3, 2.5, n)
    y = np.sin(2.5 * X.sum(1)) + 0.02 * np.arange(n) + 0.3 * rng.standard_normal(n)      # a drifting stream
    return X, y, noise, rng.uniform(-1.0, 1.0, (9, 2))


def _setup():
    g0, h, g = spec.make_grid(GB, G)
    O = dataspace.DataSpaceGP(GB, G, "rbf", ELL, OSC, S2)
    return wref.Grid(g0, h, g), O, ref.kuu_dense(O.cols), (g0, h, g)


def test_windowed_statistics_are_the_gp_of_the_points_in_the_ring():
    X, y, noise, Xs = _problem()
    grid, O, Kuu, (g0, h, g) = _setup()
    Ws = ref.dense_w(g0, h, g, Xs)
    Kt = Kuu / S2
    ring, head, fill = wref.empty_ring(CAP, 2), 0, 0
    A, b, c, ld = np.zeros((36, 36)), np.zeros(36), 0.0, 0.0
    for k in range(NB):
        sl = slice(k * Q, (k + 1) * Q)
        u = Kt @ np.linalg.solve(np.eye(36) + A @ Kt, b)              # the posterior before the batch
        Z = np.linalg.solve(Kt, u)
        R = b - Z - A @ u
        r = wref.dense_absorb(grid, ring, head, X[sl], y[sl], 1.0 / noise[sl], 1.0 / noise[sl], noise[sl], u)
        assert r["err"] == 0 and r["void_left"] == 0
        if k:
            assert _close(r["mean_out"], O.predict(X[sl])[0])         # w . u IS the predictive mean (O: the previous window)
        # the carried residual stays b - Z - A u under entering and leaving points alike; cnt is the row sums of the increment
        assert _close(R + r["res"], (b + r["b"]) - Z - (A + r["A"]) @ u, 1e-12)
        assert _close(r["cnt"], r["A"].sum(1), 1e-12)
        A, b, c, ld = A + r["A"], b + r["b"], c + r["stats"][0], ld + r["stats"][1]
        ring, head, fill = r["ring"], (head + Q) % CAP, min(CAP, fill + Q)
        hi = (k + 1) * Q
        lo = max(0, hi - CAP)
        Xw, yw, waw, wbw, nw = wref.ring_points(ring, head, fill)
        assert np.array_equal(Xw, X[lo:hi]) and np.array_equal(yw, y[lo:hi]) and np.array_equal(nw, noise[lo:hi])      # the last 30, oldest first
        mean, cov, mll = _from_stats(Kuu, A, b, c, ld, hi - lo, Ws)
        O.fit(X[lo:hi], y[lo:hi], noise[lo:hi])
        mo, co = O.predict(Xs, full_cov=True)
        assert _close(mean, mo) and _close(cov, co) and _close(mll, O.mll()), k
        if lo > 0:
            # and it is NOT the GP of all points seen (the check above can tell the two apart)
            Oall = dataspace.DataSpaceGP(GB, G, "rbf", ELL, OSC, S2).fit(X[:hi], y[:hi], noise[:hi])
            assert not _close(mean, Oall.predict(Xs)[0], 1e-2), k


def test_a_point_dropped_at_entry_takes_nothing_out_when_its_slot_comes_round():
    X, y, noise, Xs = _problem(seed=12)
    grid, O, Kuu, _ = _setup()
    cap = 8
    u = np.random.default_rng(0).standard_normal(36)
    X = X.copy()
    X[2, 0] = 5.0                                                     # outside the grid
    ring = wref.empty_ring(cap, 2)
    r1 = wref.dense_absorb(grid, ring, 0, X[:8], y[:8], 1.0 / noise[:8], 1.0 / noise[:8], noise[:8], u)
    assert r1["err"] == 1 + 2 and r1["void_left"] == 0
    rg = r1["ring"]
    assert np.isnan(rg["x"][2]).all() and rg["wa"][2] == 0 and rg["wb"][2] == 0 and rg["noise"][2] == 1
    # the void point contributed nothing: the increment is that of the other seven
    keep = np.arange(8) != 2
    r7 = wref.dense_absorb(grid, wref.empty_ring(cap, 2), 0, X[:8][keep], y[:8][keep], 1.0 / noise[:8][keep], 1.0 / noise[:8][keep], noise[:8][keep], u)
    for key in ("A", "b", "cnt", "res", "stats"):                     # (w . u comes from products of different shapes: rounding, not bits)
        assert _close(r1[key], r7[key], 1e-14), key
    # slot 2 alone comes round: the entering point is all the launch adds -- A, b, c and log|D| lose nothing -- and the void is counted
    r2 = wref.dense_absorb(grid, rg, 2, X[8:9], y[8:9], 1.0 / noise[8:9], 1.0 / noise[8:9], noise[8:9], u)
    for key in ("A", "b", "cnt", "res", "stats"):
        assert np.array_equal(r2[key], r2["before"][key]), key
    assert r2["void_left"] == 1 and r2["err"] == 0
    # a full turn later the statistics are those of the last eight points, none of them void
    tot = {key: r1[key] + r2[key] for key in ("A", "b", "stats")}
    r3 = wref.dense_absorb(grid, r2["ring"], 3, X[9:16], y[9:16], 1.0 / noise[9:16], 1.0 / noise[9:16], noise[9:16], u)
    tot = {key: tot[key] + r3[key] for key in tot}
    assert r3["void_left"] == 0
    W = ref.dense_w(*spec.make_grid(GB, G), X[8:16])
    assert _close(tot["A"], W.T @ (W / noise[8:16, None]), 1e-12) and _close(tot["b"], W.T @ (y[8:16] / noise[8:16]), 1e-12)
    assert _close(tot["stats"], [y[8:16] @ (y[8:16] / noise[8:16]), np.log(noise[8:16]).sum()], 1e-12)
    # an empty slot is not a void one
    r4 = wref.dense_absorb(grid, wref.empty_ring(cap, 2), 5, X[:4], y[:4], 1.0 / noise[:4], 1.0 / noise[:4], noise[:4], u)
    assert r4["void_left"] == 0


def test_more_entering_points_than_slots_are_refused():
    X, y, noise, Xs = _problem()
    grid = _setup()[0]
    with pytest.raises(ValueError):
        wref.dense_absorb(grid, wref.empty_ring(8, 2), 0, X[:9], y[:9], 1.0 / noise[:9], 1.0 / noise[:9], noise[:9], np.zeros(36))
    with pytest.raises(ValueError):
        wref.dense_absorb(grid, wref.empty_ring(8, 2), 8, X[:2], y[:2], 1.0 / noise[:2], 1.0 / noise[:2], noise[:2], np.zeros(36))


def test_kernel_is_declared_and_listed_for_the_build():
    from online_gp_amd import _hip

    hdr = open(os.path.join(ROOT, "include", "wiski.h")).read()
    for name in ("wiski_absorb_window_f32", "wiski_absorb_window_f64", "wiski_window_ring"):
        assert name in hdr
    assert "scatter_window.h" in _hip._HEADERS and os.path.exists(os.path.join(ROOT, "online_gp_amd", "csrc", "scatter_window.h"))
    assert '#include "scatter_window.h"' in open(os.path.join(ROOT, "online_gp_amd", "csrc", "scatter_stats.hip")).read()
    # the public argument record has not grown; the ring is five pointers and two int64
    assert ctypes.sizeof(_hip.wiski_absorb_args) == 224 and ctypes.sizeof(_hip.wiski_window_ring) == 56
