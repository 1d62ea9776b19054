"""No GPU: the host reference of the posterior sample paths (tests/sample_paths_reference.py) checked against itself -- the
generator's known answers and moments, the statistics-space path formula against its covariance and against Matheron's rule in
data space -- and the declarations the kernel needs (include/wiski.h, _hip._SOURCES)."""
import os

import numpy as np

import sample_paths_reference as ref
from oracle import spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    assert _hex(ref.philox4x32_10(np.zeros(4, dtype=np.uint64), np.zeros(2, dtype=np.uint64))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = np.full(4, 0xFFFFFFFF, dtype=np.uint64)
    assert _hex(ref.philox4x32_10(ones, ones[:2])) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_normals_moments_and_keys():
    S, n = 16, 12500                                    # 2 * 10^5 (index, s) pairs
    e = ref.normals(7, np.arange(n), S)
    assert e.shape == (n, S) and np.isfinite(e).all()
    assert abs(e.mean()) < 0.01
    assert abs(e.var() - 1.0) < 0.02
    srt = np.sort(e, axis=1)
    assert (np.diff(srt, axis=1) != 0).all()            # no two probes of a point are equal
    assert not np.array_equal(e[:100], ref.normals(8, np.arange(100), S))             # another seed
    assert not np.array_equal(e[:100], ref.normals(7, 100 + np.arange(100), S))       # other indices
    assert np.array_equal(e[100:200], ref.normals(7, 100 + np.arange(100), S))        # a function of (seed, index, s) alone
    big = ref.normals(7, (1 << 32) + np.arange(4), S)                                 # the high counter word is used
    assert not np.array_equal(big, e[:4])
    assert np.array_equal(ref.normals(7, np.arange(4), 8), e[:4, :8])                 # probe s does not depend on S


def _problem():
    rng = np.random.default_rng(3)
    gb, gs = [[-1.0, 1.0], [0.0, 2.0]], [8, 9]
    g0, h, g = spec.make_grid(gb, gs)
    cols = spec.toeplitz_columns("matern52", h, g, [0.25, 0.4], 1.3)
    Kuu = ref.kuu_dense(cols)
    n = 25
    X = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 2, n)], axis=1)
    X[0] = [-1.0 + 0.1 * h[0], 1.0]                    # a one-hot boundary cell
    W = ref.dense_w(g0, h, g, X)
    wa = rng.uniform(0.3, 3.0, n)
    y = np.sin(3 * X[:, 0]) + X[:, 1] + 0.1 * rng.standard_normal(n)
    return g0, h, g, Kuu, X, W, wa, y, 0.37, rng


def test_statistics_space_map_has_the_posterior_covariance():
    g0, h, g, Kuu, X, W, wa, y, s2, rng = _problem()
    Lz, Le, Mop = ref.statspace_map(Kuu, W, wa, s2)
    cov = Lz @ Lz.T + Le @ Le.T                        # z and eps independent standard normals
    target = s2 * Mop
    assert np.abs(cov - target).max() <= 1e-9 * np.abs(target).max()


def test_statistics_space_path_is_the_data_space_path():
    g0, h, g, Kuu, X, W, wa, y, s2, rng = _problem()
    S, seed, first = 6, 11, 40
    eps = ref.normals(seed, first + np.arange(X.shape[0]), S)
    P = ref.probes(g0, h, g, X, wa, first, seed, S)
    assert np.allclose(P, W.T @ (np.sqrt(wa)[:, None] * eps), rtol=0, atol=1e-14)
    eta = (ref.sym_sqrt(Kuu) @ rng.standard_normal((Kuu.shape[0], S))).T
    us = ref.path_statspace(Kuu, W, wa, y, s2, eta, P)
    ud = ref.path_dataspace(Kuu, W, wa, y, s2, eta, eps)
    assert np.abs(us - ud).max() <= 1e-9 * np.abs(ud).max()
    # the paths' mean over many probes approaches the posterior mean (sanity of the sign conventions)
    mean = ref.path_statspace(Kuu, W, wa, y, s2, np.zeros((1, Kuu.shape[0])), np.zeros((Kuu.shape[0], 1)))[0]
    A = W.T @ (wa[:, None] * W)
    assert np.allclose((np.linalg.inv(Kuu / s2) + A) @ mean, W.T @ (wa * y), rtol=1e-6, atol=1e-8)


def test_probe_bounds_bookkeeping():
    g0, h, g, Kuu, X, W, wa, y, s2, rng = _problem()
    P, cnt, asum = ref.probes(g0, h, g, X, wa, 0, 5, 4, with_bounds=True)
    assert cnt.shape == (W.shape[1],) and asum.shape == P.shape
    assert (np.abs(P) <= asum + 1e-15).all() and cnt.sum() == (W != 0).sum()
    Pa = ref.probes(g0, h, g, X[:10], wa[:10], 0, 5, 4) + ref.probes(g0, h, g, X[10:], wa[10:], 10, 5, 4)
    assert np.allclose(Pa, P, rtol=0, atol=1e-14)       # additive over batches when the index is carried


def test_header_and_sources_declare_the_kernel():
    hdr = open(os.path.join(ROOT, "include", "wiski.h")).read()
    assert "int wiski_scatter_probes_f32(" in hdr and "int wiski_scatter_probes_f64(" in hdr
    from online_gp_amd import _hip

    assert "sample_paths.hip" in _hip._SOURCES
    assert os.path.exists(os.path.join(ROOT, "online_gp_amd", "csrc", "sample_paths.hip"))
