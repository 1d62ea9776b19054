"""No GPU: the reference of interval sites on values and partial derivatives against the two references it combines,
the condition its kernel cases have to meet, the C ABI as declared, and the two plain-torch helpers of the model surface."""
import ctypes
import os
import re

import numpy as np
import torch

import grad_interval_reference as gir
import grad_obs_reference as gr
import interval_reference as iref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
KEYS = ("A", "A_half", "b", "cnt", "res", "stats", "mean_out")


def _close(a, b, rtol=1e-13):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and float(np.abs(a - b).max()) <= rtol * max(float(np.abs(b).max()), 1e-300)


def test_all_channels_exact_is_the_derivative_absorb_of_the_values():
    for name in gir.KGRIDS:
        c = gir.kernel_case(name)
        Y = np.where(c["present"], np.where(np.isfinite(c["lo"]), c["lo"], 0.25), 0.0)
        r = gir.dense_absorb(c["grid"], c["X"], Y, Y, c["wa"], c["wa"], c["noise"], c["pvar"], gir.KS2, c["u"])
        want = gr.dense_absorb(c["grid"], c["X"], Y, c["wa"], c["wa"], c["noise"], c["u"])
        assert all(_close(r[k], want[k]) for k in KEYS) and r["err"] == want["err"] == 3
        pres = c["present"] & c["ok"][:, None]
        assert np.array_equal(r["omega"], pres.astype(np.float64)) and np.array_equal(r["ytilde"], np.where(pres, Y, 0.0)) and not r["skipped"].any()


def test_only_the_value_channel_present_is_the_interval_absorb():
    for name in gir.KGRIDS:
        c = gir.kernel_case(name)
        only = np.zeros_like(c["present"])
        only[:, 0] = c["present"][:, 0]
        wa, noise = np.where(only, c["wa"], 0.0), np.where(only, c["noise"], 1.0)
        r = gir.dense_absorb(c["grid"], c["X"], c["lo"], c["hi"], wa, wa, noise, c["pvar"], gir.KS2, c["u"])
        w0 = np.where(wa[:, 0] != 0, wa[:, 0], 1.0)                    # (the interval reference has no absent points: left out below)
        keep = only[:, 0]
        want = iref.dense_absorb(c["grid"], c["X"][keep], c["lo"][keep, 0], c["hi"][keep, 0], w0[keep], w0[keep], noise[keep, 0], c["pvar"][keep, 0],
                                 gir.KS2, c["u"])
        assert all(_close(r[k], want[k]) for k in ("A", "A_half", "b", "cnt", "res", "stats")) and r["err"] == want["err"] == 3
        for k in ("ytilde", "omega", "log_z"):
            got, fin = r[k][keep, 0], np.isfinite(want[k])                # (the two references sum the same row . u in different orders)
            assert np.array_equal(got[~fin], want[k][~fin], equal_nan=True) and _close(got[fin], want[k][fin], 1e-12) and not r[k][:, 1:].any()
        assert _close(r["mean_out"][keep, 0], want["mean_out"])


def test_the_kernel_cases_hold_what_they_are_meant_to():
    """At least three quarters of the present channels enter, the entering omega span 1e-6 .. 1, and every kind of bound, point and
    variance the docstring of kernel_case lists is there, in every channel."""
    for name in gir.KGRIDS:
        c = gir.kernel_case(name)
        r, kind, d = c["ref"], c["kind"], c["grid"].d
        pres = c["present"] & c["ok"][:, None]
        ent = r["omega"] > 0.0
        assert list(np.nonzero(~c["ok"])[0]) == [gir.P_OUTSIDE] and r["err"] == 3
        assert not c["present"][gir.P_ABSENT].any() and list(c["present"][gir.P_VALUE_ONLY]) == [True] + [False] * d
        assert list(c["present"][gir.P_GRAD_ONLY]) == [False] + [True] * d
        assert np.array_equal(r["zero"], ~pres) and not (ent & ~pres).any()
        assert ent.sum() >= 0.75 * pres.sum() and r["omega"][ent].min() <= 1e-6 and r["omega"][ent].max() == 1.0
        Phi = gr.stacked_rows(c["grid"], c["X"])
        for q in range(d):                                              # a boundary cell of each dim: zero derivative row, site evaluated all the same
            for i in (4 + q, 16 + q):
                assert not Phi[i, 1 + q].any() and Phi[i, 0].any() and r["mean_out"][i, 1 + q] == 0.0 and pres[i, 1 + q]
        assert ent[[4 + q for q in range(d)], [1 + q for q in range(d)]].any() or ent[[16 + q for q in range(d)], [1 + q for q in range(d)]].any()
        for ch in range(d + 1):
            k, p = kind[:, ch], pres[:, ch]
            assert (k == "exact").sum() == 2 and (k == "open").sum() == 1 and (k == "far").sum() == 1 and (k == "empty").sum() == 1
            sk = r["skipped"][:, ch]
            assert np.array_equal(sk, p & np.isin(k, ("open", "far", "empty")))
            ex = p & (k == "exact")
            assert (r["omega"][ex, ch] == 1.0).all() and np.array_equal(r["ytilde"][ex, ch], c["lo"][ex, ch])
            assert np.array_equal(r["ytilde"][sk, ch], r["mean_out"][sk, ch])
            assert all((k == kk).sum() >= 10 for kk in ("lower", "upper", "two"))
            width = ((c["hi"] - c["lo"]) / c["s"])[:, ch][p & (k == "two")]
            assert 0.049 <= width.min() and width.max() <= 4.001
            assert (c["pvar"][:, ch] == 0.0).sum() == 1 and (c["pvar"][:, ch] < 0.0).sum() == 1
            assert c["pvar"][:, ch].max() <= 2.0
        print(f"{name}: {int(ent.sum())} of {int(pres.sum())} present channels enter, omega {r['omega'][ent].min():.2e} .. {r['omega'][ent].max():.1f}")


def test_dense_stream_is_the_gp_of_the_pseudo_observations():
    """DenseStream after three mixed batches equals GradObsGP (data space) fitted at (ytilde, noise / omega) of the entering channels."""
    rng = np.random.default_rng(3)
    grid = gir.Grid.from_bounds([[-1.0, 1.0], [-1.0, 1.0]], [8, 7])
    K, s2 = gr.dense_kuu(grid), 0.4
    X0, y0, n0 = rng.uniform(-0.9, 0.9, (15, 2)), rng.standard_normal(15), rng.uniform(0.5, 2.0, 15)
    S = gir.DenseStream(grid, K, s2).add_values(X0, y0, n0)
    Xa, Ya, Na, Pa = [np.pad(X0, ((0, 0), (0, 0)))], [np.stack([y0, 0 * y0, 0 * y0], 1)], [np.stack([n0, 1 + 0 * n0, 1 + 0 * n0], 1)], [np.stack([n0 > 0, n0 < 0, n0 < 0], 1)]
    for k in range(3):
        X = rng.uniform(-0.9, 0.9, (6, 2))
        kw = [dict(Y=rng.standard_normal(6), grad_lower=-0.2), dict(lower=np.full(6, -0.5), upper=np.full(6, 0.7), grad_lower=-1.0, grad_upper=1.0),
              dict(grad_lower=0.0, grad_mask=rng.uniform(size=(6, 2)) < 0.6)][k]
        lo, hi, nz, pres = gir.channels(6, 2, noise=rng.uniform(0.5, 2.0, 6), **kw)
        st = S.condition(X, lo, hi, nz, pres)
        ent = st["omega"] > 0
        Xa.append(X), Ya.append(st["ytilde"]), Na.append(nz / np.where(ent, st["omega"], 1.0)), Pa.append(ent)
    G = gr.GradObsGP(grid, K, s2).fit(np.concatenate(Xa), np.concatenate(Ya), np.concatenate(Na), np.concatenate(Pa))
    Xs = rng.uniform(-0.9, 0.9, (9, 2))
    mean, var, grad = G.predict(Xs)
    m2, v2, g2 = S.predict(Xs)
    assert S.n == G.N and _close(m2, mean, 1e-9) and _close(v2, var, 1e-9) and _close(g2, grad, 1e-9) and abs(S.mll() - G.mll()) <= 1e-9 * abs(G.mll())


def test_the_record_has_not_grown_and_the_entries_are_declared():
    from online_gp_amd import _hip, grid_ops

    assert ctypes.sizeof(_hip.wiski_absorb_args) == 224
    assert "scatter_grad_interval.h" in _hip._HEADERS and os.path.exists(os.path.join(ROOT, "online_gp_amd", "csrc", "scatter_grad_interval.h"))
    src = open(os.path.join(ROOT, "online_gp_amd", "csrc", "scatter_stats.hip")).read()
    order = [src.index(f'#include "{h}"') for h in ("scatter_grad.h", "scatter_site.h", "scatter_interval.h", "scatter_grad_interval.h")]
    assert order[3] > max(order[:3]) and callable(grid_ops.scatter_stats_grad_interval)
    # the form's prototypes (the record entries: the form has no other) parse, and their parameter kinds are the argtypes _hip.py sets
    hdr = open(os.path.join(ROOT, "include", "wiski.h")).read()
    sigs = {name: sig for name, sig in _hip.ABSORB_SIGNATURES.items() if name.startswith("wiski_absorb_grad_interval")}
    assert len(sigs) == 2
    for name, sig in sigs.items():
        m = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M)
        assert m, name
        real = "float" if name.endswith("_f32") else "double"
        kinds = []
        for prm in m.group(1).split(","):
            prm = prm.strip()
            ty = prm[:prm.rindex(" ")].replace("const ", "").strip()
            if ty == "wiski_grid*":
                kinds.append(ctypes.POINTER(_hip.wiski_grid))
            elif ty == "wiski_absorb_args*":
                kinds.append(ctypes.POINTER(_hip.wiski_absorb_args))
            elif ty.endswith("*"):
                assert ty[:-1] in (real, "double", "int32_t", "void"), (name, prm)
                kinds.append(ctypes.c_void_p)
            else:
                kinds.append({"double": ctypes.c_double, "int64_t": ctypes.c_int64}[ty])
        assert kinds == list(sig), name


def test_monotone_bounds():
    from online_gp_amd.models import monotone_bounds

    lo, hi, mask = monotone_bounds(5, 3, [0, 2])
    assert lo.shape == hi.shape == mask.shape == (5, 3) and mask.dtype == torch.bool
    assert mask.tolist() == [[True, False, True]] * 5 and lo.tolist() == [[0.0, -INF, 0.0]] * 5 and hi.tolist() == [[INF] * 3] * 5
    lo, hi, mask = monotone_bounds(2, 2, 1, sign=-1)
    assert mask.tolist() == [[False, True]] * 2 and lo.tolist() == [[-INF, -INF]] * 2 and hi.tolist() == [[INF, 0.0]] * 2
    for bad in (dict(dims=[2]), dict(dims=[0], sign=0)):
        try:
            monotone_bounds(2, 2, **bad)
            assert False
        except ValueError:
            pass


def test_gradient_interval_probability_formula():
    """The method on hand-made jet moments (a stand-in for the model: posterior_jet and _sigma2 are all it reads) against scipy."""
    from scipy import special as sp

    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    rng = np.random.default_rng(11)
    n, d, s2 = 40, 2, 0.3
    mean, var = rng.standard_normal((n, d + 1)), rng.uniform(0.0, 2.0, (n, d + 1))
    var[3, 1] = -1e-9                                                # a variance that rounding made negative counts as 0

    class Jet:
        pass

    class Stub:
        def posterior_jet(self, X):
            j = Jet()
            j.mean, j.covariance = torch.as_tensor(mean), torch.diag_embed(torch.as_tensor(var))
            return j

        def _sigma2(self, o):
            return s2

    nz = rng.uniform(0.5, 2.0, (n, d))
    s = np.sqrt(np.maximum(var[:, 1:], 0.0) + s2 * nz)
    a = rng.uniform(-4.0, 3.0, (n, d))
    b = a + rng.uniform(0.1, 3.0, (n, d))
    lo, hi = mean[:, 1:] + s * a, mean[:, 1:] + s * b
    lo[:10], hi[10:20] = -INF, INF
    a[:10], b[10:20] = -INF, INF
    want = np.log(sp.ndtr(b) - sp.ndtr(a))
    want[:10], want[10:20] = sp.log_ndtr(b[:10]), sp.log_ndtr(-a[10:20])
    got = FixedNoiseOnlineSKIGP.gradient_interval_probability(Stub(), None, torch.as_tensor(lo), torch.as_tensor(hi), noise=torch.as_tensor(nz)).numpy()
    assert got.shape == (n, d) and np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    one = FixedNoiseOnlineSKIGP.gradient_interval_probability(Stub(), None, 0.0, None).numpy()                # "increasing", unit noise
    assert np.abs(one - sp.log_ndtr(mean[:, 1:] / np.sqrt(np.maximum(var[:, 1:], 0.0) + s2))).max() <= 1e-10 * np.abs(one).max()


def test_toy_reference_pays_on_every_seed():
    """The figures DESIGN.md 3.25 tabulates and the thresholds the GPU test asserts follow from them."""
    for seed in gir.TSEEDS:
        (rc, sc), (ru, su) = gir.toy_reference(seed, True), gir.toy_reference(seed, False)
        print(f"seed {seed}: RMSE constrained {rc:.4f}  plain {ru:.4f}  ratio {rc / ru:.3f};  negative slope at {sc:.2f} / {su:.2f} of the queries")
        assert rc < ru and sc < su
