"""GPU: the rounding a long-running fp32 window leaves behind (which tabulates the figures).  A point leaves the
statistics as the negative of what it entered with, but the two atomics round differently: after many turnovers A and b carry a
residue that a fresh model on the same points does not.  200 updates of 64 points through window = 256 on a 16 x 16 grid in fp32 (50
turnovers), compared every 10 updates with a FRESH plain model on ``window_points()`` -- never with the windowed one: the largest
deviation of A and of b relative to max |.| of the fresh statistics, and of the posterior mean at 50 queries relative to max |mean|.

The bounds are 3 x the largest deviation measured on an MI355X (the project's rule for fp32 parity), the measured values being the
constants below; ``rebuild_window_()`` must bring the model back inside the plain bounds of tests/test_robust_gpu.py (scatter
10 x 2e-4 of max |fresh|, model 1e-2).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GB, GS = [[-1.0, 1.0], [-1.0, 1.0]], [16, 16]
WIN, Q, NUP, EVERY = 256, 64, 200, 10
MEASURED = {"A": 1.252e-06, "b": 1.569e-06, "mean": 1.249e-06}     # largest deviation over the 20 records, one run on one MI355X
SCATTER_BOUND, MODEL_BOUND = 10 * 2e-4, 1e-2


def _data(seed=3):
    rng = np.random.default_rng(seed)
    n = Q * (NUP + 1)
    X = rng.uniform(-0.95, 0.95, (n, 2))
    y = np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.5 * X[:, 1] + 0.3 * np.sin(np.arange(n) / 700.0) + 0.05 * rng.standard_normal(n)
    return X, y, rng.uniform(-0.95, 0.95, (50, 2))


def _model(X, y, **kw):
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    return FixedNoiseOnlineSKIGP(X, y[:, None], None, grid_bounds=torch.tensor(GB), grid_size=GS, learn_additional_noise=True, **kw).eval()


def _deviation(m, Xs):
    Xw, yw, nw = m.window_points()
    fresh = _model(Xw, yw)
    bm, _, _, Am = m.stats_buffers()
    bf, _, _, Af = fresh.stats_buffers()
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())
    with torch.no_grad():
        mean, mf = m(Xs).mean.double(), fresh(Xs).mean.double()
    return {"A": rel(Am, Af), "b": rel(bm, bf), "mean": rel(mean, mf)}


def run_stream(verbose=False):
    """The stream; returns the records [(update, {A, b, mean})...] and, last, ("rebuilt", {...})."""
    X, y, Xs = _data()
    t = lambda a: torch.as_tensor(a, device=DEV, dtype=torch.float32)
    Xt, yt, Xs = t(X), t(y), t(Xs)
    m = _model(Xt[:Q], yt[:Q], window=WIN)
    rows = []
    for k in range(1, NUP + 1):
        m.condition_on_observations(Xt[k * Q:(k + 1) * Q], yt[k * Q:(k + 1) * Q], None, inplace=True)
        if k % EVERY == 0:
            rows.append((k, _deviation(m, Xs)))
            if verbose:
                print(f"update {k:4d} ({k * Q / WIN:5.1f} turnovers): " + "  ".join(f"{key} {v:.3e}" for key, v in rows[-1][1].items()), flush=True)
    assert m.num_data == WIN
    m.rebuild_window_()
    rows.append(("rebuilt", _deviation(m, Xs)))
    if verbose:
        print("after rebuild_window_(): " + "  ".join(f"{key} {v:.3e}" for key, v in rows[-1][1].items()), flush=True)
    return rows


def test_fp32_residue_stays_within_three_times_the_measured_one_and_a_rebuild_cancels_it():
    rows = run_stream(verbose=True)
    worst = {key: max(r[key] for k, r in rows[:-1]) for key in MEASURED}
    print("largest over the records:", worst, " measured:", MEASURED)
    for key, ref in MEASURED.items():
        assert worst[key] <= 3.0 * ref, (key, worst[key], ref)
    after = rows[-1][1]
    assert after["A"] <= SCATTER_BOUND and after["b"] <= SCATTER_BOUND and after["mean"] <= MODEL_BOUND, after
