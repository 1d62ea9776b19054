"""GPU: the kernel cache through the model's hand-overs (online_gp_amd/models/kernel_cache.py) -- a functional update
leaves the parent's statistics bit for bit and shares no storage with them, and growing the grid by a node and trimming it again
returns every statistic bit for bit.  8^3 fp32, 64 points: the smallest models with a pack (out > 1), a probe- and a trend-shaped
region and both rings."""
import numpy as np
import pytest
import torch

from kernel_cache_leaves import snapshot, storages

pytestmark = pytest.mark.gpu

G, N, Q = 8, 64, 16
# (constructor options, outputs, does the form allow the trim that undoes a growth)
MODELS = {
    "out3": (dict(), 3, True),
    "probes-forgetting": (dict(num_path_probes=4, forgetting_factor=0.9), 1, True),
    "trend": (dict(trend="linear"), 1, True),
    "window": (dict(window=32), 1, False),               # (regrid_ of a window model may only grow)
    "site-memory": (dict(site_memory=32), 1, True),
}


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda:0")


@pytest.mark.parametrize("name", list(MODELS))
def test_hand_overs_keep_the_statistics(name):
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    kw, out, trims = MODELS[name]
    rng = np.random.default_rng(5)
    X = rng.uniform(-0.6, 0.6, (N + 2 * Q, 3))           # (inside the interior cells of [-1, 1]^3 at 8 nodes, and of the grown grid)
    Y = np.sin(2.0 * X.sum(1))[:, None] + 0.1 * rng.standard_normal((N + 2 * Q, out))
    m = FixedNoiseOnlineSKIGP(_t(X[:N]), _t(Y[:N]), torch.ones((N, out), dtype=torch.float32, device="cuda:0"),
                              grid_bounds=torch.tensor([[-1.0, 1.0]] * 3), grid_size=G, learn_additional_noise=True, **kw).eval()
    if "site_memory" in kw:                              # one interval batch: the ring holds sites
        lo = Y[N:N + Q, 0] - 0.3
        m.condition_on_observations(_t(X[N:N + Q]), None, None, lower=_t(lo), upper=_t(lo + 0.6), inplace=True)
        assert m._kernel_cache["_site_ring"].fill == Q
    cache = m._kernel_cache
    before, keys = snapshot(cache), set(cache) - {"_spectral"}       # (a regrid drops the spectral factors: derived, rebuilt on use)
    assert all(bool(torch.isfinite(t.double()).all()) for t in before.values()) and bool(before["interpolation_cache"].any())

    # ---- one functional update: the parent keeps its statistics bit for bit, the child's share no storage with them
    sl = slice(N + Q, N + 2 * Q)
    child = m.condition_on_observations(_t(X[sl]), _t(Y[sl]), torch.ones((Q, out), dtype=torch.float32, device="cuda:0"), inplace=False)
    assert child is not m and child._kernel_cache is not cache and m._kernel_cache is cache
    after = snapshot(cache)
    assert set(after) == set(before)
    for k, t in before.items():
        assert torch.equal(after[k], t), k
    assert not (storages(child._kernel_cache) & storages(cache))
    assert set(child._kernel_cache) - {"_spectral"} == keys
    assert not torch.equal(child._kernel_cache["interpolation_cache"], cache["interpolation_cache"])

    # ---- grow by a node on every side, then trim it again: every statistic returns bit for bit, in the same dict
    if not trims:
        return
    m.regrid_(1, 1)
    assert m._kernel_cache is cache and cache["interpolation_cache"].shape == (out, (G + 2) ** 3, 1)
    m.regrid_(-1, -1)
    assert m._kernel_cache is cache and set(cache) - {"_spectral"} == keys
    after = snapshot(cache)
    # (a root pair is derived from the grid size and dropped; nodes were removed: the sites stay in the statistics, their ring is emptied)
    back = [k for k in before if not k.endswith("root") and not k.startswith("_site_ring.")]
    assert {k for k in after if not k.startswith("_site_ring.")} == set(back)
    for k in back:
        assert torch.equal(after[k], before[k]), k
    if "site_memory" in kw:
        assert cache["_site_ring"].fill == 0
