"""GPU: the tap stage of the absorb (include/wiski.h: wiski_absorb_staged_f32, wiski_tap_fold_f32, wiski_stream_args_f32.d_tap_stage).

With a stage the atomic half-stencil absorb adds a point's b / cnt / res contributions into one 16-byte record per node and the fold
adds the records to the three arrays and zeroes them.  Everything here runs on the 8^3 fp32 grid on [-1.1, 1.1]^3 (m = 512; nodes
from -1.4667 to 1.4667, so x = -1.4 / 1.4 lie in the one-hot first / last cell of a dimension).

Absorb tests: each batch once staged + folded and once direct, from the same non-zero starting b, cnt, res and A_h.  Reference: the
oracle's interpolation rows (cport.MatrixFreeWISKI.interp, fp64) summed in numpy,
    b += W^T (wb y),  cnt += W^T wa,  res += W^T (wb y - wa (W u)),
and the tolerance of tests/test_hip_ops.py::test_scatter_stats for fp32 (10 x 2e-4 of the largest reference element), per element,
for BOTH calls.  A_h of the two calls differs by the order of its atomics only: an element receives at most one add per point that
touches its row, each of magnitude <= wa_max (|tap value| <= 1), so with c the largest number of points on one node two orders of
summation differ by at most c 2^-24 (c wa_max) -- exactly zero for the batches whose points share no element.  stats, mean_out and
the error word do not pass through the stage and are compared bit for bit (stats: one block adds it, in one order).

Step tests: three deferred wiski_stream_step_f32 calls and a flush (the second and third absorb are queued guarded, behind the
pending solve) with the stage and without it.  Tolerance 1e-4 and U within 2e-3 of its maximum as tests/test_poll_hindsight_gpu.py
(TOL, U_RTOL: the same comparison of two runs of one stream); the batch means, b and cnt at the same bound relative to their own
maxima; R, the residual of a solve converged to ||R|| < TOL ||b|| in both runs, within 2 TOL ||b||.  The first poll of every solve is
placed past convergence (FIRST_POLL), so that each guarded absorb finds its guard open; the iteration counts compared are the polls'
hindsight (first_ok), 18 in every solve of both runs when this was written.
keep = (8, 8, 8): the truncated transforms on every mode (the solve starts with k_keep_fwd, which folds); keep = 0: the full
transforms (the solve launches k_tap_fold first).
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cport

pytestmark = pytest.mark.gpu

G, GB = 8, [[-1.1, 1.1]] * 3
TOL32 = 2e-4 * 10                       # test_scatter_stats: tol * max|ref| * 10
i32, i64 = ctypes.c_int32, ctypes.c_int64


def _batches():
    rng = np.random.default_rng(23)
    out = {
        "n1": np.array([[0.13, -0.42, 0.77]]),
        "n5": rng.uniform(-1.0, 1.0, (5, 3)),
        "n257": rng.uniform(-1.45, 1.45, (257, 3)),                              # 65 blocks, a ragged last one, boundary cells
        "same_cell": np.array([[0.21, 0.33, -0.52], [0.23, 0.31, -0.50]]),
        "edges": np.array([[-1.4, 0.1, 0.2], [1.4, 0.1, 0.2], [0.1, -1.4, 0.2], [0.1, 1.4, 0.2], [0.1, 0.2, -1.4], [0.1, 0.2, 1.4],
                           [-1.4, -1.4, -1.4], [1.4, 1.4, 1.4]]),
        "outside": np.vstack([rng.uniform(-1.0, 1.0, (4, 3)), [[3.0, 0.0, 0.0]]]),
    }
    return {k: v.astype(np.float32) for k, v in out.items()}


BATCHES = _batches()


class _Case:
    """One batch: the fp64 reference increments, and the two device calls from identical starting statistics."""

    def __init__(self, name):
        from online_gp_amd import grid_ops

        self.grid = grid = grid_ops.GridSpec(GB, G)
        rng = np.random.default_rng(7)
        X = BATCHES[name]
        n, m = X.shape[0], grid.m
        self.n, self.m = n, m
        y = rng.standard_normal(n).astype(np.float32)
        noise = rng.uniform(0.5, 2.0, n).astype(np.float32)
        w = (1.0 / noise).astype(np.float32)
        u = rng.standard_normal(m).astype(np.float32)
        H = (grid.R + 1) // 2
        self.start = {k: rng.standard_normal(s).astype(np.float32) for k, s in (("b", m), ("cnt", m), ("res", m), ("A", H * m))}
        inside = np.all(np.abs(X.astype(np.float64)) <= 1.1 + 2.2 / (G - 2), axis=1)
        self.err_expected = 0 if inside.all() else 1 | 2 * int((~inside).sum())
        B = cport.MatrixFreeWISKI(GB, G, sigma2=0.5, dtype=np.float64)
        idx, val = B.interp(X[inside].astype(np.float64))
        yw, wa = (y.astype(np.float64) * w)[inside], w.astype(np.float64)[inside]
        pred = (val * u.astype(np.float64)[idx]).sum(1)
        inc = {k: np.zeros(m) for k in ("b", "cnt", "res")}
        np.add.at(inc["b"], idx, val * yw[:, None])
        np.add.at(inc["cnt"], idx, val * wa[:, None])
        np.add.at(inc["res"], idx, val * (yw - wa * pred)[:, None])
        self.ref = {k: self.start[k].astype(np.float64) + inc[k] for k in inc}
        touched = np.zeros(m)
        np.add.at(touched, idx[val != 0], 1.0)
        self.cmax, self.wa_max = float(touched.max()), float(w.max())
        mk = lambda a: torch.as_tensor(a, device="cuda")
        self.dev = dict(x=mk(X), y=mk(y), w=mk(w), noise=mk(noise), u=mk(u))

    def run(self, staged, guard=None, expect=0):
        from online_gp_amd import _hip, grid_ops

        d = self.dev
        out = {k: torch.as_tensor(v, device="cuda").clone() for k, v in self.start.items()}
        out.update(stats=torch.zeros(2, device="cuda", dtype=torch.float64), mean=torch.full((self.n,), float("nan"), device="cuda"),
                   err=grid_ops.new_err_flag("cuda"), stage=torch.zeros(self.m * 4, device="cuda"))
        p = lambda t: _hip.dptr(t).value
        a = _hip.wiski_absorb_args(d_x=p(d["x"]), d_y=p(d["y"]), d_wa=p(d["w"]), d_wb=p(d["w"]), d_noise=p(d["noise"]), n=self.n, d_b=p(out["b"]), d_A=p(out["A"]),
                                   half=1, d_cnt=p(out["cnt"]), d_stats=p(out["stats"]), d_err=p(out["err"]), d_u=p(d["u"]), d_res=p(out["res"]),
                                   d_mean_out=p(out["mean"]), nout=1, d_guard=p(guard) if guard is not None else None, guard_expect=expect)
        s = _hip.stream_ptr(d["x"].device)
        lib = _hip.lib()
        if staged:
            assert lib.wiski_absorb_staged_f32(self.grid.ref, ctypes.byref(a), _hip.dptr(out["stage"]), s) == 0
            out["staged_b"] = out["b"].clone()                     # before the fold: the three arrays have not seen the batch
            assert lib.wiski_tap_fold_f32(_hip.dptr(out["stage"]), _hip.dptr(out["b"]), _hip.dptr(out["cnt"]), _hip.dptr(out["res"]), i64(self.m), s) == 0
        else:
            assert lib.wiski_absorb_f32(self.grid.ref, ctypes.byref(a), s) == 0
        torch.cuda.synchronize()
        return out


_cases = {}


def _case(name):
    if name not in _cases:
        c = _Case(name)
        c.staged, c.direct = c.run(True), c.run(False)
        _cases[name] = c
    return _cases[name]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64)


def _bit_zero(t):
    return not bool((_bits(t) != 0).any())


@pytest.mark.parametrize("name", list(BATCHES))
def test_staged_and_direct_absorb_against_the_fp64_reference(name):
    c = _case(name)
    for k in ("b", "cnt", "res"):
        ref = c.ref[k]
        bound = TOL32 * np.abs(ref).max()
        for label, out in (("staged", c.staged), ("direct", c.direct)):
            dev = np.abs(out[k].double().cpu().numpy() - ref).max()
            print(f"{name} {k} {label}: max deviation {dev:.3e}  (bound {bound:.3e})")
            assert dev <= bound, (k, label)
    assert torch.equal(c.staged["staged_b"], torch.as_tensor(c.start["b"], device="cuda"))


@pytest.mark.parametrize("name", list(BATCHES))
def test_everything_outside_the_stage_is_unchanged(name):
    c = _case(name)
    s, d = c.staged, c.direct
    dev = float((s["A"].double() - d["A"].double()).abs().max())
    bound = c.cmax * 2.0 ** -24 * c.cmax * c.wa_max if c.cmax > 1 else 0.0
    print(f"{name}: A_h differs by {dev:.3e} (bound {bound:.3e}, {c.cmax:.0f} points on the busiest node); err = {int(s['err'].item())}")
    assert dev <= bound
    assert float((d["A"] - torch.as_tensor(c.start["A"], device="cuda")).abs().max()) > 0          # (the batch did reach A_h)
    assert torch.equal(_bits(s["stats"]), _bits(d["stats"])) and torch.equal(_bits(s["mean"]), _bits(d["mean"]))
    assert int(s["err"].item()) == int(d["err"].item()) == c.err_expected


@pytest.mark.parametrize("name", list(BATCHES))
def test_stage_is_bit_zero_after_the_fold(name):
    c = _case(name)
    assert _bit_zero(c.staged["stage"])
    assert _bit_zero(c.direct["stage"])


def test_closed_guard_stages_nothing():
    c = _case("n5")
    guard = torch.tensor([-7], device="cuda", dtype=torch.int64)
    out = c.run(True, guard, 7)
    for k in ("b", "cnt", "res", "A"):
        assert torch.equal(out[k], torch.as_tensor(c.start[k], device="cuda")), k
    assert _bit_zero(out["stage"]) and bool(torch.isnan(out["mean"]).all()) and float(out["stats"].abs().max()) == 0.0
    guard.fill_(7)
    out = c.run(True, guard, 7)                                     # the open guard: the staged absorb
    assert float((out["b"].double().cpu() - torch.as_tensor(c.ref["b"])).abs().max()) <= TOL32 * np.abs(c.ref["b"]).max()
    assert _bit_zero(out["stage"]) and not bool(torch.isnan(out["mean"]).any())


def test_refusals():
    """No stage, a grid of another dimension, no cnt, no carry, a shard, two outputs: WISKI_E_BADARG and nothing written."""
    from online_gp_amd import _hip, grid_ops

    c = _case("n5")
    d = c.dev
    p = lambda t: None if t is None else _hip.dptr(t).value
    z = lambda n: torch.zeros(n, device="cuda")
    H = (c.grid.R + 1) // 2
    t = dict(b=z(c.m), A=z(H * c.m), cnt=z(c.m), res=z(c.m), stats=torch.zeros(2, device="cuda", dtype=torch.float64), err=grid_ops.new_err_flag("cuda"),
             stage=z(4 * c.m))
    grid2 = grid_ops.GridSpec([[-1.1, 1.1]] * 2, G)
    lib, s = _hip.lib(), _hip.stream_ptr(d["x"].device)

    def call(grid=c.grid, stage=t["stage"], **over):
        f = dict(d_x=p(d["x"]), d_y=p(d["y"]), d_wa=p(d["w"]), d_wb=p(d["w"]), d_noise=p(d["noise"]), n=c.n, d_b=p(t["b"]), d_A=p(t["A"]), half=1,
                 d_cnt=p(t["cnt"]), d_stats=p(t["stats"]), d_err=p(t["err"]), d_u=p(d["u"]), d_res=p(t["res"]), nout=1)
        f.update(over)
        a = _hip.wiski_absorb_args(**f)
        return lib.wiski_absorb_staged_f32(grid.ref, ctypes.byref(a), _hip.dptr(stage), s)

    table = [("no stage", call(stage=None)), ("d = 2", call(grid=grid2)), ("no cnt", call(d_cnt=None)), ("no carry", call(d_u=None, d_res=None)),
             ("shard", call(g_lo=0, g_hi=3)), ("nout = 2", call(nout=2)), ("full stencil", call(half=0)), ("channels", call(channels=4))]
    table.append(("fold without stage", lib.wiski_tap_fold_f32(None, _hip.dptr(t["b"]), None, None, i64(c.m), s)))
    torch.cuda.synchronize()
    print(table)
    assert [(what, rc) for what, rc in table if rc != -1] == []
    assert all(float(v.abs().max()) == 0.0 for v in t.values())


# ------------------------------------------------------------------------------------------------------ wiski_stream_step_f32
Q, STEPS, TOL, U_RTOL = 64, 3, 1e-4, 2e-3
FIRST_POLL = 50     # iterations queued before the first poll: past convergence (a converged column no longer moves), so every poll finds the
                    # solve converged and the guarded absorb behind it runs; the iteration count that says something is the poll's hindsight


def _stream(keep, staged):
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(5)
    grid = grid_ops.GridSpec(GB, G)
    dev, dt = torch.device("cuda", torch.cuda.current_device()), torch.float32
    X = rng.uniform(-1.0, 1.0, (STEPS * Q, 3))
    y = np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.3 * X[:, 2] + 0.1 * rng.standard_normal(X.shape[0])
    X, y = torch.as_tensor(X, device=dev, dtype=dt), torch.as_tensor(y, device=dev, dtype=dt)
    ones = torch.ones(Q, device=dev, dtype=dt)
    B = cport.MatrixFreeWISKI(GB, G, sigma2=0.5, dtype=np.float64)
    tcol = torch.as_tensor(np.ascontiguousarray(B.tcol)).to(dev, dt)
    m, z = grid.m, lambda *s, dt=dt: torch.zeros(*s, device=dev, dtype=dt)
    st = dict(A=z(((grid.R + 1) // 2) * m), b=z(m), cnt=z(m), stats=z(2, dt=torch.float64), err=grid_ops.new_err_flag("cuda"), U=z(m), Z=z(m), R=z(m))
    step = grid_ops.StreamStep(grid, dt, dev, st["A"], st["b"], st["cnt"], st["stats"], st["err"], st["U"], st["Z"], st["R"], tcol, grid_ops.PCGWorkspace(), 200)
    step.set_solver(1.0 / B.sigma2, grid_ops.kron_eigen(grid, tcol), 0.0, TOL, 1)
    step.set_keep(keep)
    assert step.tap_stage is not None and step.args.d_tap_stage == step.tap_stage.data_ptr()
    if not staged:
        step.args.d_tap_stage = None
    iters, means, zero, first_ok = [], [], [], []
    for t in range(STEPS):
        sl = slice(t * Q, (t + 1) * Q)
        step.args.shift = (t + 1) * Q / m
        mean = torch.empty(Q, device=dev, dtype=dt)
        prev, pending = step(X[sl], y[sl], ones, ones, ones, mean, 1, FIRST_POLL, defer=True)
        assert pending and (t == 0 or step.handle.guard_ok == 1)           # from the second call on the guarded absorb is the one that ran
        zero.append(_bit_zero(step.tap_stage))                             # (a read on the stream: whenever the call has returned)
        iters.append(prev[0] if prev else None)
        first_ok.append(step.handle.first_ok if prev else None)
        means.append(mean)
    prev, pending = step(None, None, None, None, None, None, 0, 0, defer=False)
    assert not pending
    torch.cuda.synchronize()
    assert int(st["err"].item()) == 0
    first_ok.append(step.handle.first_ok)
    return dict(iters=iters + [prev[0]], first_ok=first_ok, means=torch.stack(means), zero=zero, U=st["U"].clone(), R=st["R"].clone(), b=st["b"].clone(), cnt=st["cnt"].clone())


@pytest.mark.parametrize("keep,what", [((8, 8, 8), "fold in k_keep_fwd"), (None, "k_tap_fold")], ids=["keep", "full"])
def test_stream_steps_with_and_without_the_stage(keep, what):
    from online_gp_amd import grid_ops

    if keep is not None:
        assert grid_ops.keep_accepts(grid_ops.GridSpec(GB, G), keep)
    a, b = _stream(keep, True), _stream(keep, False)
    print(f"{what}: iterations {a['iters']} / {b['iters']}, first converged slot {a['first_ok']} / {b['first_ok']}")
    assert a["zero"] == [True] * STEPS
    assert a["iters"] == b["iters"] and all(v is not None for v in a["iters"][1:])
    assert a["first_ok"] == b["first_ok"] and all(0 < v < FIRST_POLL for v in a["first_ok"][1:])
    for k in ("U", "means", "b", "cnt"):
        dev, scale = float((a[k] - b[k]).abs().max()), float(b[k].abs().max())
        print(f"{what}: {k} differs by {dev:.3e} of a maximum of {scale:.3e}")
        assert dev <= U_RTOL * scale, k
    # R is the residual of a converged solve, ||R|| < TOL ||b|| in both runs: they differ by less than twice that
    dev, scale = float((a["R"] - b["R"]).double().norm()), float(b["b"].double().norm())
    print(f"{what}: ||R - R'|| = {dev:.3e} against ||b|| = {scale:.3e}")
    assert dev <= 2 * TOL * scale
