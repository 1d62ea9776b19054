"""The convergence poll carries hindsight (include/wiski.h: wiski_pcg_async::first_ok, first_check = -1).

Every poll of a solve publishes, beside the residual norms, the first iteration at which every column had met the tolerance; a
deferred-poll handle keeps it, and `first_check = -1` places the next solve's first poll there.  Shapes: 12^3 fp32 with one column
(the fused path: the update rides in the forward kernel, the poll is published by the last-ticket block of k_pcg_update_x<float, 4>)
and 8^3 fp64 with two columns through wiski_pcg_async (the update is a launch of its own; the column maximum).  k_pcg_publish writes
the same word but is only launched for a poll at iteration 0, which no entry point reaches (max_iter >= 1 always runs an
iteration), so no case here drives it.  Systems of a few hundred random points, as tests/test_hip_ops.py builds them."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cport
from test_hip_ops import _pcg_case

pytestmark = pytest.mark.gpu

i32 = ctypes.c_int32
OK, PENDING, BADARG, NOTCONV = 0, 1, -1, -4
CASES = [(3, 12, torch.float32, np.float32, 1), (3, 8, torch.float64, np.float64, 2)]
IDS = ["12^3-f32-k1", "8^3-f64-k2"]
U_RTOL = 2e-3       # fp32: START + RESUME against a synchronous solve in tests/test_hip_ops.py (test_pcg_entry_points_agree)
# The tests compare iteration COUNTS of repeated solves of one system.  The products accumulate with atomics, so two runs differ by
# rounding, and CG amplifies that as the residual approaches the precision floor: at the tolerances of tests/test_hip_ops.py two
# runs of the fp64 case differed by up to 7 % in a relative residual of 4e-11 after 36 iterations (a count then moved from 37 to 36),
# fp32 by 1e-4 at 7e-7.  The deviation scales like eps / residual, so these tolerances leave it at 1e-5 of the residual or less
TOL = {torch.float32: 1e-4, torch.float64: 1e-6}


class _Solves:
    """One system and a way to solve it again and again from the same cold start through wiski_pcg_async."""

    def __init__(self, d, g, tdt, ndt, k):
        from online_gp_amd import _hip, grid_ops

        self.f, _, _ = _pcg_case(d, g, tdt, ndt, 300, k)
        self.tdt, self.k = tdt, k
        self.f["R"] = torch.zeros_like(self.f["U"])
        self.f["tol"] = TOL[tdt]
        self.fn = _hip.fn("wiski_pcg_async", tdt)
        self.abi = grid_ops._pcg_abi
        self.handle = grid_ops._PcgAsync()

    def __call__(self, mode, **over):
        a = {**self.f, **over}
        rc = self.fn(*self.abi(self.tdt, **a), ctypes.byref(self.handle), i32(mode))
        return rc, a["h_iters"].value, list(a["h_relres"])

    def per_iteration(self, **over):
        """The solve polled after every iteration: (iterations it needs, relres)."""
        rc, n, rel = self(0, first_check=1, check_every=1, **over)
        assert rc == OK, rc
        return n, rel

    def free(self):
        from online_gp_amd import _hip

        assert _hip.lib().wiski_pcg_async_free(ctypes.byref(self.handle)) == 0


_CACHE = {}


def _case(i):
    """Case i with its reference count `n`: the solve polled after every iteration, computed once."""
    if i not in _CACHE:
        s = _CACHE[i] = _Solves(*CASES[i])
        s.n, s.rel = s.per_iteration()
        assert s.handle.first_ok == s.n and s.handle.first_ok_valid == 1    # a poll after every iteration: the first success is the count
        print(f"{IDS[i]}, per-iteration polls: n = {s.n}, relres = {s.rel}")
    return _CACHE[i]


@pytest.fixture(scope="module", autouse=True)
def _free_handles():
    yield
    while _CACHE:
        _CACHE.popitem()[1].free()


@pytest.fixture(params=range(len(CASES)), ids=IDS)
def solves(request):
    return _case(request.param)


def test_hindsight_is_exact(solves):
    """A poll two iterations later than needed reports where the tolerance was first met; the two extra iterations are masked."""
    s, n = solves, solves.n
    rc, _, _ = s(1, first_check=n + 2, check_every=1)
    assert rc == PENDING and s.handle.state == 1 and s.handle.it == n + 2
    rc, it, rel = s(2, first_check=n + 2, check_every=1)
    print(f"late poll: first_ok = {s.handle.first_ok}, iters = {it}, relres = {rel} (per-iteration: {s.rel})")
    assert rc == OK and s.handle.state == 0
    assert s.handle.first_ok == n and s.handle.first_ok_valid == 1
    assert it == n + 2
    assert max(rel) < s.f["tol"] and max(s.rel) < s.f["tol"]


def test_first_ok_is_the_larger_count_of_two_columns():
    """Each column alone, polled after every iteration, gives its own count; the joint solve reports the larger one."""
    s = _case(1)
    assert s.k == 2
    alone = []
    for c in range(s.k):
        one = {n: s.f[n][c:c + 1] for n in ("RHS", "U", "Z", "R")}
        alone.append(s.per_iteration(k=1, h_relres=(ctypes.c_double * 1)(), **one)[0])
    print(f"columns alone: {alone}, joint: {s.n}")
    assert len(set(alone)) > 1                       # the case is chosen so that the counts differ
    rc, _, _ = s(1, first_check=s.n + 2, check_every=1)
    assert rc == PENDING
    rc, it, _ = s(2, first_check=s.n + 2, check_every=1)
    assert rc == OK and s.handle.first_ok == max(alone) == s.n and it == s.n + 2


def test_a_poll_that_fails_first(solves):
    s, n = solves, solves.n
    assert n >= 2
    rc, _, _ = s(1, first_check=n - 1, check_every=1)
    assert rc == PENDING and s.handle.it == n - 1
    rc, it, _ = s(2, first_check=n - 1, check_every=1)
    assert rc == OK and it == n and s.handle.first_ok == n and s.handle.first_ok_valid == 1
    assert s.handle.guard_ok == 0                    # the poll the START queued did not find the solve converged


def test_already_converged(solves):
    """A warm start from the converged (U, Z, R): the one iteration the solve queues is masked, first_ok = 0."""
    s = solves
    rc, _, _ = s(0, first_check=1, check_every=1)    # leaves the converged state in U, Z and the caller's R
    assert rc == OK
    rc, it, rel = s(0, warm=2, first_check=1, check_every=1)
    print(f"warm from the solution: first_ok = {s.handle.first_ok}, iters = {it}, relres = {rel}")
    assert rc == OK and it == 1 and s.handle.first_ok == 0 and s.handle.first_ok_valid == 1


def test_no_slot_met_the_tolerance(solves):
    s, n = solves, solves.n
    assert n >= 2
    rc, it, rel = s(0, max_iter=n - 1, first_check=1, check_every=1)
    print(f"max_iter = {n - 1}: rc = {rc}, first_ok = {s.handle.first_ok}, valid = {s.handle.first_ok_valid}, relres = {rel}")
    assert rc == NOTCONV and it == n - 1
    assert s.handle.first_ok == -1 and s.handle.first_ok_valid == 0
    s.per_iteration()                                # (leave the handle with history for whichever test runs next)


def test_refusals(solves):
    """-1 without a handle, -2 with one: WISKI_E_BADARG before anything is queued or a handle field written (what
    test_pcg_refusal_table of tests/test_hip_ops.py demands of every refusal)."""
    from online_gp_amd import _hip, grid_ops

    s = solves
    U, Z = torch.full_like(s.f["U"], float("nan")), torch.full_like(s.f["Z"], float("nan"))
    work = s.f["work"]
    work.fill_(0x5A)
    h = grid_ops._PcgAsync()
    h.prezeroed, h.first_ok, h.first_ok_valid = 1, 7, 1
    a = {**s.f, "U": U, "Z": Z}
    table = [("pcg -1", _hip.fn("wiski_pcg", s.tdt)(*s.abi(s.tdt, **{**a, "first_check": -1}))),
             ("async -1, no handle", s.fn(*s.abi(s.tdt, **{**a, "first_check": -1}), None, i32(0))),
             ("async -2, handle", s.fn(*s.abi(s.tdt, **{**a, "first_check": -2}), ctypes.byref(h), i32(0))),
             ("async START -2, handle", s.fn(*s.abi(s.tdt, **{**a, "first_check": -2}), ctypes.byref(h), i32(1)))]
    torch.cuda.synchronize()
    print("refusals:", table)
    assert all(rc == BADARG for _, rc in table), table
    assert bool(torch.isnan(U).all()) and bool(torch.isnan(Z).all()) and bool((work == 0x5A).all())
    assert (h.state, h.prezeroed, h.first_ok, h.first_ok_valid, h.poll) == (0, 1, 7, 1, None)


# ------------------------------------------------------------------ wiski_stream_step places the poll ---
Q, STEPS, G = 256, 12, 12


class _Stream:
    """A 12^3 fp32 stream from empty statistics through grid_ops.StreamStep (= wiski_stream_step), deferred."""

    def __init__(self):
        from online_gp_amd import grid_ops

        rng = np.random.default_rng(5)
        gb = [[-1.1, 1.1]] * 3
        self.grid = grid = grid_ops.GridSpec(gb, G)
        dev, dt = torch.device("cuda", torch.cuda.current_device()), torch.float32
        X = rng.uniform(-1.0, 1.0, (STEPS * Q, 3))
        y = np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.3 * X[:, 2] + 0.1 * rng.standard_normal(X.shape[0])
        self.X, self.y = torch.as_tensor(X, device=dev, dtype=dt), torch.as_tensor(y, device=dev, dtype=dt)
        self.ones = torch.ones(Q, device=dev, dtype=dt)
        B = cport.MatrixFreeWISKI(gb, G, sigma2=0.5, dtype=np.float64)
        self.tcol = torch.as_tensor(np.ascontiguousarray(B.tcol)).to(dev, dt)
        self.kscale = 1.0 / B.sigma2
        self.eig = grid_ops.kron_eigen(grid, self.tcol)
        self.ws = grid_ops.PCGWorkspace()
        self.dev, self.dt = dev, dt

    def fresh(self):
        from online_gp_amd import grid_ops

        m, z = self.grid.m, lambda *s, dt=self.dt: torch.zeros(*s, device=self.dev, dtype=dt)
        st = dict(A=z(((self.grid.R + 1) // 2) * m), b=z(m), cnt=z(m), stats=z(2, dt=torch.float64), err=grid_ops.new_err_flag("cuda"), U=z(m), Z=z(m), R=z(m))
        step = grid_ops.StreamStep(self.grid, self.dt, self.dev, st["A"], st["b"], st["cnt"], st["stats"], st["err"], st["U"], st["Z"], st["R"], self.tcol,
                                   self.ws, 200)
        step.set_solver(self.kscale, self.eig, 0.0, TOL[self.dt], 1)
        return step, st

    def run(self, first_checks):
        """The stream with these first_check arguments: per call (placement of the new solve's first poll, what the call reported
        of the solve it resumed, the handle's hindsight after the call), then the last solve finished, then U."""
        step, st = self.fresh()
        calls = []
        for t in range(STEPS):
            sl = slice(t * Q, (t + 1) * Q)
            step.args.shift = (t + 1) * Q / self.grid.m
            mean = torch.empty(Q, device=self.dev, dtype=self.dt)
            prev, pending = step(self.X[sl], self.y[sl], self.ones, self.ones, self.ones, mean, 1, first_checks[t], defer=True)
            assert pending and int(st["err"].item()) == 0
            h = step.handle
            calls.append(dict(placed=h.it, resumed=step.resumed.value, iters=prev[0] if prev else None, first_ok=h.first_ok, valid=h.first_ok_valid))
        prev, pending = step(None, None, None, None, None, None, 0, 0, defer=False)
        assert not pending
        torch.cuda.synchronize()
        return calls, prev[0], st["U"].clone()


@pytest.fixture(scope="module")
def stream():
    s = _Stream()
    s.auto = s.run([-1] * STEPS)
    return s


def test_auto_places_the_first_poll_at_the_previous_first_ok(stream):
    calls, last_iters, _ = stream.auto
    for t, c in enumerate(calls):
        print(f"auto step {t}: {c}")
    assert calls[0]["valid"] == 0 and calls[0]["resumed"] == 0
    for t in range(1, STEPS):
        c = calls[t]
        assert c["resumed"] == 1 and c["valid"] == 1
        # the handle's hindsight after call t is that of the solve call t resumed: the START of the same call polls there
        assert c["placed"] == max(1, c["first_ok"]), (t, c)
        assert c["first_ok"] <= c["iters"]


def test_auto_equals_the_same_stream_at_explicit_placements(stream):
    calls, last_iters, U = stream.auto
    explicit = stream.run([c["placed"] for c in calls])
    for t, (a, b) in enumerate(zip(calls, explicit[0])):
        assert (a["placed"], a["resumed"], a["iters"], a["first_ok"]) == (b["placed"], b["resumed"], b["iters"], b["first_ok"]), (t, a, b)
    assert last_iters == explicit[1]
    err = float((U - explicit[2]).abs().max()) / float(U.abs().max())
    print(f"auto against explicit placements: U differs by {err:.2e} of its maximum")
    assert err < U_RTOL


def test_auto_without_history_equals_first_check_zero(stream):
    zero = stream.run([0] + [c["placed"] for c in stream.auto[0]][1:])
    assert zero[0][0]["placed"] == stream.auto[0][0]["placed"] == 1          # check_every = 1
    assert [c["iters"] for c in zero[0]] == [c["iters"] for c in stream.auto[0]]


def test_stream_step_refusals(stream):
    """-1 without a handle, -2 with one: nothing queued (the statistics stay empty), no handle field written."""
    from online_gp_amd import _hip, grid_ops

    step, st = stream.fresh()
    h = grid_ops._PcgAsync()
    h.prezeroed, h.first_ok, h.first_ok_valid = 1, 7, 1
    mean = torch.full((Q,), float("nan"), device=stream.dev, dtype=stream.dt)
    it, rr, he, resumed = i32(0), ctypes.c_double(0), i32(0), i32(0)

    def call(fc, handle):
        p = _hip.dptr
        return step.fn(stream.grid.ref, ctypes.byref(step.args), p(stream.X[:Q]), p(stream.y[:Q]), p(stream.ones), p(stream.ones), p(stream.ones),
                       ctypes.c_int64(Q), p(mean), i32(1), i32(fc), ctypes.byref(it), ctypes.byref(rr), ctypes.byref(he), _hip.stream_ptr(stream.dev),
                       handle, i32(1 if handle is not None else 0), ctypes.byref(resumed))

    table = [("-1, no handle", call(-1, None)), ("-2, handle", call(-2, ctypes.byref(h))), ("-2, no handle", call(-2, None))]
    torch.cuda.synchronize()
    print("stream_step refusals:", table)
    assert all(rc == BADARG for _, rc in table), table
    assert all(float(st[n].abs().max()) == 0.0 for n in ("A", "b", "cnt", "U", "Z", "R")) and bool(torch.isnan(mean).all())
    assert (h.state, h.prezeroed, h.first_ok, h.first_ok_valid, h.poll) == (0, 1, 7, 1, None)


# ------------------------------------------------------------------------------------- model level ---
def test_model_stream_with_and_without_hindsight():
    """10 deferred stream_step calls of q = 512 on a 16^3 fp32 model with settings.poll_hindsight on and off: the same predictive
    means within the CG tolerance in force, and with the switch on no first poll is placed before the iteration at which the
    previous solve first met the tolerance."""
    from online_gp_amd import grid_ops, settings
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    rng = np.random.default_rng(31)
    d, g, n0, q, steps, cg_tol = 3, 16, 6000, 512, 10, 1e-5
    X = rng.uniform(-1, 1, (n0 + q * steps, d)); y = np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.3 * X[:, 2] + 0.1 * rng.standard_normal(X.shape[0])
    Xt, yt = torch.as_tensor(X, device="cuda", dtype=torch.float32), torch.as_tensor(y, device="cuda", dtype=torch.float32)[:, None]
    Xq = torch.as_tensor(rng.uniform(-1, 1, (64, d)), device="cuda", dtype=torch.float32)
    gb = torch.tensor([[-1.1, 1.1]] * d, dtype=torch.float64)
    seen = []
    orig = grid_ops.StreamStep.__call__

    def spy(self, x, y_, wa, wb, noise, mean_out, carry, first_check, defer=False):
        out = orig(self, x, y_, wa, wb, noise, mean_out, carry, first_check, defer=defer)
        if x is not None:
            seen.append(dict(first_check=int(first_check), placed=self.handle.it, first_ok=self.handle.first_ok, valid=self.handle.first_ok_valid,
                             pending=self.pending))
        return out

    means = {}
    grid_ops.StreamStep.__call__ = spy
    try:
        for on in (True, False):
            seen.clear()
            with settings.cg_tolerance(cg_tol), settings.deferred_refresh(True), settings.poll_hindsight(on), torch.no_grad():
                m = FixedNoiseOnlineSKIGP(Xt[:n0], yt[:n0], None, grid_bounds=gb, grid_size=g, learn_additional_noise=True).eval()
                m.prediction_cache
                for s in range(steps):
                    sl = slice(n0 + s * q, n0 + (s + 1) * q)
                    m.stream_step(Xt[sl], yt[sl])
                with settings.skip_posterior_variances(True):
                    means[on] = m(Xq).mean.clone()
            for c in seen:
                print(f"poll_hindsight {on}: {c}")
            # the one-call path with a handle carried the stream (a step may go through the generic path when the preconditioner ages)
            assert len(seen) >= steps - 2 and all(c["pending"] for c in seen)
            if on:
                # all but the first step after a cold solve, which keeps its explicit hint
                assert sum(c["first_check"] == -1 for c in seen) >= len(seen) - 2
                for c in seen:
                    if c["valid"]:
                        assert c["placed"] >= c["first_ok"], c
            else:
                assert all(c["first_check"] >= 0 for c in seen)
    finally:
        grid_ops.StreamStep.__call__ = orig
    err = float((means[True] - means[False]).abs().max()) / float(means[False].abs().max())
    print(f"predictive means with / without hindsight differ by {err:.2e} of their maximum (cg_tol {cg_tol})")
    assert err < cg_tol
