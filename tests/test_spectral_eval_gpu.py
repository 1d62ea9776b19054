"""GPU: the query-and-tail kernels of the spectral factor (csrc/spectral_basis.hip: wiski_spectral_evaluate and wiski_spectral_evaluate_y in both
dtypes, wiski_spectral_var, wiski_factor_tail, wiski_woodbury_c, wiski_mll_weights, wiski_basis_absorb_h in both dtypes) against the
np.longdouble reference of tests/spectral_eval_reference.py, per element, on the hand-built inputs of its case tables: both instantiations of
the one-launch evaluate (r <= 512 and 513 .. 1024), n on both sides of every multiple of 8 up to 64, ldl > r, spike rows at the 64-chunk
boundaries, tails above, below and exactly at zero, a variance that underflows in fp32, the GEMM form on a host-computed Y, both forms
alternating on one workspace, the dispatch corners of grid_ops.spectral_evaluate, the argument checks, and evaluate() of a streamed model fed
to the same reference.  Every input is fp32-representable where an fp32 entry reads it, every output array has a sentinel slot behind it,
and the 200 doubles of the workspace are bitwise zero after every call.

Bounds: spectral_eval_reference's docstring -- sums at (L + 2) eps64 sum |terms| carried through the later stages' absolute-value matrices,
the metrics through the partial derivatives at the reference, 8 eps32 per documented fp32 rounding; none taken from a kernel run.
tests/test_spectral_eval_host.py shows what share of them the reference's own plain-double and fp32 evaluations use and that eighteen
seeded defects each exceed them at least four times at some case of these tables.

Worst ratio to the bound per kernel and dtype on an MI355X: DESIGN.md 3.32."""
import ctypes

import numpy as np
import pytest
import torch

import spectral_eval_reference as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float64]
DT_IDS = ["f32", "f64"]
NP = {torch.float32: sr.F32, torch.float64: sr.F64}
F64 = sr.F64
SENT = sr.SENT
OK, BADARG = 0, -1
CASE_ID = lambda c: c["name"]        # noqa: E731
i32, i64, f64c = ctypes.c_int32, ctypes.c_int64, ctypes.c_double


def _t(x, dtype=torch.float64, pad=1):
    """A device tensor of x (flattened) with `pad` sentinel slots behind it."""
    x = np.asarray(x, F64).reshape(-1)
    return torch.tensor(np.concatenate([x, np.full(pad, SENT)]), dtype=dtype, device=DEV)


def _full(n, dtype=torch.float64):
    return torch.full((n,), SENT, dtype=dtype, device=DEV)


def _ws():
    return torch.cat([torch.zeros(200, dtype=torch.float64, device=DEV), _full(1)])


def _np(t):
    return t.detach().cpu().double().numpy()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    from online_gp_amd import _hip

    return _hip.stream_ptr(torch.device(DEV))


def _report(kernel, dtype, **ratios):
    dt = dtype if isinstance(dtype, str) else DT_IDS[DTYPES.index(dtype)]
    print(f"ratio-to-bound {kernel} {dt} " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


def _ws_is_zero(ws):
    assert float(ws[200]) == SENT, "the slot behind the workspace was written"
    assert not bool(ws[:200].view(torch.int64).any()), "the workspace was not left bitwise zero"


class _Eval:
    """The device side of one evaluate: inputs uploaded once (fp32-representable, checked), fresh sentinel-filled outputs per call."""

    def __init__(self, x, dtype, err, Y=None):
        self.x, self.dtype = x, dtype
        self.n, self.r = x["F"].shape
        self.F, self.prior, self.Linv, self.t = _t(x["F"]), _t(x["prior"]), _t(x["Linv"]), _t(x["t"])
        self.s2, self.y = _t(x["s2"], dtype), _t(x["y"], dtype)
        assert np.array_equal(_np(self.y)[:-1], x["y"]) and float(self.s2[0].double()) == x["s2"], "inputs are fp32-representable"
        self.err = None if err is None else torch.tensor([err], dtype=torch.int32, device=DEV)
        self.Y = None if Y is None else _t(Y)
        self.inputs = [t for t in (self.F, self.prior, self.Linv, self.t, self.s2, self.y, self.Y) if t is not None]
        self.before = [t.clone() for t in self.inputs]

    def call(self, form, ws, moments, **over):
        from online_gp_amd import _hip

        n, r = over.pop("n", self.n), over.pop("r", self.r)
        ldl = over.pop("ldl", self.x["ldl"])
        a = {"F": self.F, "prior": self.prior, "Linv": self.Linv, "t": self.t, "s2": self.s2, "y": self.y, "Y": self.Y, "ws": ws,
             "out": _full(5), "mean": _full(self.n + 1, self.dtype) if moments else None, "var": _full(self.n + 1, self.dtype) if moments else None}
        for k in over:
            assert k in a and over[k] is None
            a[k] = None
        if form == "one":
            rc = _hip.fn("wiski_spectral_evaluate", self.dtype)(i32(n), i32(r), _ptr(a["F"]), _ptr(a["prior"]), _ptr(a["Linv"]), i32(ldl), _ptr(a["t"]),
                                                                f64c(self.x["kscale"]), _ptr(a["s2"]), _ptr(a["y"]), _ptr(self.err), _ptr(a["ws"]),
                                                                _ptr(a["out"]), _ptr(a["mean"]), _ptr(a["var"]), _stream())
        else:
            rc = _hip.fn("wiski_spectral_evaluate_y", self.dtype)(i32(n), i32(r), _ptr(a["Y"]), _ptr(a["F"]), _ptr(a["prior"]), _ptr(a["t"]),
                                                                  f64c(self.x["kscale"]), _ptr(a["s2"]), _ptr(a["y"]), _ptr(self.err), _ptr(a["ws"]),
                                                                  _ptr(a["out"]), _ptr(a["mean"]), _ptr(a["var"]), _stream())
        torch.cuda.synchronize()
        return rc, a

    def check(self, a, ref, ws):
        """Sentinels, read-only inputs, the zero workspace; the worst ratio to the bound of the four slots and, if asked for, the moments."""
        for t, b in zip(self.inputs, self.before):
            assert torch.equal(t, b), "an input was written"
        assert float(a["out"][4]) == SENT
        _ws_is_zero(ws)
        got = _np(a["out"])[:4]
        assert got[2] == ref["out"][2]                                 # the flag: exact
        w = {k: float(r_) for k, r_ in zip(("rmse", "nll", "flag", "max_abs_mean"), sr.ratios(got, ref["out"], ref["d_out"]))}
        del w["flag"]
        if a["mean"] is not None:
            assert float(a["mean"][self.n]) == SENT and float(a["var"][self.n]) == SENT
            w["mean"] = float(sr.ratios(_np(a["mean"])[:self.n], ref["mean"], ref["d_mean"]).max())
            w["var"] = float(sr.ratios(_np(a["var"])[:self.n], ref["var"], ref["d_var"]).max())
        return w


# ---------------------------------------------------------------------------------------------------- a. the one-launch evaluate
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", sr.EVAL_CASES, ids=CASE_ID)
def test_spectral_evaluate_one_launch(case, dtype):
    ref = sr.held_to(case["name"], NP[dtype])
    ev = _Eval(sr.case_inputs(case["name"]), dtype, case["err"])
    ws = _ws()
    rc, a = ev.call("one", ws, case["moments"])
    assert rc == OK
    w = ev.check(a, ref, ws)
    rc, b = ev.call("one", ws, not case["moments"])                    # the same workspace again, the moments the other way round
    assert rc == OK
    w2 = ev.check(b, ref, ws)
    _report("spectral_evaluate", dtype, **{k: max(w.get(k, 0.0), w2.get(k, 0.0)) for k in {**w, **w2}})
    assert max(w.values()) <= 1.0 and max(w2.values()) <= 1.0, (w, w2)


# ------------------------------------------------------------------------------------------------------------ b. the GEMM form
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", sr.EVAL_Y_CASES, ids=CASE_ID)
def test_spectral_evaluate_y_on_a_host_computed_product(case, dtype):
    """Y = chol^-1 F^T comes from the host (rounded to fp64 once): the kernel is held, not the GEMM."""
    ref = sr.held_to(case["name"], NP[dtype], given_y=True)
    ev = _Eval(sr.case_inputs(case["name"]), dtype, case["err"], Y=sr.case_solve(case["name"])[0].astype(F64))
    ws = _ws()
    rc, a = ev.call("y", ws, case["moments"])
    assert rc == OK
    w = ev.check(a, ref, ws)
    rc, b = ev.call("y", ws, not case["moments"])
    assert rc == OK
    w2 = ev.check(b, ref, ws)
    _report("spectral_evaluate_y", dtype, **{k: max(w.get(k, 0.0), w2.get(k, 0.0)) for k in {**w, **w2}})
    assert max(w.values()) <= 1.0 and max(w2.values()) <= 1.0, (w, w2)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_both_forms_alternate_on_one_workspace(dtype):
    ws = _ws()
    worst = {}
    for form, case in sr.SEQUENCE:
        given = form == "y"
        ref = sr.held_to(case["name"], NP[dtype], given_y=given)
        ev = _Eval(sr.case_inputs(case["name"]), dtype, case["err"], Y=sr.case_solve(case["name"])[0].astype(F64) if given else None)
        rc, a = ev.call(form, ws, True)
        assert rc == OK
        w = ev.check(a, ref, ws)
        assert max(w.values()) <= 1.0, (case["name"], w)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
    _report("spectral_evaluate_alternating", dtype, **worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", sr.DISPATCH_CASES, ids=CASE_ID)
def test_grid_ops_spectral_evaluate_at_the_dispatch_corners(case, dtype, monkeypatch):
    """(64, 1024) is one launch; (65, 1024), (64, 1025) and (1, 1025) are GEMM + wiski_spectral_evaluate_y.  The GEMM's own rounding enters: the
    reference's bound of Y is carried through dg as an input error."""
    from online_gp_amd import grid_ops

    x = sr.case_inputs(case["name"])
    n, r = x["F"].shape
    ref = sr.held_to(case["name"], NP[dtype])
    gemms = []
    real_gemm = grid_ops.gemm
    monkeypatch.setattr(grid_ops, "gemm", lambda *a_, **k_: gemms.append(1) or real_gemm(*a_, **k_))
    dev = lambda v, dt=torch.float64: torch.tensor(np.asarray(v, F64), dtype=dt, device=DEV)      # noqa: E731
    err = None if case["err"] is None else torch.tensor([case["err"]], dtype=torch.int32, device=DEV)
    ws = _ws()
    worst = {}
    for moments in (True, False):
        res = grid_ops.spectral_evaluate(dev(x["F"]), dev(x["prior"]), dev(x["Linv"]), dev(x["t"]), x["kscale"], dev([x["s2"]], dtype), dev(x["y"], dtype), err,
                                         ws[:200], want_moments=moments)
        torch.cuda.synchronize()
        out, mean, var = res if moments else (res, None, None)
        _ws_is_zero(ws)
        got = _np(out)
        assert got[2] == ref["out"][2]
        w = dict(zip(("rmse", "nll", "flag", "max_abs_mean"), (float(v) for v in sr.ratios(got, ref["out"], ref["d_out"]))))
        if moments:
            assert mean.dtype == dtype and mean.shape == (n,) and var.shape == (n,)
            w["mean"] = float(sr.ratios(_np(mean), ref["mean"], ref["d_mean"]).max())
            w["var"] = float(sr.ratios(_np(var), ref["var"], ref["d_var"]).max())
        assert max(w.values()) <= 1.0, w
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
    assert len(gemms) == (0 if (n <= 64 and r <= 1024) else 2), "the dispatch took the other form"
    _report("grid_ops.spectral_evaluate", dtype, **worst)


# ------------------------------------------------------------------------------------------------------------- c. spectral_var
@pytest.mark.parametrize("case", sr.VAR_CASES, ids=CASE_ID)
def test_spectral_var_both_kernels(case):
    from online_gp_amd import _hip, grid_ops

    Y, F, prior, ksc = sr.var_inputs(case["name"])
    r, n = Y.shape
    ref = sr.spectral_var(Y, F, prior, ksc)
    if n >= 7:
        pre = prior * ksc - (F * F).sum(1)
        assert (pre > 0).any() and (pre < 0).any() and (pre == 0).any()
    Yd, Fd, pd, diag, tail = _t(Y), _t(F), _t(prior), _full(n + 1), _full(n + 1)
    rc = _hip.lib().wiski_spectral_var(i32(n), i32(r), _ptr(Yd), _ptr(Fd), _ptr(pd), f64c(ksc), _ptr(diag), _ptr(tail), _stream())
    torch.cuda.synchronize()
    assert rc == OK and float(diag[n]) == SENT and float(tail[n]) == SENT
    w = {"diag": float(sr.ratios(_np(diag)[:n], ref["diag"], ref["d_diag"]).max()), "tail": float(sr.ratios(_np(tail)[:n], ref["tail"], ref["d_tail"]).max())}
    _report("spectral_var", "f64", **w)
    assert max(w.values()) <= 1.0, w
    assert bool((tail[:n] >= 0).all()) and np.array_equal(_np(tail)[:n] == 0.0, ref["tail"] == 0.0)          # clamped where the reference clamps
    d2, t2 = grid_ops.spectral_var(Yd[:-1].view(r, n), Fd[:-1].view(n, r), pd[:-1], ksc)                    # the wrapper: the same launch
    assert torch.equal(d2, diag[:n]) and torch.equal(t2, tail[:n])


# -------------------------------------------------------------------------------------------------------------- d. factor tail
@pytest.mark.parametrize("shape", sr.TAIL_CASES, ids=lambda s: f"r{s[0]}_rref{s[1]}")
def test_factor_tail_all_seven_outputs(shape):
    from online_gp_amd import _hip, grid_ops

    r, r_ref = shape
    x = sr.tail_inputs(r, r_ref)
    ref = sr.factor_tail(**x)
    TS, h, sq, Linv, chol = (_t(x[k]) for k in ("TS", "h_ref", "sq", "Linv", "chol"))
    out = _full(6 * r + 3)
    rc = _hip.lib().wiski_factor_tail(i32(r_ref), i32(r), _ptr(TS), _ptr(h), _ptr(sq), _ptr(Linv), _ptr(chol), _ptr(out), _stream())
    torch.cuda.synchronize()
    assert rc == OK and float(out[6 * r + 2]) == SENT, "the slot behind 6 r + 2 was written"
    o = _np(out)
    got = {"hr": o[:r], "c": o[r:2 * r], "t": o[2 * r:3 * r], "coef": o[3 * r:4 * r], "zeta": o[4 * r:5 * r], "bMb": o[5 * r], "logdet": o[5 * r + 1]}
    w = {k: float(np.max(sr.ratios(got[k], ref[k], ref["d_" + k]))) for k in sr.TAIL_KEYS}
    _report("factor_tail", "f64", **w)
    assert max(w.values()) <= 1.0, w
    views = grid_ops.factor_tail(TS[:-1].view(r_ref, r), h[:-1], sq[:-1], Linv[:-1].view(r, r), chol[:-1].view(r, r))          # the wrapper: same launches
    for k, v in zip(sr.TAIL_KEYS, views):
        assert np.array_equal(_np(v).reshape(-1), np.atleast_1d(got[k])), k


# ------------------------------------------------------------------------------------------------ e. woodbury_c and mll_weights
@pytest.mark.parametrize("r", sr.WOODBURY_R)
def test_woodbury_c_and_mll_weights(r):
    from online_gp_amd import _hip

    x = sr.woodbury_inputs(r)
    G, P, zeta, lamk = _t(x["G"]), _t(x["P"]), _t(x["zeta"]), _t(x["lam_kuu"])
    ref = sr.woodbury_c(x["G"], x["lam_kuu"], x["kscale"])
    first = None
    for with_sqG in (True, False):
        C, lam, sq, sqG = _full(r * r + 1), _full(r + 1), _full(r + 1), _full(r * r + 1)
        rc = _hip.lib().wiski_woodbury_c(i32(r), _ptr(G), _ptr(lamk), f64c(x["kscale"]), _ptr(C), _ptr(lam), _ptr(sq), _ptr(sqG) if with_sqG else None, _stream())
        torch.cuda.synchronize()
        assert rc == OK and all(float(b[-1]) == SENT for b in (C, lam, sq, sqG))
        if with_sqG:
            first = (C, lam, sq)
            w = {k: float(sr.ratios(_np(b)[:-1], ref[k].reshape(-1), ref["d_" + k].reshape(-1)).max()) for k, b in (("C", C), ("lam", lam), ("sq", sq), ("sqG", sqG))}
        else:
            assert bool((sqG == SENT).all()) and all(torch.equal(a_, b_) for a_, b_ in zip(first, (C, lam, sq)))
    _report("woodbury_c", "f64", **w)
    assert max(w.values()) <= 1.0, w
    mref = sr.mll_weights(x["G"], x["P"], x["zeta"], x["lam_kuu"], x["g_b"], x["g_ld"])
    Wt, g_kap, g_b, g_ld = _full(r * r + 1), _full(2), _t(x["g_b"]), _t(x["g_ld"])      # (named: a tensor must outlive the pointer taken from it)
    rc = _hip.lib().wiski_mll_weights(i32(r), _ptr(G), _ptr(P), _ptr(zeta), _ptr(lamk), _ptr(g_b), _ptr(g_ld), _ptr(Wt), _ptr(g_kap), _stream())
    torch.cuda.synchronize()
    assert rc == OK and float(Wt[-1]) == SENT and float(g_kap[1]) == SENT
    w = {"Wt": float(sr.ratios(_np(Wt)[:-1], mref["Wt"].reshape(-1), mref["d_Wt"].reshape(-1)).max()),
         "g_kap": float(sr.ratios(_np(g_kap)[0], mref["g_kap"], mref["d_g_kap"]))}
    _report("mll_weights", "f64", **w)
    assert max(w.values()) <= 1.0, w
    for t, v in ((G, x["G"]), (P, x["P"]), (zeta, x["zeta"]), (lamk, x["lam_kuu"])):
        assert np.array_equal(_np(t)[:-1], v.reshape(-1)), "an input was written"


# ----------------------------------------------------------------------------------------------------------------- f. absorb_h
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", sr.ABSORB_CASES, ids=lambda c: f"n{c[0]}_r{c[1]}_pad{c[2]}_{'scaled' if c[3] else 'plain'}")
def test_basis_absorb_h_adds_plainly_and_atomically(case, dtype):
    from online_gp_amd import _hip

    n, r, pad, _ = case
    x = sr.absorb_inputs(*case)
    ref = sr.absorb_h(x["h"], x["F"][:, :r], x["wby"], x["scale"])
    F, wby, h = _t(x["F"]), _t(x["wby"], dtype), _t(x["h"])
    scale = None if x["scale"] is None else _t(x["scale"], dtype)
    assert np.array_equal(_np(wby)[:-1], x["wby"])
    rc = _hip.fn("wiski_basis_absorb_h", dtype)(i64(n), i32(r), _ptr(F), i64(r + pad), _ptr(wby), _ptr(scale), _ptr(h), _stream())
    torch.cuda.synchronize()
    assert rc == OK and float(h[r]) == SENT
    w = float(sr.ratios(_np(h)[:r], ref["h"], ref["d_h"]).max())
    _report("basis_absorb_h", dtype, h=w)
    assert w <= 1.0
    assert np.array_equal(_np(F)[:-1], x["F"].reshape(-1)) and np.array_equal(_np(wby)[:-1], x["wby"])


# ---------------------------------------------------------------------------------------------------------------- g. refusals
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bad_arguments_are_refused_before_any_launch(dtype):
    """Every buffer is large enough for the largest shape a table names, so that even a call let through by mistake stays inside its arrays."""
    from online_gp_amd import _hip

    lib, st = _hip.lib(), _stream()
    N, R = 65, 1025
    big, vec, one = _full(R * R + 1), _full(R * 2 + 1), _full(2)
    realv, s2 = _full(R * 2 + 1, dtype), _t(sr.S2, dtype)
    out = {"ws": _full(201), "out": _full(5), "mean": _full(N + 1, dtype), "var": _full(N + 1, dtype), "a": _full(R * R + 1), "b": _full(R * R + 1),
           "c": _full(6 * R + 3), "d": _full(R + 1), "e": _full(R + 1)}
    refused = {}

    def ev(n=8, r=16, ldl=16, **nulls):
        a = {k: (None if k in nulls else v) for k, v in (("F", big), ("prior", vec), ("Linv", big), ("t", vec), ("s2", s2), ("y", realv), ("ws", out["ws"]),
                                                           ("out", out["out"]))}
        return _hip.fn("wiski_spectral_evaluate", dtype)(i32(n), i32(r), _ptr(a["F"]), _ptr(a["prior"]), _ptr(a["Linv"]), i32(ldl), _ptr(a["t"]), f64c(0.5),
                                                         _ptr(a["s2"]), _ptr(a["y"]), None, _ptr(a["ws"]), _ptr(a["out"]), _ptr(out["mean"]), _ptr(out["var"]), st)

    def evy(n=8, r=16, **nulls):
        a = {k: (None if k in nulls else v) for k, v in (("Y", big), ("F", big), ("prior", vec), ("t", vec), ("s2", s2), ("y", realv), ("ws", out["ws"]),
                                                           ("out", out["out"]))}
        return _hip.fn("wiski_spectral_evaluate_y", dtype)(i32(n), i32(r), _ptr(a["Y"]), _ptr(a["F"]), _ptr(a["prior"]), _ptr(a["t"]), f64c(0.5), _ptr(a["s2"]),
                                                           _ptr(a["y"]), None, _ptr(a["ws"]), _ptr(a["out"]), _ptr(out["mean"]), _ptr(out["var"]), st)

    def pick(names, nulls, bufs):
        return [None if k in nulls else _ptr(b) for k, b in zip(names, bufs)]

    def var(n=8, r=16, **nulls):
        return lib.wiski_spectral_var(i32(n), i32(r), *pick(("Y", "F", "prior"), nulls, (big, big, vec)), f64c(0.5), *pick(("diag", "tail"), nulls, (out["d"], out["e"])), st)

    def tail(r_ref=8, r=16, **nulls):
        return lib.wiski_factor_tail(i32(r_ref), i32(r), *pick(("TS", "href", "sq", "Linv", "chol", "out"), nulls, (big, vec, vec, big, big, out["c"])), st)

    def wood(r=16, **nulls):
        return lib.wiski_woodbury_c(i32(r), *pick(("G", "lam_kuu"), nulls, (big, vec)), f64c(0.5), *pick(("C", "lam", "sq"), nulls, (out["a"], out["d"], out["e"])),
                                    _ptr(out["b"]), st)

    def mll(r=16, **nulls):
        return lib.wiski_mll_weights(i32(r), *pick(("G", "P", "zeta", "lam_kuu", "gb", "gld", "Wt", "gkap"), nulls, (big, big, vec, vec, one, one, out["a"], out["d"])), st)

    def absorb(n=8, r=16, ldf=16, **nulls):
        return _hip.fn("wiski_basis_absorb_h", dtype)(i64(n), i32(r), *pick(("F",), nulls, (big,)), i64(ldf), *pick(("wby", "scale", "h"), nulls, (realv, realv, out["d"])),
                                                      st)

    for name, kw in (("n 0", {"n": 0}), ("n -1", {"n": -1}), ("n 65", {"n": 65}), ("r 0", {"r": 0, "ldl": 16}), ("r 1025", {"r": 1025, "ldl": 1025}),
                     ("ldl r - 1", {"ldl": 15})):
        refused["evaluate: " + name] = ev(**kw)
    for k in ("F", "prior", "Linv", "t", "s2", "y", "ws", "out"):
        refused["evaluate: null " + k] = ev(**{k: 1})
    for name, kw in (("n 0", {"n": 0}), ("n -1", {"n": -1}), ("r 0", {"r": 0})):
        refused["evaluate_y: " + name] = evy(**kw)
    for k in ("Y", "F", "prior", "t", "s2", "y", "ws", "out"):
        refused["evaluate_y: null " + k] = evy(**{k: 1})
    refused.update({"var: n 0": var(n=0), "var: r 0": var(r=0), "tail: r_ref 0": tail(r_ref=0), "tail: r 0": tail(r=0), "woodbury: r 0": wood(r=0),
                    "mll: r 0": mll(r=0), "absorb: r 0": absorb(r=0, ldf=16), "absorb: ldf r - 1": absorb(ldf=15), "absorb: n -1": absorb(n=-1),
                    "absorb: n 2^30 + 1": absorb(n=2 ** 30 + 1)})
    for fn, tag, names in ((var, "var", ("Y", "F", "prior", "diag", "tail")), (tail, "tail", ("TS", "href", "sq", "Linv", "chol", "out")),
                           (wood, "woodbury", ("G", "lam_kuu", "C", "lam", "sq")), (mll, "mll", ("G", "P", "zeta", "lam_kuu", "gb", "gld", "Wt", "gkap")),
                           (absorb, "absorb", ("F", "wby", "h"))):
        for k in names:
            refused[f"{tag}: null {k}"] = fn(**{k: 1})
    empty = absorb(n=0)                                                # nothing to add: fine, and nothing written
    torch.cuda.synchronize()
    wrong = {k: rc for k, rc in refused.items() if rc != BADARG}
    assert not wrong, wrong
    assert empty == OK
    for k, t in out.items():
        assert bool((t == SENT).all()), f"{k} was written by a refused call"


# -------------------------------------------------------------------------------------------------------------- h. model level
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_model_evaluate_is_the_reference_on_the_factor_it_reads(dtype, monkeypatch):
    """evaluate() of a streamed 2-D model on a 16^2 grid, batch sizes 1, 8 and 65 (one launch, one launch, GEMM form) on the model's one reused
    workspace: before each call the factor's own F, prior, chol^-1, t, kscale and the likelihood's s2 are read and fed to the reference, and the
    returned (rmse, nll) held to its bound -- which s2, which targets, chol^-1's leading dimension and the workspace across varying batches."""
    from online_gp_amd.models import Identity, OnlineSKIRegression

    T = NP[dtype]
    rng = np.random.default_rng(21)
    d, g, n0 = 2, 16, 160
    sizes = (4, 4, 1, 8, 65, 8, 1, 65)                                  # (the first two warm the stream up: the PCG state serves the first)
    X = rng.uniform(-1, 1, (n0 + sum(sizes), d))
    y = np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.05 * rng.standard_normal(len(X))
    Xg, yg = torch.as_tensor(X, device=DEV, dtype=dtype), torch.as_tensor(y, device=DEV, dtype=dtype)[:, None]
    reg = OnlineSKIRegression(Identity(d), Xg[:n0], yg[:n0], 5e-3, g, 1.0)
    taken = []
    real = reg._evaluate_from_factor
    monkeypatch.setattr(reg, "_evaluate_from_factor", lambda *a_, **k_: taken.append(real(*a_, **k_)) or taken[-1])
    lo, worst = n0, {"rmse": 0.0, "nll": 0.0}
    for step, q in enumerate(sizes):
        xb, yb = Xg[lo:lo + q], yg[lo:lo + q]
        lo += q
        if step >= 2:
            gp = reg.gp
            reg._ensure_eval()
            fac, st, tcol64 = gp._spectral_state(0)
            assert st is fac.cur
            qy = fac.query(st, xb.reshape(-1, d).contiguous(), tcol64)
            r = qy.Fs.shape[1]
            assert st["Linv"].shape == (r, r) and st["Linv"].is_contiguous()
            s2 = gp.likelihood.second_noise.detach().reshape(-1).to(dtype)
            ref = sr.evaluate_held(T, _np(qy.Fs), _np(qy.prior), _np(st["Linv"]), _np(st["t"]), float(st["kscale"]), float(s2.double()), _np(yb.reshape(-1)))
        rmse, nll = reg.evaluate(xb, yb)
        if step >= 2:
            assert taken[-1] is not None and taken[-1] == (rmse, nll), "evaluate() did not come from the spectral factor"
            _ws_is_zero(torch.cat([fac._eval_ws, _full(1)]))
            w = dict(zip(("rmse", "nll"), (float(v) for v in sr.ratios([rmse, nll], ref["out"][:2], ref["d_out"][:2]))))
            assert max(w.values()) <= 1.0, (step, q, r, w, (rmse, nll), ref["out"])
            worst = {k: max(v, worst[k]) for k, v in w.items()}
        reg.update(xb, yb)
    assert len(taken) == len(sizes)
    _report("model.evaluate", dtype, **worst)
