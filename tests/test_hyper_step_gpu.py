"""GPU: the three kernels of the fused hyper-parameter step (csrc/hyper_step.hip: wiski_hyper_columns, wiski_hyper_mid,
wiski_hyper_adam; both the _f32 and the _f64 entry points) against the plain fp64 reference of tests/hyper_step_reference.py, on plans
built by hand over small device tensors: the constraint edges (softplus threshold, fp32 overflow of exp, saturated sigmoids), columns
with g > 256 and unequal h, the MLL tail at n = 1 .. 21743 and s2 = 1e-4 .. 7, single Adam steps from the zero state (bias corrections
of step 1, gradients of 1e-7 where the placement of eps decides the update), warm states, per-element step counters, a five-step
trajectory, and the argument checks.  Every kernel input is fp32-representable, so the fp64 reference and an fp32 kernel start from
the same numbers.

Bounds: hyper_step_reference's docstring -- K eps max(|ref|, S) with K eps = 64 eps64 / 8 eps32 and S the largest operand, none taken
from a kernel run; tests/test_hyper_step_host.py shows that the reference's own fp32 emulation uses at most a quarter of the fp32
bound and that eleven seeded defects each exceed it at least four times at some case.  wiski_hyper_mid works in fp64 on the
(fp32-representable) sigma2 in both instantiations and is held to the fp64 bound in both.  In the trajectory the state a step starts
from carries the error of the steps before it, so step t is held to t times the bound, in both dtypes.

Worst ratio to the bound per kernel on an MI355X: DESIGN.md 3.18."""
import ctypes

import numpy as np
import pytest
import torch

import hyper_step_reference as hr

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float64]
DT_IDS = ["f32", "f64"]
NP = {torch.float32: hr.F32, torch.float64: hr.F64}
F64 = hr.F64
SENT = -777.25
BADARG = -1
CASE_ID = lambda c: c["name"]        # noqa: E731


class _Grid:
    """A wiski_grid filled in by hand (grid_ops.GridSpec builds interpolation grids, g >= 4; the columns kernel needs d, g and h only)."""

    def __init__(self, g, h):
        from online_gp_amd import _hip

        c = _hip.wiski_grid()
        c.d = len(g)
        for q in range(len(g)):
            c.g[q], c.g0[q], c.h[q] = int(g[q]), 0.0, float(h[q])
        self.c = c

    @property
    def ref(self):
        return ctypes.byref(self.c)


def _t(x, dtype, pad=0):
    """A device tensor of x with `pad` sentinel slots behind it."""
    x = np.atleast_1d(np.asarray(x, F64))
    return torch.tensor(np.concatenate([x, np.full(pad, SENT)]), dtype=dtype, device=DEV)


def _full(n, dtype):
    return torch.full((n,), SENT, dtype=dtype, device=DEV)


def _alloc(records, dtype):
    """raw, m, v (dtype) and step (fp32) of every record, each with one sentinel slot behind its last element."""
    return [{"raw": _t(r["raw"], dtype, 1), "m": _t(r["m"], dtype, 1), "v": _t(r["v"], dtype, 1), "step": _t(r["step"], torch.float32, 1)} for r in records]


def _plan(records, keep):
    from online_gp_amd import _hip

    plan = _hip.wiski_hyper_plan()
    plan.count = len(records)
    for e, r, t in zip(plan.p, records, keep):
        e.raw, e.exp_avg, e.exp_avg_sq, e.step = t["raw"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["step"].data_ptr()
        e.numel, e.step_numel, e.role, e.kind, e.lower, e.upper = r["raw"].size, r["step_numel"], r["role"], r["kind"], r["lower"], r["upper"]
    return plan


def _np(t):
    return t.detach().cpu().double().numpy()


def _state(records, keep):
    """The device state in adam_step's layout, after checking that the sentinel behind every array is still there."""
    out = []
    for r, t in zip(records, keep):
        n, ns = r["raw"].size, r["step_numel"]
        for k, cnt in (("raw", n), ("m", n), ("v", n), ("step", ns)):
            assert float(t[k][cnt]) == SENT, f"{k}: the slot behind the last element was written"
        out.append({"raw": _np(t["raw"])[:n], "m": _np(t["m"])[:n], "v": _np(t["v"])[:n], "step": _np(t["step"])[:ns]})
    return out


def _report(kernel, dtype, **ratios):
    print(f"ratio-to-bound {kernel} {DT_IDS[DTYPES.index(dtype)]} " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


# ------------------------------------------------------------------------------------------------------ a. transforms and columns
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", hr.COLUMN_CASES, ids=CASE_ID)
def test_hyper_columns_values_and_columns(case, dtype):
    from online_gp_amd import grid_ops

    T = NP[dtype]
    recs = case["records"]
    keep = _alloc(recs, dtype)
    plan = _plan(recs, keep)
    grid = _Grid(case["g"], case["h"])
    ng = sum(case["g"])
    nell = next(r["raw"].size for r in recs if r["role"] == 0)
    has_scale = any(r["role"] == 1 for r in recs)
    lower = {r["role"]: abs(r["lower"]) for r in recs}
    ell_ref, scale_ref, s2_ref = hr.constrained(recs, F64)
    ell_T, _, s2_T = hr.constrained(recs, T)
    sc_ref = 1.0 if scale_ref is None else float(scale_ref)
    worst = {"value": 0.0, "column": 0.0, "column_of_own_values": 0.0}
    first = None
    for kind in hr.KINDS:
        ell, s2, s2_64 = _full(nell + 2, dtype), _full(2, dtype), _full(2, torch.float64)
        scale = _full(2, dtype) if has_scale else None                 # no scale factor: NULL, nothing to write through
        tc64, tc = _full(ng + 3, torch.float64), _full(ng + 3, dtype)
        grid_ops.hyper_columns(plan, grid, kind, ell, scale, s2, s2_64, tc64, tc)
        torch.cuda.synchronize()
        for buf, n in ((ell, nell), (s2, 1), (s2_64, 1), (tc64, ng), (tc, ng)) + (((scale, 1),) if has_scale else ()):
            assert bool((buf[n:] == SENT).all()), "a slot beyond the output was written"
        e_got, s2_got = _np(ell)[:nell], _np(s2)[:1]
        worst["value"] = max(worst["value"], float(hr.ratios(e_got, ell_ref, lower[0], T).max()), float(hr.ratios(s2_got, s2_ref, lower[2], T).max()))
        if has_scale:
            worst["value"] = max(worst["value"], float(hr.ratios(_np(scale)[:1], scale_ref, 0.0, T).max()))
        for r, got, emu in [(r, e_got, ell_T) for r in recs if r["role"] == 0] + [(r, s2_got, np.atleast_1d(s2_T)) for r in recs if r["role"] == 2]:
            sat = hr.saturated(r["kind"], r["raw"])                    # exactly saturated in fp64: constants only, equal bit for bit
            assert np.array_equal(got[sat], emu.astype(F64)[sat])
        assert torch.equal(s2_64[:1], s2[:1].double())
        assert torch.equal(tc[:ng], tc64[:ng].to(dtype))
        col = _np(tc64)[:ng]
        worst["column"] = max(worst["column"], float(hr.ratios(col, hr.columns(kind, case["g"], case["h"], ell_ref, sc_ref), sc_ref, T).max()))
        # whatever the dtype of the values, the columns are fp64 functions of them: held to the fp64 bound against the kernel's own ell, scale
        sc_got = float(_np(scale)[0]) if has_scale else 1.0
        worst["column_of_own_values"] = max(worst["column_of_own_values"],
                                            float(hr.ratios(col, hr.columns(kind, case["g"], case["h"], e_got, sc_got), sc_got, F64).max()))
        if first is None:
            first = (ell, scale, s2)
    # without columns the three values are still written (and are the same bits)
    ell, s2, scale = _full(nell + 2, dtype), _full(2, dtype), (_full(2, dtype) if has_scale else None)
    grid_ops.hyper_columns(plan, grid, 0, ell, scale, s2)
    torch.cuda.synchronize()
    assert torch.equal(ell, first[0]) and torch.equal(s2, first[2]) and (not has_scale or torch.equal(scale, first[1]))
    for r, t in zip(recs, keep):                                       # the plan's own tensors are read only
        assert np.array_equal(_np(t["raw"])[:-1], r["raw"]) and float(t["raw"][-1]) == SENT and np.array_equal(_np(t["step"])[:-1], r["step"])
    _report("hyper_columns", dtype, **worst)
    assert worst["value"] <= 1.0 and worst["column"] <= 1.0 and worst["column_of_own_values"] <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------- b. mid
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_hyper_mid_slots_and_mll_value_bits(dtype):
    from online_gp_amd import grid_ops

    x = hr.MID_INPUTS
    bMb, c, ld, logdet = (_t(x[k], torch.float64) for k in ("bMb", "c", "ld", "logdet"))
    worst = 0.0
    for with_logdet in (False, True):
        for n in hr.MID_N:
            for s2 in hr.MID_S2:
                s2t, n_dev = _t(s2, dtype), _t(n, torch.float64)
                assert float(s2t.double()) == s2
                out, loss = _full(11, torch.float64), _full(2, torch.float64)
                grid_ops.hyper_mid(bMb, logdet if with_logdet else None, s2t, c, ld, n_dev, out, loss)
                val, coef = grid_ops.mll_value(bMb, logdet if with_logdet else None, s2t, c, ld, n_dev)
                torch.cuda.synchronize()
                ref, S = hr.mid(x["bMb"], x["logdet"] if with_logdet else None, s2, x["c"], x["ld"], n)
                got = _np(out)
                assert got[9] == SENT and got[10] == SENT and float(loss[1]) == SENT
                worst = max(worst, float(hr.ratios(got[:9], ref, S, F64).max()))
                assert float(loss[0]) == got[7]
                # wiski_mll_value promises the same arithmetic: the same bits
                assert float(val) == got[0] and np.array_equal(_np(coef), got[1:4]), (with_logdet, n, s2)
    out = _full(9, torch.float64)
    grid_ops.hyper_mid(bMb, None, _t(hr.MID_S2[1], dtype), c, ld, _t(600.0, torch.float64), out)          # (no loss output)
    assert float(out[7]) == -float(out[0]) / 600.0
    _report("hyper_mid", dtype, slots=worst)
    assert worst <= 1.0


# --------------------------------------------------------------------------------------------------------------------- c. Adam
def _adam_inputs(case, dtype):
    return {"scale": _t(case["scale"], dtype), "s2": _t(case["s2"], dtype), "g_ell": _t(case["g_ell"], dtype), "g_scale": _t(case["g_scale"], dtype),
            "mid": _t(case["mid"], torch.float64), "g_kap": _t(case["g_kap"], torch.float64), "n": _t(case["n"], torch.float64)}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", hr.ADAM_CASES, ids=CASE_ID)
def test_hyper_adam_single_step(case, dtype):
    from online_gp_amd import grid_ops

    T = NP[dtype]
    recs = case["records"]
    keep = _alloc(recs, dtype)
    plan = _plan(recs, keep)
    inp = _adam_inputs(case, dtype)
    for k in ("scale", "s2", "g_ell", "g_scale"):
        assert np.array_equal(_np(inp[k]), np.atleast_1d(case[k])), "inputs are fp32-representable"
    before = {k: v.clone() for k, v in inp.items()}
    grid_ops.hyper_adam(plan, inp["scale"], inp["s2"], inp["g_ell"], inp["g_scale"], inp["mid"], inp["g_kap"], inp["n"], case["lr"], case["b1"], case["b2"],
                        case["eps"])
    torch.cuda.synchronize()
    ref = hr.adam_step(recs, case["scale"], case["s2"], case["g_ell"], case["g_scale"], case["mid"], case["g_kap"], case["n"], case["lr"], case["b1"],
                       case["b2"], case["eps"], T=F64)
    got = _state(recs, keep)
    for r, g_ in zip(recs, got):                                       # every counter up by exactly one, once
        assert g_["step"].size == r["step_numel"] and np.array_equal(g_["step"], r["step"].astype(F64) + 1.0)
    for k, v in inp.items():
        assert torch.equal(v, before[k]), f"{k} was written"
    w = hr.step_ratios(got, ref, T)
    _report("hyper_adam", dtype, **w)
    assert max(w.values()) <= 1.0, w


# --------------------------------------------------------------------------------------------------------------- d. trajectory
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_five_step_trajectory_carries_state_and_counters(dtype):
    from online_gp_amd import grid_ops

    T = NP[dtype]
    lr, b1, b2, eps = 0.05, 0.9, 0.999, 1e-8
    ref = hr.trajectory_reference(F64, lr, b1, b2, eps)
    recs = hr._adam_plan()
    keep = _alloc(recs, dtype)
    plan = _plan(recs, keep)
    grid = _Grid((5, 6, 7), (0.25, 0.5, 0.125))
    ell, scale, s2, mid = _full(3, dtype), _full(1, dtype), _full(1, dtype), _full(9, torch.float64)
    worst = 0.0
    for t in range(hr.TRAJECTORY_STEPS):
        x = hr.trajectory_inputs(t)
        n_dev = _t(x["n"], torch.float64)
        grid_ops.hyper_columns(plan, grid, 0, ell, scale, s2)
        grid_ops.hyper_mid(_t(x["bMb"], torch.float64), None, s2, _t(x["c"], torch.float64), _t(x["ld"], torch.float64), n_dev, mid)
        grid_ops.hyper_adam(plan, scale, s2, _t(x["g_ell"], dtype), _t(x["g_scale"], dtype), mid, _t(x["g_kap"], torch.float64), n_dev, lr, b1, b2, eps)
        torch.cuda.synchronize()
        got = _state(recs, keep)
        for g_ in got:
            assert np.array_equal(g_["step"], np.full(1, t + 1.0))
        w = hr.step_ratios(got, ref[t], T)
        worst = max(worst, max(w.values()) / (t + 1))
        assert max(w.values()) <= t + 1, (t, w)
    _report("trajectory", dtype, per_step=worst)


# ----------------------------------------------------------------------------------------------------------------- e. refusals
def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bad_arguments_are_refused_before_any_launch(dtype):
    from online_gp_amd import _hip

    base = hr._adam_plan()                                             # [scale, scale, lengthscale (3), noise]
    keep = _alloc(base, dtype)
    grid = _Grid((5, 6, 7), (0.25, 0.5, 0.125))
    out = {"ell": _full(4, dtype), "scale": _full(2, dtype), "s2": _full(2, dtype), "s2_64": _full(2, torch.float64), "tc64": _full(20, torch.float64),
           "tc": _full(20, dtype), "mid": _full(9, torch.float64), "loss": _full(1, torch.float64)}
    inp = _adam_inputs(hr.ADAM_CASES[0], dtype)
    stream = _hip.stream_ptr(out["ell"].device)

    def columns(plan, g=grid, kind=0, **nulls):
        a = {k: (None if k in nulls else out[k]) for k in ("ell", "scale", "s2", "s2_64", "tc64", "tc")}
        return _hip.fn("wiski_hyper_columns", dtype)(ctypes.byref(plan), g.ref, ctypes.c_int32(kind), _ptr(a["ell"]), _ptr(a["scale"]), _ptr(a["s2"]),
                                                     _ptr(a["s2_64"]), _ptr(a["tc64"]), _ptr(a["tc"]), stream)

    def adam(plan, **nulls):
        a = {k: (None if k in nulls else inp[k]) for k in inp}
        return _hip.fn("wiski_hyper_adam", dtype)(ctypes.byref(plan), _ptr(a["scale"]), _ptr(a["s2"]), _ptr(a["g_ell"]), _ptr(a["g_scale"]), _ptr(a["mid"]),
                                                  _ptr(a["g_kap"]), _ptr(a["n"]), ctypes.c_double(0.01), ctypes.c_double(0.9), ctypes.c_double(0.999),
                                                  ctypes.c_double(1e-8), stream)

    def plan_of(idx, **fields):
        """The plan over entries idx of the base plan, with `fields` (name -> (entry, value)) overwritten."""
        plan = _plan([base[i] for i in idx], [keep[i] for i in idx])
        for name, (i, value) in fields.items():
            setattr(plan.p[i], name, value)
        return plan

    def count(c):
        plan = plan_of([0, 1, 2, 3])
        plan.count = c
        return plan

    SA, SB, ELL, NOISE = 0, 1, 2, 3
    both = {
        "count 0": count(0), "count 7": count(7),
        "no lengthscale": plan_of([SA, SB, NOISE]), "two lengthscales": plan_of([SA, ELL, ELL, NOISE]),
        "no noise": plan_of([SA, SB, ELL]), "two noises": plan_of([SA, NOISE, ELL, NOISE]),
        "role-1 numel 2": plan_of([SA, SB, ELL, NOISE], numel=(SA, 2)),
        "role 3": plan_of([SA, SB, ELL, NOISE], role=(SB, 3)), "kind 2": plan_of([SA, SB, ELL, NOISE], kind=(NOISE, 2)),
        "null raw": plan_of([SA, SB, ELL, NOISE], raw=(ELL, None)),
    }
    good = plan_of([SA, SB, ELL, NOISE])
    refused = {}
    for name, plan in both.items():
        refused["columns: " + name] = columns(plan)
        refused["adam: " + name] = adam(plan)
    # the columns call knows the grid: a lengthscale of 2 elements on a 3-dim grid (the Adam call cannot know, and takes any numel)
    refused["columns: lengthscale numel 2, d 3"] = columns(plan_of([SA, SB, ELL, NOISE], numel=(ELL, 2), step_numel=(ELL, 1)))
    refused["columns: null d_ell"] = columns(good, ell=1)
    refused["columns: null d_s2"] = columns(good, s2=1)
    refused["columns: kind 4"] = columns(good, kind=4)
    refused["columns: kind -1"] = columns(good, kind=-1)
    refused["columns: h = 0"] = columns(good, g=_Grid((5, 6, 7), (0.25, 0.0, 0.125)))
    refused["columns: g = 0"] = columns(good, g=_Grid((5, 0, 7), (0.25, 0.5, 0.125)))
    refused["adam: null exp_avg"] = adam(plan_of([SA, SB, ELL, NOISE], exp_avg=(SB, None)))
    refused["adam: null exp_avg_sq"] = adam(plan_of([SA, SB, ELL, NOISE], exp_avg_sq=(ELL, None)))
    refused["adam: null step"] = adam(plan_of([SA, SB, ELL, NOISE], step=(NOISE, None)))
    refused["adam: step_numel 2 of numel 3"] = adam(plan_of([SA, SB, ELL, NOISE], step_numel=(ELL, 2)))
    refused["adam: step_numel 0"] = adam(plan_of([SA, SB, ELL, NOISE], step_numel=(SA, 0)))
    refused["adam: role 1 without d_scale"] = adam(good, scale=1)
    refused["adam: role 1 without d_gscale"] = adam(good, g_scale=1)
    refused["adam: null d_s2"] = adam(good, s2=1)
    refused["adam: null d_gell"] = adam(good, g_ell=1)
    refused["adam: null d_mid"] = adam(good, mid=1)
    refused["adam: null d_gkap"] = adam(good, g_kap=1)
    refused["adam: null d_n"] = adam(good, n=1)
    one = _t(1.0, torch.float64)
    refused["mid: null d_out"] = _hip.fn("wiski_hyper_mid", dtype)(_ptr(one), None, _ptr(inp["s2"]), _ptr(one), _ptr(one), _ptr(inp["n"]), None, _ptr(out["loss"]),
                                                                   stream)
    refused["mid: null d_s2"] = _hip.fn("wiski_hyper_mid", dtype)(_ptr(one), None, None, _ptr(one), _ptr(one), _ptr(inp["n"]), _ptr(out["mid"]), _ptr(out["loss"]),
                                                                  stream)
    torch.cuda.synchronize()
    wrong = {k: rc for k, rc in refused.items() if rc != BADARG}
    assert not wrong, wrong
    for k, t in out.items():
        assert bool((t == SENT).all()), f"{k} was written by a refused call"
    for r, t in zip(base, keep):
        for k in ("raw", "m", "v", "step"):
            assert np.array_equal(_np(t[k])[:-1], np.asarray(r[k], F64)) and float(t[k][-1]) == SENT, f"{k} was changed by a refused call"
