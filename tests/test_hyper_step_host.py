"""Host: checks of the reference of the fused hyper-parameter step (tests/hyper_step_reference.py) that tests/test_hyper_step_gpu.py
holds wiski_hyper_columns / wiski_hyper_mid / wiski_hyper_adam to, and of the case tables both files share.  No GPU:
  - the fp64 reference against torch (F.softplus, torch.sigmoid, autograd through a product of two scales and through the MLL tail,
    torch.optim.Adam) over six steps;
  - at every case of the tables, the reference's own fp32 emulation stays within a quarter of the fp32 bound: the bound is not tight
    for a correct fp32 implementation in the kernel's operation order;
  - every wrong variant in MUTANTS moves some output of some case by at least four times the fp32 bound: the bound is not loose, and
    the table reaches the places where those defects show."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hyper_step_reference as hr

F64, F32 = hr.F64, hr.F32


def test_reference_matches_torch_softplus_sigmoid_autograd_and_adam():
    rng = np.random.default_rng(0)
    recs = hr._adam_plan(ell_raw=(0.3, -1.2, 21.5), sa_raw=0.7, sb_raw=-0.4, noise_raw=-2.0)
    lr, b1, b2, eps = 0.03, 0.9, 0.999, 1e-8
    tp = [torch.tensor(r["raw"], dtype=torch.float64, requires_grad=True) for r in recs]
    opt = torch.optim.Adam(tp, lr=lr, betas=(b1, b2), eps=eps, foreach=False)

    def value(r, p):
        if r["kind"] == 0:
            return r["lower"] + F.softplus(p)
        return r["lower"] + (r["upper"] - r["lower"]) * torch.sigmoid(p)

    worst = 0.0
    for t in range(6):
        a = rng.uniform(-2, 2, 3)
        b, g_kap = rng.uniform(-1, 1), rng.uniform(-0.5, 0.5)
        bMb, c, ld, n = rng.uniform(300, 400), rng.uniform(400, 500), rng.uniform(-50, 50), 600.0 + 32 * t
        # torch: loss = sum a_e ell_e + b scale + L(s2), L the MLL tail -val / n plus g_kap / s2
        opt.zero_grad()
        sa, sb, ell, s2 = (value(r, p) for r, p in zip(recs, tp))
        val = -0.5 * ((c - bMb) / s2 + ld + n * (hr.LOG_2PI + torch.log(s2)))
        loss = (torch.as_tensor(a) * ell).sum() + b * (sa * sb).sum() + (-val / n + g_kap / s2).sum()
        loss.backward()
        opt.step()
        # reference
        ell_r, scale_r, s2_r = hr.constrained(recs)
        assert np.array_equal(ell_r, ell.detach().numpy()) or np.abs(ell_r - ell.detach().numpy()).max() <= 1e-15 * np.abs(ell_r).max()
        m9, _ = hr.mid(bMb, None, s2_r, c, ld, n)
        assert abs(m9[0] - float(val.detach())) <= 1e-14 * abs(m9[0])
        new = hr.adam_step(recs, scale_r, s2_r, a, b, m9, g_kap, n, lr, b1, b2, eps)
        recs = [dict(r, raw=u["raw"], m=u["m"], v=u["v"], step=u["step"]) for r, u in zip(recs, new)]
        for r, p in zip(recs, tp):
            st = opt.state[p]
            assert float(st["step"]) == float(r["step"][0]) == t + 1
            for got, want in ((r["raw"], p.detach().numpy()), (r["m"], st["exp_avg"].numpy()), (r["v"], st["exp_avg_sq"].numpy())):
                rel = np.abs(got - want) / np.abs(want)
                worst = max(worst, float(rel.max()))
    print(f"reference vs torch.optim.Adam, 6 steps: worst relative difference {worst:.2e}")
    assert worst <= 1e-14


def test_sigma2_gradient_is_the_derivative_of_the_tail():
    """The hand derivative against a central difference of L(s2) = -val(s2) / n + g_kap / s2 in fp64 (relative step 1e-5: error ~1e-10)."""
    for s2 in hr.MID_S2:
        for n in hr.MID_N:
            A, g_kap = 18.375, -0.21

            def L(x):
                return -hr.mid(0.0, -3.0, x, A, 11.0, n)[0][0] / n + g_kap / x

            h = 1e-5 * s2
            fd = (L(s2 + h) - L(s2 - h)) / (2 * h)
            an = hr.sigma2_grad(A, s2, g_kap, n)
            assert abs(fd - an) <= 1e-7 * abs(an), (s2, n, fd, an)


def _emul_vs_ref(case):
    args = (case["records"], case["scale"], case["s2"], case["g_ell"], case["g_scale"], case["mid"], case["g_kap"], case["n"], case["lr"], case["b1"],
            case["b2"], case["eps"])
    return hr.adam_step(*args, T=F32), hr.adam_step(*args, T=F64), args


@pytest.mark.parametrize("case", hr.ADAM_CASES, ids=lambda c: c["name"])
def test_fp32_emulation_of_an_adam_step_stays_within_a_quarter_of_the_fp32_bound(case):
    emul, ref, _ = _emul_vs_ref(case)
    w = hr.step_ratios(emul, ref, F32)
    print(f"{case['name']}: fp32 emulation / fp32 bound  raw {w['raw']:.3f}  m {w['m']:.3f}  v {w['v']:.3f}")
    assert max(w.values()) <= 0.25, w


@pytest.mark.parametrize("case", hr.COLUMN_CASES, ids=lambda c: c["name"])
def test_fp32_emulation_of_transforms_and_columns_stays_within_a_quarter_of_the_fp32_bound(case):
    e32, s32, n32 = hr.constrained(case["records"], F32)
    e64, s64, n64 = hr.constrained(case["records"], F64)
    lo = {r["role"]: abs(r["lower"]) for r in case["records"]}
    worst = max(float(hr.ratios(e32, e64, lo[0], F32).max()), float(hr.ratios(n32, n64, lo[2], F32).max()))
    if s64 is not None:
        worst = max(worst, float(hr.ratios(s32, s64, 0.0, F32).max()))
    for kind in hr.KINDS:
        c32 = hr.columns(kind, case["g"], case["h"], e32, 1.0 if s32 is None else s32)
        c64 = hr.columns(kind, case["g"], case["h"], e64, 1.0 if s64 is None else s64)
        worst = max(worst, float(hr.ratios(c32, c64, 1.0 if s64 is None else float(s64), F32).max()))      # (|column| <= scale: absolute)
    for r in case["records"]:                        # exact saturation: the emulation in each dtype is lower (+ range), without a library call
        sat = hr.saturated(r["kind"], r["raw"])
        if sat.any():
            for T in (F32, F64):
                v = hr.transform(r["kind"], r["lower"], r["upper"], r["raw"], T)[sat]
                ends = (T(r["lower"]), T(r["lower"]) + T(r["upper"] - r["lower"]))
                assert all(x in ends for x in v)
    print(f"{case['name']}: fp32 emulation / fp32 bound {worst:.3f}")
    assert worst <= 0.25


def test_fp32_emulation_of_the_trajectory_stays_within_a_quarter_of_the_scaled_bound():
    emul, ref = hr.trajectory_reference(F32), hr.trajectory_reference(F64)
    for t, (a, b) in enumerate(zip(emul, ref)):
        w = hr.step_ratios(a, b, F32)
        print(f"trajectory step {t + 1}: fp32 emulation / fp32 bound  raw {w['raw']:.3f}  m {w['m']:.3f}  v {w['v']:.3f}")
        assert max(w.values()) <= 0.25 * (t + 1), (t, w)


@pytest.mark.parametrize("name", list(hr.MUTANTS))
def test_every_mutant_is_separated_by_some_case_of_the_table(name):
    """In the fp64 reference or in its fp32 emulation (softplus_without_threshold is wrong only where fp32 exp overflows), against the
    same arithmetic without the defect; the distance in units of the fp32 bound."""
    best, where = 0.0, None
    for case in hr.ADAM_CASES:
        _, _, args = _emul_vs_ref(case)
        for T in (F64, F32):
            good = hr.adam_step(*args, T=T)
            bad = hr.MUTANTS[name](*args, T=T)
            ref = hr.adam_step(*args, T=F64)
            for g_, b_, r_ in zip(good, bad, ref):
                for k in ("raw", "m", "v"):
                    d = float(np.max(hr.ratios(b_[k], g_[k], r_["S_" + k], F32)))
                    if d > best:
                        best, where = d, (case["name"], T.__name__, k)
    print(f"{name}: {best:.3g} x the fp32 bound at {where}")
    assert best >= 4.0, (name, best, where)


def test_case_tables_hold_what_the_gpu_test_relies_on():
    soft = sorted(float(x) for c in hr.COLUMN_CASES for r in c["records"] if r["kind"] == 0 for x in r["raw"])
    sig = sorted(float(x) for c in hr.COLUMN_CASES for r in c["records"] if r["kind"] == 1 for x in r["raw"])
    assert set(float(x) for x in hr.f32r(hr.SOFTPLUS_RAWS)) <= set(soft) and set(hr.INTERVAL_RAWS) <= set(sig)
    assert float(hr.f32r(19.999)) < 20.0 < float(hr.f32r(20.001))
    assert sorted(sum(1 for r in c["records"] if r["role"] == 1) for c in hr.COLUMN_CASES) == [0, 1, 2, 2, 3]
    assert {c["g"] for c in hr.COLUMN_CASES} == {(300,), (257, 3), (5, 7, 64, 9)}
    assert any(len(c["g"]) == 4 and next(r for r in c["records"] if r["role"] == 0)["raw"].size == 1 for c in hr.COLUMN_CASES)
    for c in hr.COLUMN_CASES + hr.ADAM_CASES:
        assert 2 <= len(c["records"]) <= 5            # (2: a lengthscale and a noise, no scale factor)
        for r in c["records"]:
            for k in ("raw", "m", "v"):
                assert np.array_equal(r[k], hr.f32r(r[k]))
    for c in hr.ADAM_CASES:
        assert all(float(x) == float(F32(x)) for x in (c["scale"], c["s2"], c["g_scale"])) and np.array_equal(c["g_ell"], hr.f32r(c["g_ell"]))
