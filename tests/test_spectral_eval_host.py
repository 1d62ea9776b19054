"""Host (no GPU): the reference of tests/spectral_eval_reference.py against independent forms (a triangular solve on the Cholesky factor of a
random SPD matrix, mpmath for the metrics, numpy.linalg.solve for the factor tail), its plain-double and fp32 evaluations against its own
bounds at every case of the tables the GPU test runs, and the seeded defects: each must exceed the bound at least four times at the case the
tables name for it -- a table that did not tell a defect from the reference would not tell a kernel with that defect from a correct one."""
import numpy as np
import pytest

import spectral_eval_reference as sr

F64, F32, LD = sr.F64, sr.F32, sr.LD
ALL_EVAL = sr.EVAL_CASES + sr.EVAL_Y_CASES + sr.DISPATCH_CASES + [c for _, c in sr.SEQUENCE]
EVAL_KEYS = ("out", "mean", "var")


def _spd(r, seed):
    rng = np.random.default_rng(seed)
    R = rng.standard_normal((r, r))
    C = R @ R.T / r + np.eye(r)
    L = np.linalg.cholesky(C)
    return rng, C, L, np.linalg.inv(L)


def _worst(got, ref, keys):
    return {k: float(np.max(sr.ratios(got[k], ref[k], ref["d_" + k]))) for k in keys}


# ------------------------------------------------------------------------------------------------- a. against independent forms
def test_dg_is_the_quadratic_form_of_the_inverse_of_an_spd_matrix():
    """With Linv the inverse of the Cholesky factor of C:  dg_j = F_j^T C^-1 F_j  (numpy.linalg.solve on C itself, no triangle anywhere)."""
    for r, n in ((5, 3), (40, 9), (130, 17)):
        rng, C, _, Linv = _spd(r, r)
        F = rng.standard_normal((n, r))
        ref = sr.evaluate(F, np.zeros(n), Linv, np.zeros(r), 1.0, 0.3, np.zeros(n))
        quad = np.einsum("jk,kj->j", F, np.linalg.solve(C, F.T))
        assert np.abs(ref["dg"] - quad).max() <= 1e-11 * np.abs(quad).max()


def test_metrics_against_mpmath():
    import mpmath as mp

    mp.mp.dps = 40
    rng, _, _, Linv = _spd(7, 1)
    n, r = 5, 7
    F, t, y, prior, s2, ksc = rng.standard_normal((n, r)), rng.standard_normal(r), rng.standard_normal(n), rng.uniform(5, 25, n), 0.37, 0.8
    ref = sr.evaluate(F, prior, Linv, t, ksc, s2, y, err=3)
    sq_sum, nll_sum, mx = mp.mpf(0), mp.mpf(0), mp.mpf(0)
    for j in range(n):
        fj = [mp.mpf(float(x)) for x in F[j]]
        mean = sum(f * mp.mpf(float(tk)) for f, tk in zip(fj, t))
        dg = sum(sum(mp.mpf(float(Linv[i, k])) * fj[k] for k in range(i + 1)) ** 2 for i in range(r))
        tail = max(mp.mpf(float(prior[j])) * mp.mpf(ksc) - sum(f * f for f in fj), mp.mpf(0))
        var = max((dg + tail) * mp.mpf(s2), mp.mpf(0))
        v = var + mp.mpf(s2)
        s = (mean - mp.mpf(float(y[j]))) ** 2
        sq_sum += s
        nll_sum += (s / v + mp.log(v) + mp.log(2 * mp.pi)) / 2
        mx = max(mx, abs(mean))
        assert abs(float(mean) - ref["mean"][j]) <= 1e-15 * max(1.0, abs(float(mean))) and abs(float(var) - ref["var"][j]) <= 1e-15 * float(var)
    want = [float(mp.sqrt(sq_sum / n)), float(nll_sum / n), 3.0, float(mx)]
    assert np.abs(ref["out"] - want).max() <= 1e-15 * np.abs(want).max()
    assert (ref["d_out"][[0, 1, 3]] > 0).all() and (ref["d_out"][[0, 1, 3]] < 1e-12).all() and ref["d_out"][2] == 0.0


def test_factor_tail_against_a_dense_solve():
    """t = C^-1 (sq o hr),  bMb = (sq o hr)^T C^-1 (sq o hr),  logdet = log det C  with numpy.linalg on C itself."""
    for r, r_ref in ((6, 9), (50, 31), (129, 200)):
        rng, C, L, Linv = _spd(r, 10 + r)
        TS, h_ref, sq = rng.standard_normal((r_ref, r)), rng.standard_normal(r_ref), rng.uniform(0.5, 2.0, r)
        ref = sr.factor_tail(TS, h_ref, sq, Linv, L)
        hr = TS.T @ h_ref
        t = np.linalg.solve(C, sq * hr)
        for key, want in (("hr", hr), ("t", t), ("coef", sq * t), ("zeta", t / sq), ("bMb", (sq * hr) @ t), ("logdet", np.linalg.slogdet(C)[1]),
                          ("c", np.linalg.solve(L, sq * hr))):
            assert np.abs(ref[key] - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), key


def test_small_operations_against_plain_numpy():
    rng = np.random.default_rng(4)
    x = sr.woodbury_inputs(17)
    w = sr.woodbury_c(x["G"], x["lam_kuu"], x["kscale"])
    lam = x["lam_kuu"] * x["kscale"]
    assert np.allclose(w["C"], np.sqrt(lam)[:, None] * x["G"] * np.sqrt(lam)[None, :] + np.eye(17), rtol=1e-14, atol=0)
    m = sr.mll_weights(x["G"], x["P"], x["zeta"], x["lam_kuu"], x["g_b"], x["g_ld"])
    Wt = x["g_ld"] * (x["G"] - x["P"]) + x["g_b"] * np.outer(x["zeta"], x["zeta"])
    assert np.allclose(m["Wt"], Wt, rtol=1e-13, atol=1e-15) and abs(m["g_kap"] - np.diagonal(Wt) @ x["lam_kuu"]) <= 1e-13
    F, wby, sc, h = rng.standard_normal((9, 4)), rng.standard_normal(9), rng.uniform(1, 2, 9), rng.standard_normal(4)
    assert np.allclose(sr.absorb_h(h, F, wby, sc)["h"], h + F.T @ (wby / sc), rtol=1e-14)
    assert np.allclose(sr.absorb_h(h, F, wby, None)["h"], h + F.T @ wby, rtol=1e-14)
    Y = rng.standard_normal((4, 9))
    v = sr.spectral_var(Y, F, np.full(9, 3.0), 1.5)
    assert np.allclose(v["diag"], (Y * Y).sum(0), rtol=1e-14) and np.allclose(v["tail"], np.maximum(4.5 - (F * F).sum(1), 0), rtol=1e-13, atol=1e-15)


# ---------------------------------------------------------------------------------------------------- b. the tables themselves
def test_case_tables_cover_the_edges_the_inputs_promise():
    for c in sr.EVAL_CASES:
        x = sr.case_inputs(c["name"])
        n, r = c["n"], c["r"]
        assert np.array_equal(x["F"], sr.f32r(x["F"])) and np.array_equal(x["Linv"], sr.f32r(x["Linv"])) and np.array_equal(x["y"], sr.f32r(x["y"]))
        if not c["kw"].get("upper"):
            assert not np.triu(x["Linv"][:, :r], 1).any()
        assert (np.diagonal(x["Linv"][:, :r]) > 0).all()
        ref = sr.case_reference(c["name"])
        if n >= 7:
            pre = x["prior"] * x["kscale"] - (x["F"] * x["F"]).sum(1)
            assert (pre < 0).sum() >= n // 4 and (pre > 0).sum() >= n // 4 and pre[1] == 0.0 and ref["tail"][1] == 0.0
        if n >= 7 and x["s2"] > 0:
            # (dg + tail) s2 of row 2 is positive in double and rounds to zero in fp32
            assert ref["var"][2] > 0.0 and float(F32(ref["var"][2])) == 0.0
            assert 0 < ref["var"][4] < 1e-3 * abs(x["s2"])
    assert {(c["n"], c["r"]) for c in sr.EVAL_CASES} >= {(n, r) for n in (1, 9, 64) for r in (513, 1000, 1024)}
    assert any(c["moments"] and c["err"] for c in sr.EVAL_CASES) and any(not c["moments"] and c["err"] is None for c in sr.EVAL_CASES)


# --------------------------------------------------------------------------------- c. plain double and fp32 against the bounds
def test_plain_double_and_fp32_evaluations_stay_within_their_bounds():
    worst = {"f64": 0.0, "f32": 0.0}
    for c in ALL_EVAL:
        for tag, T in (("f64", F64), ("f32", F32)):
            w = max(_worst(sr.case_reference(c["name"], T=T, A=F64), sr.held_to(c["name"], T), EVAL_KEYS).values())
            assert w <= 1.0, (c["name"], tag, w)
            worst[tag] = max(worst[tag], w)
    for name in (c["name"] for c in sr.VAR_CASES):
        Y, F, prior, ksc = sr.var_inputs(name)
        worst["f64"] = max(worst["f64"], *_worst(sr.spectral_var(Y, F, prior, ksc, A=F64), sr.spectral_var(Y, F, prior, ksc), ("diag", "tail")).values())
    for r, r_ref in sr.TAIL_CASES:
        x = sr.tail_inputs(r, r_ref)
        worst["f64"] = max(worst["f64"], *_worst(sr.factor_tail(A=F64, **x), sr.factor_tail(**x), sr.TAIL_KEYS).values())
    for case in sr.ABSORB_CASES:
        x = sr.absorb_inputs(*case)
        r = case[1]
        worst["f64"] = max(worst["f64"], *_worst(sr.absorb_h(x["h"], x["F"][:, :r], x["wby"], x["scale"], A=F64),
                                                 sr.absorb_h(x["h"], x["F"][:, :r], x["wby"], x["scale"]), ("h",)).values())
    print(f"share of the bound used by the host evaluations: plain double {worst['f64']:.3g}, fp32 emulation {worst['f32']:.3g}")
    assert worst["f64"] <= 1.0 and worst["f32"] <= 1.0


# ----------------------------------------------------------------------------------------------------------- d. seeded defects
def _report(name, case, factor):
    print(f"seeded defect {name}: case {case}, {factor:.3g} times the bound")
    assert factor >= 4.0, (name, case, factor)


@pytest.mark.parametrize("name", [m for m in sr.MUTANTS if m not in ("max_of_signed_means", "workspace_not_reset")])
def test_seeded_defect_of_evaluate_breaks_the_bound(name):
    case = sr.MUTANTS[name]
    T = F32 if name.startswith("f32_") else F64
    ref = sr.held_to(case, T)
    _report(name, case, max(_worst(sr.case_reference(case, T=T, mutant=name), ref, EVAL_KEYS).values()))


def test_seeded_defect_max_of_signed_means():
    cases = [c["name"] for c in sr.EVAL_CASES if (lambda m: -m.min() > m.max())(sr.case_reference(c["name"])["mean"])]
    assert cases, "no case whose largest |mean| belongs to a negative mean"
    for case in cases[:3]:
        ref = sr.case_reference(case)
        _report("max_of_signed_means", case, float(sr.ratios(sr.case_reference(case, mutant="max_of_signed_means")["out"], ref["out"], ref["d_out"])[3]))


def test_seeded_defect_workspace_not_reset():
    """The third call of the alternating sequence with what the first one would have left in the accumulators."""
    (_, first), _, (_, third), _ = sr.SEQUENCE
    assert sr.MUTANTS["workspace_not_reset"] == third["name"]
    carry = sr.case_reference(first["name"])["dg"]
    ref = sr.case_reference(third["name"])
    _report("workspace_not_reset", third["name"], max(_worst(sr.case_reference(third["name"], mutant="workspace_not_reset", carry=carry), ref, EVAL_KEYS).values()))


@pytest.mark.parametrize("name", list(sr.OTHER_MUTANTS))
def test_seeded_defect_of_the_other_operations_breaks_the_bound(name):
    case = sr.OTHER_MUTANTS[name]
    if name.startswith("tail_"):
        x = sr.tail_inputs(*case)
        assert case in sr.TAIL_CASES
        factor = max(_worst(sr.factor_tail(mutant=name, **x), sr.factor_tail(**x), sr.TAIL_KEYS).values())
    elif name.startswith("spectral_var"):
        a = sr.var_inputs(case)
        factor = max(_worst(sr.spectral_var(*a, mutant=name), sr.spectral_var(*a), ("diag", "tail")).values())
    else:
        x = sr.absorb_inputs(*case)
        assert case in sr.ABSORB_CASES
        r = case[1]
        a = (x["h"], x["F"][:, :r], x["wby"], x["scale"])
        factor = float(np.max(sr.ratios(sr.absorb_h(*a, mutant=name)["h"], sr.absorb_h(*a)["h"], sr.absorb_h(*a)["d_h"])))
    _report(name, case, factor)
