"""Host: checks of the reference of the Kronecker mode products (tests/kron_reference.py) that tests/test_kron_products_gpu.py holds
wiski_kron_toeplitz_mm and wiski_kron_spectral_mm to, and of the case tables both files share.  No GPU:
  - at every table case with m <= 4096 the reference equals the brute-force dense Kronecker matrix product to 1e-12 relative;
  - at every case the fp32 emulations of the kernels' operation order (contracted to fused multiply-adds and not) stay inside the
    derived bound, ratio < 1: a theorem if the operation counts of kron_reference.toeplitz_n / spectral_n are right;
  - the emulations reproduce the exact line-end probes bit for bit, and the line-end defects do not;
  - every wrong variant in MUTANTS leaves the bound at some case: the bound is not loose, and the tables reach the places where those
    defects show.  The test prints, per mutant, which cases catch it and by what ratio."""
import numpy as np
import pytest

import kron_reference as kr

F32, F64 = kr.F32, kr.F64
IDS = dict(ids=kr.case_id)


@pytest.fixture(scope="module")
def toeplitz_refs():
    """case -> (inputs, ref, absref) in fp32, computed once."""
    out = {}
    for case in kr.TOEPLITZ_CASES:
        inp = kr.toeplitz_inputs(case, F32)
        out[case] = (inp,) + kr.toeplitz_ref(case[0], inp["tcol"], inp["V"], inp["scale"])
    return out


@pytest.fixture(scope="module")
def spectral_refs():
    """(case, params) -> (inputs, params as the kernel gets them, ref, absref) in fp32, computed once."""
    out = {}
    for case in kr.SPECTRAL_CASES:
        inp = kr.spectral_inputs(case, F32)
        for params in kr.SPECTRAL_PARAMS:
            pw, rw, sh, ks = kr.spectral_params(params, F32)
            out[case, params] = (inp, (pw, rw, sh, ks)) + kr.spectral_ref(case[0], inp["F"], inp["evals"], inp["V"], ks, sh, pw, rw)
    return out


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


_dense_cache = {}


def _toeplitz_dense(gs, tcol):
    key = (gs, tcol.tobytes())
    if key not in _dense_cache:
        _dense_cache.clear()                       # one 4096 x 4096 matrix at a time
        _dense_cache[key] = kr.kron_dense([kr.sym_toeplitz(c) for c in kr.split(gs, tcol)])
    return _dense_cache[key]


@pytest.mark.parametrize("case", [c for c in kr.TOEPLITZ_CASES if np.prod(c[0]) <= 4096], **IDS)
def test_toeplitz_reference_is_the_dense_kronecker_product(case):
    gs = case[0]
    for real in (F32, F64):
        inp = kr.toeplitz_inputs(case, real)
        ref, absref = kr.toeplitz_ref(gs, inp["tcol"], inp["V"], inp["scale"])
        K = _toeplitz_dense(gs, inp["tcol"])
        V = inp["V"].astype(F64)
        assert _rel(ref, inp["scale"] * V @ K.T) <= 1e-12
        assert _rel(absref, abs(inp["scale"]) * np.abs(V) @ np.abs(K).T) <= 1e-12


@pytest.mark.parametrize("case", kr.SPECTRAL_CASES, **IDS)
def test_spectral_reference_is_the_dense_kronecker_product(case):
    gs = case[0]
    assert np.prod(gs) <= 4096
    for real in (F32, F64):
        inp = kr.spectral_inputs(case, real)
        K = kr.kron_dense([f.astype(F64) for f in kr.split(gs, inp["F"], square=True)])
        V = inp["V"].astype(F64)
        for params in kr.SPECTRAL_PARAMS:
            pw, rw, sh, ks = kr.spectral_params(params, real)
            ref, absref = kr.spectral_ref(gs, inp["F"], inp["evals"], inp["V"], ks, sh, pw, rw)
            lam, f = kr.spectral_factor(gs, inp["evals"], ks, sh, pw, rw)
            # the factor, element by element from its definition
            ev = kr.split(gs, inp["evals"])
            for e in (0, len(lam) // 3, len(lam) - 1):
                iq = np.unravel_index(e, gs)
                l = ks * np.prod([float(ev[q][iq[q]]) for q in range(len(gs))])
                want = (1.0 if pw == 0 else (l ** pw if l > 0 else 0.0)) * (1.0 if rw == 0 else (1 + sh * l) ** -rw)
                assert abs(f[e] - want) <= 1e-13 * abs(want)
            assert _rel(ref, (V @ K) * f @ K.T) <= 1e-12          # rows of V: (K diag(f) K^T v)^T = v^T K diag(f) K^T
            assert _rel(absref, (np.abs(V) @ np.abs(K)) * np.abs(f) @ np.abs(K).T) <= 1e-12
    if case[2] == "eigen":                         # the zero eigenvalue is there, and the guard decides f at it
        lam, f = kr.spectral_factor(gs, kr.spectral_inputs(case, F32)["evals"], 1.0, 0.0, -0.5, 0.0)
        assert (lam == 0).sum() == len(lam) // gs[0] and (f[lam == 0] == 0).all() and lam[lam > 0].min() > 1e-30


def test_emulations_stay_inside_the_bound(toeplitz_refs, spectral_refs):
    worst = {"toeplitz": (0.0, None), "spectral": (0.0, None)}
    for case, (inp, ref, absref) in toeplitz_refs.items():
        for fma in (True, False):
            r = kr.ratio(kr.emu_toeplitz(case[0], inp["tcol"], inp["V"], inp["scale"], fma=fma), ref, kr.toeplitz_bound(case[0], absref, F32))
            worst["toeplitz"] = max(worst["toeplitz"], (r, kr.case_id(case)))
            assert r < 1, (case, fma, r)
    for (case, params), (inp, (pw, rw, sh, ks), ref, absref) in spectral_refs.items():
        for fma in (True, False):
            out = kr.emu_spectral(case[0], inp["F"], inp["evals"], inp["V"], ks, sh, pw, rw, fma=fma)
            r = kr.ratio(out, ref, kr.spectral_bound(case[0], absref, F32))
            worst["spectral"] = max(worst["spectral"], (r, kr.case_id(case) + f"-{params}"))
            assert r < 1, (case, params, fma, r)
            if case[2] == "eigen" and pw == 0 and rw == 0:      # orthogonal tables, f = 1: the product gives V back
                assert kr.ratio(out, inp["V"].astype(F64), kr.spectral_bound(case[0], absref, F32)) < 1, (case, fma)
    for name, (r, where) in worst.items():
        print(f"fp32 emulation of the {name} product: largest error / bound {r:.3f} at {where}")


def test_emulations_reproduce_the_exact_probes_and_line_end_defects_do_not():
    for gs in kr.PROBE_GRIDS:
        caught = set()
        for s, tcol, V, want in kr.probes(gs):
            tc, V32 = tcol.astype(F32), V.astype(F32)
            assert np.array_equal(kr.emu_toeplitz(gs, tc, V32, 1.0), want), (gs, s)
            for mutant in ("no zero at lane 63", "no zero at lane 0", "tcol[sft-1]", "line kernel at g = 65"):
                if not np.array_equal(kr.emu_toeplitz(gs, tc, V32, 1.0, mutant=mutant), want):
                    caught.add(mutant)
        want_caught = {"no zero at lane 0", "tcol[sft-1]", "no zero at lane 63"} if gs[-1] == 64 else {"line kernel at g = 65"}
        assert caught == want_caught, (gs, caught)


def test_every_mutant_leaves_the_bound_somewhere(toeplitz_refs, spectral_refs):
    missed = []
    for mutant, product in kr.MUTANTS.items():
        hits = []
        if product == "toeplitz":
            for case, (inp, ref, absref) in toeplitz_refs.items():
                r = kr.ratio(kr.emu_toeplitz(case[0], inp["tcol"], inp["V"], inp["scale"], mutant=mutant), ref, kr.toeplitz_bound(case[0], absref, F32))
                if r > 1:
                    hits.append((r, kr.case_id(case)))
        else:
            for (case, params), (inp, (pw, rw, sh, ks), ref, absref) in spectral_refs.items():
                r = kr.ratio(kr.emu_spectral(case[0], inp["F"], inp["evals"], inp["V"], ks, sh, pw, rw, mutant=mutant), ref,
                             kr.spectral_bound(case[0], absref, F32))
                if r > 1:
                    hits.append((r, kr.case_id(case) + f"-{params}"))
        total = len(toeplitz_refs) if product == "toeplitz" else len(spectral_refs)
        if not hits:
            missed.append(mutant)
            print(f"{mutant}: NOT CAUGHT")
            continue
        print(f"{mutant}: caught at {len(hits)} of {total} cases, smallest ratio {min(hits)[0]:.3g} ({min(hits)[1]}); "
              + ", ".join(f"{w} {r:.3g}" for r, w in hits))
    assert not missed, missed
