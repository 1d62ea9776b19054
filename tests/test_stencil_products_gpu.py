"""GPU: the block-stencil products of csrc/solve.hip (wiski_stencil_spmv and wiski_stencil_spmv_sym, both the _f32 and the _f64 entry)
against the plain fp64 reference of tests/stencil_reference.py, through the C entries with a hand-filled wiski_grid, on every kernel
path behind them and at every case of that file's table: one to four dimensions, grids smaller than a row block, ragged last blocks,
m % 4 both ways, 1 .. 100 columns, and the innermost sizes on either side of the points where one kernel hands over to another.

Integer data (exact in any summation order) is compared bit for bit, also between two calls on the same buffers; real data is held,
element by element, to gamma_n absref with n counted from the kernels (stencil_reference's docstring; no other constant).  out, A, V
and add each lie inside a NaN-filled buffer with a band of at least 3 sum(stride) + 1024 elements on each side -- wider than any
window a kernel forms -- and after every call the bands of out are still NaN, the inputs unchanged bit for bit and no element of out
is NaN (a stray read of a band meets a zero coefficient and gives one).  wiski_stencil_spmv_path must name the kernel the Python
mirror of the dispatch expects, and the table must reach every code.  The switched configurations (WISKI_SYM_DMA=0
WISKI_SPMM_BCAST=0, and WISKI_SYM_XCD=0: read once per process) run the half-stencil table in fresh child processes."""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import stencil_reference as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
DTYPES = [torch.float32, torch.float64]
DT_IDS = ["f32", "f64"]
NP = {torch.float32: sr.F32, torch.float64: sr.F64}
BITS = {torch.float32: torch.int32, torch.float64: torch.int64}
BADARG = -1
SENT = -777.25
# The half-stencil table of one child (both precisions, both kinds of data) was measured at 4.0 s inside the parent process on an
# MI355X (3.5 s on a second pass); a child gets ten times that for the interpreter, the ROCm start-up and the load of the code
# object.  (The two children took 5.7 s each from start to exit there.)
CHILD_TABLE_S = 4.0
CHILD_TIMEOUT_S = 10 * CHILD_TABLE_S


class _Grid:
    """A wiski_grid filled in by hand: the products read d and g only."""

    def __init__(self, gs):
        from online_gp_amd import _hip

        c = _hip.wiski_grid()
        c.d = len(gs)
        for q, g in enumerate(gs):
            c.g[q], c.g0[q], c.h[q] = int(g), 0.0, 1.0
        self.c = c

    @property
    def ref(self):
        return ctypes.byref(self.c)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(x):
    """A (read-only) numpy array of the reference as a device tensor of its own type and shape."""
    return torch.from_numpy(np.array(x)).to(DEV)


class _Banded:
    """n elements inside a NaN-filled buffer, `band` elements on each side; an input keeps a snapshot of the whole buffer."""

    def __init__(self, n, band, dtype, data=None):
        self.n, self.band = n, band
        self.buf = torch.full((n + 2 * band,), float("nan"), dtype=dtype, device=DEV)
        self.t = self.buf[band:band + n]
        self.snap = None
        if data is not None:
            self.t.copy_(_dev(data).reshape(-1))
            self.snap = self.buf.clone()

    def bands_nan(self):
        return bool(torch.isnan(self.buf[:self.band]).all()) and bool(torch.isnan(self.buf[self.band + self.n:]).all())

    def unchanged(self):
        return torch.equal(self.buf.view(BITS[self.buf.dtype]), self.snap.view(BITS[self.buf.dtype]))


def _path(gs, k, dtype, half):
    from online_gp_amd import _hip

    kc = ctypes.c_int32(-1)
    code = _hip.lib().wiski_stencil_spmv_path(_Grid(gs).ref, ctypes.c_int32(k), ctypes.c_int32(4 if dtype == torch.float32 else 8), ctypes.c_int32(int(half)),
                                              ctypes.byref(kc))
    return code, kc.value


def _product(half, gs, A, V, add, beta, dtype, twice=False):
    """One product through the C entry, every buffer banded.  Returns (out as fp64 numpy [k, m], list of failed checks)."""
    from online_gp_amd import _hip

    band = sr.geometry(gs).band
    k, m = V.shape
    dA, dV, dout = _Banded(A.size, band, dtype, A), _Banded(k * m, band, dtype, V), _Banded(k * m, band, dtype)
    dadd = _Banded(k * m, band, dtype, add) if add is not None else None
    fn = _hip.fn("wiski_stencil_spmv_sym" if half else "wiski_stencil_spmv", dtype)
    fails = []

    def call():
        rc = fn(_Grid(gs).ref, _ptr(dA.t), _ptr(dV.t), ctypes.c_int32(k), _ptr(dadd.t) if dadd else None, _hip.creal(dtype)(beta), _ptr(dout.t),
                _hip.stream_ptr(dV.t.device))
        torch.cuda.synchronize()
        if rc != 0:
            fails.append(f"return code {rc}")
        if not dout.bands_nan():
            fails.append("bands of out overwritten")
        for name, b in (("A", dA), ("V", dV), ("add", dadd)):
            if b is not None and not b.unchanged():
                fails.append(f"{name} (or its bands) changed")
        if bool(torch.isnan(dout.t).any()):
            fails.append(f"{int(torch.isnan(dout.t).sum())} NaN in out")
        return dout.t.clone()

    out = call()
    if twice and not torch.equal(out, call()):
        fails.append("a second call on the same buffers gives other bits")
    return out.cpu().double().numpy().reshape(k, m), fails


def run_case(gs, k, dtype, forms=("half", "full"), switches=None, worst=None, codes=None):
    """Every check of one table case in one precision; returns the list of failures (empty: all good).  worst[(code, precision)]
    collects the largest error / bound of the real data, codes the (precision bytes, d, half, code, kc) reached."""
    real, es = NP[dtype], 4 if dtype == torch.float32 else 8
    tag = f"{sr.case_id((gs, k))} {DT_IDS[DTYPES.index(dtype)]}"
    fails = []

    def note(form, what, f):
        fails.extend(f"{tag} {form} {what}: {x}" for x in f)

    I, X = sr.make_data(gs, k, "int", real), sr.make_data(gs, k, "real", real)
    iref = I["ref"]
    iref0 = iref - I["beta"] * I["add"].astype(np.float64)              # integers: exact
    xref, xabs = X["ref"], X["absref"]
    for form in forms:
        half = form == "half"
        code, kc = _path(gs, k, dtype, half)
        want = sr.expected_path(gs, k, es, half, **(switches or {}))
        if (code, kc) != want:
            fails.append(f"{tag} {form}: wiski_stencil_spmv_path says {(code, kc)}, the dispatch mirror {want}")
            if not 0 <= code <= 7:
                continue
        if codes is not None:
            codes.add((es, len(gs), int(half), code, kc))
        key = "half" if half else "full"
        out, f = _product(half, gs, I[key], I["V"], I["add"], I["beta"], dtype, twice=True)
        note(form, "integer", f)
        if not np.array_equal(out, iref):
            note(form, "integer", [f"{int((out != iref).sum())} of {out.size} elements differ, first at {np.argwhere(out != iref)[:4].tolist()}"])
        out, f = _product(half, gs, I[key], I["V"], None, 0.0, dtype)
        note(form, "integer, add = NULL", f)
        if not np.array_equal(out, iref0):
            note(form, "integer, add = NULL", [f"{int((out != iref0).sum())} of {out.size} elements differ"])
        out, f = _product(half, gs, X[key], X["V"], X["add"], X["beta"], dtype)
        note(form, "real", f)
        r = sr.ratio(out, xref, sr.bound(gs, code, xabs, real))
        if worst is not None:
            worst[(code, es)] = max(worst.get((code, es), 0.0), r)
        if not r <= 1.0:
            note(form, "real", [f"largest error / bound {r:.3g}"])
        if not half:                                                     # independent draws at all R offsets
            N = sr.make_data(gs, k, "real", real, symmetric=False)
            nref, nabs = N["ref"], N["absref"]
            out, f = _product(False, gs, N["full"], N["V"], N["add"], N["beta"], dtype)
            note(form, "real, non-symmetric", f)
            r = sr.ratio(out, nref, sr.bound(gs, code, nabs, real))
            if worst is not None:
                worst[(code, es)] = max(worst.get((code, es), 0.0), r)
            if not r <= 1.0:
                note(form, "real, non-symmetric", [f"largest error / bound {r:.3g}"])
    return fails


def _report(worst):
    for (code, es), r in sorted(worst.items()):
        print(f"path {code} fp{8 * es}: largest error / bound {r:.3f}")


def _run(cases, dtype):
    worst = {}
    fails = [f for gs, k in cases for f in run_case(gs, k, dtype, worst=worst)]
    _report(worst)
    assert not fails, fails[:20]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("d", [1, 2])
def test_products_in_one_and_two_dimensions(d, dtype):
    _run(sr.cases_of(d), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("gs", sr.GRIDS[3], ids=lambda gs: "x".join(map(str, gs)))
def test_products_in_three_dimensions(gs, dtype):
    _run([c for c in sr.CASES if c[0] == gs], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", list(sr.HANDOVER))
def test_products_on_both_sides_of_an_lds_handover(name, dtype):
    g, k = sr.HANDOVER[name], sr.HANDOVER_K[name]
    _run([((4, 4, g), k), ((4, 4, g + 1), k)], dtype)
    if dtype == torch.float32:
        below, above = _path((4, 4, g), k, dtype, True)[0], _path((4, 4, g + 1), k, dtype, True)[0]
        assert below == (4 if name == "dma" else 5) and above == 3


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("gs", sr.GRIDS[4], ids=lambda gs: "x".join(map(str, gs)))
def test_products_in_four_dimensions(gs, dtype):
    _run([c for c in sr.CASES if c[0] == gs], dtype)


def test_path_query_agrees_with_the_mirror_and_the_table_reaches_every_kernel():
    seen = set()
    for gs, k in sr.CASES:
        for dtype in DTYPES:
            for half in (False, True):
                es = 4 if dtype == torch.float32 else 8
                got = _path(gs, k, dtype, half)
                assert got == sr.expected_path(gs, k, es, half), (gs, k, es, half, got)
                seen.add(got)
    assert {c for c, _ in seen} == {0, 1, 2, 3, 4, 5, 6}
    for code in (0, 1, 2, 3):
        assert {1, 2, 4} <= {kc for c, kc in seen if c == code}, code
    assert {kc for c, kc in seen if c == 5} == {2, 4}
    from online_gp_amd import _hip

    path = _hip.lib().wiski_stencil_spmv_path
    kc = ctypes.c_int32(-5)
    assert path(_Grid((4, 4)).ref, ctypes.c_int32(0), ctypes.c_int32(4), ctypes.c_int32(1), ctypes.byref(kc)) == BADARG
    assert path(_Grid((4, 4)).ref, ctypes.c_int32(1), ctypes.c_int32(2), ctypes.c_int32(1), ctypes.byref(kc)) == BADARG
    assert path(_Grid((4, 3)).ref, ctypes.c_int32(1), ctypes.c_int32(4), ctypes.c_int32(1), ctypes.byref(kc)) == BADARG
    assert path(None, ctypes.c_int32(1), ctypes.c_int32(4), ctypes.c_int32(1), ctypes.byref(kc)) == BADARG and kc.value == -5
    assert path(_Grid((4, 4)).ref, ctypes.c_int32(1), ctypes.c_int32(8), ctypes.c_int32(1), None) == 3


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_layout_helpers_agree_with_the_reference_packers(dtype):
    from online_gp_amd import grid_ops

    for gs in [(7,), (7, 9), (8, 5, 9), (4, 5, 4, 6)]:
        G, grid = sr.geometry(gs), _Grid(gs)                  # the helpers read grid.ref only
        D = sr.make_data(gs, 1, "real", NP[dtype])
        om = _dev(sr.half_om_from_full(gs, D["full"]))
        native = _dev(D["half"]).view(G.H, G.m)
        assert torch.equal(grid_ops.half_stencil_from_offset_major(grid, om), native)
        assert torch.equal(grid_ops.half_stencil_to_offset_major(grid, native), om)
        base = _dev(sr.make_data(gs, 1, "int", NP[dtype], symmetric=False)["full"])
        I = sr.make_data(gs, 1, "int", NP[dtype])
        full, delta = base.clone(), _dev(I["half"]).view(G.H, G.m)
        grid_ops.stencil_expand_add(grid, delta, full)
        torch.cuda.synchronize()
        assert torch.equal(full, base + _dev(I["full"]))      # small integers: the sum is exact
        assert not delta.any()                                                  # the half is zeroed once expanded


# ---------------------------------------------------------------------------------------------------------------- refusals --
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
def test_refusals_write_nothing(half, dtype):
    from online_gp_amd import _hip

    fn, cr, st = _hip.fn("wiski_stencil_spmv_sym" if half else "wiski_stencil_spmv", dtype), _hip.creal(dtype), _hip.stream_ptr(torch.device(DEV))
    for gs in ((4, 4), (7, 9)):                       # the wide and the generic kernel
        G = sr.geometry(gs)
        A = torch.ones((G.H if half else G.R) * G.m, dtype=dtype, device=DEV)
        V = torch.full((G.m,), SENT, dtype=dtype, device=DEV)
        out = torch.full((G.m,), SENT, dtype=dtype, device=DEV)
        one = ctypes.c_int32(1)
        for a, v, o, k in ((None, V, out, one), (A, None, out, one), (A, V, None, one), (A, V, out, ctypes.c_int32(0)), (A, V, out, ctypes.c_int32(-3)),
                           (A, V, V, one)):
            assert fn(_Grid(gs).ref, _ptr(a), _ptr(v), k, None, cr(0.0), _ptr(o), st) == BADARG
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and bool((V == SENT).all())


# ------------------------------------------------------------------------------------------------- switched configurations --
def half_table(switches):
    """The half-stencil table, both precisions, both kinds of data: what a child process runs."""
    fails, codes, worst = [], set(), {}
    for dtype in DTYPES:
        for gs, k in sr.CASES:
            fails += run_case(gs, k, dtype, forms=("half",), switches=switches, worst=worst, codes=codes)
    return fails, codes, worst


def child_main():
    switches = {"sym_dma": os.environ.get("WISKI_SYM_DMA", "1") != "0", "spmm_bcast": os.environ.get("WISKI_SPMM_BCAST", "1") != "0"}
    t0 = time.perf_counter()
    fails, codes, worst = half_table(switches)
    print(json.dumps({"failures": fails[:50], "nfail": len(fails), "codes": sorted(codes), "worst": {f"{c}/fp{8 * e}": r for (c, e), r in sorted(worst.items())},
                      "seconds": time.perf_counter() - t0}), flush=True)


def _child(env):
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child"], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT_S)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(env, {k: rep[k] for k in ("nfail", "worst", "seconds")})
    assert rep["nfail"] == 0, rep["failures"]
    return {tuple(c) for c in rep["codes"]}


def test_switched_configurations_in_fresh_processes():
    # the LDS-window kernel on the fp32 d = 3 route and the lanes-are-columns kernel (kp = 64 and kp < 64)
    codes = _child({"WISKI_SYM_DMA": "0", "WISKI_SPMM_BCAST": "0"})
    assert {c[3] for c in codes} == {2, 3, 7}
    assert any(es == 4 and d == 3 and code == 3 for es, d, _, code, _ in codes)
    for es in (4, 8):
        kps = {kc for e, _, _, code, kc in codes if code == 7 and e == es}
        assert 64 in kps and min(kps) < 64 and max(kps) > 64, kps
    # the plain row-block mapping of kernels 3, 4 and 5
    codes = _child({"WISKI_SYM_XCD": "0"})
    assert {c[3] for c in codes} == {2, 3, 4, 5, 6}


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    if sys.argv[1:] == ["--child"]:
        child_main()
