"""GPU: the Kronecker mode products of csrc/solve.hip (wiski_kron_toeplitz_mm: k_toeplitz_line_shfl and k_toeplitz_mode;
wiski_kron_spectral_mm: k_dense_mode<., 0> and k_spectral_scale; both the _f32 and the _f64 entry points) against the plain fp64
references of tests/kron_reference.py, through the C entry points, at the case tables of that file: line lengths 63 / 64 / 65 / 256
on the innermost and on strided modes, anisotropic grids of one to four dimensions, 9216 lines of four points (the line kernel's
grid-stride loop), dense factors up to g = 128 (128 KB of LDS in fp64), orthogonal tables with a zero eigenvalue and random dense
ones, and every (power, rpower, shift, kscale) of kron_reference.SPECTRAL_PARAMS.

Every element of every output is held to the componentwise bound gamma_n absref derived in kron_reference's docstring (n counted from
the kernels, u = 2^-24 or 2^-53, no other constant); tests/test_kron_reference_host.py shows that fp32 emulations of the kernels stay
inside it and that fourteen seeded defects each leave it at some case.  The line-end probes are compared bit for bit.  `out` and
`tmp` lie inside NaN-filled buffers, 256 elements of padding on each side, and the padding must still be NaN after every call; an
output element left unwritten is a NaN and fails the comparison.  The refusals return WISKI_E_BADARG and write nothing."""
import ctypes

import numpy as np
import pytest
import torch

import kron_reference as kr

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float64]
DT_IDS = ["f32", "f64"]
NP = {torch.float32: kr.F32, torch.float64: kr.F64}
PAD = 256
BADARG = -1
SENT = -777.25


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


def _t(x, dtype):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def _np(t):
    return t.detach().cpu().double().numpy()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Guarded:
    """n elements inside a NaN-filled buffer with PAD elements on each side."""

    def __init__(self, n, dtype):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + n]

    def intact(self):
        return bool(torch.isnan(self.buf[:PAD]).all()) and bool(torch.isnan(self.buf[PAD + self.n:]).all())


def _toeplitz(gs, tcol, V, scale, dtype):
    """The product through the C entry, out and tmp guarded; returns out as fp64 numpy [k, m]."""
    from online_gp_amd import _hip

    k, m = V.shape
    out, tmp = _Guarded(k * m, dtype), _Guarded(k * m, dtype)
    tc, Vd = _t(tcol, dtype), _t(V, dtype)
    rc = _hip.fn("wiski_kron_toeplitz_mm", dtype)(_Grid(gs).ref, _ptr(tc), _ptr(Vd), ctypes.c_int32(k), _hip.creal(dtype)(scale),
                                                  _ptr(tmp.t) if len(gs) > 1 else None, _ptr(out.t), _hip.stream_ptr(Vd.device))
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert out.intact() and tmp.intact(), "guard padding overwritten"
    assert np.array_equal(_np(Vd), np.asarray(V, np.float64)), "input overwritten"
    return _np(out.t).reshape(k, m)


def _spectral(gs, F, evals, V, ks, sh, pw, rw, dtype):
    from online_gp_amd import _hip

    k, m = V.shape
    cr = _hip.creal(dtype)
    out, tmp = _Guarded(k * m, dtype), _Guarded(k * m, dtype)
    Fd, ed, Vd = _t(F, dtype), _t(evals, dtype), _t(V, dtype)
    rc = _hip.fn("wiski_kron_spectral_mm", dtype)(_Grid(gs).ref, _ptr(Fd), _ptr(ed), cr(ks), cr(sh), cr(pw), cr(rw), _ptr(Vd), ctypes.c_int32(k),
                                                  _ptr(tmp.t), _ptr(out.t), _hip.stream_ptr(Vd.device))
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert out.intact() and tmp.intact(), "guard padding overwritten"
    assert np.array_equal(_np(Vd), np.asarray(V, np.float64)), "input overwritten"
    return _np(out.t).reshape(k, m)


def _within(out, ref, bound):
    """Every element: |out - ref| <= bound (a NaN fails)."""
    return bool((np.abs(out - ref) <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", kr.TOEPLITZ_CASES, ids=kr.case_id)
def test_toeplitz_product_within_the_bound_at_every_element(case, dtype):
    gs, real = case[0], NP[dtype]
    inp = kr.toeplitz_inputs(case, real)
    ref, absref = kr.toeplitz_ref(gs, inp["tcol"], inp["V"], inp["scale"])
    bound = kr.toeplitz_bound(gs, absref, real)
    out = _toeplitz(gs, inp["tcol"], inp["V"], inp["scale"], dtype)
    print(f"{kr.case_id(case)} {real.__name__}: largest error / bound {kr.ratio(out, ref, bound):.3f} over {out.size} elements")
    assert _within(out, ref, bound), kr.ratio(out, ref, bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("gs", kr.PROBE_GRIDS, ids=lambda gs: "x".join(map(str, gs)))
def test_toeplitz_line_end_probes_are_bit_equal(gs, dtype):
    for s, tcol, V, want in kr.probes(gs):
        out = _toeplitz(gs, tcol, V, 1.0, dtype)
        assert np.array_equal(out, want), (s, np.argwhere(out != want)[:8].tolist())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", kr.SPECTRAL_CASES, ids=kr.case_id)
def test_spectral_product_within_the_bound_at_every_element(case, dtype):
    gs, real = case[0], NP[dtype]
    inp = kr.spectral_inputs(case, real)
    bad, worst = [], 0.0
    for params in kr.SPECTRAL_PARAMS:
        pw, rw, sh, ks = kr.spectral_params(params, real)
        ref, absref = kr.spectral_ref(gs, inp["F"], inp["evals"], inp["V"], ks, sh, pw, rw)
        bound = kr.spectral_bound(gs, absref, real)
        out = _spectral(gs, inp["F"], inp["evals"], inp["V"], ks, sh, pw, rw, dtype)
        r = kr.ratio(out, ref, bound)
        worst = max(worst, r)
        if not _within(out, ref, bound):
            bad.append((params, r))
        if case[2] == "eigen" and pw == 0 and rw == 0 and not _within(out, inp["V"].astype(np.float64), bound):
            bad.append((params, "V not reproduced", kr.ratio(out, inp["V"].astype(np.float64), bound)))   # orthogonal tables, f = 1
    print(f"{kr.case_id(case)} {real.__name__}: largest error / bound {worst:.3f}")
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- refusals --
def _sent(n, dtype):
    return torch.full((n,), SENT, dtype=dtype, device=DEV)


def _untouched(*ts):
    torch.cuda.synchronize()
    return all(bool((t == SENT).all()) for t in ts)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_toeplitz_refusals(dtype):
    from online_gp_amd import _hip

    fn, cr, st = _hip.fn("wiski_kron_toeplitz_mm", dtype), _hip.creal(dtype), _hip.stream_ptr(torch.device(DEV))
    # g = 257: one more than k_toeplitz_mode's coefficient table holds
    tc, V, out = torch.ones(257, dtype=dtype, device=DEV), torch.ones(257, dtype=dtype, device=DEV), _sent(257, dtype)
    assert fn(_Grid((257,)).ref, _ptr(tc), _ptr(V), ctypes.c_int32(1), cr(1.0), None, _ptr(out), st) == BADARG
    assert _untouched(out)
    tmp = _sent(4 * 257, dtype)
    out = _sent(4 * 257, dtype)
    V = torch.ones(4 * 257, dtype=dtype, device=DEV)
    for gs in ((4, 257), (257, 4)):
        tc = torch.ones(261, dtype=dtype, device=DEV)
        assert fn(_Grid(gs).ref, _ptr(tc), _ptr(V), ctypes.c_int32(1), cr(1.0), _ptr(tmp), _ptr(out), st) == BADARG
        assert _untouched(out, tmp)
    # d > 1 without the scratch
    tc, V, out = torch.ones(8, dtype=dtype, device=DEV), torch.ones(16, dtype=dtype, device=DEV), _sent(16, dtype)
    assert fn(_Grid((4, 4)).ref, _ptr(tc), _ptr(V), ctypes.c_int32(1), cr(1.0), None, _ptr(out), st) == BADARG
    assert _untouched(out)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_spectral_refusals(dtype):
    from online_gp_amd import _hip

    fn, cr, st = _hip.fn("wiski_kron_spectral_mm", dtype), _hip.creal(dtype), _hip.stream_ptr(torch.device(DEV))
    one = ctypes.c_int32(1)

    def call(gs, F, ev, V, k, tmp, out):
        return fn(_Grid(gs).ref, _ptr(F), _ptr(ev), cr(1.0), cr(0.0), cr(0.5), cr(0.0), _ptr(V), k, _ptr(tmp), _ptr(out), st)

    # g = 129: above the supported range stated in include/wiski.h, on either mode
    for gs in ((129,), (4, 129), (129, 4)):
        m = int(np.prod(gs))
        F, ev, V = (torch.ones(n, dtype=dtype, device=DEV) for n in (sum(g * g for g in gs), sum(gs), m))
        tmp, out = _sent(m, dtype), _sent(m, dtype)
        assert call(gs, F, ev, V, one, tmp, out) == BADARG
        assert _untouched(tmp, out)
    F, ev = torch.ones(16, dtype=dtype, device=DEV), torch.ones(4, dtype=dtype, device=DEV)
    # out aliasing V
    V, tmp = _sent(4, dtype), _sent(4, dtype)
    assert call((4,), F, ev, V, one, tmp, V) == BADARG
    assert _untouched(V, tmp)
    # k = 0
    V, tmp, out = torch.ones(4, dtype=dtype, device=DEV), _sent(4, dtype), _sent(4, dtype)
    assert call((4,), F, ev, V, ctypes.c_int32(0), tmp, out) == BADARG
    assert _untouched(tmp, out)
