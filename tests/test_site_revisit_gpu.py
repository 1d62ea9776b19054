"""GPU: revisiting stored sites -- expectation-propagation sweeps over a ring of interval and count observations --
against the fp64 reference of tests/revisit_reference.py: the kernel through the C ABI, the contract, and the model surface
(site_memory, refine_sites_) against the data-space driver ``ep_stream``.

Bounds.  Statistics: those of tests/test_interval_gpu.py (scatter 1e-11 / 2e-4, x 10, relative to max |reference|).  Sites in fp64:
1e-9 on ytilde (of max |ytilde|) and on omega (of each omega), 1e-11 on log Z (of each log Z).  Sites in fp32: cavity, site and damping
are evaluated in fp64 in both precisions, but the predictive mean, the variance and the stored site reach them in fp32, and the cavity
magnifies that by v / v_cavity (up to 5 here).  FP32_SITE_DEV holds the deviations from the fp64 reference measured on one MI355X (the
largest over the grids, forms and dampings), and the test asserts three times those, the project's rule for fp32 parity.  Model:
MODEL_DEV holds the measured deviations from ``ep_stream``, asserted with the same factor.  All of them are tabulated in DESIGN.md 3.28.
"""
import ctypes

import numpy as np
import pytest
import torch

import revisit_reference as rv
from oracle import dataspace

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
DTYPES = [(torch.float64, 1e-11), (torch.float32, 2e-4)]          # the scatter tolerances of tests/test_grad_obs_gpu.py
KGRIDS = {"d1": [8], "d2": [8, 8], "d3": [8, 8, 8], "d4": [6, 6, 6, 6]}
CAP = 37                                                          # three blocks of 16; the last pass of the last block holds one slot
EMPTY_SLOTS = (11, 20, 35, 36)                                    # 33 of the 37 slots are filled
OTHER_SLOTS = (8, 9, 30)                                          # slots of another form
KS2 = 0.7
KEYS = ("A", "b", "cnt", "stats", "res")
FORMS = {"interval": rv.INTERVAL, "poisson": rv.POISSON, "binomial": rv.BINOMIAL}
FP64_SITE = dict(ytilde=1e-9, omega=1e-9, log_z=1e-11)
# measured on one MI355X, fp32 against the fp64 reference, largest over grids, forms and dampings
FP32_SITE_DEV = dict(ytilde=1.723e-07, omega=7.552e-07, log_z=3.107e-06)
f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
_cases = {}


def _kernel_case(name, form):
    """Grid, a ring of 37 slots (fp64 values that are exact in fp32), the marginal variances and the dense reference at damping 1 and
    0.5; built once.  Every filled slot holds an old site with tau_old v in (0, 0.8): a cavity precision of at least a fifth of 1 / v.
      0, 1: exact values (interval form; left alone)   2: omega_old = 0, the fresh site enters   3: the fresh site is below OMEGA_MIN
      (leaves at damping 1) while its log Z is of order ten: a bound satisfied by 12 s, an event at exposure 1e-25, a failure at mean +60   4: tau_old v = 1.5, a negative cavity   5: tau_old v = 1 - 5e-6, a cavity below CAVITY_MIN (both left
      alone)   6: pvar = 0 (left alone)   10: outside the grid (left alone)   8, 9, 30: another form's   11, 20, 35, 36: empty
      12 .. 16 share one interior cell (colliding atomics)."""
    key = (name, form)
    if key in _cases:
        return _cases[key]
    from online_gp_amd import grid_ops

    g = KGRIDS[name]
    d = len(g)
    code = FORMS[form]
    other = rv.POISSON if code != rv.POISSON else rv.INTERVAL
    rng = np.random.default_rng(400 + 10 * d + code)
    grid = grid_ops.GridSpec([[-1.0, 1.0 + 0.25 * q] for q in range(d)], g)
    cell = np.stack([rng.integers(0, gq - 1, CAP) for gq in g], 1).astype(np.float64)
    frac = 0.5 + rng.choice([-1.0, 1.0], (CAP, d)) * rng.uniform(0.05, 0.45, (CAP, d))
    for q in range(d):
        cell[22 + q, q] = 0                                         # first (boundary) cell of dim q
        cell[26 + q, q] = g[q] - 2                                  # last (boundary) cell of dim q
    cell[12:17] = 1
    X = np.array(grid.g0) + np.array(grid.h) * (cell + frac)
    X[10, 0] = grid.g0[0] - 1.0
    X = f32(X)
    forms = np.full(CAP, code, dtype=np.int64)
    forms[list(OTHER_SLOTS)] = other
    forms[list(EMPTY_SLOTS)] = rv.EMPTY
    if code == rv.INTERVAL:
        noise = f32(rng.uniform(0.5, 2.0, CAP))
        wa = f32(1.0 / noise)
    else:
        noise, wa = np.ones(CAP), np.ones(CAP)
    pvar = f32(rng.uniform(0.1, 1.5, CAP))
    pvar[6] = 0.0
    u = f32(0.7 * rng.standard_normal(grid.m))
    dn = KS2 * noise
    tv = rng.uniform(0.05, 0.8, CAP)                                # tau_old v
    tv[2], tv[4], tv[5] = 0.0, 1.5, 1.0 - 5e-6
    omega = f32(dn * tv / np.where(pvar > 0, pvar, 1.0))
    import interp_reference as ir

    mean = ir.dense_rows(grid, torch.as_tensor(X)).numpy() @ u
    ytilde = mean + np.sqrt(pvar) * rng.uniform(-1.0, 1.0, CAP)
    if code == rv.BINOMIAL:                                          # slot 3: an old site that puts the cavity mean at +60
        p3 = 1.0 / pvar[3] - omega[3] / dn[3]
        ytilde[3] = (mean[3] / pvar[3] - 60.0 * p3) / (omega[3] / dn[3])
    ytilde = f32(ytilde)
    # the cavity of the reference itself, to place the data around
    tau = omega / dn
    with np.errstate(divide="ignore", invalid="ignore"):
        vc = 1.0 / (1.0 / pvar - tau)
        muc = vc * (mean / pvar - tau * ytilde)
    good = np.isfinite(vc) & (vc > 0)
    vc, muc = np.where(good, vc, 1.0), np.where(good, muc, 0.0)
    s = np.sqrt(vc + dn)
    d0, d1 = np.zeros(CAP), np.ones(CAP)

    def interval_data(i, turn):
        k = ("lower", "upper", "two")[turn % 3]
        if k == "two":
            width = np.exp(rng.uniform(np.log(0.05), np.log(4.0)))
            a = rng.uniform(-6.0, 4.0 - width)
            return muc[i] + s[i] * a, muc[i] + s[i] * (a + width)
        t = rng.uniform(-6.0, 4.0)                                   # > 0: satisfied by t s, < 0: violated
        return (muc[i] - t * s[i], INF) if k == "lower" else (-INF, muc[i] + t * s[i])

    def count_data(i, c):
        f = muc[i] + np.sqrt(vc[i]) * rng.standard_normal()
        if c == rv.POISSON:
            t = float(f32(np.exp(rng.uniform(-1.0, 1.5))))
            return float(rng.poisson(min(t * np.exp(f), 50.0))), t
        t = float(rng.integers(1, 13))
        return float(rng.binomial(int(t), 1.0 / (1.0 + np.exp(-f)))), t

    for i in range(CAP):
        if forms[i] == rv.EMPTY:
            noise[i], wa[i], omega[i], ytilde[i] = 1.0, 0.0, 0.0, 0.0
            X[i] = 0.0
        elif forms[i] == rv.INTERVAL:
            d0[i], d1[i] = interval_data(i, i)
        else:
            d0[i], d1[i] = count_data(i, forms[i])
    if code == rv.INTERVAL:
        d0[0] = d1[0] = ytilde[0]
        d0[1] = d1[1] = ytilde[1]
        omega[0] = omega[1] = 1.0
        d0[3], d1[3] = muc[3] - 12.0 * s[3], INF                     # a bound satisfied by twelve standard deviations says nothing
    elif code == rv.POISSON:
        d0[3], d1[3] = 1.0, 1e-25                                    # one event at a vanishing exposure: log Z = -57 or so, tau = E[t e^f] = 1e-21
    else:
        d0[3], d1[3] = 0.0, 1.0                                      # no success in one trial at a cavity mean of +60: log Z = -60 or so, tau = 1e-21
    d0, d1 = f32(d0), f32(d1)
    ring = dict(x=X, d0=d0, d1=d1, noise=noise, wa=wa, wb=wa.copy(), ytilde=ytilde, omega=omega, form=forms)
    refs = {dmp: rv.dense_revisit(grid, ring, code, pvar, KS2, u, dmp) for dmp in (1.0, 0.5)}
    _cases[key] = dict(grid=grid, ring=ring, pvar=pvar, u=u, refs=refs, code=code)
    return _cases[key]


KERNEL_CASES = [(n, "interval") for n in KGRIDS] + [(n, f) for n in ("d1", "d3") for f in ("poisson", "binomial")]


def _device_ring(c, tdt):
    from online_gp_amd import grid_ops

    r = c["ring"]
    ring = grid_ops.SiteRing(CAP, c["grid"].d, tdt, DEV)
    for k in rv.RING_KEYS:
        getattr(ring, k).copy_(torch.as_tensor(r[k]).to(getattr(ring, k)))
    return ring


def _buffers(grid, tdt, init=None):
    H = (grid.R + 1) // 2
    z = lambda *s: torch.zeros(s, device=DEV, dtype=tdt)
    out = dict(b=z(grid.m), A=z(H * grid.m), cnt=z(grid.m), res=z(grid.m), stats=torch.zeros(2, device=DEV, dtype=torch.float64))
    if init is not None:
        for k, v in out.items():
            v.copy_(torch.as_tensor(init[k]).to(v))
    return out


def _compare(got, ref, tol, keys, label):
    for k in keys:
        r = np.asarray(ref[k], dtype=np.float64)
        e = float(np.abs(got[k].double().cpu().numpy() - r).max())
        bound = 10 * tol * float(np.abs(r).max())
        print(f"{label} {k}: max err {e:.3e}  bound {bound:.3e}")
        assert e <= bound, (label, k, e, bound)


def _site_deviation(yt, om, lz, ref):
    """ytilde: largest error over max |ytilde|; omega: relative to each omega (where it is not 0); log Z: relative to each log Z, over
    the re-matched slots."""
    nz_o, t = ref["omega"] != 0, ref["touched"] & (ref["log_z"] != 0)
    return dict(ytilde=float(np.abs(yt - ref["ytilde"]).max() / np.abs(ref["ytilde"]).max()),
                omega=float((np.abs(om - ref["omega"])[nz_o] / ref["omega"][nz_o]).max()),
                log_z=float((np.abs(lz - ref["log_z"])[t] / np.abs(ref["log_z"][t])).max()))


@pytest.mark.parametrize("name,form", KERNEL_CASES)
def test_reference_split_of_the_kernel_case(name, form):
    """What the ring is meant to contain, on the reference alone: which slots are left alone, enter and leave, and that no decision lies
    within a factor 10 of CAVITY_MIN or of OMEGA_MIN."""
    c = _kernel_case(name, form)
    code = c["code"]
    alone = {4, 5, 6, 10} | set(OTHER_SLOTS) | set(EMPTY_SLOTS) | ({0, 1} if code == rv.INTERVAL else set())
    for dmp, r in c["refs"].items():
        assert set(np.nonzero(~r["touched"])[0]) == alone
        assert list(np.nonzero(r["entered"])[0]) == [2] and list(np.nonzero(r["left"])[0]) == ([3] if dmp == 1.0 else [])
        t = r["touched"]
        assert (r["rel_p"][t] >= 10 * rv.CAVITY_MIN).all() and r["rel_p"][4] < 0 and 0 < r["rel_p"][5] <= rv.CAVITY_MIN / 10
        on = r["omega"][t]
        assert ((on == 0.0) | (on >= 10 * rv.OMEGA_MIN)).all() and np.isfinite(r["log_z"][t]).all() and np.isnan(r["log_z"][~t]).all()
        assert (r["change"][~t] == 0).all() and (r["change"][t] > 0).all()
        for k in ("ytilde", "omega"):
            assert np.array_equal(r[k][~t], c["ring"][k][~t])
    # the fresh site of slot 3 is below a tenth of OMEGA_MIN: at damping 0.5 the slot keeps half of its old weight
    half = c["refs"][0.5]
    assert abs(half["omega"][3] / c["ring"]["omega"][3] - 0.5) < 1e-10
    print(f"{name} {form}: omega_new {c['refs'][1.0]['omega'][c['refs'][1.0]['touched']].max():.3f} at most, smallest cavity {c['refs'][1.0]['rel_p'][c['refs'][1.0]['touched']].min():.3f} / v")


@pytest.mark.parametrize("tdt,tol", DTYPES)
@pytest.mark.parametrize("damping", [1.0, 0.5])
@pytest.mark.parametrize("name,form", KERNEL_CASES)
def test_kernel_matches_the_dense_reference(name, form, damping, tdt, tol):
    from online_gp_amd import grid_ops

    test_reference_split_of_the_kernel_case(name, form)              # the split holds on the reference before the kernel is looked at
    c = _kernel_case(name, form)
    grid, ref = c["grid"], c["refs"][damping]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    pvar, u = mk(c["pvar"]), mk(c["u"])
    rname = dict(ref, A=ref["A_half"])
    ring, got, err = _device_ring(c, tdt), _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    lz, ch = grid_ops.revisit_sites(grid, ring, form, pvar, KS2, damping, got["b"], got["A"], got["cnt"], got["stats"], err, u, res=got["res"])
    assert lz.dtype == torch.float64 and ch.dtype == tdt and lz.shape == ch.shape == (CAP,) and int(err.item()) == 0
    yt, om, lz, ch = (t.double().cpu().numpy() for t in (ring.ytilde, ring.omega, lz, ch))
    dev = _site_deviation(yt, om, lz, ref)
    bound = FP64_SITE if tdt == torch.float64 else {k: (None if v is None else 3.0 * v) for k, v in FP32_SITE_DEV.items()}
    print(f"{name} {form} damping {damping} {tdt} sites: " + "  ".join(f"{k} {dev[k]:.3e} (bound {bound[k]})" for k in dev))
    e_ch = float(np.abs(ch - ref["change"]).max())
    print(f"{name} {form} damping {damping} {tdt} change: max err {e_ch:.3e}")
    # which slots are left alone, enter or leave: exactly the reference's
    t = ref["touched"]
    start = c["ring"]
    assert np.array_equal(yt[~t], f32(start["ytilde"])[~t]) and np.array_equal(om[~t], f32(start["omega"])[~t])       # left alone: bit for bit
    assert np.array_equal(np.isnan(lz), ~t) and np.array_equal(ch == 0.0, ~t)
    assert np.array_equal(om == 0.0, ref["omega"] == 0.0)
    assert np.array_equal((start["omega"] == 0) & (om > 0), ref["entered"]) and np.array_equal((start["omega"] > 0) & (om == 0), ref["left"])
    for k in rv.RING_KEYS[:6] + ("form",):                            # the kernel writes the site alone
        assert torch.equal(getattr(ring, k).cpu(), torch.as_tensor(start[k]).to(getattr(ring, k).dtype).reshape(getattr(ring, k).shape))
    _compare(got, rname, tol, KEYS, f"{name} {form} damping {damping} zero-init")
    for k in dev:
        assert bound[k] is not None and dev[k] <= bound[k], (name, form, k, dev[k], bound[k])
    assert e_ch <= (1e-9 if tdt == torch.float64 else 3.0 * FP32_SITE_DEV["omega"])
    # on top of non-zero buffers: every statistic is added, none assigned; the sites do not depend on what the buffers hold
    rng = np.random.default_rng(5)
    init = {k: 0.5 * float(np.abs(rname[k]).max()) * rng.standard_normal(np.shape(rname[k])) for k in KEYS}
    got = _buffers(grid, tdt, init)
    first = {k: v.double().cpu().numpy().copy() for k, v in got.items()}
    ring2 = _device_ring(c, tdt)
    lz2, ch2 = grid_ops.revisit_sites(grid, ring2, form, pvar, KS2, damping, got["b"], got["A"], got["cnt"], got["stats"], err, u, res=got["res"])
    _compare(got, {k: first[k] + rname[k] for k in KEYS}, tol, KEYS, f"{name} {form} on top")
    assert torch.equal(ring2.ytilde, ring.ytilde) and torch.equal(ring2.omega, ring.omega) and torch.equal(ch2.cpu().double(), torch.as_tensor(ch))


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
def test_damping_zero_changes_nothing_bit_for_bit(tdt):
    from online_gp_amd import grid_ops

    for form in FORMS:
        c = _kernel_case("d3", form)
        grid = c["grid"]
        mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
        rng = np.random.default_rng(9)
        H = (grid.R + 1) // 2
        init = dict(b=rng.standard_normal(grid.m), A=rng.standard_normal(H * grid.m), cnt=rng.standard_normal(grid.m), res=rng.standard_normal(grid.m),
                    stats=rng.standard_normal(2))
        got, err = _buffers(grid, tdt, init), grid_ops.new_err_flag(DEV)
        before = {k: v.clone() for k, v in got.items()}
        ring = _device_ring(c, tdt)
        start = ring.clone()
        lz, ch = grid_ops.revisit_sites(grid, ring, form, mk(c["pvar"]), KS2, 0.0, got["b"], got["A"], got["cnt"], got["stats"], err, mk(c["u"]), res=got["res"])
        torch.cuda.synchronize()
        assert all(torch.equal(got[k], before[k]) for k in got) and int(err.item()) == 0
        assert all(torch.equal(a, b) for a, b in zip(ring.tensors(), start.tensors()))
        assert float(ch.abs().max()) == 0.0 and bool(torch.isnan(lz).all())


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
def test_absorb_refuses_the_revisit_group_with_what_the_kernel_does_not_do(tdt):
    """Through the full argument record plus the revisit group (wiski_absorb_revisit): every combination the contract refuses is
    WISKI_E_BADARG before any launch -- every buffer and the ring untouched -- while the record without the offending field runs and
    equals grid_ops.revisit_sites; res is optional, the record's points are not looked at; an empty ring is WISKI_OK and does nothing."""
    from online_gp_amd import _hip, grid_ops

    c = _kernel_case("d3", "interval")
    grid = c["grid"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    pvar, u = mk(c["pvar"]), mk(c["u"])
    ring = _device_ring(c, tdt)
    start = ring.clone()
    buf, err = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    logz = torch.full((CAP,), 7.0, device=DEV, dtype=torch.float64)
    change = torch.full((CAP,), 7.0, device=DEV, dtype=tdt)
    mean = torch.full((CAP,), float("nan"), device=DEV, dtype=tdt)
    full = torch.zeros((grid.R, grid.m), device=DEV, dtype=tdt)
    guard = torch.tensor([7], device=DEV, dtype=torch.int64)
    z1 = torch.full((2,), 0x01010101, device=DEV, dtype=torch.int32)
    bin_ws = torch.zeros(1 << 16, device=DEV, dtype=torch.uint8)
    p = lambda t: t.data_ptr()
    stream = _hip.stream_ptr(torch.device("cuda", torch.cuda.current_device()))

    def call(ring_=ring, form=rv.INTERVAL, pvar_=pvar, sigma2=KS2, damping=1.0, logz_=logz, change_=change, drop=None, **kw):
        a = _hip.wiski_absorb_args(d_x=None, d_y=None, d_wa=None, d_wb=None, d_noise=None, n=0, d_b=p(buf["b"]), d_A=p(buf["A"]), half=1, channels=0,
                                   d_cnt=p(buf["cnt"]), d_stats=p(buf["stats"]), d_err=p(err), d_u=p(u), d_res=p(buf["res"]), d_mean_out=None, nout=1)
        for k, v in kw.items():
            setattr(a, k, v)
        r = ring_.ref()
        if drop is not None:
            setattr(r, drop, None)
        return _hip.fn("wiski_absorb_revisit", tdt)(grid.ref, ctypes.byref(a), ctypes.byref(r), form, _hip.dptr(pvar_), sigma2, damping, _hip.dptr(logz_),
                                                    _hip.dptr(change_), stream)

    refused = [("no u", call(d_u=None, d_res=None)), ("full stencil", call(half=0, d_A=p(full))), ("no A", call(d_A=None)), ("no cnt", call(d_cnt=None)),
               ("no b", call(d_b=None)), ("no stats", call(d_stats=None)), ("no err", call(d_err=None)), ("nout = 2", call(nout=2)),
               ("channels", call(channels=4)), ("mean_out", call(d_mean_out=p(mean))), ("guard", call(d_guard=p(guard), guard_expect=7)),
               ("zero region", call(z1=p(z1), n1_bytes=8)), ("shard", call(g_lo=0, g_hi=3)), ("owner workspace", call(d_bin=p(bin_ws), bin_bytes=bin_ws.numel())),
               ("sigma2 = 0", call(sigma2=0.0)), ("sigma2 < 0", call(sigma2=-1.0)), ("sigma2 = inf", call(sigma2=float("inf"))),
               ("sigma2 = nan", call(sigma2=float("nan"))), ("damping < 0", call(damping=-0.1)), ("damping > 1", call(damping=1.5)),
               ("damping = nan", call(damping=float("nan"))), ("form 0", call(form=0)), ("form 4", call(form=4)), ("no pvar", call(pvar_=None)),
               ("no logz_out", call(logz_=None)), ("no change_out", call(change_=None))]
    refused += [(f"ring without {k}", call(drop=k)) for k in ("d_x", "d_d0", "d_d1", "d_noise", "d_wa", "d_wb", "d_ytilde", "d_omega", "d_form")]
    torch.cuda.synchronize()
    assert [(what, rc) for what, rc in refused if rc != -1] == []
    assert all(float(v.abs().max()) == 0.0 for v in buf.values()) and float(full.abs().max()) == 0.0 and int(err.item()) == 0
    assert bool((logz == 7.0).all()) and bool((change == 7.0).all()) and bool(torch.isnan(mean).all()) and bool((z1 == 0x01010101).all())
    assert all(torch.equal(a, b) for a, b in zip(ring.tensors(), start.tensors()))
    # an empty ring: cap = 0 (whatever else the call holds), and a ring whose slots are all empty
    r0 = ring.ref()
    r0.cap = 0
    a = _hip.wiski_absorb_args(nout=1)
    assert _hip.fn("wiski_absorb_revisit", tdt)(grid.ref, ctypes.byref(a), ctypes.byref(r0), rv.INTERVAL, None, KS2, 1.0, None, None, stream) == 0
    empty = grid_ops.SiteRing(CAP, grid.d, tdt, DEV)
    assert call(ring_=empty) == 0
    torch.cuda.synchronize()
    assert all(float(v.abs().max()) == 0.0 for v in buf.values()) and bool((logz == 7.0).all()) and bool((change == 7.0).all())
    # the record runs and equals the flat entry
    assert call() == 0
    want, e2, ring2 = _buffers(grid, tdt), grid_ops.new_err_flag(DEV), _device_ring(c, tdt)
    lz2, ch2 = grid_ops.revisit_sites(grid, ring2, "interval", pvar, KS2, 1.0, want["b"], want["A"], want["cnt"], want["stats"], e2, u, res=want["res"])
    _compare(buf, {k: v.double().cpu().numpy() for k, v in want.items()}, dict(DTYPES)[tdt], KEYS, "record")
    assert torch.equal(ring.ytilde, ring2.ytilde) and torch.equal(ring.omega, ring2.omega)
    mine = torch.as_tensor(c["ring"]["form"] == rv.INTERVAL, device=DEV)
    assert torch.equal(change[mine], ch2[mine]) and bool((change[~mine] == 7.0).all()) and bool((logz[~mine] == 7.0).all())   # other forms' slots: not written
    assert call(d_res=None) == 0                                     # res is optional
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- the model
TB, TG, TELL, TOSC, TS2 = [[-0.15, 1.15]], [32], [0.25], 1.0, 0.05     # the toy of DESIGN.md 3.20
# The seed is fixed on the fp64 reference alone (ep_stream on this grid, seeds 0 - 9): at seed 1 all four streams of the regime tests
# -- censored and Poisson, one batch of 48 and four of 12 -- have a change list that does not increase after the first sweep and ends
# below 1e-6, and the RMSE ratio of the 128-point batch is 0.281.  (At seeds 3 - 5 the four-batch censored list of the reference
# itself zig-zags on its way down -- two modes of the parallel iteration with contraction factors of opposite sign.)
TSEED, TLIMIT, TEXPOSURE = 1, 0.6, 1.5
BASE = (np.array([[0.5]]), np.array([0.0]), np.array([1e6]))          # the one point that says nothing every toy model starts from
# measured on one MI355X, fp64 against ep_stream: relative to max |reference| (omega: to each omega)
MODEL_DEV = {"dense": dict(mean=4.279e-08, var=1.390e-07, ytilde=2.271e-08, omega=1.180e-07, log_z=1.096e-07, pair=2.554e-10),
             "matrix-free": dict(mean=4.279e-08, var=1.390e-07, ytilde=2.271e-08, omega=1.180e-07, log_z=1.096e-07, pair=2.554e-10)}


def _t(a, dtype=torch.float64):
    return torch.as_tensor(a, device=DEV, dtype=dtype)


def _toy_f(x):
    return np.sin(6.0 * x) + 0.5 * x


def _toy(n, kind="censored", seed=TSEED):
    """n points of sin 6x + x / 2 on [0, 1] at noise variance 0.05, readings above 0.6 censored (the others exact values) -- or Poisson
    counts at log rate sin 6x + x / 2 - 0.4 and exposure 1.5 -- as (form, X, d0, d1), and 50 queries."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, 1))
    Xs = np.linspace(0.02, 0.98, 50)[:, None]
    if kind == "censored":
        y = _toy_f(X[:, 0]) + np.sqrt(TS2) * rng.standard_normal(n)
        return rv.INTERVAL, X, np.where(y > TLIMIT, TLIMIT, y), np.where(y > TLIMIT, INF, y), Xs
    return rv.POISSON, X, rng.poisson(TEXPOSURE * np.exp(_toy_f(X[:, 0]) - 0.4)).astype(np.float64), np.full(n, TEXPOSURE), Xs


def _oracle():
    return dataspace.DataSpaceGP(TB, TG, "rbf", TELL, TOSC, TS2)


def _toy_model(**kw):
    from online_gp_amd.kernels import GridInterpolationKernel, RBFKernel, ScaleKernel
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    with torch.no_grad():
        k = GridInterpolationKernel(ScaleKernel(RBFKernel(ard_num_dims=1)), grid_size=TG, num_dims=1, grid_bounds=torch.tensor(TB))
        k.base_kernel.outputscale = TOSC
        k.base_kernel.base_kernel.lengthscale = torch.as_tensor(TELL)
        m = FixedNoiseOnlineSKIGP(_t(BASE[0]), _t(BASE[1])[:, None], _t(BASE[2])[:, None], covar_module=k, learn_additional_noise=True, **kw)
        m.likelihood.second_noise = TS2
    return m.eval()


def _give(m, form, X, d0, d1, inplace=True):
    if form == rv.INTERVAL:
        return m.condition_on_observations(_t(X), None, None, lower=_t(d0), upper=_t(d1), inplace=inplace)
    return m.condition_on_observations(_t(X), None, counts=_t(d0), exposure=_t(d1), inplace=inplace)


def _slices(n, q):
    return [slice(a, a + q) for a in range(0, n, q)]


_streams = {}


def _reference(kind, n, q, cap, sweeps, per_batch=0):
    key = (kind, n, q, cap, sweeps, per_batch)
    if key not in _streams:
        form, X, d0, d1, Xs = _toy(n, kind)
        S = rv.ep_stream(_oracle(), [(form, X[sl], d0[sl], d1[sl]) for sl in _slices(n, q)], cap, sweeps, sweeps_per_batch=per_batch, base=BASE)
        _streams[key] = (S, *S.marginals(Xs))
    return _streams[key]


def _posterior(m, Xs):
    with torch.no_grad():
        mvn = m(_t(Xs))
    return mvn.mean.double().cpu().numpy(), mvn.variance.double().cpu().numpy()


def _model_deviation(m, S, mean_r, var_r, Xs):
    mean, var = _posterior(m, Xs)
    yt, om, lz = (t.double().cpu().numpy() for t in m.last_refined_sites)
    t = np.isfinite(S.last["log_z"])
    assert np.array_equal(np.isnan(lz), ~t)                          # who was re-matched in the last sweep: exactly the reference's
    return dict(mean=float(np.abs(mean - mean_r).max() / np.abs(mean_r).max()), var=float(np.abs(var - var_r).max() / np.abs(var_r).max()),
                ytilde=float(np.abs(yt - S.ring["ytilde"]).max() / np.abs(S.ring["ytilde"]).max()),
                omega=float((np.abs(om - S.ring["omega"]) / S.ring["omega"]).max()),
                log_z=float((np.abs(lz - S.last["log_z"])[t] / np.abs(S.last["log_z"][t])).max()))


def _check_regime(regime, kind):
    """One batch of 48 followed by 15 sweeps, against four batches of 12 followed by the same: both against ep_stream, and the two
    posteriors with each other; the figures are printed before the asserts."""
    n, sweeps = 48, 15
    form, X, d0, d1, Xs = _toy(n, kind)
    out, bound = {}, {k: (None if v is None else 3.0 * v) for k, v in MODEL_DEV[regime].items()}
    for q in (48, 12):
        S, mean_r, var_r = _reference(kind, n, q, 64, sweeps)
        m = _toy_model(site_memory=64)
        before = None
        for sl in _slices(n, q):
            if q == 12 and sl.start == 36:                           # the last batch through the functional form
                before = ([t.clone() for t in m.stats_buffers()], m._kernel_cache["_site_ring"].clone(), m.num_data)
                child = _give(m, form, X[sl], d0[sl], d1[sl], inplace=False)
                ring = m._kernel_cache["_site_ring"]
                assert all(torch.equal(a, b) for a, b in zip(before[0], m.stats_buffers())) and m.num_data == before[2]
                assert all(torch.equal(a, b) for a, b in zip(before[1].tensors(), ring.tensors())) and (ring.head, ring.fill) == (36, 36)
                parent, m = m, child.eval()
            else:
                _give(m, form, X[sl], d0[sl], d1[sl])
        assert m.last_refined_sites is None and m._kernel_cache["_site_ring"].fill == n
        changes = m.refine_sites_(sweeps)
        if before is not None:                                       # the child's sweeps never reach the parent
            ring = parent._kernel_cache["_site_ring"]
            assert all(torch.equal(a, b) for a, b in zip(before[0], parent.stats_buffers())) and parent.num_data == before[2]
            assert all(torch.equal(a, b) for a, b in zip(before[1].tensors(), ring.tensors()))
        print(f"{regime} {kind} batches of {q}: changes {['%.1e' % c for c in changes]}  reference {['%.1e' % c for c in S.changes]}")
        dev = _model_deviation(m, S, mean_r, var_r, Xs)
        print(f"{regime} {kind} batches of {q}: " + "  ".join(f"{k} {v:.3e} (bound {bound[k]})" for k, v in dev.items()))
        out[q] = (m, dev, changes, S)
    pair = float(np.abs(_posterior(out[48][0], Xs)[0] - _posterior(out[12][0], Xs)[0]).max() / np.abs(_reference(kind, n, 48, 64, sweeps)[1]).max())
    print(f"{regime} {kind}: one batch against four, posterior mean {pair:.3e} (bound {bound['pair']})")
    for q, (m, dev, changes, S) in out.items():
        assert len(changes) == sweeps and all(b <= a for a, b in zip(changes[1:], changes[2:])) and changes[-1] < 1e-6
        assert m.num_data == S.num_data
        pts = m.site_memory_points()
        assert np.array_equal(pts["X"].cpu().numpy(), X) and np.array_equal(pts["d0"].cpu().numpy(), d0) and np.array_equal(pts["d1"].cpu().numpy(), d1)
        assert pts["form"] == [rv.FORM_NAMES[form]] * n and torch.equal(pts["ytilde"], m.last_refined_sites[0]) and torch.equal(pts["omega"], m.last_refined_sites[1])
        for k, v in dev.items():
            assert bound[k] is not None and v <= bound[k], (regime, kind, q, k, v, bound[k])
    assert bound["pair"] is not None and pair <= bound["pair"]
    return out[12][0]


@pytest.mark.parametrize("kind", ["censored", "poisson"])
def test_dense_regime_matches_ep_stream(kind):
    _check_regime("dense", kind)


@pytest.mark.parametrize("kind", ["censored", "poisson"])
def test_matrix_free_regime_matches_ep_stream(kind):
    from online_gp_amd import settings

    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(1e-12):
        m = _check_regime("matrix-free", kind)
        assert m._mean_state is not None                             # (the mean came from the PCG solve)


def test_tol_stops_the_sweeps_and_refine_after_update_is_the_same_as_calling_it():
    form, X, d0, d1, Xs = _toy(48)
    m = _toy_model(site_memory=64)
    _give(m, form, X, d0, d1)
    changes = m.refine_sites_(15, tol=1e-3)
    assert 3 <= len(changes) < 15 and changes[-1] <= 1e-3 and all(c > 1e-3 for c in changes[:-1])
    assert m.refine_sites_(0) == [] and _toy_model(site_memory=8).refine_sites_(3) == [0.0, 0.0, 0.0]
    # site_refine_sweeps = 2 with damping 0.8 behind every update, against the reference that does the same
    S, mean_r, var_r = _reference("censored", 48, 12, 64, 0, per_batch=2)
    S8 = rv.ep_stream(_oracle(), [(form, X[sl], d0[sl], d1[sl]) for sl in _slices(48, 12)], 64, 0, damping=0.8, sweeps_per_batch=2, base=BASE)
    auto = _toy_model(site_memory=64, site_refine_sweeps=2, site_refine_damping=0.8)
    for sl in _slices(48, 12):
        _give(auto, form, X[sl], d0[sl], d1[sl])
    e = float(np.abs(_posterior(auto, Xs)[0] - S8.marginals(Xs)[0]).max() / np.abs(mean_r).max())
    far = float(np.abs(S.marginals(Xs)[0] - S8.marginals(Xs)[0]).max() / np.abs(mean_r).max())
    bound = None if MODEL_DEV["dense"]["mean"] is None else 3.0 * MODEL_DEV["dense"]["mean"]
    print(f"site_refine_sweeps=2, damping 0.8: mean {e:.3e} (bound {bound}); undamped reference {far:.3e} away")
    assert bound is not None and e <= bound < far and auto.num_data == S8.num_data


def test_eviction_freezes_what_leaves_the_ring():
    """site_memory = 16 under three batches of 12: the ring holds the last 16 points with the sites they entered with, bit for bit; the
    sweeps revisit those alone, and the posterior is ep_stream's with a ring of 16 -- whose 20 evicted sites are frozen -- and not the
    one of a ring that holds all 36."""
    form, X, d0, d1, Xs = _toy(36)
    m = _toy_model(site_memory=16)
    adf = []
    for sl in _slices(36, 12):
        _give(m, form, X[sl], d0[sl], d1[sl])
        adf.append(tuple(t.clone() for t in m.last_interval_sites))
    pts = m.site_memory_points()
    yt, om = torch.cat([a[0] for a in adf])[20:], torch.cat([a[1] for a in adf])[20:]
    assert np.array_equal(pts["X"].cpu().numpy(), X[20:]) and torch.equal(pts["ytilde"], yt) and torch.equal(pts["omega"], om)
    ring = m._kernel_cache["_site_ring"]
    assert (ring.head, ring.fill, ring.cap) == (36 % 16, 16, 16)
    changes = m.refine_sites_(15)
    S, mean_r, var_r = _reference("censored", 36, 12, 16, 15)
    S_all, mean_all, _ = _reference("censored", 36, 12, 64, 15)
    mean, _ = _posterior(m, Xs)
    e, far = float(np.abs(mean - mean_r).max() / np.abs(mean_r).max()), float(np.abs(mean_all - mean_r).max() / np.abs(mean_r).max())
    bound = None if MODEL_DEV["dense"]["mean"] is None else 3.0 * MODEL_DEV["dense"]["mean"]
    print(f"eviction: mean {e:.3e} (bound {bound}); the ring of 64 lies {far:.3e} away; changes {['%.1e' % c for c in changes]}")
    assert np.array_equal(m.site_memory_points()["X"].cpu().numpy(), X[20:]) and m.last_refined_sites[0].shape == (16,)
    assert bound is not None and e <= bound < far and m.num_data == S.num_data == 37


def test_sweeps_pay_on_a_batch_matched_against_the_prior():
    """The censored toy absorbed as ONE batch of 128: every site is matched against the prior.  RMSE to the noise-free truth at 50
    queries after refine_sites_(10) is at most 0.6 x the RMSE before (asserted first on the fp64 reference: below 0.5 at this seed)."""
    form, X, d0, d1, Xs = _toy(128)
    truth = _toy_f(Xs[:, 0])
    rmse = lambda mean: float(np.sqrt(np.mean((mean - truth) ** 2)))
    r0, r10 = rmse(_reference("censored", 128, 128, 128, 0)[1]), rmse(_reference("censored", 128, 128, 128, 10)[1])
    print(f"reference RMSE: ADF {r0:.4f}  after 10 sweeps {r10:.4f}  ratio {r10 / r0:.3f}")
    assert r10 <= 0.5 * r0
    m = _toy_model(site_memory=128)
    _give(m, form, X, d0, d1)
    g0 = rmse(_posterior(m, Xs)[0])
    m.refine_sites_(10)
    g10 = rmse(_posterior(m, Xs)[0])
    print(f"model RMSE: ADF {g0:.4f}  after 10 sweeps {g10:.4f}  ratio {g10 / g0:.3f}")
    assert g10 <= 0.6 * g0


def test_default_model_never_enters_the_revisit_path(monkeypatch):
    """Without site_memory no ring is made, nothing is stored and the revisit launch is never made (the bindings are replaced by ones
    that raise); refine_sites_ and site_memory_points raise."""
    from online_gp_amd import grid_ops

    def forbidden(*a, **k):
        raise AssertionError("the site revisit was reached by a model built without site_memory")

    monkeypatch.setattr(grid_ops, "revisit_sites", forbidden)
    monkeypatch.setattr(grid_ops, "SiteRing", forbidden)
    form, X, d0, d1, Xs = _toy(48)
    m = _toy_model()
    for sl in _slices(48, 12):
        _give(m, form, X[sl], d0[sl], d1[sl])
    cform, cX, cy, ct, _ = _toy(12, "poisson")
    child = _give(m, cform, cX, cy, ct, inplace=False)
    assert "_site_ring" not in m._kernel_cache and "_site_ring" not in child._kernel_cache and m.last_refined_sites is None and m.site_memory is None
    for call in (lambda: m.refine_sites_(1), m.site_memory_points):
        with pytest.raises(RuntimeError, match="site_memory"):
            call()
    with pytest.raises(AssertionError):                             # (and the replacement is what a model with site memory would have called)
        _toy_model(site_memory=8)


def test_refusals_and_ring_lifetime():
    from online_gp_amd.distributed import ShardedStatsUpdater
    from online_gp_amd.models import OnlineSKIBotorchModel

    form, X, d0, d1, Xs = _toy(24)
    m = _toy_model(site_memory=32)
    _give(m, form, X[:12], d0[:12], d1[:12])
    before = [t.clone() for t in m.stats_buffers()]
    with pytest.raises(NotImplementedError, match="site_memory"):
        m.forget_(0.9)
    with pytest.raises(NotImplementedError, match="site_memory"):
        m.enter_stencil_shard(0, 2, None)
    with pytest.raises(NotImplementedError, match="site_memory"):
        m._absorb(m._kernel_cache, _t(X[:4]), _t(d0[:4]), None, init=False, half_delta=m._half_buffers())
    with pytest.raises(NotImplementedError):
        ShardedStatsUpdater(m).update(_t(X[:4]), None, None, lower=_t(d0[:4]), upper=_t(d1[:4]))
    for bad in (dict(sweeps=-1), dict(sweeps=1.5), dict(damping=-0.1), dict(damping=1.1)):
        with pytest.raises(ValueError):
            m.refine_sites_(**bad)
    assert all(torch.equal(a, b) for a, b in zip(before, m.stats_buffers())) and m._kernel_cache["_site_ring"].fill == 12
    # values take their usual path and are not stored; a handed-over cache must carry the ring
    m.condition_on_observations(_t(X[12:16]), _t(d0[12:16]), None, inplace=True)
    assert m._kernel_cache["_site_ring"].fill == 12 and m.num_data == 1 + 12 + 4
    with pytest.raises(ValueError, match="site"):
        type(m)(covar_module=m.covar_module, kernel_cache=_toy_model()._kernel_cache, likelihood=m.likelihood, learn_additional_noise=True, num_data=1, site_memory=32)
    # a batch larger than the ring: its last `site_memory` points are stored
    small = _toy_model(site_memory=8)
    _give(small, form, X, d0, d1)
    assert np.array_equal(small.site_memory_points()["X"].cpu().numpy(), X[16:]) and small.num_data == 25
    # growing the grid keeps the ring; dropping nodes, set_train_data and _clear_statistics empty it
    m.regrid_(2, 3)
    assert m._kernel_cache["_site_ring"].fill == 12 and len(m.refine_sites_(2)) == 2
    m.regrid_(-2, -3, drop="any")
    assert m._kernel_cache["_site_ring"].fill == 0 and m.refine_sites_(1) == [0.0]
    _give(m, form, X[:12], d0[:12], d1[:12])
    assert m._kernel_cache["_site_ring"].fill == 12
    m.set_train_data(_t(BASE[0]), _t(BASE[1])[:, None], _t(BASE[2])[:, None])
    assert m._kernel_cache["_site_ring"].fill == 0 and m.num_data == 1
    # stream_step takes its fallback, and the BoTorch-facing wrapper passes the keywords through
    m.stream_step(_t(X[:4]), _t(d0[:4])[:, None])
    assert m.num_data == 5 and m._kernel_cache["_site_ring"].fill == 0
    b = OnlineSKIBotorchModel(_t(BASE[0]), _t(BASE[1])[:, None], _t(BASE[2])[:, None], grid_bounds=torch.tensor(TB), grid_size=TG, site_memory=16,
                              site_refine_sweeps=1)
    b.eval()
    _give(b, form, X[:12], d0[:12], d1[:12])
    assert b.site_memory == 16 and b.last_refined_sites is not None and b.last_refined_sites[0].shape == (12,)
