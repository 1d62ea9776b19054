"""Plain reference of the fused hyper-parameter step (csrc/hyper_step.hip: wiski_hyper_columns, wiski_hyper_mid, wiski_hyper_adam),
numpy only: no torch, no project imports.

Every function takes the dtype `T` its arithmetic runs in.  With T = np.float64 it is the reference the kernels are held to; with
T = np.float32 the same lines are an emulation of the fp32 instantiation in the kernel's operation order (every intermediate rounded
to fp32, the few places where the kernel works in double and rounds once kept that way), which tests/test_hyper_step_host.py uses to
show that the fp32 bound below is neither loose nor tight.  What is stated here independently of the kernel: the constraint
transforms and their derivatives, the stationary profiles, the MLL tail as include/wiski.h documents it, torch.optim.Adam's update
(checked against torch.optim.Adam on the host), and the gradient w.r.t. sigma2, which is the hand derivative of
    L(s2) = -val(s2) / n + g_kap / s2,     val(s2) = -1/2 ( A / s2 + logdet + ld + n (log 2 pi + log s2) ),   A = c - b^T M b
with A, logdet and ld held fixed:   dL/ds2 = ( n / s2 - A / s2^2 ) / (2 n) - g_kap / s2^2.

Bounds (none taken from a kernel run).  Every output is a chain of fewer than 16 roundings and a few library calls (exp, log1p, pow,
sqrt) of a few ulp each, so an output with reference value ref is held to
    K eps max(|ref|, S),     K eps = 64 eps64 for the fp64 entry points, 8 eps32 for the fp32 ones,
S the largest operand of the expression that forms it (a sum that cancels is as accurate as its operands, not as its result):
  constrained value   S = |lower|
  column              S = scale (the lag-0 entry).  In an fp32 run the columns are fp64 functions of the fp32-rounded ell and scale, so an
                      error d of ell moves a column by scale |r phi'(r)| d: the bound is 8 eps32 scale max_r |r phi'(r)| with the maximum
                      (0.74 for RBF, below 0.6 for the Matern profiles) replaced by 1
  MLL tail            S = the largest term of the sum, with |c| and |bMb| in place of c - bMb
  raw gradient        S_g = |gv| for a softplus, |gv| (upper - lower) for a sigmoid, gv the gradient w.r.t. the constrained value: the
                      sigmoid's backward forms 1 - y, whose error is absolute, so a saturated sigmoid has the error of its largest factor;
                      for sigma2, |gv| is replaced by the largest of the three terms of dL/ds2 above, which may cancel
  exp_avg             S = max(S_g, |m|)
  exp_avg_sq          S = max((1 - beta2) S_g^2, |v|)
  raw                 S = max(|raw|, 1)
Where the reference saturates exactly (a sigmoid that is 0 or 1 in fp64) the value is a sum of rounded constants and must be equal
bit for bit to the emulation in the kernel's dtype."""
import numpy as np

F64, F32 = np.float64, np.float32
EPS = {F64: float(np.finfo(np.float64).eps), F32: float(np.finfo(np.float32).eps)}
K = {F64: 64.0, F32: 8.0}
LOG_2PI = 1.8378770664093453


def keps(T):
    return K[T] * EPS[T]


def f32r(x):
    """x rounded to fp32, as fp64 (inputs every dtype starts from)."""
    return np.asarray(x, F32).astype(F64)


# ------------------------------------------------------------------------------------------------------------------ constraints
def transform(kind, lower, upper, raw, T=F64, mutant=None):
    raw = np.asarray(raw, T)
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == 0:
            sp = np.log1p(np.exp(raw))
            if mutant != "softplus_without_threshold":
                sp = np.where(raw > T(20), raw, sp)
            return (sp + T(lower)).astype(T)
        sg = T(1) / (T(1) + np.exp(-raw))
        return (T(lower) + T(upper - lower) * sg).astype(T)


def backward(kind, lower, upper, raw, g, T=F64, mutant=None):
    raw, g = np.asarray(raw, T), np.asarray(g, T)
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == 0:
            z = np.exp(raw)
            out = g * z / (z + T(1))
            if mutant != "softplus_without_threshold":
                out = np.where(raw > T(20), g, out)
            return out.astype(T)
        y = T(1) / (T(1) + np.exp(-raw))
        w = T(1) if mutant == "sigmoid_backward_without_range" else T(upper - lower)
        return (((g * w) * (T(1) - y)) * y).astype(T)


def saturated(kind, raw):
    """Elements at which the fp64 sigmoid is exactly 0 or 1."""
    raw = np.asarray(raw, F64)
    if kind == 0:
        return np.zeros(raw.shape, bool)
    with np.errstate(over="ignore"):
        sg = 1.0 / (1.0 + np.exp(-raw))
    return (sg == 0.0) | (sg == 1.0)


# ---------------------------------------------------------------------------------------------------------------------- columns
def profile(kind, r):
    r = np.asarray(r, F64)
    if kind == 0:
        return np.exp(-0.5 * r * r)
    if kind == 1:
        return np.exp(-r)
    if kind == 2:
        s = np.sqrt(3.0) * r
        return (1.0 + s) * np.exp(-s)
    s = np.sqrt(5.0) * r
    return (1.0 + s + s * s / 3.0) * np.exp(-s)


def columns(kind, g, h, ell, scale):
    """The concatenated Toeplitz columns scale phi(h_q l / ell_q), l = 0 .. g_q - 1, in fp64 (as the kernel forms them in every dtype)."""
    ell = np.asarray(ell, F64).reshape(-1)
    if ell.size == 1:
        ell = np.repeat(ell, len(g))
    return np.concatenate([float(scale) * profile(kind, (float(h[q]) * np.arange(g[q], dtype=F64)) / ell[q]) for q in range(len(g))])


def constrained(records, T=F64, mutant=None):
    """(ell [numel], scale or None, s2) of a plan: the product of the role-1 factors in plan order, in T."""
    ell = scale = s2 = None
    for r in records:
        v = transform(r["kind"], r["lower"], r["upper"], r["raw"], T, mutant)
        if r["role"] == 0:
            ell = v
        elif r["role"] == 1:
            scale = v[0] if scale is None else T(scale * v[0])
        else:
            s2 = v[0]
    return ell, scale, s2


# --------------------------------------------------------------------------------------------------------------------- MLL tail
def mid(bMb, logdet, s2, c, ld, n):
    """out [9] = {val, 1/2 / s2, -1/2, c - bMb, g = -1/n, g / (2 s2), -g / 2, loss = -val / n, 1 / s2} and the largest operand of each."""
    bMb, s2, c, ld, n = float(bMb), float(s2), float(c), float(ld), float(n)
    lg = 0.0 if logdet is None else float(logdet)
    A = c - bMb
    tail = n * (LOG_2PI + np.log(s2))
    val = -0.5 * (A / s2 + lg + ld + tail)
    g = -1.0 / n
    out = np.array([val, 0.5 / s2, -0.5, A, g, g * (0.5 / s2), g * -0.5, -val / n, 1.0 / s2])
    s_a = max(abs(c), abs(bMb))
    s_val = max(s_a / s2, abs(lg), abs(ld), abs(n * LOG_2PI), abs(n * np.log(s2)))
    S = np.array([s_val, 0, 0, s_a, 0, 0, 0, s_val / n, 0])
    return out, S


def sigma2_grad(A, s2, g_kap, n):
    """d/ds2 of -val(s2) / n + g_kap / s2 (module docstring), A = c - bMb held fixed."""
    return (n / s2 - A / (s2 * s2)) / (2.0 * n) - g_kap / (s2 * s2)


# ------------------------------------------------------------------------------------------------------------------------- Adam
def adam_step(plan_state, scale, s2, g_ell, g_scale, mid, g_kap, n, lr, b1, b2, eps, T=F64, mutant=None):
    """One torch.optim.Adam step (no weight decay, no amsgrad) of every record of plan_state after the chain rule to its raw values.
    Records: dict(role, kind, lower, upper, raw[], m[], v[], step[] (fp32 counters), step_numel).  Returns one dict per record with the
    new raw, m, v, step and the operand sizes (S_m, S_v, S_raw) of the bounds.  The constants as the framework's fused kernel forms
    them: 1 - beta and beta^step in double, then rounded to T; the moment update is m + (1 - beta1)(g - m)."""
    out = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for r in plan_state:
            raw, m, v = (np.asarray(r[k], T) for k in ("raw", "m", "v"))
            val = transform(r["kind"], r["lower"], r["upper"], raw, T, mutant)
            if r["role"] == 0:
                gv = np.asarray(g_ell, T)
            elif r["role"] == 1:
                gv = T(g_scale) * T(scale) if mutant == "scale_grad_without_division" else T(g_scale) * (T(scale) / val)
            else:
                s2d = float(T(s2))                                   # fp64 arithmetic on the T-rounded sigma2, one rounding to T
                gk = 0.0 if mutant == "sigma2_grad_without_kappa_term" else float(g_kap)
                gv = np.full(1, sigma2_grad(float(mid[3]), s2d, gk, float(n)))
            gv = np.asarray(gv, T).reshape(raw.shape)
            grad = backward(r["kind"], r["lower"], r["upper"], raw, gv, T, mutant)
            cnt = np.asarray(r["step"], F32)
            assert cnt.size == r["step_numel"] and r["step_numel"] in (1, raw.size)
            idx = np.arange(raw.size) if (cnt.size == raw.size and mutant != "shared_step_for_all_elements") else np.zeros(raw.size, int)
            step = (cnt[idx] + F32(1)).astype(F64)
            used = step - 1.0 if mutant == "step_off_by_one" else step
            omb1 = T(1.0 - b1)
            omb2 = T(1.0 - float(F32(b2))) if mutant == "one_minus_beta_in_fp32" else T(1.0 - b2)
            mn = m + omb1 * (grad - m)
            vn = T(b2) * v + omb2 * grad * grad
            bc1 = np.ones(raw.size, T) if mutant == "no_bias_correction_1" else (1.0 - np.power(float(b1), used)).astype(T)
            bc2 = np.ones(raw.size, T) if mutant == "no_bias_correction_2" else (1.0 - np.power(float(b2), used)).astype(T)
            step_size = T(lr) / bc1
            if mutant == "eps_inside_root":
                denom = np.sqrt(vn + T(eps)) / np.sqrt(bc2)
            elif mutant == "eps_before_bias_division":
                denom = (np.sqrt(vn) + T(eps)) / np.sqrt(bc2)
            else:
                denom = np.sqrt(vn) / np.sqrt(bc2) + T(eps)
            new = raw - step_size * (mn / denom)
            s_gv = np.abs(gv.astype(F64))
            if r["role"] == 2:                                       # the terms of sigma2_grad, which may cancel
                s_gv = np.maximum(s_gv, max(abs(float(mid[3])) / (s2d * s2d) / (2.0 * n), 0.5 / s2d, abs(float(g_kap)) / (s2d * s2d)))
            s_g = s_gv * (abs(r["upper"] - r["lower"]) if r["kind"] == 1 else 1.0)
            out.append({"raw": new.astype(T), "m": mn.astype(T), "v": vn.astype(T), "step": cnt + F32(1),
                        "S_m": np.maximum(s_g, np.abs(m.astype(F64))), "S_v": np.maximum((1.0 - b2) * s_g * s_g, np.abs(v.astype(F64))),
                        "S_raw": np.maximum(np.abs(raw.astype(F64)), 1.0)})
    return out


_MUTANT_NAMES = ["eps_inside_root", "eps_before_bias_division", "no_bias_correction_1", "no_bias_correction_2", "step_off_by_one",
                 "one_minus_beta_in_fp32", "shared_step_for_all_elements", "scale_grad_without_division", "sigma2_grad_without_kappa_term",
                 "softplus_without_threshold", "sigmoid_backward_without_range"]


def _mutant(name):
    def step(*a, **kw):
        return adam_step(*a, mutant=name, **kw)

    return step


# wrong variants of adam_step (same signature), for tests/test_hyper_step_host.py only: a case table that does not tell each of them from
# the reference would not tell a kernel with that defect from a correct one either
MUTANTS = {name: _mutant(name) for name in _MUTANT_NAMES}


def ratios(got, ref, S, T):
    """|got - ref| / (K eps max(|ref|, S)) per element; a non-finite difference counts as infinite."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    err = np.where(got == ref, 0.0, err)
    return err / (keps(T) * np.maximum(np.abs(ref), S))


def step_ratios(got, ref, T):
    """Worst ratio to the bound of raw, m and v over the records of one step (got, ref: adam_step's lists; ref carries the S)."""
    worst = {"raw": 0.0, "m": 0.0, "v": 0.0}
    for a, b in zip(got, ref):
        for k in worst:
            worst[k] = max(worst[k], float(np.max(ratios(a[k], b[k], b["S_" + k], T))))
    return worst


# ------------------------------------------------------------------------------------------------------------------- case tables
def _rec(role, kind, raw, lower=0.0, upper=0.0, m=None, v=None, step=(0,), step_numel=None):
    raw = f32r(np.atleast_1d(raw))
    z = np.zeros(raw.size)
    step = np.asarray(step, F32)
    return {"role": role, "kind": kind, "lower": float(lower), "upper": float(upper), "raw": raw, "m": z.copy() if m is None else f32r(np.atleast_1d(m)),
            "v": z.copy() if v is None else f32r(np.atleast_1d(v)), "step": step, "step_numel": step.size if step_numel is None else step_numel}


LO, HI = 1e-4, 12.0          # the interval of the sigmoid-constrained entries; the softplus noise has the likelihood's lower bound LO


def _adam_plan(ell_raw=(0.3, -1.2, 2.0), sa_raw=0.7, sb_raw=-0.4, noise_raw=-2.0, ell_kind=0, warm=None, steps=None):
    """ARD lengthscales (numel 3), a softplus and an interval scale factor, a softplus noise."""
    recs = [_rec(1, 0, sa_raw), _rec(1, 1, sb_raw, LO, HI), _rec(0, ell_kind, ell_raw, *((LO, HI) if ell_kind else (0.0, 0.0))), _rec(2, 0, noise_raw, LO)]
    if warm is not None:
        rng = np.random.default_rng(warm)
        for r in recs:
            r["m"] = f32r(rng.uniform(-0.5, 0.5, r["raw"].size))
            r["v"] = f32r(rng.uniform(0.01, 0.3, r["raw"].size))
    if steps is not None:
        for r, s in zip(recs, steps):
            r["step"] = np.asarray(s, F32)
            r["step_numel"] = r["step"].size
    return recs


def _adam_case(name, recs, g_ell, g_scale, gv_s2=None, A=37.5, n=600.0, g_kap=-0.21, lr=0.01, b1=0.9, b2=0.999, eps=1e-8):
    """scale and s2 as wiski_hyper_columns would hand them over (fp32-representable, so that both dtypes start from the same numbers);
    gv_s2 != None: A and g_kap chosen so that the gradient w.r.t. sigma2 is gv_s2 (A = n s2 cancels the MLL's own part exactly)."""
    _, scale, s2 = constrained(recs, F32)
    scale, s2 = float(scale), float(s2)
    if gv_s2 is not None:
        A, g_kap = n * s2, -gv_s2 * s2 * s2
    m9, _ = mid(0.0, None, s2, A, 11.0, n)
    return {"name": name, "records": recs, "scale": scale, "s2": s2, "g_ell": f32r(g_ell), "g_scale": float(f32r(g_scale)), "mid": m9, "g_kap": float(g_kap),
            "n": float(n), "lr": lr, "b1": b1, "b2": b2, "eps": eps}


ADAM_CASES = [
    _adam_case("zero_state_step0", _adam_plan(), [0.8, -1.7, 0.35], -0.6),
    _adam_case("zero_state_step0_grad1e-7", _adam_plan(), [1e-7, -1e-7, 1e-7], 1e-7, gv_s2=1e-7, lr=0.05),
    _adam_case("warm_step3", _adam_plan(warm=3, steps=[[3], [3], [3], [3]]), [0.8, -1.7, 0.35], -0.6, lr=0.05),
    _adam_case("warm_step99_grad1e-7", _adam_plan(warm=4, steps=[[99], [99], [99], [99]]), [1e-7, -1e-7, 1e-7], 1e-7, gv_s2=-1e-7),
    _adam_case("softplus_above_threshold_step1000", _adam_plan(ell_raw=(25.0, 20.0, 100.0), sa_raw=25.0, noise_raw=25.0, warm=5,
                                                                 steps=[[1000], [1000], [1000], [1000]]), [0.8, -1.7, 0.35], -0.6, n=21743.0),
    _adam_case("saturated_sigmoid", _adam_plan(ell_raw=(-30.0, 30.0, 2.0), sb_raw=30.0, ell_kind=1), [0.8, -0.9, 0.35], -0.6),
    _adam_case("per_element_steps", _adam_plan(warm=6, steps=[[7], [7], [0, 4, 99], [7]]), [0.8, -1.7, 0.35], -0.6, lr=0.05),
    _adam_case("shared_step", _adam_plan(warm=6, steps=[[7], [7], [4], [7]]), [0.8, -1.7, 0.35], -0.6, lr=0.05),
]

KINDS = (0, 1, 2, 3)         # RBF, Matern 1/2, 3/2, 5/2
SOFTPLUS_RAWS = (-30.0, -5.0, 0.3, 19.999, 20.0, 20.001, 40.0, 100.0)
INTERVAL_RAWS = (-100.0, -30.0, -2.0, 0.0, 3.0, 30.0, 100.0)
_G4 = ((5, 7, 64, 9), (0.11, 0.07, 0.013, 0.2))
_G2 = ((257, 3), (0.004, 0.9))
_G1 = ((300,), (0.0075,))


def _col_case(name, grid, recs):
    return {"name": name, "g": grid[0], "h": tuple(float(x) for x in f32r(grid[1])), "records": recs}


# between them: every raw value of SOFTPLUS_RAWS and INTERVAL_RAWS, ARD and broadcast lengthscales, 0 / 1 / 2 scale factors of both kinds,
# the three grids (g = 300 and 257: the 256-thread stride loop), unequal h
COLUMN_CASES = [
    _col_case("d4_ard_two_scales", _G4, [_rec(1, 0, 20.001), _rec(0, 0, (-5.0, 0.3, 19.999, 20.0)), _rec(1, 1, 3.0, LO, HI), _rec(2, 0, -30.0, LO)]),
    _col_case("d4_iso_one_scale", _G4, [_rec(1, 1, -2.0, LO, HI), _rec(0, 0, 0.3), _rec(2, 1, 0.0, LO, HI)]),
    _col_case("d2_ard_no_scale", _G2, [_rec(0, 1, (0.0, 30.0), LO, HI), _rec(2, 0, 40.0, LO)]),
    _col_case("d1_two_scales_saturated", _G1, [_rec(1, 1, -100.0, LO, HI), _rec(1, 0, -30.0, LO), _rec(2, 1, 100.0, LO, HI), _rec(0, 0, 100.0)]),
    _col_case("d1_big_scales", _G1, [_rec(2, 1, -30.0, LO, HI), _rec(0, 1, -2.0, LO, HI), _rec(1, 0, 100.0), _rec(1, 0, 40.0), _rec(1, 0, -5.0, LO)]),
]

MID_N = (1.0, 600.0, 21743.0)
MID_S2 = tuple(float(x) for x in f32r((1e-4, 0.3, 7.0)))
MID_INPUTS = {"bMb": 412.625, "logdet": -93.4375, "c": 431.0, "ld": 57.8125}

TRAJECTORY_STEPS = 5


def trajectory_inputs(step):
    """Fresh synthetic gradients and statistics of trajectory step `step` (fp32-representable)."""
    rng = np.random.default_rng(100 + step)
    return {"g_ell": f32r(rng.uniform(-2, 2, 3)), "g_scale": float(f32r(rng.uniform(-1, 1))), "g_kap": float(f32r(rng.uniform(-0.5, 0.5))),
            "bMb": float(f32r(rng.uniform(300, 400))), "c": float(f32r(rng.uniform(400, 500))), "ld": float(f32r(rng.uniform(-50, 50))), "n": 600.0 + 32 * step}


def trajectory_reference(T=F64, lr=0.05, b1=0.9, b2=0.999, eps=1e-8):
    """TRAJECTORY_STEPS times constrained -> mid -> adam_step from the zero state of _adam_plan(); the state after each step."""
    recs = _adam_plan()
    states = []
    for t in range(TRAJECTORY_STEPS):
        x = trajectory_inputs(t)
        _, scale, s2 = constrained(recs, T)
        m9, _ = mid(x["bMb"], None, float(s2), x["c"], x["ld"], x["n"])
        new = adam_step(recs, scale, s2, x["g_ell"], x["g_scale"], m9, x["g_kap"], x["n"], lr, b1, b2, eps, T)
        recs = [dict(r, raw=u["raw"], m=u["m"], v=u["v"], step=u["step"]) for r, u in zip(recs, new)]
        states.append(new)
    return states
