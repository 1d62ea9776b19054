"""Plain reference of the query-and-tail side of the spectral factor (csrc/spectral_basis.hip: wiski_spectral_evaluate, wiski_spectral_evaluate_y,
wiski_spectral_var, wiski_factor_tail, wiski_woodbury_c, wiski_mll_weights, wiski_basis_absorb_h), numpy only: no torch, no project imports.

Every operation is stated as include/wiski.h documents it and evaluated in np.longdouble (`A`, the accumulation type; 64-bit mantissa on x86).
It returns the value and a per-element bound.  evaluate() takes the data dtype `T`: with T = float64 it is the reference; with T = float32 the
same lines emulate the fp32 instantiation's documented rounding places (mean and latent variance rounded to fp32, then df, v, s and the nll
term formed in fp32; the reductions over the queries stay in double).  With A = float64 every function is a plain double-precision
evaluation in numpy's own order, which tests/test_spectral_eval_host.py uses to show that the bounds are not too tight.

Evaluate:  mean_j = F_j . t,  dg_j = sum_i (sum_{k <= i} Linv[i, k] F[j, k])^2,  tail_j = max(prior_j kscale - |F_j|^2, 0),
var_j = max((dg_j + tail_j) s2, 0) (the latent variance),  v_j = var_j + s2,  rmse = sqrt(mean_j (mean_j - y_j)^2),
nll = mean_j 1/2 ((mean_j - y_j)^2 / v_j + log v_j + log 2 pi),  out = {rmse, nll, flag, max_j |mean_j|}.

Bounds (none taken from a kernel run; e = eps64 = 2^-52, e32 = 2^-23, K = 8 as in hyper_step_reference).
  sums       A sum of L products, accumulated in any order, is held to (L + 2) e sum |terms|; the sums of absolute values are formed here.
             Y = Linv F^T has L = r terms per entry (the matrix product does not know the triangle; the zero terms add nothing to sum |terms|):
             dY_ij = (r + 2) e sum_k |Linv_ik F_jk|.
  stages     A later stage carries the earlier one's bound through its own absolute-value matrix and adds its own rounding:
             d dg_j   = sum_i (2 |Y_ij| dY_ij + dY_ij^2) + (r + 2) e dg_j              (a Y handed in from outside brings its own dY)
             d mean_j = (r + 2) e sum_k |F_jk t_k|
             d tail_j = (r + 2) e |F_j|^2 + 2 e max(|prior_j kscale|, |F_j|^2)         (the clamp is 1-Lipschitz)
             d var_j  = |s2| (d dg_j + d tail_j) + 2 e |(dg_j + tail_j) s2|             (the clamp is 1-Lipschitz)
             factor_tail:  d hr = (r_ref + 2) e |TS|^T |h_ref|;  d v = sq d hr + e |v|;  d c = |Linv| d v + (r + 2) e |Linv| |v|;
             d t = |Linv|^T d c + (r + 2) e |Linv|^T |c|;  d coef = sq d t + e |coef|;  d zeta = d t / sq + e |zeta|;
             d bMb = sum (2 |c| d c + d c^2) + (r + 2) e bMb;  d logdet = 2 (r + 6) e sum |log chol_ii|  (a library log of 4 ulp).
  fp32       Each documented rounding to fp32 adds K e32 max(|value|, largest operand) + 2^-149 (the smallest fp32 subnormal: a value
             that underflows loses all of itself):  mean <- mean,  var <- var,  df <- max(|df|, |mean|, |y|),  s <- s,  v <- v,
             nll term <- max(|term|, s / v, |log v|, log 2 pi).  In fp64 the same places carry K e (a chain of fewer than 8 roundings and one log).
  metrics    with df = mean - y, s = df^2, v = var + s2, term = 1/2 (s / v + log v + log 2 pi), the partial derivatives at the reference:
             d df = d mean + rounding;  d s = 2 |df| d df + (d df)^2 + rounding  (the second-order term of the square);  d v = d var + rounding;
             d term = 1/2 (d s / v + (s / v^2 + 1 / |v|) d v) + rounding;
             S = mean_j s_j:  d S = mean_j d s_j + (n + 2) e S;   d rmse = min(d S / sqrt(S), sqrt(d S)) + 2 e rmse   (|sqrt a - sqrt b| <=
             |a - b| / (sqrt a + sqrt b) and <= sqrt |a - b|);   d nll = mean_j d term_j + (n + 2) e mean_j |term_j|.
             max_j |mean_j| is formed from the unrounded means in both instantiations: d = max_j of the fp64 d mean_j.  The flag is exact.
  element-wise   wiski_woodbury_c and the entries of wiski_mll_weights are chains of fewer than 8 roundings: K e max(|value|, largest operand);
             g_kap = sum_i Wt_ii lam_i is held to the bound of its r-term sum, (r + 2) e sum |Wt_ii lam_i| + sum d Wt_ii |lam_i|.
  absorb_h   h_j + sum_p F_pj t_p, t_p = wby_p / scale_p (one rounding): (n + 4) e (|h_j| + sum_p |F_pj t_p|), plain or atomic.
Where the reference itself is not finite (log of a negative v: the case with s2 < 0 that tells a clamped variance from an unclamped one) the
kernel must give the same non-finite value; a non-finite difference anywhere else counts as infinite.

Seeded defects: every function takes `mutant=`; MUTANTS names, for each, the case of the tables below at which it must exceed the bound at
least four times.  A case table that does not tell a defect from the reference would not tell a kernel with that defect from a correct one."""
import functools

import numpy as np

F64, F32, LD = np.float64, np.float32, np.longdouble
E64, E32 = float(np.finfo(np.float64).eps), float(np.finfo(np.float32).eps)
TINY32 = 2.0 ** -149
K = 8.0
LOG_2PI = 1.8378770664093453
LOG_2PI_LD = np.log(2 * np.pi * LD(1))
SENT = -777.25
KSCALE = 0.5            # a power of two: prior * kscale is exact, so that a tail can be made exactly zero
S2 = float(F32(0.3))


def f32r(x):
    """x rounded to fp32, as fp64 (inputs every dtype starts from)."""
    return np.asarray(x, F32).astype(F64)


def _keps(T):
    return K * (E32 if T is F32 else E64)


def _round_bound(T, *sizes):
    """Bound of one documented rounding place: K eps_T max(sizes) (+ the fp32 subnormal)."""
    m = functools.reduce(np.maximum, [np.abs(np.asarray(s, F64)) for s in sizes])
    return _keps(T) * m + (TINY32 if T is F32 else 0.0)


def ratios(got, ref, bound):
    """|got - ref| / bound per element; equal values (and equal non-finite ones) count 0, any other non-finite difference infinite."""
    got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(bound, F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        same = (got == ref) | (np.isnan(got) & np.isnan(ref))
        err = np.where(np.isfinite(err), err, np.inf)
        out = np.where(same, 0.0, err / bound)
    return np.where(np.isnan(out), np.inf, out)


# --------------------------------------------------------------------------------------------------------------------- evaluate
def solve_rows(Linv, F, A=LD, mutant=None):
    """Y = tril(Linv) F^T [r, n] and its bound dY (module docstring).  Linv: [r, ldl >= r], only [:, :r] is read."""
    r = F.shape[1]
    L = np.asarray(Linv, A)[:, :r]
    if mutant != "upper_triangle_included":
        L = np.tril(L)
    if mutant == "row_chunk_512_dropped":
        L = L.copy()
        L[:, 512:] = 0
    Ft = np.asarray(F, A).T
    return L @ Ft, ((r + 2) * E64 * (np.abs(L) @ np.abs(Ft))).astype(F64)


def evaluate(F, prior, Linv, t, kscale, s2, y, err=None, T=F64, A=LD, mutant=None, Y=None, dY=None, carry=None):
    """The evaluate of n queries (module docstring).  Y / dY: chol^-1 F^T handed in from outside with its own error bound (None: formed here
    from Linv); carry: what a call that did not reset the workspace left in the dg accumulators (mutant workspace_not_reset).
    Returns dict(out [4], mean [n], var [n], dg [n], tail [n]) and the same keys with prefix d_ for the bounds; all fp64."""
    F, prior, t, y = (np.asarray(a, F64) for a in (F, prior, t, y))
    n, r = F.shape
    s2 = float(s2)
    if Y is None:
        Yv, dYv = solve_rows(Linv, F, A, mutant)
    else:
        Yv, dYv = np.asarray(Y, A), (np.zeros((r, n)) if dY is None else np.asarray(dY, F64))
    Fa, ta = F.astype(A), t.astype(A)
    dg = (Yv * Yv).sum(0)
    if mutant == "last_n_mod_8_missing_from_dg":
        dg[8 * (n // 8):] = 0
    if mutant == "workspace_not_reset":
        m = min(n, len(carry))
        dg[:m] += np.asarray(carry, A)[:m]
    absY = np.abs(Yv).astype(F64)
    d_dg = (2 * absY * dYv + dYv * dYv).sum(0) + (r + 2) * E64 * dg.astype(F64)
    mean = Fa @ ta
    d_mean = (r + 2) * E64 * (np.abs(F) @ np.abs(t))
    cap = (Fa * Fa).sum(1)
    p = prior.astype(A) * (A(1) if mutant == "kscale_not_applied" else A(kscale))
    tail = p - cap
    if mutant != "tail_not_clamped":
        tail = np.maximum(tail, 0)
    d_tail = (r + 2) * E64 * cap.astype(F64) + 2 * E64 * np.maximum(np.abs(p), cap).astype(F64)
    var_pre = (dg + tail) * A(s2)
    d_var = abs(s2) * (d_dg + d_tail) + 2 * E64 * np.abs(var_pre).astype(F64)
    clamp = (lambda x: x) if mutant == "var_not_clamped" else (lambda x: np.maximum(x, 0))
    d_mean64 = d_mean.copy()
    W = A if T is F64 else F32                       # the type the metrics are formed in
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        if mutant == "f32_var_rounded_after_s2":     # v = round(var + s2) in one rounding, the latent variance recovered from it
            v_w = (clamp(var_pre) + A(s2)).astype(F64).astype(W)
            var_w = (v_w - W(s2)).astype(W)
        else:
            var_w = clamp(var_pre.astype(F64).astype(W) if T is F32 else var_pre)
            v_w = ((var_w.astype(F64) + s2).astype(W) if T is F32 else var_w + A(s2))
        if mutant == "s2_not_added_in_v":
            v_w = var_w
        mean_w = mean.astype(F64).astype(W) if T is F32 else mean
        df = mean_w - y.astype(W)
        s = df * df
        lg = np.log(v_w.astype(F64)).astype(W) if T is F32 else np.log(v_w)
        c2pi = W(0) if mutant == "log_2pi_missing" else (W(LOG_2PI) if T is F32 else LOG_2PI_LD)
        term = W(0.5) * (s / v_w + lg + c2pi)
        # bounds of the documented places, at the reference values
        dfr, sr, vr = (a.astype(F64) for a in (df, s, v_w))
        d_mean = d_mean + _round_bound(T, mean)
        d_var = d_var + _round_bound(T, var_w)
        d_df = d_mean + _round_bound(T, dfr, mean, y)
        d_s = 2 * np.abs(dfr) * d_df + d_df * d_df + _round_bound(T, sr)
        d_v = d_var + _round_bound(T, vr)
        d_term = 0.5 * (d_s / np.abs(vr) + (sr / (vr * vr) + 1 / np.abs(vr)) * d_v) + _round_bound(T, term, sr / vr, lg, LOG_2PI)
        acc = A if A is LD else F64                  # the reductions over the queries: double in both instantiations
        S = s.astype(acc).sum() / (64 if mutant == "rmse_divided_by_64" else n)
        rmse = np.sqrt(S)
        nll = term.astype(acc).sum() / n
        d_S = d_s.sum() / n + (n + 2) * E64 * float(S)
        d_rmse = (min(d_S / float(rmse), np.sqrt(d_S)) if float(rmse) > 0 else np.sqrt(d_S)) + 2 * E64 * float(rmse)
        d_nll = d_term.sum() / n + (n + 2) * E64 * float(np.abs(term.astype(F64)).sum()) / n
    mx = mean.max() if mutant == "max_of_signed_means" else np.abs(mean).max()
    flag = 0.0 if err is None else float(err)
    return {"out": np.array([rmse, nll, flag, mx], F64), "d_out": np.array([d_rmse, d_nll, 0.0, d_mean64.max()], F64),
            "mean": mean_w.astype(F64), "d_mean": d_mean, "var": var_w.astype(F64), "d_var": d_var,
            "dg": dg.astype(F64), "d_dg": d_dg, "tail": tail.astype(F64), "d_tail": d_tail, "Y": Yv.astype(F64), "dY": dYv}


def spectral_var(Y, F, prior, kscale, A=LD, mutant=None):
    """(diag, tail) and their bounds: diag_j = |Y[:, j]|^2, tail_j = max(prior_j kscale - |F_j|^2, 0)."""
    Yv, Fa = np.asarray(Y, A), np.asarray(F, A)
    r = Fa.shape[1]
    if mutant == "spectral_var_rows_3_mod_4_dropped":
        Yv = Yv.copy()
        Yv[3::4] = 0
    diag = (Yv * Yv).sum(0)
    cap = (Fa * Fa).sum(1)
    p = np.asarray(prior, A) * A(kscale)
    tail = np.maximum(p - cap, 0)
    d_tail = (r + 2) * E64 * cap.astype(F64) + 2 * E64 * np.maximum(np.abs(p), cap).astype(F64)
    return {"diag": diag.astype(F64), "d_diag": (r + 2) * E64 * diag.astype(F64), "tail": tail.astype(F64), "d_tail": d_tail}


# ------------------------------------------------------------------------------------------------------------------ factor tail
def factor_tail(TS, h_ref, sq, Linv, chol, A=LD, mutant=None):
    """hr, c, t, coef, zeta [r], bMb, logdet from TS [r_ref, r], h_ref [r_ref], sq [r], Linv (lower triangular), chol [r, r]; bounds d_*."""
    TSa, ha, sqa = np.asarray(TS, A), np.asarray(h_ref, A), np.asarray(sq, A)
    r_ref, r = TSa.shape
    L = np.tril(np.asarray(Linv, A))
    aL = np.abs(L).astype(F64)
    sqf = sqa.astype(F64)
    hr = TSa.T @ ha
    if mutant == "tail_last_column_tile_dropped":
        hr[16 * (r // 16):] = 0
    d_hr = (r_ref + 2) * E64 * (np.abs(TSa).T @ np.abs(ha)).astype(F64)
    v = sqa * hr
    d_v = sqf * d_hr + E64 * np.abs(v).astype(F64)
    c = L @ v
    d_c = aL @ d_v + (r + 2) * E64 * (aL @ np.abs(v).astype(F64))
    t = L.T @ c
    d_t = aL.T @ d_c + (r + 2) * E64 * (aL.T @ np.abs(c).astype(F64))
    coef, zeta = sqa * t, t / sqa
    d_coef = sqf * d_t + E64 * np.abs(coef).astype(F64)
    d_zeta = d_t / sqf + E64 * np.abs(zeta).astype(F64)
    if mutant == "tail_coef_zeta_swapped":
        coef, zeta = zeta, coef
    bMb = (c * c).sum()
    ac = np.abs(c).astype(F64)
    d_bMb = (2 * ac * d_c + d_c * d_c).sum() + (r + 2) * E64 * float(bMb)
    lg = np.log(np.diagonal(np.asarray(chol, A)))
    logdet = (1 if mutant == "tail_logdet_without_2" else 2) * lg.sum()
    d_logdet = 2 * (r + 6) * E64 * float(np.abs(lg).sum())
    f = lambda x: np.asarray(x, F64)                # noqa: E731
    return {"hr": f(hr), "d_hr": d_hr, "c": f(c), "d_c": d_c, "t": f(t), "d_t": d_t, "coef": f(coef), "d_coef": d_coef, "zeta": f(zeta), "d_zeta": d_zeta,
            "bMb": f(bMb), "d_bMb": d_bMb, "logdet": f(logdet), "d_logdet": d_logdet}


TAIL_KEYS = ("hr", "c", "t", "coef", "zeta", "bMb", "logdet")


def woodbury_c(G, lam_kuu, kscale, A=LD):
    """C = I + Lam^1/2 G Lam^1/2, lam = lam_kuu kscale, sq = sqrt(lam), sqG = Lam^1/2 G; element-wise bounds."""
    Ga, lam = np.asarray(G, A), np.asarray(lam_kuu, A) * A(kscale)
    sq = np.sqrt(lam)
    sqG = sq[:, None] * Ga
    P = sqG * sq[None, :]
    C = P + np.eye(len(lam), dtype=A)
    ke = K * E64
    f = lambda x: np.asarray(x, F64)                # noqa: E731
    return {"C": f(C), "d_C": ke * np.maximum(np.abs(f(C)), np.maximum(np.abs(f(P)), np.eye(len(lam)))), "lam": f(lam), "d_lam": ke * np.abs(f(lam)),
            "sq": f(sq), "d_sq": ke * f(sq), "sqG": f(sqG), "d_sqG": ke * np.abs(f(sqG))}


def mll_weights(G, P, zeta, lam_kuu, g_b, g_ld, A=LD):
    """Wt = g_ld (G - P) + g_b zeta zeta^T and g_kap = sum_i Wt_ii lam_kuu_i; g_kap is held to the bound of its r-term sum."""
    Ga, Pa, za, la = (np.asarray(a, A) for a in (G, P, zeta, lam_kuu))
    r = len(za)
    zz = A(g_b) * np.outer(za, za)
    Wt = A(g_ld) * (Ga - Pa) + zz
    f = lambda x: np.asarray(x, F64)                # noqa: E731
    d_Wt = K * E64 * np.maximum(np.abs(f(Wt)), np.maximum(abs(float(g_ld)) * np.maximum(np.abs(f(Ga)), np.abs(f(Pa))), np.abs(f(zz))))
    terms = np.diagonal(Wt) * la
    d_kap = (r + 2) * E64 * float(np.abs(terms).sum()) + float((np.diagonal(d_Wt) * np.abs(f(la))).sum())
    return {"Wt": f(Wt), "d_Wt": d_Wt, "g_kap": f(terms.sum()), "d_g_kap": d_kap}


def absorb_h(h, F, wby, scale, A=LD, mutant=None):
    """h + F^T (wby / scale) (scale None: none) and its bound; F [n, r]."""
    Fa, ha, w = np.asarray(F, A), np.asarray(h, A), np.asarray(wby, A)
    n = Fa.shape[0]
    if scale is not None:
        w = w * np.asarray(scale, A) if mutant == "absorb_h_scale_multiplied" else w / np.asarray(scale, A)
    add = Fa.T @ w
    out = add if mutant == "absorb_h_overwrites" else ha + add
    bound = (n + 4) * E64 * (np.abs(ha) + np.abs(Fa).T @ np.abs(w)).astype(F64)
    return {"h": out.astype(F64), "d_h": bound}


# ------------------------------------------------------------------------------------------------------------------- case tables
def spike_columns(r):
    return sorted({k for k in (0, 63, 64, 511, 512, r - 1) if 0 <= k < r})


def eval_inputs(n, r, seed, ldl=None, upper=False, s2=S2):
    """Hand-built inputs of one evaluate, all fp32-representable.  Linv: random lower triangular, entries ~ 1 / sqrt(r), positive diagonal, the
    strict upper triangle zero (upper: filled with 1e3 -- the one-launch kernel reads k <= i only) and the columns beyond r (ldl > r) filled
    with 1e6.  Rows of F: even rows Gaussian, odd rows a single 4.0 in one of spike_columns(r) (the first of them has a tail of exactly zero:
    prior 32, kscale 1/2); row 2 (n >= 4) is 2^-100 everywhere with prior 0, so that (dg + tail) s2 underflows in fp32; row 4 (n >= 6) is
    Gaussian / 4096 with prior 0, a latent variance far below s2.  The other priors put half of the tails below zero."""
    rng = np.random.default_rng(seed)
    ldl = r if ldl is None else ldl
    L = np.tril(rng.standard_normal((r, r)) / np.sqrt(r))
    L[np.arange(r), np.arange(r)] = np.abs(np.diagonal(L)) + 0.5
    if upper:
        L = L + np.triu(np.full((r, r), 1e3), 1)
    Linv = np.full((r, ldl), 1e6)
    Linv[:, :r] = L
    F = rng.standard_normal((n, r))
    ks = spike_columns(r)
    prior = np.zeros(n)
    for j in range(n):
        if j % 2 == 1:
            F[j] = 0.0
            F[j, ks[(j // 2) % len(ks)]] = 4.0
        elif j == 2 and n >= 4:
            F[j] = 2.0 ** -100
        elif j == 4 and n >= 6:
            F[j] /= 4096.0
    F = f32r(F)
    cap = (F * F).sum(1)
    for j in range(n):
        if j == 1:
            prior[j] = 32.0                                   # 32 * 1/2 - 16 = 0 exactly
        elif not (j in (2, 4) and n >= 4 and (j == 2 or n >= 6)):
            prior[j] = cap[j] / KSCALE * (0.5 if (j // 2) % 2 else 1.5)
    t = f32r(rng.standard_normal(r))
    y = f32r(rng.standard_normal(n))
    return {"F": F, "prior": f32r(prior), "Linv": f32r(Linv), "ldl": ldl, "t": t, "kscale": KSCALE, "s2": float(F32(s2)), "y": y}


def _ecase(n, r, idx, tag="", **kw):
    name = tag + f"n{n}_r{r}" + "".join(f"_{k}{v}" for k, v in kw.items())
    # moments given / both NULL and the flag NULL / holding 3 alternate over the table
    return {"name": name, "n": n, "r": r, "seed": 1000 + idx, "moments": idx % 2 == 0, "err": None if (idx // 2) % 2 == 0 else 3, "kw": kw}


_pairs = [(n, r) for n in (1, 7, 8, 9, 63, 64) for r in (1, 63, 64, 65, 511, 512)] + [(n, r) for n in (1, 9, 64) for r in (513, 1000, 1024)]
EVAL_CASES = [_ecase(n, r, i) for i, (n, r) in enumerate(_pairs)]
EVAL_CASES += [_ecase(9, 65, 45, ldl=70), _ecase(9, 65, 46, upper=True), _ecase(8, 63, 47, s2=-0.3), _ecase(64, 1024, 48, ldl=1029)]
EVAL_Y_CASES = [_ecase(n, r, 60 + i, "y_") for i, (n, r) in enumerate([(1, 1), (63, 1), (64, 3), (65, 4), (130, 5), (1024, 327), (1, 1025), (65, 1025)])]
# one workspace: one launch, GEMM form, one launch, GEMM form
SEQUENCE = [("one", _ecase(64, 65, 80, "seq_")), ("y", _ecase(130, 65, 81, "seq_")), ("one", _ecase(7, 65, 82, "seq_")), ("y", _ecase(1, 65, 83, "seq_"))]
DISPATCH_CASES = [_ecase(n, r, 90 + i, "dispatch_") for i, (n, r) in enumerate([(64, 1024), (65, 1024), (64, 1025), (1, 1025)])]
VAR_CASES = [_ecase(n, r, 100 + i, "var_") for i, (n, r) in enumerate([(1, 1025), (15, 1), (16, 3), (17, 4), (63, 5), (64, 255), (65, 256), (300, 257), (15, 257),
                                                               (16, 1025)])]
TAIL_CASES = [(1, 1), (15, 63), (16, 64), (17, 65), (63, 63), (64, 1300), (65, 1), (327, 327), (1024, 64), (17, 1300)]          # (r, r_ref)
WOODBURY_R = (1, 16, 17, 512, 513, 1024)
# (n, r, ldf - r, scale given)
ABSORB_CASES = [(1, 1, 0, False), (63, 255, 3, True), (64, 256, 0, True), (65, 257, 3, False), (200, 256, 3, True), (200, 1, 0, False), (65, 255, 0, True),
                (64, 257, 3, False), (1, 256, 0, True), (63, 1, 3, True)]
CASE_BY_NAME = {c["name"]: c for c in EVAL_CASES + EVAL_Y_CASES + DISPATCH_CASES + VAR_CASES + [c for _, c in SEQUENCE]}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    c = CASE_BY_NAME[name]
    return eval_inputs(c["n"], c["r"], c["seed"], **c["kw"])


@functools.lru_cache(maxsize=None)
def case_solve(name):
    """(Y, dY) of a case, shared by everything that is held to it (computed once, never modified)."""
    x = case_inputs(name)
    Y, dY = solve_rows(x["Linv"], x["F"])
    Y.setflags(write=False), dY.setflags(write=False)
    return Y, dY


def case_reference(name, T=F64, A=LD, mutant=None, carry=None, given_y=False):
    """evaluate() of a case.  given_y: Y is an exact input (rounded to fp64 once here, as the test uploads it), not a product to be formed."""
    c, x = CASE_BY_NAME[name], case_inputs(name)
    kw = {}
    if A is LD and mutant not in _SOLVE_MUTANTS:           # (a defect of the product itself, or plain double arithmetic, forms its own)
        Y, dY = case_solve(name)
        kw = {"Y": Y.astype(F64), "dY": None} if given_y else {"Y": Y, "dY": dY}
    return evaluate(x["F"], x["prior"], x["Linv"], x["t"], x["kscale"], x["s2"], x["y"], c["err"], T=T, A=A, mutant=mutant, carry=carry, **kw)


def evaluate_held(T, *args, **kw):
    """The fp64 reference values of evaluate(*args) with the bounds of the instantiation T (the product Y is formed once)."""
    ref = evaluate(*args, T=F64, **kw)
    if T is F32:
        kw = dict(kw, Y=kw.get("Y", ref["Y"]), dY=kw.get("dY", ref["dY"]))
        ref = {**ref, **{k: v for k, v in evaluate(*args, T=F32, **kw).items() if k.startswith("d_")}}
    return ref


def held_to(name, T, given_y=False):
    """The same for a case of the tables."""
    ref = case_reference(name, given_y=given_y)
    if T is F32:
        ref = {**ref, **{k: v for k, v in case_reference(name, T=F32, given_y=given_y).items() if k.startswith("d_")}}
    return ref


_SOLVE_MUTANTS = ("row_chunk_512_dropped", "upper_triangle_included")


def var_inputs(name):
    """wiski_spectral_var: F, prior as eval_inputs (tails above, below and exactly at zero), Y [r, n] a Gaussian input of its own."""
    c, x = CASE_BY_NAME[name], case_inputs(name)
    return f32r(np.random.default_rng(c["seed"] + 7).standard_normal((c["r"], c["n"]))), x["F"], x["prior"], x["kscale"]


@functools.lru_cache(maxsize=None)
def tail_inputs(r, r_ref):
    rng = np.random.default_rng(2000 + 7 * r + r_ref)
    L = np.tril(rng.standard_normal((r, r)) / np.sqrt(r))
    L[np.arange(r), np.arange(r)] = np.abs(np.diagonal(L)) + 0.5
    chol = np.tril(rng.standard_normal((r, r)))
    chol[np.arange(r), np.arange(r)] = rng.uniform(0.2, 3.0, r)
    return {"TS": f32r(rng.standard_normal((r_ref, r)) / np.sqrt(r_ref)), "h_ref": f32r(rng.standard_normal(r_ref)), "sq": f32r(rng.uniform(0.5, 2.0, r)),
            "Linv": f32r(L), "chol": f32r(chol)}


@functools.lru_cache(maxsize=None)
def woodbury_inputs(r):
    rng = np.random.default_rng(3000 + r)
    R = rng.standard_normal((r, r))
    return {"G": f32r(R @ R.T / r), "P": f32r(rng.standard_normal((r, r))), "zeta": f32r(rng.standard_normal(r)), "lam_kuu": f32r(rng.uniform(0.1, 1.1, r)),
            "kscale": 1.75, "g_b": 0.375, "g_ld": -0.5}


def absorb_inputs(n, r, pad, scaled):
    """F [n, r + pad] (the padding columns hold 1e6), wby, scale (or None) and a non-zero h, all fp32-representable."""
    rng = np.random.default_rng(4000 + 1000 * n + 10 * r + pad + scaled)
    F = np.full((n, r + pad), 1e6)
    F[:, :r] = f32r(rng.standard_normal((n, r)))
    return {"F": F, "wby": f32r(rng.standard_normal(n)), "scale": f32r(rng.uniform(0.5, 3.0, n)) if scaled else None, "h": f32r(rng.standard_normal(r))}


# seeded defect -> (the case that must tell it from the reference, the outputs to look at); tests/test_spectral_eval_host.py
MUTANTS = {
    "row_chunk_512_dropped": "n9_r513",
    "upper_triangle_included": "n9_r65_upperTrue",
    "last_n_mod_8_missing_from_dg": "n9_r65",
    "tail_not_clamped": "n7_r63",
    "var_not_clamped": "n8_r63_s2-0.3",
    "kscale_not_applied": "n8_r64",
    "s2_not_added_in_v": "n7_r64",
    "log_2pi_missing": "n1_r1",
    "rmse_divided_by_64": "n63_r65",
    "max_of_signed_means": None,                     # the host test finds the cases whose largest |mean| is negative, and asserts there is one
    "f32_var_rounded_after_s2": "n9_r511",
    "workspace_not_reset": "seq_n7_r65",                # the third call of SEQUENCE, after the first left its dg behind
}
# the same for the other operations: defect -> the entry of TAIL_CASES / VAR_CASES / ABSORB_CASES
OTHER_MUTANTS = {
    "tail_coef_zeta_swapped": (17, 65), "tail_logdet_without_2": (17, 65), "tail_last_column_tile_dropped": (17, 65),
    "spectral_var_rows_3_mod_4_dropped": "var_n17_r4",
    "absorb_h_overwrites": (63, 255, 3, True), "absorb_h_scale_multiplied": (63, 255, 3, True),
}
