"""TEST INFRASTRUCTURE -- closed forms of the Toeplitz columns of a term list and of their derivatives w.r.t. every parameter
(DESIGN.md 3.29), independent of the package: once in numpy fp64 (`columns`), once in mpmath at 40 digits (`columns_mp`).

A kernel is a list of terms (dim, kind, i_ell, i_aux) over a parameter vector theta; the column of grid dimension q is

    out[q][l] = S * prod_{terms of dim q} k_kind(l h_q; theta[i_ell], theta[i_aux])

kind 0  RBF          exp(-r^2 / 2),                         r = tau / ell
     1  Matern 1/2   exp(-r)
     2  Matern 3/2   (1 + s) exp(-s),                       s = sqrt(3) r
     3  Matern 5/2   (1 + s + s^2 / 3) exp(-s),             s = sqrt(5) r
     4  periodic     exp(-2 sin^2(pi tau / p) / ell^2),     p = theta[i_aux]
     5  RQ           (1 + x)^-alpha, x = tau^2 / (2 alpha ell^2),  alpha = theta[i_aux]

`columns` and `columns_mp` share `_assemble` (the product rule and the index handling), so their agreement checks only the per-profile
closed forms independently; the assembly is checked independently by CPU autograd through the classes (tests/test_kernel_families_host.py).

`mutant` swaps in a deliberately wrong form, for the tests that check that the bounds tell it apart:
    "ell_not_squared"   the periodic profile with ell in place of ell^2
    "alpha_no_log1p"    the alpha-derivative of RQ without its log1p term
"""
import numpy as np

KINDS = {"rbf": 0, "matern12": 1, "matern32": 2, "matern52": 3, "periodic": 4, "rq": 5}


def profile(kind, tau, ell, aux, mutant=None):
    """(k, dk / d ell, dk / d aux) at the lags tau (numpy fp64)."""
    tau = np.asarray(tau, dtype=np.float64)
    if kind <= 3:
        r = tau / ell
        if kind == 0:
            k = np.exp(-0.5 * r * r)
            dr = -r * k
        elif kind == 1:
            k = np.exp(-r)
            dr = -k
        elif kind == 2:
            s = np.sqrt(3.0) * r
            k = (1.0 + s) * np.exp(-s)
            dr = -np.sqrt(3.0) * s * np.exp(-s)
        else:
            s = np.sqrt(5.0) * r
            k = (1.0 + s + s * s / 3.0) * np.exp(-s)
            dr = -np.sqrt(5.0) * (s / 3.0) * (1.0 + s) * np.exp(-s)
        return k, dr * (-r / ell), np.zeros_like(tau)
    if kind == 4:
        u = np.pi * tau / aux
        s, c = np.sin(u), np.cos(u)
        if mutant == "ell_not_squared":
            k = np.exp(-2.0 * s * s / ell)
            return k, k * 2.0 * s * s / ell ** 2, k * 4.0 * s * c * u / (ell * aux)
        k = np.exp(-2.0 * s * s / ell ** 2)
        return k, k * 4.0 * s * s / ell ** 3, k * 4.0 * s * c * u / (ell ** 2 * aux)
    x = tau * tau / (2.0 * aux * ell * ell)
    lg = np.log1p(x)
    k = np.exp(-aux * lg)
    da = k * (x / (1.0 + x) - (0.0 if mutant == "alpha_no_log1p" else lg))
    return k, k * 2.0 * aux * x / ((1.0 + x) * ell), da


def _assemble(g, h, terms, theta, S, prof, one, zero):
    """out [sum g], d out / d theta [nparams][sum g], d out / d S [sum g] as nested lists of scalars of the arithmetic `prof` works in."""
    n = sum(g)
    out, dS, dth = [zero] * n, [zero] * n, [[zero] * n for _ in theta]
    off = 0
    for q in range(len(g)):
        mine = [t for t in terms if t[0] == q]
        for l in range(g[q]):
            tau = h[q] * l
            vals = [prof(t[1], tau, theta[t[2]], theta[t[3]] if t[3] >= 0 else None) for t in mine]
            prod = one
            for v in vals:
                prod = prod * v[0]
            out[off + l], dS[off + l] = S * prod, prod
            for j, t in enumerate(mine):
                others = one
                for i, v in enumerate(vals):
                    if i != j:
                        others = others * v[0]
                dth[t[2]][off + l] = dth[t[2]][off + l] + S * others * vals[j][1]
                if t[3] >= 0:
                    dth[t[3]][off + l] = dth[t[3]][off + l] + S * others * vals[j][2]
        off += g[q]
    return out, dth, dS


def columns(g, h, terms, theta, S=1.0, mutant=None):
    """numpy fp64: (out [sum g], d out / d theta [nparams, sum g], d out / d S [sum g])."""
    theta = [float(t) for t in theta]

    def prof(kind, tau, ell, aux):
        k, de, da = profile(kind, tau, ell, aux, mutant)
        return float(k), float(de), float(da)

    out, dth, dS = _assemble([int(x) for x in g], [float(x) for x in h], terms, theta, float(S), prof, 1.0, 0.0)
    return np.array(out), np.array(dth).reshape(len(theta), -1), np.array(dS)


def profile_mp(kind, tau, ell, aux):
    """The same closed forms in mpmath (the caller sets the precision)."""
    import mpmath as mp

    if kind <= 3:
        r = tau / ell
        if kind == 0:
            k = mp.exp(-r * r / 2)
            dr = -r * k
        elif kind == 1:
            k = mp.exp(-r)
            dr = -k
        elif kind == 2:
            s = mp.sqrt(3) * r
            k = (1 + s) * mp.exp(-s)
            dr = -mp.sqrt(3) * s * mp.exp(-s)
        else:
            s = mp.sqrt(5) * r
            k = (1 + s + s * s / 3) * mp.exp(-s)
            dr = -mp.sqrt(5) * (s / 3) * (1 + s) * mp.exp(-s)
        return k, dr * (-r / ell), mp.mpf(0)
    if kind == 4:
        u = mp.pi * tau / aux
        s, c = mp.sin(u), mp.cos(u)
        k = mp.exp(-2 * s * s / ell ** 2)
        return k, k * 4 * s * s / ell ** 3, k * 4 * s * c * u / (ell ** 2 * aux)
    x = tau * tau / (2 * aux * ell * ell)
    lg = mp.log1p(x)
    k = mp.exp(-aux * lg)
    return k, k * 2 * aux * x / ((1 + x) * ell), k * (x / (1 + x) - lg)


def columns_mp(g, h, terms, theta, S=1.0, digits=40):
    """mpmath at `digits` digits, from the same fp64 inputs; results rounded to fp64 arrays."""
    import mpmath as mp

    with mp.workdps(digits):
        th = [mp.mpf(float(t)) for t in theta]
        out, dth, dS = _assemble([int(x) for x in g], [mp.mpf(float(x)) for x in h], terms, th, mp.mpf(float(S)), profile_mp, mp.mpf(1), mp.mpf(0))
        conv = lambda v: np.array([float(x) for x in v])
        return conv(out), np.stack([conv(r) for r in dth]), conv(dS)


def grid_steps(bounds, g):
    """Spacing of the inducing grid over `bounds` with `g` points per dim: linspace(lo - delta, hi + delta, g), delta = (hi - lo) / (g - 2)
    (GridSpec's rule, in its operation order)."""
    out = []
    for (lo, hi), gi in zip(bounds, g):
        dl = (hi - lo) / (gi - 2)
        out.append(((hi + dl) - (lo - dl)) / (gi - 1))
    return out


def cases():
    """[(name, bounds, g, terms, theta, S)]: the column cases shared by the host and the GPU tests.  Every case keeps
    (g - 1) h / p <= 10 and ell >= 0.3, the range in which the numpy forms agree with mpmath to 1e-13 (d / dp is ill-conditioned
    beyond it: the argument of the sine grows with span / p)."""
    out = []
    for name, kind in KINDS.items():
        out.append((f"one_{name}", [[-1.0, 1.0]], [4], [(0, kind, 0, 1 if kind >= 4 else -1)], [0.7, 0.9 if kind == 4 else 1.3][:2 if kind >= 4 else 1], 1.0))
    b4, g4 = [[-1.0, 1.0 + 0.3 * q] for q in range(4)], [9, 12, 7, 6]
    # dimension 0 periodic x RBF, 1 RQ, 2 Matern-5/2, 3 no term
    out.append(("mixed4", b4, g4, [(0, 4, 0, 1), (0, 0, 2, -1), (1, 5, 3, 4), (2, 3, 5, -1)], [0.8, 0.9, 1.1, 0.6, 1.7, 0.5], 1.3))
    h = grid_steps([[-1.0, 1.0], [0.0, 1.0]], [300, 5])
    out.append(("stride", [[-1.0, 1.0], [0.0, 1.0]], [300, 5], [(0, 4, 0, 1), (1, 0, 2, -1)], [0.9, 0.37 * 299 * h[0], 0.4], 0.7))
    out.append(("shared_ell", b4[:3], g4[:3], [(0, 0, 0, -1), (1, 3, 0, -1), (2, 5, 0, 1)], [0.65, 2.0], 1.1))
    h12 = grid_steps([[-1.0, 1.0]], [12])[0]
    out.append(("commensurate", [[-1.0, 1.0]], [12], [(0, 4, 0, 1)], [0.5, 4.0 * h12], 1.0))
    out.append(("p_gt_span", [[-1.0, 1.0]], [12], [(0, 4, 0, 1)], [0.5, 1.7 * 11 * h12], 0.9))
    out.append(("p_lt_2h", [[-1.0, 1.0]], [12], [(0, 4, 0, 1)], [0.6, 1.5 * h12], 1.0))
    out.append(("rq_small_alpha", [[-1.0, 1.0]], [12], [(0, 5, 0, 1)], [0.4, 0.05], 1.2))
    out.append(("rq_large_alpha", [[-1.0, 1.0]], [12], [(0, 5, 0, 1)], [0.4, 1.0e4], 1.0))
    return out


def softplus(x):
    return np.logaddexp(0.0, x)


def softplus_grad(x):
    return 1.0 / (1.0 + np.exp(-x))


def err(got, ref):
    """max |got - ref| relative to max(1, max |ref|): the measure every bound of these tests is stated in."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0
