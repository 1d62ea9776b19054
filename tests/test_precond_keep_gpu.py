"""GPU: the truncated form of the fused fp32 preconditioner (csrc/spectral_keep.h, grid_ops.keep_counts): only the eigenmodes on
which the separable model differs from the identity by more than 2^-30 are transformed.  Reference and tolerances are those of
test_two_level_gpu.py::test_slab_kernel_block_against_numpy: the UNTRUNCATED operator in fp64 numpy on the fp32 tables, 2e-4 of
the largest element for y and t, 1e-4 relative for rho, three applications in a row."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
DEV = "cuda"
KSCALE, SHIFT = 1.3, 2.5


def _basis(g, ell, profiled, seed=5):
    """Grid, fp32 eigen tables decomposed from fp64 Toeplitz columns (what the model hands the solve), their host copies, and the
    tables as the kernel sees them (fp32 values in fp64) for the reference."""
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(seed)
    grid = grid_ops.GridSpec([[-1.1, 1.1]] * 3, list(g))
    cols = [np.exp(-0.5 * (np.arange(gq) * hq / ell) ** 2) * 0.7 for gq, hq in zip(g, grid.h)]
    tcol = torch.as_tensor(np.concatenate(cols), device=DEV, dtype=torch.float64)
    profiles = [np.clip(0.2 + rng.uniform(0, 1, gq), 1e-2, None) for gq in g] if profiled else None
    host = {}
    eig = grid_ops.kron_eigen(grid, tcol, profiles=profiles, host_out=host, dtype=torch.float32)
    X = [h.astype(np.float32).astype(np.float64) for h in host["X"]]
    D = [d.astype(np.float32).astype(np.float64) for d in host["D"]]
    Z = X if profiles is None else [np.asarray(p)[:, None] * x for p, x in zip(profiles, host["X"])]
    Z = [z.astype(np.float32).astype(np.float64) for z in Z]
    return grid, eig, host, X, D, Z, rng


def _reference(g, X, D, Z, r, blk=None, N=None):
    """y, t, rho of the untruncated operator (with the exact block on blk's modes)."""
    c = np.einsum("ai,bj,ck,abc->ijk", X[0], X[1], X[2], r.reshape(g), optimize=True)
    lam = KSCALE * np.einsum("i,j,k->ijk", *D)
    f1 = 1.0 / (1.0 + SHIFT * lam)
    cy, ct = c * lam * f1, c * f1
    if blk is not None:
        i0, i1, i2 = blk.idx_host
        ns = N @ c[i0, i1, i2]
        cy[i0, i1, i2] = ns
        ct[i0, i1, i2] = ns / lam[i0, i1, i2]
    y = np.einsum("ai,bj,ck,ijk->abc", X[0], X[1], X[2], cy, optimize=True).reshape(-1)
    t = np.einsum("ai,bj,ck,ijk->abc", Z[0], Z[1], Z[2], ct, optimize=True).reshape(-1)
    return y, t, float((c * cy).sum())


def _block(grid, host, rank, rng):
    from online_gp_amd.lazy import two_level as tlm

    blk = tlm.TwoLevelBlock(grid, torch.device(DEV), host, KSCALE, rank, None)
    A = rng.standard_normal((blk.r, blk.r))
    N = (A @ A.T / blk.r + np.diag(rng.uniform(0.5, 2.0, blk.r))) * 0.3
    blk.N[0].copy_(torch.as_tensor(N, dtype=torch.float32))
    return blk, N


@pytest.mark.parametrize("rank", [0, 40])
@pytest.mark.parametrize("profiled", [False, True])
def test_truncation_bites_against_the_untruncated_operator(profiled, rank):
    """Grid (20, 16, 12), lengthscale 0.9: the rule keeps 11 modes per dimension, rounded to 12 -- truncation in two dimensions,
    K_2 = g_2 the edge case in the third -- with and without density profiles, with and without a rank-40 exact block."""
    from online_gp_amd import grid_ops

    g = (20, 16, 12)
    grid, eig, host, X, D, Z, rng = _basis(g, 0.9, profiled)
    K, lo, hi = grid_ops.keep_counts(host["D"], KSCALE, SHIFT)
    assert K == (12, 12, 12) and lo < SHIFT <= hi
    assert grid_ops.keep_accepts(grid, K, two_level=rank > 0)
    blk, N = _block(grid, host, rank, rng) if rank else (None, None)
    if blk is not None:
        assert all(int(blk.idx_host[q].min()) >= g[q] - K[q] for q in range(3))      # the block's modes lie inside the box
    for trial in range(3):
        r = rng.standard_normal(grid.m)
        y_ref, t_ref, rho_ref = _reference(g, X, D, Z, r, blk, N)
        y, t, rho = grid_ops.precond_apply_keep(grid, eig, KSCALE, SHIFT, torch.as_tensor(r, device=DEV, dtype=torch.float32), K,
                                                two_level=blk.struct if blk is not None else None)
        torch.cuda.synchronize()
        ey, et = np.abs(y.cpu().numpy() - y_ref).max() / np.abs(y_ref).max(), np.abs(t.cpu().numpy() - t_ref).max() / np.abs(t_ref).max()
        er = abs(float(rho) - rho_ref) / abs(rho_ref)
        print(f"MEASURED keep {K} profiled={profiled} rank={rank} trial {trial}: y {ey:.2e} t {et:.2e} rho {er:.2e}")
        assert ey < 2e-4 and et < 2e-4, trial
        assert er < 1e-4, trial


def test_dropped_modes_pass_t_and_vanish_in_y():
    """r = Z e_k for a dropped mode k (and a sum of ten such modes): t returns r -- the identity on the dropped modes that Z = Kt^-1 U
    converges through -- and y is zero, to the tolerance of the first test scaled by the y of a random r of the same size."""
    from online_gp_amd import grid_ops

    g = (20, 16, 12)
    grid, eig, host, X, D, Z, rng = _basis(g, 0.9, True)
    K, _, _ = grid_ops.keep_counts(host["D"], KSCALE, SHIFT)
    o = [g[q] - K[q] for q in range(3)]
    r_rand = rng.standard_normal(grid.m)
    y_rand, _, _ = grid_ops.precond_apply_keep(grid, eig, KSCALE, SHIFT, torch.as_tensor(r_rand, device=DEV, dtype=torch.float32), K)
    y_scale = y_rand.abs().max().item()

    def dropped():
        q = int(rng.choice([q for q in range(3) if o[q] > 0]))                       # the dimension whose index lies outside the box
        k = [int(rng.integers(0, g[p])) for p in range(3)]
        k[q] = int(rng.integers(0, o[q]))
        return np.einsum("a,b,c->abc", Z[0][:, k[0]], Z[1][:, k[1]], Z[2][:, k[2]]).reshape(-1)

    for name, r in (("one mode", dropped()), ("ten modes", sum(dropped() * rng.uniform(0.5, 2.0) for _ in range(10)))):
        r = r * (np.abs(r_rand).max() / np.abs(r).max())
        rd = torch.as_tensor(r, device=DEV, dtype=torch.float32)
        y, t, _ = grid_ops.precond_apply_keep(grid, eig, KSCALE, SHIFT, rd, K)
        torch.cuda.synchronize()
        et, ey = (t - rd).abs().max().item() / rd.abs().max().item(), y.abs().max().item() / y_scale
        print(f"MEASURED dropped {name}: |t - r| / |r| {et:.2e}, |y| / |y(random r)| {ey:.2e}")
        assert et < 2e-4, name
        assert ey < 2e-4, name


def test_fallback_when_nothing_is_dropped():
    """Grid (12, 8, 16), lengthscale 0.5: the rule keeps every mode (12, 8, 14 -> 16) and reports no counts; without counts the entry
    point IS the full path (bit for bit), and the truncated kernels given the full box give its result within the tolerance."""
    from online_gp_amd import grid_ops

    g = (12, 8, 16)
    grid, eig, host, X, D, Z, rng = _basis(g, 0.5, True)
    K, _, _ = grid_ops.keep_counts(host["D"], KSCALE, SHIFT)
    assert K is None
    r = rng.standard_normal(grid.m)
    rd = torch.as_tensor(r, device=DEV, dtype=torch.float32)
    y_ref, t_ref, rho_ref = _reference(g, X, D, Z, r)
    y0, t0, rho0 = grid_ops.precond_apply(grid, eig, KSCALE, SHIFT, rd)
    y1, t1, rho1 = grid_ops.precond_apply_keep(grid, eig, KSCALE, SHIFT, rd, K)
    assert torch.equal(y0, y1) and torch.equal(t0, t1)
    assert abs(float(rho0) - float(rho1)) <= 1e-12 * abs(float(rho0))     # (fp64 atomics of the same per-block terms: only their order varies)
    y2, t2, rho2 = grid_ops.precond_apply_keep(grid, eig, KSCALE, SHIFT, rd, g)
    torch.cuda.synchronize()
    for y, t, rho in ((y1, t1, rho1), (y2, t2, rho2)):
        assert np.abs(y.cpu().numpy() - y_ref).max() < 2e-4 * np.abs(y_ref).max()
        assert np.abs(t.cpu().numpy() - t_ref).max() < 2e-4 * np.abs(t_ref).max()
        assert abs(float(rho) - rho_ref) < 1e-4 * abs(rho_ref)


def test_stream_steps_with_and_without_the_truncation():
    """Eight one-call streaming steps of a road-like stream on 14^3 (the smallest grid with m % 4 == 0 beyond the dense regime;
    lengthscale 1.5, so that the rule drops modes: K = 12 of 14), two-level block forced, switch on and off from the same data.
    After every step the posterior mean against an fp64 solve to 1e-10 of the model's own statistics: the error with the truncated
    preconditioner is at most 1.5 times the error without (both stop somewhere inside the tolerance band), and the summed
    iteration counts differ by at most one."""
    import bench
    from online_gp_amd import grid_ops, settings
    from online_gp_amd.kernels import RBFKernel, ScaleKernel
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    g, n0, q, steps = 14, 1500, 250, 8
    X, y = bench.synth_stream(n0 + steps * q, 3, 3, torch.device(DEV), torch.float32, "clustered")
    gb = torch.tensor([[-1.1, 1.1]] * 3)
    out = {}
    for on in (False, True):
        with settings.truncated_preconditioner(on), settings.skip_posterior_variances(True), settings.two_level_rank(64), \
                settings.two_level_min_iters(0.0), settings.two_level_growth(1.0), settings.two_level_lockstep(True), torch.no_grad():
            cov = ScaleKernel(RBFKernel(ard_num_dims=3))
            cov.base_kernel.lengthscale = torch.full((1, 3), 1.5)
            m = FixedNoiseOnlineSKIGP(X[:n0], y[:n0], None, covar_module=cov, grid_bounds=gb, grid_size=g, learn_additional_noise=True).eval()
            m.prediction_cache
            errs, its, keeps, blocks = [], [], [], 0
            for s in range(steps):
                sl = slice(n0 + s * q, n0 + (s + 1) * q)
                m.stream_step(X[sl], y[sl])
                step = m.__dict__["_stream_step_cache"][1]
                keeps.append(tuple(step.args.keep))
                blocks += step.args.two_level is not None
                its.append(m._last_iters[0])
                tcol, s2, tcol64 = m._hyper()[0]
                A64 = m._kernel_cache["WtW"].stencil.double().contiguous()
                b64 = m._kernel_cache["interpolation_cache"][0, :, 0].double().contiguous()
                Uref, _, _, rel = grid_ops.pcg(m._grid, A64, tcol64.contiguous(), 1.0 / s2, b64[None], tol=1e-10, max_iter=2000,
                                               eigen=grid_ops.kron_eigen(m._grid, tcol64), shift=float(m._wsum[0]) / m._grid.m)
                assert rel[0] < 1e-10
                errs.append(((m._mean_state["U"][0].double() - Uref[0]).abs().max() / Uref[0].abs().max()).item())
            out[on] = (errs, its, keeps, blocks)
    (e_off, it_off, k_off, b_off), (e_on, it_on, k_on, b_on) = out[False], out[True]
    print("MEASURED stream 14^3: err off", ["%.1e" % e for e in e_off], "on", ["%.1e" % e for e in e_on], "iters off", it_off, "on", it_on,
          "keep", k_on, "steps with the block", b_off, b_on)
    assert all(k == (0, 0, 0) for k in k_off) and all(k == (12, 12, 12) for k in k_on)       # the switch is what differs
    assert b_on >= 1 and b_off >= 1                                                          # the exact block was in use
    for s in range(steps):
        assert e_on[s] <= 1.5 * e_off[s], (s, e_on[s], e_off[s])
    assert abs(sum(it_on) - sum(it_off)) <= 1, (it_on, it_off)


def test_keep_refusals():
    """Kept-mode counts a solve cannot take are refused before anything is queued (pcg_validate, through wiski_stream_step with no
    batch: the call is the solve alone): fp64, above the cap of 24, not a multiple of 4, above g_q, some but not all counts, and
    off the fused path (no eigen tables).  U and Z keep their NaN fill.  The apply entry point refuses the same counts.
    (No row for k != 1: the counts travel in wiski_stream_args and wiski_precond_apply_keep only, both one-column by construction, so
    no public entry can express it; pcg_validate and launch_spectral_fused_cg refuse it for callers inside the library.)"""
    from test_hip_ops import _pcg_case

    from online_gp_amd import _hip, grid_ops

    BADARG, i32 = -1, ctypes.c_int32
    table = []
    cases = {}
    for dt, nd, Args in ((torch.float32, np.float32, grid_ops._StreamArgs32), (torch.float64, np.float64, grid_ops._StreamArgs64)):
        f = cases[dt] = _pcg_case(3, 8, dt, nd, 5, 1)[0]
        R = torch.zeros_like(f["U"])

        def call(keep, eigen=True, f=f, R=R, Args=Args, dt=dt):
            sa = Args()
            sa.d_A_half, sa.d_b, sa.d_U, sa.d_Z, sa.d_R, sa.d_tcol = [f[n].data_ptr() for n in ("A", "RHS", "U", "Z")] + [R.data_ptr(), f["tcol"].data_ptr()]
            sa.kscale, sa.shift, sa.tol, sa.max_iter, sa.check_every = f["kscale"], f["shift"], f["tol"], f["max_iter"], 5
            sa.d_work, sa.work_bytes = f["work"].data_ptr(), f["work_bytes"]
            if eigen:
                sa.d_evec, sa.d_eval = f["evec"].data_ptr(), f["eval"].data_ptr()
            sa.keep[:] = keep
            it, rr, he, resumed = i32(0), ctypes.c_double(0), i32(0), i32(0)
            return _hip.fn("wiski_stream_step", dt)(f["grid"].ref, ctypes.byref(sa), None, None, None, None, None, ctypes.c_int64(0), None, i32(1), i32(0),
                                                    ctypes.byref(it), ctypes.byref(rr), ctypes.byref(he), f["stream"], None, i32(0), ctypes.byref(resumed))

        if dt == torch.float64:
            table.append(("f64 keep", call((4, 4, 4)), BADARG))
        else:
            table += [("f32 above the cap", call((28, 8, 8)), BADARG), ("f32 not a multiple of 4", call((6, 8, 8)), BADARG),
                      ("f32 above g", call((12, 8, 8)), BADARG), ("f32 partial counts", call((4, 0, 0)), BADARG), ("f32 partial counts, first zero", call((0, 4, 4)), BADARG),
                      ("f32 no eigen tables", call((4, 4, 4), eigen=False), BADARG)]
    torch.cuda.synchronize()
    for what, rc, want in table:
        print(f"refusal {what}: {rc}")
    assert [(what, rc, want) for what, rc, want in table if rc != want] == []
    assert all(bool(torch.isnan(c[n]).all()) for c in cases.values() for n in ("U", "Z"))
    f = cases[torch.float32]
    r = torch.ones(f["grid"].m, device=DEV, dtype=torch.float32)
    for keep in ((28, 8, 8), (6, 8, 8), (12, 8, 8), (4, 0, 0)):
        assert not grid_ops.keep_accepts(f["grid"], keep)
        with pytest.raises(RuntimeError):
            grid_ops.precond_apply_keep(f["grid"], (f["evec"], f["eval"]), 1.0, 1.0, r, keep)
    assert grid_ops.keep_accepts(f["grid"], (8, 4, 8))
