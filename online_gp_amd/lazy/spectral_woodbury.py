"""Dense Woodbury factor in the dominant Kronecker eigenspace of Kuu ("spectral factor").

The reference reaches the posterior through a rank-limited root space: L L^T ~ W^T D^-1 W with at most
``max_root_decomposition_size`` columns, Q = I + L^T Kt L, Cholesky of Q (BFN:343-404, URLT:74-76).  On grids where
the matrix-free path (wiski_pcg) is the only exact option this module offers the same thing with the roles swapped:
the low-rank object is the *prior*.  For a smooth stationary kernel Kt = kron_q K_q / sigma2 has a tiny numerical rank:
with K_q = V_q diag(ev_q) V_q^T the r tensor-product eigenvectors b_j = kron_q V_q[:, S_q[j]] of largest eigenvalue
lam_j carry all but a fraction ``settings.spectral_tail`` of trace(Kt) (r ~ 330 for the default RBF hyper-parameters
on a 50^3 grid at 1e-6, 430 at 1e-7).  With B = [b_j] and Kt_B = B Lam B^T,

    G = B^T A B,  h = B^T b                      (A = W^T D^-1 W, b = W^T D^-1 y: the model's statistics)
    C = I + Lam^1/2 G Lam^1/2 = chol chol^T      (SPD, eigenvalues >= 1: no jitter; wiski_potrf, fp64)
    M_B = (Kt_B^+ + A)^-1 restricted to span(B) = B Lam^1/2 C^-1 Lam^1/2 B^T
    w^T M_B w = |chol^-1 Lam^1/2 B^T w|^2        (wiski_basis_project + wiski_trsm)
    b^T M_B b = |chol^-1 Lam^1/2 h|^2,  logdet(I + Kt_B A) = 2 sum log diag chol        (BWM:27-35)

Error control.  K -> (K^-1 + A)^-1 is operator monotone and 0 <= M(Kt) - M(Kt_B) <= Kt - Kt_B, so for every query
    0 <= w^T M w - w^T M_B w <= w^T Kt w - sum_j lam_j (b_j^T w)^2 =: tail(w),
and tail(w) costs nothing (the prior variance is a product of d 4x4 quadratic forms).  The returned variance is
w^T M_B w + tail(w) -- exact wherever the data do not inform the left-out directions, which is what "left out" means --
and ``last_rel_bound`` records max tail / variance.

Hyper-parameter steps.  The eigenvectors move with the lengthscales, G = B^T A B does not survive that.  The factor
therefore keeps G_ref, h_ref in a *reference* basis taken with a margin (tail x 1e-2) at the hyper-parameters it was
built for, follows streaming updates there (G_ref += F^T diag(wa) F with F = W B_ref: one projection kernel + one MFMA
GEMM), and re-expresses it in the current eigenbasis by the Kronecker-structured change of basis
T[i, j] = prod_q (V_ref,q^T V_q)[S_ref[q, i], S[q, j]]:  G = T^T G_ref T.  The part of a current basis vector outside
the reference span ("defect") is monitored, weighted by its eigenvalue; when it exceeds the tail budget the reference
is rebuilt from the stencil (r_ref SpMV columns).  Everything dense runs in fp64 on wiski_gemm / potrf / trsm.

Per-batch hyper-parameter steps (the reference's online loop) never leave the device: the eigenvectors are REFINED from the
previous ones by wiski_basis_eig_update (subspace iteration + Rayleigh-Ritz, one workgroup per dim), the index set is kept,
wiski_basis_change builds T together with a three-number verdict (eigen-residual, trace left out, reference-span defect) that
is read back before the state is handed out; a failed verdict -- or every 64th step -- takes the host path (eigh + selection).
Then wiski_woodbury_c, wiski_potrf_inverse (one-workgroup Cholesky + explicit inverse for r <= 480) and wiski_factor_tail
(DESIGN 3.9).
"""
import ctypes

import numpy as np
import torch

from .. import _hip, grid_ops, settings

KMAX = 32
GUARD = 6          # extra eigenvectors per dim carried for the device-side subspace iteration
RESELECT_EVERY = 64
MEAN_CHECK_EVERY = 32  # factor states between two evaluations of the mean-truncation bound (~0.13 ms each: a Kronecker product + dots)
MEAN_MEASURE_EVERY = 512   # monitor calls a MEASURED mean error (against a PCG solve, when the bound has become too loose to decide) stays valid


def default_tail(dtype):
    v = settings.spectral_tail.value()
    if v is not None:
        return float(v)
    return 1e-6 if dtype == torch.float32 else 1e-9


class SpectralBasis:
    """Index set + per-dim eigenvector tables for one set of Toeplitz columns.  Device copies are made with two uploads
    (one packed fp64 array, one int32 index array; the latter is shared with `like` when the index set did not change)."""

    def __init__(self, grid, evs, Vs, S, lam_kuu, kmax, device, like=None):
        self.grid, self.kmax, self.r = grid, kmax, S.shape[1]
        self.evs, self.Vs = evs, Vs                    # host: per-dim eigenvalues (descending, >= 0) / eigenvectors [g_q, g_q]
        self.S_host = S                                # [d, r] int
        self.lam_kuu_host = lam_kuu                    # [r] eigenvalues of Kuu (not yet divided by sigma2), descending
        d = grid.d
        tabs = [np.ascontiguousarray(V[:, :kmax]) if V.shape[1] >= kmax else np.pad(V, ((0, 0), (0, kmax - V.shape[1]))) for V in Vs]
        self.Vtab_host = tabs
        ev_tab = np.zeros((d, kmax))
        for q in range(d):
            kq = min(kmax, len(evs[q]))
            ev_tab[q, :kq] = evs[q][:kq]
        nV = sum(t.size for t in tabs)
        packed = torch.as_tensor(np.concatenate([t.reshape(-1) for t in tabs] + [ev_tab.reshape(-1), np.asarray(lam_kuu, dtype=np.float64)])).to(device)
        self.Vtab = packed[:nV]
        self.Vq, off = [], 0
        for t in tabs:
            self.Vq.append(packed[off:off + t.size].view(t.shape))                              # [g_q, kmax] each
            off += t.size
        self.ev_tab = packed[nV:nV + d * kmax].view(d, kmax)
        self.lam_kuu = packed[nV + d * kmax:]
        if like is not None and like.S_host.shape == S.shape and np.array_equal(like.S_host, S):
            self.S, self.S_long = like.S, like.S_long
        else:
            self.S = torch.as_tensor(S.astype(np.int32)).to(device).contiguous()
            self.S_long = self.S.long()
        self.kuse = int(S.max()) + 1                   # eigenvectors per dim the index set actually refers to
        self.short0 = 0.0                              # fraction of trace(Kuu) the index set left out when it was selected
        self.total = None                              # trace(Kuu) as a device scalar (device-refreshed bases only)

    @classmethod
    def on_device(cls, like, Vtab, ev_tab, total, lam=None):
        """The basis with `like`'s index set and device-refreshed eigenvector tables (wiski_basis_eig_update): no host copies."""
        self = cls.__new__(cls)
        self.grid, self.kmax, self.r, self.kuse, self.short0 = like.grid, like.kmax, like.r, like.kuse, like.short0
        self.evs = self.Vs = self.Vtab_host = self.lam_kuu_host = None
        self.S_host, self.S, self.S_long = like.S_host, like.S, like.S_long
        self.Vtab, self.ev_tab, self.total = Vtab, ev_tab, total
        self.Vq, off = [], 0
        for g in like.grid.g:
            self.Vq.append(Vtab[off:off + g * like.kmax].view(g, like.kmax))
            off += g * like.kmax
        if lam is None:
            lam = ev_tab[0][self.S_long[0]]
            for q in range(1, like.grid.d):
                lam = lam * ev_tab[q][self.S_long[q]]
        self.lam_kuu = lam
        return self

    def device_refreshable(self):
        """wiski_basis_eig_update's limits: even table width <= 32 that leaves room for guard vectors, factors of <= 64 nodes."""
        return self.kmax % 2 == 0 and self.kmax <= KMAX and self.kmax >= min(self.kuse + 2, min(self.grid.g)) and max(self.grid.g) <= 64 \
            and self.kmax <= min(self.grid.g)


def host_eig(grid, tcol_host):
    """Per-dim eigen-decomposition (fp64, descending, clamped >= 0) of the symmetric Toeplitz factors."""
    evs, Vs, off = [], [], 0
    for g in grid.g:
        c = tcol_host[off:off + g]
        idx = np.abs(np.arange(g)[:, None] - np.arange(g)[None, :])
        w, V = np.linalg.eigh(c[idx])
        evs.append(np.clip(w[::-1], 0.0, None))
        Vs.append(np.ascontiguousarray(V[:, ::-1]))
        off += g
    return evs, Vs


def select_basis(grid, tcol_host, tail, max_rank, device, eig=None, like=None, truncate=False):
    """The smallest set of tensor-product eigenvectors leaving out at most `tail` of trace(Kuu); None if it needs more than
    `max_rank` vectors (or more than KMAX eigenvectors of one dim).  truncate: instead of giving up, keep the `max_rank`
    vectors of largest eigenvalue (settings.fast_pred_var: a rank cap, as upstream's Lanczos root; the left-out prior variance
    of every query is still added back and reported)."""
    evs, Vs = eig if eig is not None else host_eig(grid, tcol_host)
    d = grid.d
    total, off = 1.0, 0
    for g in grid.g:
        total *= g * float(tcol_host[off])
        off += g
    if not total > 0:
        return None
    # candidates: per dim, the eigenvalues that can take part in a product above the threshold (ratio to the largest)
    cut = min(tail, 1e-6) * 1e-3
    kc = [max(1, int((ev / ev[0] >= cut).sum())) for ev in evs]
    if truncate:                                   # a capped basis never needs more than max_rank eigenvectors of one dim
        kc = [min(k_, KMAX, max_rank) for k_ in kc]
        while int(np.prod(kc)) > 400_000:
            kc[int(np.argmax(kc))] -= 1
    if max(kc) > KMAX or int(np.prod(kc)) > 400_000:
        return None
    lam = evs[0][:kc[0]]
    for q in range(1, d):
        lam = np.multiply.outer(lam, evs[q][:kc[q]])
    flat = lam.reshape(-1)
    order = np.argsort(-flat, kind="stable")
    cs = np.cumsum(flat[order])
    need = total * (1.0 - tail)
    if cs[-1] < need:
        if not truncate:
            return None
        r = len(flat)
    else:
        r = int(np.searchsorted(cs, need) + 1)
    if r > max_rank:
        if not truncate:
            return None
        r = max_rank
    sel = order[:r]
    S = np.stack(np.unravel_index(sel, lam.shape)).astype(np.int64)            # [d, r]
    kmax = int(S.max()) + 1
    # table width: a few guard vectors beyond the ones the index set uses, even -- what the device-side refresh of the
    # eigenvectors after a hyper-parameter step (wiski_basis_eig_update: subspace iteration) wants; costs nothing elsewhere
    kw = min(KMAX, (kmax + GUARD + 1) & ~1, min(grid.g) & ~1)
    basis = SpectralBasis(grid, evs, Vs, S, flat[sel], max(kmax, kw), device, like=like)
    basis.short0 = max(0.0, 1.0 - float(cs[r - 1]) / total)
    return basis


class SpectralWoodburyFactor:
    """Reduced-basis statistics (G_ref, h_ref) of ONE output and the factor derived from them for the current
    hyper-parameters.  Owned by the model, which tells it about every change of the statistics."""

    def __init__(self, grid, dtype, device, err):
        self.grid, self.dtype, self.device, self.err = grid, dtype, device, err
        self.ref = None            # SpectralBasis of the reference
        self.G_ref = self.h_ref = None
        self.data_version = 0
        self.cur = None
        self.stale = False         # the statistics changed behind the factor's back (large batch, all-reduce, idle): rebuild from the stencil when next asked
        self.rebuilds = 0          # reference builds from the stencil (diagnostics / tests)
        self.idle_absorbs = 0      # batches followed since anybody last asked for a state (see the model's _spectral_absorb)
        self.last_rel_bound = 0.0
        self._chk = None           # pending verdict of a device-side eigenvector refresh
        self._dev_refreshes = 0
        self.device_refreshes = 0  # diagnostics / tests
        self.last_verdict = None
        # monitor of the truncated MEAN (the variance has its own per-query bound): see mean_bound()
        self.mean_ok = True
        self.last_mean_bound = None
        self._mean_chk = None
        self._mean_countdown = 0
        self.measure_due = False   # the bound exceeded its limit: the next mean request compares the factor's mean with a PCG solve first
        self.last_measured = None  # max |mean_factor - mean_pcg| / max |mean_pcg| on the probe set, when last measured
        self._measured_at = 0
        self.measurements = 0

    def clone(self):
        """A factor for a COPY of the statistics (functional conditioning clones the caches, BFN:276-285): own G_ref / h_ref, the
        bases and the current state shared (they are never written in place), nothing in flight carried over."""
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new.G_ref = None if self.G_ref is None else self.G_ref.clone()
        new.h_ref = None if self.h_ref is None else self.h_ref.clone()
        new._chk = new._mean_chk = None
        for k in ("_bc_work", "_chk_hosts", "_chk_events", "_mean_host", "_eval_ws", "_info", "_last"):
            new.__dict__.pop(k, None)               # (buffers kernels of the original may still be writing)
        return new

    # ---------------------------------------------------------------------- mean-truncation monitor --
    def mean_monitor(self, st, query, b, tcol_dev, scale):
        """Bound on what the truncation does to the predictive MEAN, evaluated every MEAN_CHECK_EVERY-th call and read one call late.

        With Delta = M(Kt) - M(Kt_B), 0 <= Delta <= Kt - Kt_B (module docstring), Cauchy-Schwarz in the PSD form Delta gives for
        every query   |w^T M b - w^T M_B b| <= sqrt(w^T Delta w  b^T Delta b) <= sqrt(tail(w) * btail),
            btail = b^T Kt b - sum_j lam_j (b_j^T b)^2       (one Kronecker-Toeplitz product + two dots, fp64),
        and tail(w) is the left-out prior variance of the query that the variance path adds back anyway.  The variance bound says
        nothing about the mean: btail grows with the data (b = W^T D^-1 y) while tail(w) does not, so a long stream / small noise can
        move the factor's mean although its variances stay inside their bound.  ``scale`` = max |mean| of the batch (device
        scalar).  The ratio bound / scale is copied to pinned memory asynchronously; the NEXT call reads it (long since arrived)
        and sets ``mean_ok`` -- the model then serves means from its PCG state until a later check passes again."""
        lim = settings.spectral_mean_tolerance.value()
        if lim is None:
            lim = 1e-2 if self.dtype == torch.float32 else 1e-4
        self._monitor_calls = self.__dict__.get("_monitor_calls", 0) + 1
        if self._monitor_calls - self._measured_at >= 4 * MEAN_MEASURE_EVERY:
            self.measure_due = True                    # (an audit whatever the bound says: one PCG solve per 2048 calls)
        if self._mean_chk is not None:
            host, ev = self._mean_chk
            ev.synchronize()
            self.last_mean_bound = float(host[0])
            self._mean_chk = None
            if self.last_mean_bound <= lim:
                self.mean_ok, self.measure_due = True, False
            elif (self.last_measured is not None and self.last_measured <= 0.25 * lim
                  and self._monitor_calls - self._measured_at < MEAN_MEASURE_EVERY):
                pass                                   # the bound cannot decide any more, a recent measurement can: keep serving
            else:
                # Cauchy-Schwarz is loose (measured: bound 1e-2 where the error is 4e-5, 50 000 points into a stream): before the factor's
                # mean is given up, the model MEASURES it against a PCG solve on a probe set (measure_mean, called by the model)
                self.measure_due = True
        self._mean_countdown -= 1
        if self._mean_countdown > 0:
            return
        self._mean_countdown = MEAN_CHECK_EVERY
        b64 = b.reshape(-1).double()
        Kb = grid_ops.kron_toeplitz_mm(self.grid, tcol_dev.double() if tcol_dev.dtype != torch.float64 else tcol_dev, b64, scale=float(st["kscale"]))
        btail = (torch.dot(b64, Kb) - torch.dot(st["lam"], st["hr"] * st["hr"])).clamp_min(0.0)
        tailw = (query.prior * float(st["kscale"]) - (query.Fs * query.Fs).sum(1)).clamp_min(0.0).max()
        ratio = (torch.sqrt(tailw * btail) / scale.double().clamp_min(1e-300)).reshape(1)
        host = self.__dict__.get("_mean_host")
        if host is None:
            host = self._mean_host = torch.empty(1, dtype=torch.float64).pin_memory()
        host.copy_(ratio, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._mean_chk = (host, ev)

    def probe_points(self, n=256):
        """A fixed set of points inside the grid (seeded uniform) on which a measured mean error is taken."""
        pp = self.__dict__.get("_probe")
        if pp is None or pp.shape[0] != n:
            gen = torch.Generator(device="cpu").manual_seed(0x9E3779B1)
            u = torch.rand((n, self.grid.d), generator=gen, dtype=torch.float64)
            lo = torch.tensor([b[0] for b in self.grid.grid_bounds], dtype=torch.float64)
            hi = torch.tensor([b[1] for b in self.grid.grid_bounds], dtype=torch.float64)
            pp = self._probe = (lo + (0.02 + 0.96 * u) * (hi - lo)).to(self.device, self.dtype).contiguous()
        return pp

    def measure_mean(self, st, tcol64_dev, mean_pcg_at):
        """The bound of mean_monitor has grown past its limit (it grows with the data, the error need not): compare the factor's mean with
        the PCG mean on the probe set.  mean_pcg_at(points) -> PCG means [n] (the caller solves).  Within a quarter of the tolerance the
        factor keeps serving the mean for the next MEAN_MEASURE_EVERY monitor calls; otherwise it is switched off, as before."""
        lim = settings.spectral_mean_tolerance.value()
        if lim is None:
            lim = 1e-2 if self.dtype == torch.float32 else 1e-4
        pts = self.probe_points()
        m_pcg = mean_pcg_at(pts).double().reshape(-1)
        m_fac = SpectralQuery(self, st, pts, tcol64_dev).mean().reshape(-1)
        self.last_measured = float(((m_fac - m_pcg).abs().max() / m_pcg.abs().max().clamp_min(1e-300)))
        self._measured_at = self.__dict__.get("_monitor_calls", 0)
        self.measurements += 1
        self.measure_due = False
        self.mean_ok = self.last_measured <= 0.25 * lim
        return self.mean_ok

    # ------------------------------------------------------------------ reference statistics --
    def _project_grid_vectors(self, basis, Vm):
        """B^T v for grid vectors: Vm [c, m] (any float dtype) -> fp64 [c, r] by d mode products + a gather."""
        g = self.grid.g
        P = Vm.double().reshape((Vm.shape[0],) + tuple(g))
        for q in range(self.grid.d):
            P = torch.tensordot(P, basis.Vq[q], dims=([1], [0]))             # contracts the leading grid dim, appends k_q
        idx = (slice(None),) + tuple(basis.S_long[q] for q in range(self.grid.d))
        return P[idx]

    def _basis_columns(self, basis, lo, hi):
        """Basis functions lo..hi as grid vectors [hi - lo, m] in the model dtype."""
        c = hi - lo
        Bc = basis.Vq[0][:, basis.S_long[0, lo:hi]].t()                      # [c, g_0]
        for q in range(1, self.grid.d):
            col = basis.Vq[q][:, basis.S_long[q, lo:hi]].t()                 # [c, g_q]
            Bc = Bc.reshape(c, -1, 1) * col.reshape(c, 1, -1)
        return Bc.reshape(c, self.grid.m).to(self.dtype).contiguous()

    def build_reference(self, basis, stencil, b):
        """G_ref = B^T A B, h_ref = B^T b from the model's statistics (r SpMV columns in chunks of 64)."""
        r = basis.r
        if self.grid.m <= settings.max_cholesky_size.value():
            # small grid (the dense regime, where this build recurs: fit() rebuilds the statistics every epoch): all r basis functions as
            # ONE many-column stencil product and one MFMA GEMM instead of r / 64 chunks of product + d mode products + gather each
            Bc = self._basis_columns(basis, 0, r)                                  # [r, m], model dtype
            AB = grid_ops.stencil_spmv(self.grid, stencil, Bc)                     # rows = A b_j
            Bd = Bc.double().contiguous()
            G = grid_ops.gemm(AB.double().contiguous(), Bd, tb=True)               # (A B)^T B
            self.G_ref = (0.5 * (G + G.t())).contiguous()
            self.h_ref = torch.mv(Bd, b.reshape(-1).double()).contiguous()
            self.ref = basis
            self.cur = None
            self.data_version += 1
            self.rebuilds += 1
            return
        G = torch.empty((r, r), dtype=torch.float64, device=self.device)
        for lo in range(0, r, 64):
            hi = min(lo + 64, r)
            AB = grid_ops.stencil_spmv(self.grid, stencil, self._basis_columns(basis, lo, hi))
            G[lo:hi] = self._project_grid_vectors(basis, AB)
        self.G_ref = (0.5 * (G + G.t())).contiguous()
        self.h_ref = self._project_grid_vectors(basis, b.reshape(1, -1))[0].contiguous()
        self.ref = basis
        self.cur = None
        self.data_version += 1
        self.rebuilds += 1

    def absorb(self, X, wa, wby):
        """Statistics += the points X with weights wa (None: unit) and weighted targets wby = y / noise: follow in the
        reference basis.  One projection kernel + one fp64 MFMA GEMM."""
        if self.ref is None:
            return
        sc = None if wa is None else wa.sqrt().contiguous()
        F = grid_ops.basis_project(self.grid, X, self.ref.Vtab, self.ref.kmax, self.ref.S, scale=sc, err=self.err)
        grid_ops.gemm(F, F, ta=True, alpha=1.0, beta=1.0, C=self.G_ref)
        # h_ref += F^T t, t = wby (/ sqrt(wa): the rows of F already carry it) -- one small launch (wiski_basis_absorb_h)
        wby = wby.contiguous()
        rc = _hip.fn("wiski_basis_absorb_h", wby.dtype)(ctypes.c_int64(F.shape[0]), ctypes.c_int32(F.shape[1]), _hip.dptr(F), ctypes.c_int64(F.shape[1]),
                                                        _hip.dptr(wby), _hip.dptr(sc), _hip.dptr(self.h_ref), _hip.stream_ptr(self.device))
        _hip.check(rc, "wiski_basis_absorb_h")
        self.data_version += 1
        self.idle_absorbs += 1

    # --------------------------------------------------------------------------- derived state --
    def state(self, key, tcol64, kscale, eig=None, _host_path=False):
        """The factor for the hyper-parameters identified by `key` (Toeplitz columns tcol64 on the host or device, fp64;
        Kt = kscale * Kuu).  None when the reduced basis would exceed settings.spectral_max_rank."""
        cur = self.cur
        self.idle_absorbs = 0
        if cur is not None and cur["key"] == key and cur["data_version"] == self.data_version and cur["kscale"] == kscale:
            return cur
        tail = default_tail(self.dtype)
        if cur is not None and cur["key"] == key:
            basis, TS, defect_ok = cur["basis"], cur["TS"], True
        elif not _host_path and cur is not None and self.ref is not None and torch.is_tensor(tcol64) and tcol64.is_cuda \
                and self._device_refresh_ok(cur, key):
            if settings.fused_factor_refresh.on():
                # the whole refresh -- eigenvectors, change of basis, G, C, Cholesky + inverse, tail -- behind ONE C call (wiski_factor_refresh)
                new = self._device_refresh_fused(cur, key, tcol64, tail, kscale)
                if self._chk is not None and not self._verdict():
                    self.cur = None
                    return self.state(key, tcol64, kscale, eig=eig, _host_path=True)
                self.cur = new
                return new
            basis, TS = self._device_refresh(cur, tcol64, tail)
            defect_ok = True
        else:
            self._chk = None
            self._dev_refreshes = 0
            tc = tcol64.detach().to("cpu", torch.float64).numpy() if torch.is_tensor(tcol64) else np.asarray(tcol64, dtype=np.float64)
            fast = settings.fast_pred_var.on()
            cap = min(settings.spectral_max_rank.value(), settings.max_root_decomposition_size.value()) if fast else settings.spectral_max_rank.value()
            basis = select_basis(self.grid, tc, tail, cap, self.device, eig=eig, like=None if cur is None else cur["basis"], truncate=fast)
            if basis is None:
                return None
            TS, defect_ok = None, False
        if self.ref is None:
            return {"need_reference": True, "basis": basis, "tail": tail}
        if TS is None:
            TS, wdef = self._change_of_basis(basis)
            defect_ok = wdef <= tail
            if not defect_ok:
                return {"need_reference": True, "basis": basis, "tail": tail}
        GT = grid_ops.gemm(self.G_ref, TS, ta=True)                           # G_ref TS [r_ref, r]: G_ref is symmetric, and A^T B is the faster form of the fp64 tile kernels
        G = grid_ops.gemm(TS, GT, ta=True)                                    # T^T G_ref T
        C, lam, sq, sqG = grid_ops.woodbury_c(G, basis.lam_kuu, kscale)       # I + Lam^1/2 G Lam^1/2 (and Lam^1/2 G for the MLL backward)
        # C = I + PSD: cannot fail on finite input.  With the factor its explicit inverse (r^3 / 3 flop more): every later solve
        # against it -- mean, variances, MLL terms -- is then ONE GEMM / GEMV launch instead of a blocked sweep of ~2 r / 64
        # launches.  Two launches in all for r <= 480 (dense_small.h).
        info = self.__dict__.get("_info")                 # (never read back: C = I + PSD; one persistent word instead of a fill launch per refresh)
        if info is None:
            info = self._info = torch.zeros(1, dtype=torch.int32, device=self.device)
        Linv, info = grid_ops.potrf_inverse_(C, info=info)
        cur = {"key": key, "kscale": kscale, "data_version": self.data_version, "basis": basis, "TS": TS, "lam": lam, "sq": sq, "G": G,
               "chol": C, "Linv": Linv, "info": info, "tail": tail, "sqG": sqG}
        # hr = T^T h_ref, c = chol^-1 Lam^1/2 hr, b^T M b = |c|^2, t = chol^-T c, the mean coefficients and logdet (wiski_factor_tail)
        hr, ch, t, coef, zeta, bMb, logdet = grid_ops.factor_tail(TS, self.h_ref, sq, Linv, C)
        cur.update(hr=hr, c_half=ch, t=t, coef=coef, zeta=zeta, bMb=bMb, logdet=logdet)
        if self._chk is not None and not self._verdict():
            # the device-refreshed basis failed its check (eigen-residual, trace left out by the kept index set, defect of the
            # reference span): nothing built on it is used -- the host path selects afresh.  The verdict was copied back right
            # after the change of basis was queued, so by now (a factorisation's worth of launches later) it has arrived.
            self.cur = None
            return self.state(key, tcol64, kscale, eig=eig, _host_path=True)
        self.cur = cur
        return cur

    # ---- hyper-parameter step without a host round trip: refine the eigenvectors on the device, keep the index set, verify late
    def _device_refresh_ok(self, cur, key):
        basis = cur["basis"]
        if key[1:] != cur["key"][1:] or not basis.device_refreshable() or not settings.spectral_device_refresh.on():
            return False
        if self._dev_refreshes >= RESELECT_EVERY and basis.r < self.grid.m:      # re-select the index set now and then (it only ever grows stale;
            return False                                                         #  a FULL basis -- small grids, no spectral gap -- has nothing to select)
        return True

    def _verdict(self):
        """Verdict of the device refresh just queued (its three numbers were copied to pinned memory asynchronously)."""
        host, ev, lim = self._chk
        ev.synchronize()
        resid, short, wdef = (float(v) for v in host)
        self._chk = None
        self.last_verdict = (resid, short, wdef)
        return resid <= lim[0] and short <= lim[1] and wdef <= lim[2]

    def _grid_dev(self):
        gd = self.__dict__.get("_g_dev")
        if gd is None:
            gd = self._g_dev = (torch.tensor(list(self.grid.g), dtype=torch.int32, device=self.device),)
        return gd

    def _device_refresh(self, cur, tcol64, tail):
        old = cur["basis"]
        gd = self._grid_dev()
        # three launches: the eigenvector refresh, the change of basis with its verdict, the verdict's copy to pinned memory
        ref = self.ref
        # (adaptive: Rayleigh-Ritz in the previous span; subspace iteration only if the residual gets within a factor 8 of the verdict's limit)
        Vtab, ev_tab, resid, Tq = grid_ops.basis_eig_update(gd[0], tcol64, old.Vtab, old.kmax, old.kuse, ref.Vtab, ref.kmax,
                                                            resid_ok=tail * 1e-3 / 8.0)
        work = self.__dict__.get("_bc_work")
        if work is None or work.shape[0] < old.r + 1:
            work = self._bc_work = torch.zeros(max(old.r + 1, 2049), dtype=torch.float64, device=self.device)
        # (the verdict goes straight into pinned host memory from the kernel -- no copy launch; two alternating buffers: the previous
        #  verdict may not have been read yet when the next refresh is queued)
        host, ev = self._verdict_slot()
        TS, lam, _ = grid_ops.basis_change(gd[0], Tq, ref.kmax, ref.S, old.kmax, old.S, ev_tab, tcol64, resid, work[:old.r + 1], verdict_pinned=host)
        basis = SpectralBasis.on_device(old, Vtab, ev_tab, None, lam=lam)
        ev.record()
        # limits: the eigen-residual far below the tail; the index set may leave out up to 1.5 x the tail (or what a rank-capped
        # selection left out to begin with) before it is re-selected
        self._chk = (host, ev, (tail * 1e-3, 1.5 * max(tail, old.short0), tail))
        self._dev_refreshes += 1
        self.device_refreshes += 1
        return basis, TS

    def _verdict_slot(self):
        """(pinned verdict buffer, event) of the next refresh: two alternating pairs, the previous verdict may not have been read yet
        when the next refresh is queued.  The events are recorded once where they are made -- torch creates the handle at the first
        record, and the C call (verdict_event) records a handle, not the Python object -- so a factor that makes its own pair (a
        clone() drops the original's) never hands C a null handle."""
        hosts = self.__dict__.get("_chk_hosts")
        if hosts is None:
            hosts = self._chk_hosts = [torch.zeros(3, dtype=torch.float64).pin_memory(), torch.zeros(3, dtype=torch.float64).pin_memory()]
            self._chk_events = [torch.cuda.Event(), torch.cuda.Event()]
            for e_ in self._chk_events:
                e_.record()
        slot = self._dev_refreshes_total = (self.__dict__.get("_dev_refreshes_total", 0) + 1) & 1
        return hosts[slot], self._chk_events[slot]

    def _device_refresh_fused(self, cur, key, tcol64, tail, kscale):
        """_device_refresh + everything state() builds on it, queued by one call (grid_ops.factor_refresh); returns the new state."""
        old, ref = cur["basis"], self.ref
        gd = self._grid_dev()
        work = self.__dict__.get("_bc_work")
        if work is None or work.shape[0] < old.r + 1:
            work = self._bc_work = torch.zeros(max(old.r + 1, 2049), dtype=torch.float64, device=self.device)
        host, ev = self._verdict_slot()
        info = self.__dict__.get("_info")
        if info is None:
            info = self._info = torch.zeros(1, dtype=torch.int32, device=self.device)
        o = grid_ops.factor_refresh(gd[0], tcol64, old.Vtab, old.kmax, old.kuse, ref.Vtab, ref.kmax, ref.S, old.S, work, host, self.G_ref, self.h_ref,
                                    kscale, info, resid_ok=tail * 1e-3 / 8.0, verdict_event=ev)
        basis = SpectralBasis.on_device(old, o["Vtab"], o["ev"], None, lam=o["lam_kuu"])
        self._chk = (host, ev, (tail * 1e-3, 1.5 * max(tail, old.short0), tail))
        self._dev_refreshes += 1
        self.device_refreshes += 1
        hr, ch, t, coef, zeta, bMb, logdet = o["tail"]
        return {"key": key, "kscale": kscale, "data_version": self.data_version, "basis": basis, "TS": o["TS"], "lam": o["lam"], "sq": o["sq"], "G": o["G"],
                "chol": o["chol"], "Linv": o["Linv"], "info": info, "tail": tail, "sqG": o["sqG"], "hr": hr, "c_half": ch, "t": t, "coef": coef,
                "zeta": zeta, "bMb": bMb, "logdet": logdet}

    def _change_of_basis(self, basis):
        """T [r_ref, r] and the eigenvalue-weighted defect max_j lam_j (1 - |T[:, j]|^2) / trace (what the reference
        span misses of each current basis vector, in units of the trace)."""
        ref = self.ref
        d = self.grid.d
        if ref.Vtab_host is None or basis.Vtab_host is None:
            raise RuntimeError("change of basis on the host needs host copies of both bases")
        Th = [ref.Vtab_host[q].T @ basis.Vtab_host[q] for q in range(d)]                        # [kmax_ref, kmax] per dim
        packed = torch.as_tensor(np.concatenate([t.reshape(-1) for t in Th])).to(self.device)
        TS, off = None, 0
        for q in range(d):
            Tq = packed[off:off + Th[q].size].view(Th[q].shape)
            off += Th[q].size
            blk = Tq[ref.S_long[q]][:, basis.S_long[q]]
            TS = blk if TS is None else TS * blk
        TS = TS.contiguous()
        defect = (1.0 - (TS * TS).sum(0)).clamp_min(0.0)
        total = 1.0
        for q in range(d):
            total *= float(basis.evs[q].sum())
        wdef = float((basis.lam_kuu * defect).max()) / total * basis.r        # as if every vector missed as much as the worst
        return TS, wdef

    # ----------------------------------------------------------------------------- consumers --
    def coefficients(self, st):
        """Posterior-mean coefficients c (mu_u ~= B c) and zeta = B^T Kt^-1 mu_u = c / lam."""
        if "coef" not in st:
            if "t" not in st:
                st["t"] = torch.mv(st["Linv"].t(), st["c_half"])
            st["coef"] = st["sq"] * st["t"]
            st["zeta"] = st["t"] / st["sq"]
        return st["coef"], st["zeta"]

    def query(self, st, X, tcol64_dev):
        return SpectralQuery(self, st, X, tcol64_dev)

    def rel_bound(self):
        """max over the last query batch of tail / variance (host sync; diagnostics and tests)."""
        tailv, diag = self._last
        self.last_rel_bound = float((tailv / (diag + tailv).clamp_min(1e-300)).max())
        return self.last_rel_bound

    def mll_backward(self, st, g_bMb, g_logdet, kap=None):
        """(d/d tcol [sum g] fp64, d/d kscale) of  g_bMb * b^T M b + g_logdet * logdet(I + Kt A)  in the reduced basis:
        d(b^T M b) = zeta^T (B^T dKt B) zeta,  d logdet = tr(S_B B^T dKt B),  S_B = G - G M_r G,  M_r = Lam^1/2 C^-1 Lam^1/2."""
        basis, G, sq = st["basis"], st["G"], st["sq"]
        if kap is None:
            kap = st["kscale"]                   # (a device scalar is handed in when the call is recorded into a captured graph)
        _, zeta = self.coefficients(st)
        # (the incoming gradients stay on the device: reading them would stall the host behind everything queued so far)
        sqG = st.get("sqG")
        Y2 = grid_ops.gemm(st["Linv"], sqG if sqG is not None else (sq[:, None] * G).contiguous())   # chol^-1 Lam^1/2 G
        P = grid_ops.gemm(Y2, Y2, ta=True)                                        # G M_r G
        if not torch.is_tensor(g_bMb):
            g_bMb = torch.tensor(float(g_bMb), dtype=torch.float64, device=self.device)
        if not torch.is_tensor(g_logdet):
            g_logdet = torch.tensor(float(g_logdet), dtype=torch.float64, device=self.device)
        # Wt = g_logdet S_B + g_bMb zeta zeta^T and its trace against lam in one launch (wiski_mll_weights)
        Wt, g_kap = grid_ops.mll_weights(G, P, zeta.contiguous(), basis.lam_kuu, g_bMb.double().contiguous(), g_logdet.double().contiguous())
        D = grid_ops.basis_pair_reduce(Wt, basis.S, basis.ev_tab, basis.kmax)
        gs = self.grid.g
        if max(gs) <= 64:
            # the d congruences V_q D_q V_q^T and their lag sums in one launch
            g_tcol = grid_ops.basis_lag_grad(self._grid_dev()[0], basis.Vtab, basis.kmax, D, kap)
            return g_tcol, g_kap
        else:
            g_tcol = torch.zeros(sum(gs), dtype=torch.float64, device=self.device)
            off = 0
            for q, gq in enumerate(gs):
                H = basis.Vq[q] @ D[q, :basis.kmax, :basis.kmax] @ basis.Vq[q].t()                 # [g_q, g_q]
                g_tcol[off:off + gq] = torch.mv(self._lag_matrix(gq), H.reshape(-1))               # sums along the lag diagonals
                off += gq
        return g_tcol * kap, g_kap

    def _lag_matrix(self, g):
        """One-hot [g, g * g]: row l selects the entries (i, j) of a g x g matrix with |i - j| = l (a GEMV instead of an
        index_add: 5 us instead of 31)."""
        cache = self.__dict__.setdefault("_lag_cache", {})
        if g not in cache:
            i = torch.arange(g, device=self.device)
            lag = (i[:, None] - i[None, :]).abs().reshape(-1)
            Lm = torch.zeros((g, g * g), dtype=torch.float64, device=self.device)
            Lm[lag, torch.arange(g * g, device=self.device)] = 1.0
            cache[g] = Lm
        return cache[g]


class SpectralQuery:
    """Predictive moments of one query batch from a factor state: ONE projection kernel (F = W(X) B Lam^1/2 and the prior
    variances), then mean = F t with t = chol^-T chol^-1 Lam^1/2 h, variances = column norms of chol^-1 F^T + the left-out
    prior variance, covariance blocks by one more GEMM.  Everything un-scaled (multiply by sigma2 for BFN:227-228)."""

    def __init__(self, fac, st, X, tcol64_dev):
        self.fac, self.st = fac, st
        basis = st["basis"]
        self.Fs, prior = grid_ops.basis_project(fac.grid, X, basis.Vtab, basis.kmax, basis.S, colscale=st["sq"], tcol=tcol64_dev, want_prior=True,
                                                err=fac.err)
        self.prior = prior
        self.X, self.tcol = X, tcol64_dev
        self._Y = self._diag = self._tail = None

    def mean(self):
        st = self.st
        if "t" not in st:
            st["t"] = torch.mv(st["Linv"].t(), st["c_half"])
        return torch.mv(self.Fs, st["t"])

    def _solve(self):
        if self._Y is None:
            st = self.st
            if self.Fs.shape[0] == 1:                                            # one query: a matrix-vector product, not a 64-wide GEMM tile
                self._Y = torch.mv(st["Linv"], self.Fs[0])[:, None]
            else:
                self._Y = grid_ops.gemm(st["Linv"], self.Fs, tb=True)            # chol^-1 F^T  [r, n]
            # |Y[:, j]|^2 and the left-out prior variance prior_j - sum_k lam_k (b_k^T w_j)^2, clamped
            self._diag, self._tail = grid_ops.spectral_var(self._Y, self.Fs, self.prior, st["kscale"])
            self.fac._last = (self._tail, self._diag)
        return self._Y

    def diag(self):
        self._solve()
        return self._diag + self._tail

    def full(self, block=None):
        Y = self._solve()
        if block is None:
            full = grid_ops.gemm(Y, Y, ta=True)
            full.diagonal().add_(self._tail)
            return full
        Yb = Y.reshape(Y.shape[0], -1, block).permute(1, 0, 2)                   # [nb, r, q]
        full = torch.bmm(Yb.transpose(1, 2), Yb)
        full.diagonal(dim1=-2, dim2=-1).add_(self._tail.reshape(-1, block))
        return full

    # ---- input gradients (the posterior w.r.t. its query points; DESIGN.md "Posterior gradients"): every moment is a function of F
    # (and of the prior variances through the tail), so each backward below reduces the upstream gradient to (G_F, G_prior) in fp64
    # and ends in ONE wiski_basis_project_vjp launch for the whole batch
    def grad_x(self, GF, Gprior=None):
        """d/dX of sum(GF * F) + sum(Gprior * prior): [n, d] in X's dtype."""
        basis = self.st["basis"]
        return grid_ops.basis_project_vjp(self.fac.grid, self.X, basis.Vtab, basis.kmax, basis.S, GF, Gprior, colscale=self.st["sq"], tcol=self.tcol)

    def mean_grad(self, g):
        """mean = F t."""
        self.mean()
        return self.grad_x(g.double()[:, None] * self.st["t"][None, :])

    def _tail_grad(self, g, GF):
        """tail = max(kscale prior - |F_p|^2, 0) with upstream g [n]: subtracts its F part from GF, returns G_prior."""
        on = (self._tail > 0).double() * g
        GF.sub_(2.0 * on[:, None] * self.Fs)
        return on * self.st["kscale"]

    def diag_grad(self, g):
        """diag() = |Y_p|^2 + tail, Y = chol^-1 F^T: G_F[p] = 2 g_p (chol^-T Y_p)."""
        g = g.double()
        Y = self._solve()
        GF = 2.0 * g[:, None] * (Y.t() @ self.st["Linv"])
        return self.grad_x(GF, self._tail_grad(g, GF))

    def full_grad(self, G, block=None):
        """full(block) = Y^T Y + diag(tail) (per block of q): G_Y = Y (G + G^T), G_F = G_Y^T chol^-1."""
        G = G.double()
        Gs = G + G.transpose(-1, -2)
        Y = self._solve()
        r, n = Y.shape
        if block is None:
            GY, gd = Y @ Gs, G.diagonal()
        else:
            Yb = Y.reshape(r, -1, block).permute(1, 0, 2)
            GY, gd = torch.bmm(Yb, Gs).permute(1, 0, 2).reshape(r, n), G.diagonal(dim1=-2, dim2=-1).reshape(-1)
        GF = GY.t() @ self.st["Linv"]
        return self.grad_x(GF, self._tail_grad(gd, GF))

    def root_grad(self, GR=None, gextra=None):
        """The root Y^T [n, r] and the diagonal term tail of ``root_decomposition``."""
        self._solve()
        n, r = self.Fs.shape
        GF = torch.zeros((n, r), dtype=torch.float64, device=self.Fs.device) if GR is None else GR.double() @ self.st["Linv"]
        return self.grad_x(GF, None if gextra is None else self._tail_grad(gextra.double(), GF))
