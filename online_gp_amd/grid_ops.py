"""Torch-tensor front-end of the C ABI (include/wiski.h): one function per
entry point, device pointers borrowed from contiguous ROCm tensors, launches on
torch's current stream.  Host-side plumbing only -- all arithmetic happens in
the HIP kernels under csrc/.
"""
import ctypes
import math
import time
import warnings

import numpy as np

import torch

from . import _hip


class GridSpec:
    """Inducing-grid geometry.  Mirrors gpytorch's GridInterpolationKernel grid
    (reference call site online_gp/models/batched_fixed_noise_online_gp.py:114-120):
    ``delta=(hi-lo)/(g-2)``, ``grid=linspace(lo-delta, hi+delta, g)``."""

    def __init__(self, grid_bounds, grid_size):
        gb = [[float(lo), float(hi)] for lo, hi in (torch.as_tensor(grid_bounds, dtype=torch.float64).reshape(-1, 2).tolist())]
        d = len(gb)
        if not 1 <= d <= _hip.MAX_DIM:
            raise ValueError(f"grid dimension must be 1..{_hip.MAX_DIM}, got {d}")
        if isinstance(grid_size, int):
            g = [grid_size] * d
        else:
            g = [int(v) for v in grid_size]
        if len(g) != d:
            raise ValueError("grid_size / grid_bounds mismatch")
        if min(g) < 4:
            raise ValueError("cubic interpolation needs at least 4 grid points per dim")
        self.d = d
        self.g = g
        self.grid_bounds = gb
        delta = [(hi - lo) / (gi - 2) for (lo, hi), gi in zip(gb, g)]
        self.g0 = [lo - dl for (lo, hi), dl in zip(gb, delta)]
        self.h = [((hi + dl) - g0) / (gi - 1) for (lo, hi), dl, g0, gi in zip(gb, delta, self.g0, g)]
        from . import settings

        if settings.float32_grid.on():          # gpytorch's float32 grid, promoted
            for q, ((lo, hi), gi) in enumerate(zip(gb, g)):
                dl = torch.tensor(hi - lo, dtype=torch.float32) / (gi - 2)
                pts = torch.linspace(float(torch.tensor(lo, dtype=torch.float32) - dl), float(torch.tensor(hi, dtype=torch.float32) + dl), gi,
                                     dtype=torch.float32)
                self.g0[q] = float(pts[0])
                self.h[q] = float(pts[1] - pts[0])
        self.m = int(math.prod(g))
        self.T = 4 ** d
        self.R = 7 ** d
        c = _hip.wiski_grid()
        c.d = d
        for q in range(d):
            c.g[q] = g[q]
            c.g0[q] = self.g0[q]
            c.h[q] = self.h[q]
        self.c = c

    @property
    def ref(self):
        return ctypes.byref(self.c)

    def shifted(self, below, above):
        """The grid changed by whole nodes at unchanged spacing: ``below[q]`` nodes added in front of dim q and ``above[q]`` behind it
        (ints or per-dim sequences, negative: removed).  Node arithmetic, ``g0' = g0 - below h``, ``h' = h``, ``g' = g + below + above``
        -- nothing is recomputed from bounds, so the nodes both grids have coincide up to the rounding of one product and one sum (with
        ``settings.float32_grid`` on, ``g0'`` is rounded to float32 as the constructor's grid is).  ``grid_bounds`` become the bounds from
        which the constructor's recipe (``delta = (hi - lo) / (g - 2)``, ``linspace(lo - delta, hi + delta, g)``) builds this very grid:
        ``lo' = g0' + h (g' - 1) / g'`` and ``hi' = g0' + h (g' - 1)^2 / g'``, so that ``GridSpec(new.grid_bounds, new.g)`` has the same
        nodes up to rounding and ``shifted(0, 0)`` returns the old bounds.  (That recipe's spacing is ``delta g / (g - 1)``, not delta: lo
        and hi lie a little outside node 1 and node g - 2, the box whose points are interior.)  The statistics of a model move with
        ``regrid_stats``."""
        a = [int(below)] * self.d if isinstance(below, int) else [int(v) for v in below]
        b = [int(above)] * self.d if isinstance(above, int) else [int(v) for v in above]
        if len(a) != self.d or len(b) != self.d:
            raise ValueError(f"below / above need one entry per grid dim ({self.d})")
        g = [gq + aq + bq for gq, aq, bq in zip(self.g, a, b)]
        if min(g) < 4:
            raise ValueError("cubic interpolation needs at least 4 grid points per dim")
        if any(aq <= -gq or aq >= gn for gq, aq, gn in zip(self.g, a, g)):
            raise ValueError("the shifted grid must share at least one node with the old one in every dim")
        from . import settings

        new = object.__new__(GridSpec)
        new.d, new.g, new.h = self.d, g, list(self.h)
        new.g0 = [g0 - aq * h for g0, aq, h in zip(self.g0, a, self.h)]
        if settings.float32_grid.on():
            new.g0 = [float(torch.tensor(v, dtype=torch.float32)) for v in new.g0]
        new.grid_bounds = [[g0 + h * (gq - 1) / gq, g0 + h * (gq - 1) ** 2 / gq] for g0, h, gq in zip(new.g0, new.h, g)]
        new.m = int(math.prod(g))
        new.T, new.R = self.T, self.R
        c = _hip.wiski_grid()
        c.d = new.d
        for q in range(new.d):
            c.g[q], c.g0[q], c.h[q] = g[q], new.g0[q], new.h[q]
        new.c = c
        return new

    def grid_points(self, dtype=torch.float64, device="cpu"):
        """Per-dim 1-D grids (list of d tensors), as gpytorch's ``covar_module.grid``."""
        return [self.g0[q] + self.h[q] * torch.arange(self.g[q], dtype=dtype, device=device) for q in range(self.d)]

    def stencil_offsets(self, device="cpu"):
        offs = torch.zeros(1, dtype=torch.int64)
        stride = [int(math.prod(self.g[q + 1:])) for q in range(self.d)]
        for q in range(self.d):
            offs = (offs[:, None] + (torch.arange(7) - 3)[None, :] * stride[q]).reshape(-1)
        return offs.to(device)


def new_err_flag(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


def read_flag(flag):
    """Host value of a device int32 flag after everything queued so far on the current stream (no stream sync)."""
    val = ctypes.c_int32(0)
    rc = _hip.lib().wiski_read_flag(_hip.dptr(flag), ctypes.byref(val), _hip.stream_ptr(flag.device))
    _hip.check(rc, "wiski_read_flag")
    return int(val.value)


def _x2d(x, grid):
    if x.dim() != 2 or x.shape[1] != grid.d:
        raise ValueError(f"expected inputs of shape [n, {grid.d}], got {tuple(x.shape)}")
    return x.contiguous()


def interp(grid, x, err):
    """(idx int32 [n,T], val [n,T]) -- a1."""
    x = _x2d(x, grid)
    n = x.shape[0]
    idx = torch.empty((n, grid.T), dtype=torch.int32, device=x.device)
    val = torch.empty((n, grid.T), dtype=x.dtype, device=x.device)
    rc = _hip.fn("wiski_interp", x.dtype)(grid.ref, _hip.dptr(x), ctypes.c_int64(n), _hip.dptr(idx), _hip.dptr(val), _hip.dptr(err),
                                          _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_interp")
    return idx, val


def gather(grid, x, V, err, diag=False):
    """W(x) @ V for V given as [k, m]; returns [n, k] (or [n] when diag) -- a14."""
    x = _x2d(x, grid)
    V = V.contiguous()
    if V.dim() == 1:
        V = V[None]
    k = V.shape[0]
    n = x.shape[0]
    assert V.shape[1] == grid.m and V.dtype == x.dtype
    out = torch.empty((n,) if diag else (n, k), dtype=x.dtype, device=x.device)
    rc = _hip.fn("wiski_gather", x.dtype)(grid.ref, _hip.dptr(x), ctypes.c_int64(n), _hip.dptr(V), ctypes.c_int32(k), ctypes.c_int32(int(diag)),
                                          _hip.dptr(out), _hip.dptr(err), _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_gather")
    return out


def gather_grad(grid, x, V, diag=False):
    """d/dx of W(x_p) . V_c  (c = 0, or c = p when diag): [n, d]."""
    x = _x2d(x, grid)
    V = V.contiguous()
    out = torch.empty((x.shape[0], grid.d), dtype=x.dtype, device=x.device)
    rc = _hip.fn("wiski_gather_grad", x.dtype)(grid.ref, _hip.dptr(x), ctypes.c_int64(x.shape[0]), _hip.dptr(V), ctypes.c_int32(int(diag)),
                                               _hip.dptr(out), _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_gather_grad")
    return out


class InterpDot(torch.autograd.Function):
    """f(x)_p = W(x_p) . V_c (c = 0 or c = p), differentiable w.r.t. the inputs x only."""

    @staticmethod
    def forward(ctx, grid, x, V, diag, err):
        xd = x.detach().contiguous()
        Vd = V.detach().contiguous().reshape(-1, grid.m)
        ctx.grid, ctx.diag = grid, diag
        ctx.save_for_backward(xd, Vd)
        out = gather(grid, xd, Vd, err, diag=diag)
        return out if diag else out[:, 0]

    @staticmethod
    def backward(ctx, g):
        xd, Vd = ctx.saved_tensors
        gx = gather_grad(ctx.grid, xd, Vd, diag=ctx.diag) * g[:, None]
        return None, gx, None, None, None


def gather_rows(grid, x, Vr, err):
    """W(x) @ Vr for a row-major dense operand Vr [m, ncols]; returns [n, ncols]."""
    x = _x2d(x, grid)
    Vr = Vr.contiguous()
    assert Vr.shape[0] == grid.m and Vr.dtype == x.dtype
    out = torch.empty((x.shape[0], Vr.shape[1]), dtype=x.dtype, device=x.device)
    rc = _hip.fn("wiski_gather_rows", x.dtype)(grid.ref, _hip.dptr(x), ctypes.c_int64(x.shape[0]), _hip.dptr(Vr), ctypes.c_int32(Vr.shape[1]),
                                               _hip.dptr(out), _hip.dptr(err), _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_gather_rows")
    return out


def gather_rows_vjp(grid, x, Vr, G):
    """Input gradient of :func:`gather_rows`: gx[p] = sum_c G[p, c] d/dx_p (W(x_p) Vr)[c], [n, d] (``wiski_gather_rows_vjp``)."""
    x = _x2d(x, grid)
    Vr, G = Vr.contiguous(), G.contiguous().to(x.dtype)
    assert Vr.shape[0] == grid.m and Vr.dtype == x.dtype and G.shape == (x.shape[0], Vr.shape[1])
    gx = torch.empty((x.shape[0], grid.d), dtype=x.dtype, device=x.device)
    rc = _hip.fn("wiski_gather_rows_vjp", x.dtype)(grid.ref, _hip.dptr(x), ctypes.c_int64(x.shape[0]), _hip.dptr(Vr), ctypes.c_int32(Vr.shape[1]),
                                                   _hip.dptr(G), _hip.dptr(gx), _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_gather_rows_vjp")
    return gx


class Gather(torch.autograd.Function):
    """:func:`gather` (k columns, or ``diag``) differentiable w.r.t. the inputs x and the dense operand V [k, m] (or [n, m] with
    ``diag``).  x: a few columns take wiski_gather_grad per column (``InterpDot``'s kernel), many take wiski_gather_rows_vjp on V^T;
    V: the sparse scatter of g_p w_p (``scatter_stats`` per column, ``wt_columns`` rows for ``diag``) -- W itself is never formed."""

    @staticmethod
    def forward(ctx, grid, x, V, err, diag=False):
        xd, Vd = x.detach().contiguous(), V.detach().contiguous()
        ctx.grid, ctx.diag, ctx.err = grid, diag, err
        ctx.save_for_backward(xd, Vd)
        return gather(grid, xd, Vd, err, diag=diag)

    @staticmethod
    def backward(ctx, g):
        xd, Vd = ctx.saved_tensors
        grid, V2 = ctx.grid, Vd.reshape(-1, ctx.grid.m)
        g = g.contiguous()
        gx = gV = None
        if ctx.needs_input_grad[1]:
            if ctx.diag:
                gx = gather_grad(grid, xd, V2, diag=True) * g[:, None]
            elif V2.shape[0] <= 4:
                gx = sum(gather_grad(grid, xd, V2[c]) * g[:, c, None] for c in range(V2.shape[0]))
            else:
                gx = gather_rows_vjp(grid, xd, V2.t(), g)
        if ctx.needs_input_grad[2]:
            if ctx.diag:
                gV = wt_columns(grid, xd, ctx.err) * g[:, None]
            else:
                gV = torch.zeros_like(V2)
                ones = torch.ones(xd.shape[0], dtype=xd.dtype, device=xd.device)
                stats = torch.zeros(2, dtype=torch.float64, device=xd.device)
                for c in range(V2.shape[0]):
                    scatter_stats(grid, xd, g[:, c].contiguous(), ones, ones, ones, gV[c], None, stats, ctx.err)
            gV = gV.reshape(Vd.shape)
        return None, gx, gV, None, None


class GatherRows(torch.autograd.Function):
    """:func:`gather_rows` differentiable w.r.t. the inputs x (wiski_gather_rows_vjp); Vr is a constant."""

    @staticmethod
    def forward(ctx, grid, x, Vr, err):
        xd, Vd = x.detach().contiguous(), Vr.detach().contiguous()
        ctx.grid = grid
        ctx.save_for_backward(xd, Vd)
        return gather_rows(grid, xd, Vd, err)

    @staticmethod
    def backward(ctx, g):
        xd, Vd = ctx.saved_tensors
        return None, gather_rows_vjp(ctx.grid, xd, Vd, g), None, None


def _bilinear_args(grid, A, xL, xR):
    """(A, lda, xL [nb, qL, d], xR [nb, qR, d] or None) checked for wiski_interp_bilinear(_vjp)."""
    if A.dim() != 2 or A.shape[0] != grid.m or A.shape[1] < grid.m or A.stride(1) != 1:
        raise ValueError(f"interp_bilinear needs a row-major table A [{grid.m}, >= {grid.m}], got {tuple(A.shape)}")
    if xL.dim() != 3 or xL.shape[-1] != grid.d or A.dtype != xL.dtype:
        raise ValueError(f"interp_bilinear needs xL [nbatch, q, {grid.d}] in A's dtype, got {tuple(xL.shape)} ({xL.dtype})")
    if xR is not None and (xR.dim() != 3 or xR.shape[0] != xL.shape[0] or xR.shape[-1] != grid.d or xR.dtype != xL.dtype):
        raise ValueError(f"interp_bilinear needs xR [{xL.shape[0]}, q', {grid.d}] in xL's dtype, got {tuple(xR.shape)} ({xR.dtype})")
    return A, A.stride(0), xL.contiguous(), None if xR is None else xR.contiguous()


def interp_bilinear_raw(grid, A, xL, xR, err):
    """out[s, a, b] = w(xL[s, a])^T A w(xR[s, b]) for a dense symmetric A [m, m] (``wiski_interp_bilinear``); xR None: xL against
    itself in the kernel's symmetric mode.  xL [nb, qL, d], xR [nb, qR, d] -> [nb, qL, qR]."""
    A, lda, xL, xR = _bilinear_args(grid, A, xL, xR)
    nb, qL = xL.shape[0], xL.shape[1]
    qR = qL if xR is None else xR.shape[1]
    out = torch.empty((nb, qL, qR), dtype=xL.dtype, device=xL.device)
    if out.numel() == 0:
        return out
    rc = _hip.fn("wiski_interp_bilinear", xL.dtype)(grid.ref, _hip.dptr(A), ctypes.c_int64(lda), _hip.dptr(xL), ctypes.c_int32(qL), _hip.dptr(xR),
                                                    ctypes.c_int32(qR), ctypes.c_int64(nb), _hip.dptr(out), _hip.dptr(err), _hip.stream_ptr(xL.device))
    _hip.check(rc, "wiski_interp_bilinear")
    return out


def interp_bilinear_vjp(grid, A, xL, xR, G, want_left=True, want_right=True):
    """Input gradients of :func:`interp_bilinear_raw` for the upstream gradient G [nb, qL, qR]: (gxL, gxR) -- gxR is None in the
    symmetric mode (xR None), where gxL carries the whole gradient (``wiski_interp_bilinear_vjp``)."""
    A, lda, xL, xR = _bilinear_args(grid, A, xL, xR)
    nb, qL = xL.shape[0], xL.shape[1]
    qR = qL if xR is None else xR.shape[1]
    G = G.to(xL.dtype).contiguous()
    assert G.shape == (nb, qL, qR)
    gxL = torch.empty_like(xL) if (want_left or xR is None) else None
    gxR = torch.empty_like(xR) if (want_right and xR is not None) else None
    if nb * qL * qR == 0:                                     # no pairs: zero gradients
        return (None if gxL is None else gxL.zero_()), (None if gxR is None else gxR.zero_())
    rc = _hip.fn("wiski_interp_bilinear_vjp", xL.dtype)(grid.ref, _hip.dptr(A), ctypes.c_int64(lda), _hip.dptr(xL), ctypes.c_int32(qL), _hip.dptr(xR),
                                                        ctypes.c_int32(qR), ctypes.c_int64(nb), _hip.dptr(G), _hip.dptr(gxL), _hip.dptr(gxR),
                                                        _hip.stream_ptr(xL.device))
    _hip.check(rc, "wiski_interp_bilinear_vjp")
    return gxL, gxR


class InterpBilinear(torch.autograd.Function):
    """:func:`interp_bilinear_raw` differentiable w.r.t. the points xL and xR (wiski_interp_bilinear_vjp); the table A is a constant."""

    @staticmethod
    def forward(ctx, grid, A, xL, xR, err):
        xLd = xL.detach().contiguous()
        xRd = None if xR is None else xR.detach().contiguous()
        Ad = A.detach()
        ctx.grid, ctx.sym = grid, xR is None
        ctx.save_for_backward(Ad, xLd, *(() if xRd is None else (xRd,)))
        return interp_bilinear_raw(grid, Ad, xLd, xRd, err)

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        Ad, xLd = saved[0], saved[1]
        xRd = None if ctx.sym else saved[2]
        gxL, gxR = interp_bilinear_vjp(ctx.grid, Ad, xLd, xRd, g, want_left=ctx.needs_input_grad[2],
                                       want_right=(not ctx.sym) and ctx.needs_input_grad[3])
        return None, None, gxL, gxR, None


def interp_bilinear(grid, A, xL, xR=None, err=None):
    """w(xL)^T A w(xR) for a dense symmetric table A [m, m] (the posterior M of the dense regime, or qNIPV's H): xL [..., qL, d] and
    xR [..., qR, d] with the same leading dimensions -> [..., qL, qR]; xR None: xL against itself (exactly symmetric output).
    Differentiable w.r.t. xL and xR.  `err`: the out-of-grid flag to set (a fresh one when None)."""
    lead = tuple(xL.shape[:-2])
    if xR is not None and tuple(xR.shape[:-2]) != lead:
        raise ValueError(f"interp_bilinear: leading dimensions of xL {tuple(xL.shape)} and xR {tuple(xR.shape)} differ")
    err = new_err_flag(xL.device) if err is None else err
    nb = math.prod(lead)
    xL3 = xL.reshape((nb,) + tuple(xL.shape[-2:]))
    xR3 = None if xR is None else xR.reshape((nb,) + tuple(xR.shape[-2:]))
    out = InterpBilinear.apply(grid, A, xL3, xR3, err)
    return out.reshape(lead + tuple(out.shape[-2:]))


_ELL_PACK = {}


def gather_ell(idx, val, v, grid=None):
    """out[r] = sum_t val[r, t] * v[idx[r, t]] from stored interpolation rows (a14, ELL form; BFN:206-210).  With ``grid`` -- the
    rows were written by :func:`interp` on that grid -- large row counts go through ``wiski_gather_ell_grid``: v is first copied
    into a blocked layout in which a row's taps touch about half as many cache lines (csrc/gather_ell_dma.h)."""
    n, T = idx.shape
    out = torch.empty((n,), dtype=val.dtype, device=val.device)
    v = v.contiguous()
    if grid is not None and grid.d >= 2 and T == grid.T:
        f = _hip.lib().wiski_gather_ell_pack_elems
        f.restype = ctypes.c_int64
        ne = int(f(grid.ref))
        key = (val.device, val.dtype)
        pack = _ELL_PACK.get(key)
        if ne and (pack is None or pack.numel() < ne):
            pack = _ELL_PACK[key] = torch.empty((ne,), dtype=val.dtype, device=val.device)
        rc = _hip.fn("wiski_gather_ell_grid", val.dtype)(grid.ref, _hip.dptr(idx), _hip.dptr(val), ctypes.c_int64(n), _hip.dptr(v),
                                                         _hip.dptr(pack) if ne else None, _hip.dptr(out), _hip.stream_ptr(val.device))
        _hip.check(rc, "wiski_gather_ell_grid")
        return out
    rc = _hip.fn("wiski_gather_ell", val.dtype)(_hip.dptr(idx), _hip.dptr(val), ctypes.c_int64(n), ctypes.c_int32(T), _hip.dptr(v),
                                                _hip.dptr(out), _hip.stream_ptr(val.device))
    _hip.check(rc, "wiski_gather_ell")
    return out


def scatter_stats(grid, x, y, wa, wb, noise, b, A_st, stats, err):
    """In-place accumulation of (b, A_st, stats) -- a3/a4/a5."""
    x = _x2d(x, grid)
    n = x.shape[0]
    rc = _hip.fn("wiski_scatter_stats", x.dtype)(grid.ref, _hip.dptr(x), _hip.dptr(y.contiguous()), _hip.dptr(wa.contiguous()),
                                                 _hip.dptr(wb.contiguous()), _hip.dptr(noise.contiguous()), ctypes.c_int64(n), _hip.dptr(b),
                                                 _hip.dptr(A_st), _hip.dptr(stats), _hip.dptr(err), _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_scatter_stats")


def scatter_stats_sym(grid, x, y, wa, wb, noise, b, A_half, stats, err):
    """As scatter_stats, but W^T diag(wa) W goes into a symmetric half-stencil delta [(R+1)/2, m]."""
    x = _x2d(x, grid)
    rc = _hip.fn("wiski_scatter_stats_sym", x.dtype)(grid.ref, _hip.dptr(x), _hip.dptr(y.contiguous()), _hip.dptr(wa.contiguous()),
                                                     _hip.dptr(wb.contiguous()), _hip.dptr(noise.contiguous()), ctypes.c_int64(x.shape[0]),
                                                     _hip.dptr(b), _hip.dptr(A_half), _hip.dptr(stats), _hip.dptr(err), _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_scatter_stats_sym")


def scatter_stats_cnt(grid, x, y, wa, wb, noise, b, A, half, cnt, stats, err, u=None, res=None):
    """One launch: (b, A full or symmetric half, stats) as scatter_stats[_sym] plus cnt += W^T wa and, with
    (u, res) given, the residual carry-over res += W^T (wb y - wa (W u))."""
    x = _x2d(x, grid)
    rc = _hip.fn("wiski_scatter_stats_cnt", x.dtype)(grid.ref, _hip.dptr(x), _hip.dptr(y.contiguous()), _hip.dptr(wa.contiguous()),
                                                     _hip.dptr(wb.contiguous()), _hip.dptr(noise.contiguous()), ctypes.c_int64(x.shape[0]),
                                                     _hip.dptr(b), _hip.dptr(A), ctypes.c_int32(int(half)), _hip.dptr(cnt), _hip.dptr(u), _hip.dptr(res),
                                                     _hip.dptr(stats), _hip.dptr(err), _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_scatter_stats_cnt")


def scatter_stats_multi(grid, x, Yt, wa, wb, noise, b, A_pack, cnt, stats, err, u=None, res=None):
    """ONE absorb launch for all outputs (``wiski_scatter_stats_multi``): Yt [out, n]; wa / wb / noise [out, n] or [n] (shared by
    the outputs); b / cnt / u / res [out, m]; A_pack [out, H, m] half stencils; stats [out, 2]."""
    x = _x2d(x, grid)
    out, n = Yt.shape
    shared = wa.dim() == 1
    rc = _hip.fn("wiski_scatter_stats_multi", x.dtype)(grid.ref, _hip.dptr(x), _hip.dptr(Yt), _hip.dptr(wa), _hip.dptr(wb), _hip.dptr(noise), ctypes.c_int64(n),
                                                       ctypes.c_int32(out), ctypes.c_int64(n), ctypes.c_int64(0 if shared else n), _hip.dptr(b), _hip.dptr(A_pack),
                                                       ctypes.c_int64(A_pack.shape[1] * A_pack.shape[2]), _hip.dptr(cnt), _hip.dptr(u), _hip.dptr(res), _hip.dptr(stats),
                                                       _hip.dptr(err), _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_scatter_stats_multi")


def _absorb_points(op, grid, x, u, groups, u_is="the grid mean"):
    """What the forms of the absorb check alike: x as [n, d]; every tensor of ``groups`` -- (shape, {name: tensor}, optional)
    triples, a shape spelling the number of points as "n" -- of its shape in x's dtype; u [m] (``u_is`` None: the form checks its
    own).  ``optional`` None: an absent tensor is not looked at; else the names that may be absent.  Returns (x, n)."""
    x = _x2d(x, grid)
    n = x.shape[0]
    for shape, tensors, optional in groups:
        shape = tuple(n if k == "n" else k for k in shape)
        for name, t in tensors.items():
            if t is None and (optional is None or name in optional):
                continue
            if t is not None and tuple(t.shape) == shape and t.dtype == x.dtype:
                continue
            got = f"{tuple(t.shape)} {t.dtype}" if optional is None else None if t is None else (tuple(t.shape), t.dtype)
            raise ValueError(f"{op}: {name} must be {list(shape)} {x.dtype}, got {got}")
    if u_is is not None and (u is None or tuple(u.shape) != (grid.m,) or u.dtype != x.dtype):
        raise ValueError(f"{op}: u must be {u_is} [{grid.m}] {x.dtype}")
    return x, n


def _site_outputs(x, shape, logz_shape=None):
    """The outputs of a moment-matched form: (ytilde, omega) of ``shape`` in x's dtype, log_z float64 (of ``logz_shape``, if it differs)."""
    return (torch.empty(shape, dtype=x.dtype, device=x.device), torch.empty(shape, dtype=x.dtype, device=x.device),
            torch.empty(shape if logz_shape is None else logz_shape, dtype=torch.float64, device=x.device))


def _absorb_record(x, points, targets, carry, nout=1, w_stride=0, A_stride=0, channels=0):
    """The argument record (``wiski_absorb_args``) of one form call on the symmetric half stencil, from tensors: ``x`` [n, d] as
    _absorb_points returned it (None: the form brings its own points, n = 0); ``points`` = (y, wa, wb, noise), made contiguous here,
    None where the form ignores one; ``targets`` = (b, A_half, cnt, stats, err), accumulated in place, and ``carry`` = (u, res,
    mean_out), both taken as they are.  What the record has besides (guard, zero regions, shard, owner workspace) stays zero."""
    y, wa, wb, noise = (None if t is None else _hip.dptr(t.contiguous()) for t in points)
    b, A_half, cnt, stats, err = (_hip.dptr(t) for t in targets)
    u, res, mean_out = (_hip.dptr(t) for t in carry)
    return _hip.wiski_absorb_args(d_x=_hip.dptr(x), d_y=y, d_wa=wa, d_wb=wb, d_noise=noise, n=0 if x is None else x.shape[0], d_b=b, d_A=A_half, half=1,
                                  channels=channels, d_cnt=cnt, d_stats=stats, d_err=err, d_u=u, d_res=res, d_mean_out=mean_out, nout=nout,
                                  w_stride=w_stride, A_stride=A_stride)


def _absorb_call(entry, grid, dtype, device, rec, *own):
    """Run the record through ``entry`` (a ``wiski_absorb*`` name) with the form's own arguments, on the current stream of ``device``."""
    _hip.check(_hip.fn(entry, dtype)(grid.ref, ctypes.byref(rec), *own, _hip.stream_ptr(device)), entry)


def scatter_stats_grad(grid, x, Y, wa, wb, noise, b, A_half, cnt, stats, err, u=None, res=None, mean_out=None):
    """Values and gradients in ONE absorb launch (``wiski_absorb`` with channels = d + 1): Y / wa / wb / noise (and
    mean_out) are [n, d + 1] -- column 0 the observation of f, column 1 + q that of df/dx_q; an absent one has wa = wb = 0, noise = 1.
    (b, A_half, cnt, stats) accumulate in place; with u given, mean_out receives the predictive mean and gradient of every point
    before the update and res the carried residual's increment."""
    C = grid.d + 1
    x, n = _absorb_points("scatter_stats_grad", grid, x, u, [(("n", C), dict(Y=Y, wa=wa, wb=wb, noise=noise, mean_out=mean_out), None)], u_is=None)
    _absorb_call("wiski_absorb", grid, x.dtype, x.device, _absorb_record(x, (Y, wa, wb, noise), (b, A_half, cnt, stats, err), (u, res, mean_out), channels=C))


def scatter_stats_robust(grid, x, y, wa, wb, noise, inv_scale, c, b, A_half, cnt, stats, err, u, res=None, mean_out=None):
    """The outlier-robust absorb in ONE launch (``wiski_absorb_robust``): every point is Huber-weighted
    against the posterior mean ``u`` [m] before the batch, z = (y - w . u) inv_scale, omega = min(1, c / |z|), and enters
    (b, A_half, cnt, stats) -- and the carried residual ``res``, if given -- as the same point at noise / omega.  ``inv_scale``
    [n] (0 exempts a point).  Returns omega [n] (0 for a point outside the grid); ``mean_out`` [n] receives w . u."""
    x, n = _absorb_points("scatter_stats_robust", grid, x, u, [(("n",), dict(y=y, wa=wa, wb=wb, noise=noise, inv_scale=inv_scale, mean_out=mean_out), None)])
    omega = torch.empty(n, dtype=x.dtype, device=x.device)
    if n == 0:
        return omega
    _absorb_call("wiski_absorb_robust", grid, x.dtype, x.device, _absorb_record(x, (y, wa, wb, noise), (b, A_half, cnt, stats, err), (u, res, mean_out)),
                 _hip.dptr(inv_scale.contiguous()), float(c), _hip.dptr(omega))
    return omega


def scatter_stats_interval(grid, x, lower, upper, pvar, sigma2, wa, wb, noise, b, A_half, cnt, stats, err, u, res=None, mean_out=None):
    """The interval-observation absorb in ONE launch (``wiski_absorb_interval``): point i says
    lower_i <= f(x_i) + eps_i <= upper_i (either end may be infinite; equal ends are an exact value).  It is moment-matched against
    the posterior before the batch -- the grid mean ``u`` [m], the posterior variance ``pvar`` [n] of f at x, the noise
    ``sigma2 * noise`` -- and enters (b, A_half, cnt, stats) -- and the carried residual ``res``, if given -- as the target ytilde_i
    at noise_i / omega_i.  Returns (ytilde [n], omega [n], log_z [n] float64); a skipped point (nothing to say: omega below 1e-12,
    lower > upper, a NaN bound) has omega = 0 and ytilde = w . u, a point outside the grid (0, 0, 0).  ``mean_out`` [n] receives w . u."""
    x, n = _absorb_points("scatter_stats_interval", grid, x, u,
                          [(("n",), dict(lower=lower, upper=upper, pvar=pvar, wa=wa, wb=wb, noise=noise, mean_out=mean_out), None)])
    ytilde, omega, log_z = _site_outputs(x, (n,))
    if n == 0:
        return ytilde, omega, log_z
    _absorb_call("wiski_absorb_interval", grid, x.dtype, x.device, _absorb_record(x, (None, wa, wb, noise), (b, A_half, cnt, stats, err), (u, res, mean_out)),
                 _hip.dptr(lower.contiguous()), _hip.dptr(upper.contiguous()), _hip.dptr(pvar.contiguous()), float(sigma2), _hip.dptr(ytilde),
                 _hip.dptr(omega), _hip.dptr(log_z))
    return ytilde, omega, log_z


def scatter_stats_grad_interval(grid, x, lower, upper, pvar, sigma2, wa, wb, noise, b, A_half, cnt, stats, err, u, res=None, mean_out=None):
    """Interval sites on values AND partial derivatives in ONE absorb launch (``wiski_absorb_grad_interval``).
    lower / upper / pvar / wa / wb / noise (and mean_out) are [n, d + 1] -- column 0 the channel of f, column 1 + q that of df/dx_q;
    an absent channel has wa = wb = 0, noise = 1.  Every present channel says lower <= (its row . f) + eps <= upper (either end may be
    infinite; equal ends are an exact value) and is moment-matched, independently of the point's other channels, against the
    posterior before the batch -- the grid mean ``u`` [m], the posterior variance ``pvar`` of the channel, the noise ``sigma2 *
    noise`` -- and enters (b, A_half, cnt, stats) -- and the carried residual ``res``, if given -- as the target ytilde at noise /
    omega.  Returns (ytilde, omega, log_z float64), [n, d + 1] each: a skipped channel has omega = 0 and ytilde = its predictive mean,
    an absent channel and every channel of a point outside the grid (0, 0, 0).  ``mean_out`` receives the predictive mean and gradient."""
    C = grid.d + 1
    per_channel = dict(lower=lower, upper=upper, pvar=pvar, wa=wa, wb=wb, noise=noise, mean_out=mean_out)
    x, n = _absorb_points("scatter_stats_grad_interval", grid, x, u, [(("n", C), per_channel, ("mean_out",))])
    ytilde, omega, log_z = _site_outputs(x, (n, C))
    if n == 0:
        return ytilde, omega, log_z
    _absorb_call("wiski_absorb_grad_interval", grid, x.dtype, x.device,
                 _absorb_record(x, (None, wa, wb, noise), (b, A_half, cnt, stats, err), (u, res, mean_out), channels=C),
                 _hip.dptr(lower.contiguous()), _hip.dptr(upper.contiguous()), _hip.dptr(pvar.contiguous()), float(sigma2), _hip.dptr(ytilde),
                 _hip.dptr(omega), _hip.dptr(log_z))
    return ytilde, omega, log_z


COUNT_FAMILIES = {"poisson": 0, "binomial": 1}      # WISKI_COUNT_POISSON, WISKI_COUNT_BINOMIAL


def scatter_stats_count(grid, x, counts, t, family, pvar, sigma2, wa, wb, noise, b, A_half, cnt, stats, err, u, res=None, mean_out=None):
    """The count-observation absorb in ONE launch (``wiski_absorb_count``): point i carries the count
    ``counts_i`` at exposure (``family`` "poisson": y ~ Poisson(t exp f)) or out of trials (``"binomial"``, logit link) ``t_i``.  It is
    moment-matched against the posterior before the batch -- the grid mean ``u`` [m], the posterior variance ``pvar`` [n] of f at x --
    by a quadrature over the lanes of its wave and enters (b, A_half, cnt, stats) -- and the carried residual ``res``, if given -- as
    the target ytilde_i at noise_i / omega_i, omega = sigma2 noise tau (effective noise variance 1 / tau; not capped).  Returns
    (ytilde [n], omega [n], log_z [n] float64); a skipped point (omega below 1e-12, an invalid datum) has omega = 0 and ytilde = w . u,
    a point outside the grid (0, 0, 0).  ``mean_out`` [n] receives w . u."""
    if family not in COUNT_FAMILIES:
        raise ValueError(f"scatter_stats_count: family must be one of {sorted(COUNT_FAMILIES)}, got {family!r}")
    x, n = _absorb_points("scatter_stats_count", grid, x, u,
                          [(("n",), dict(counts=counts, t=t, pvar=pvar, wa=wa, wb=wb, noise=noise, mean_out=mean_out), None)])
    ytilde, omega, log_z = _site_outputs(x, (n,))
    if n == 0:
        return ytilde, omega, log_z
    _absorb_call("wiski_absorb_count", grid, x.dtype, x.device, _absorb_record(x, (None, wa, wb, noise), (b, A_half, cnt, stats, err), (u, res, mean_out)),
                 _hip.dptr(counts.contiguous()), _hip.dptr(t.contiguous()), COUNT_FAMILIES[family], _hip.dptr(pvar.contiguous()), float(sigma2),
                 _hip.dptr(ytilde), _hip.dptr(omega), _hip.dptr(log_z))
    return ytilde, omega, log_z


def scatter_stats_input_noise(grid, x, y, xvar, gvar, pvar, sigma2, wa, wb, noise, b, A_half, cnt, stats, err, u, res=None, mean_out=None,
                              want_grad=False):
    """The noisy-input absorb in ONE launch (``wiski_absorb_input_noise``): point i was taken at x_i + e_i,
    e_i ~ N(0, diag(xvar_i)) (``xvar`` [n, d], in the grid's units squared).  Against the posterior before the batch -- the grid mean
    ``u`` [m] with its slope g_i at x_i, the posterior variances ``pvar`` [n] of f and ``gvar`` [n, d] of its partial derivatives
    (None: 0, the slope of the mean alone) -- the location error is the extra output noise s_in = sum_k xvar_k (g_k^2 + gvar_k), and the
    point enters (b, A_half, cnt, stats) -- and the carried residual ``res``, if given -- as y_i at noise_i / omega_i, omega = dn /
    (dn + s_in), dn = sigma2 noise_i.  Returns (omega [n], log_z [n] float64) and, with ``want_grad``, the slopes g [n, d] as the
    kernel reduced them; a skipped point (omega below 1e-12, a negative or NaN xvar) has omega = 0, a point outside the grid zeros.
    ``mean_out`` [n] receives w . u."""
    x, n = _absorb_points("scatter_stats_input_noise", grid, x, u, [(("n",), dict(y=y, pvar=pvar, wa=wa, wb=wb, noise=noise, mean_out=mean_out), None),
                                                                    (("n", grid.d), dict(xvar=xvar, gvar=gvar), ("gvar",))])
    omega = torch.empty(n, dtype=x.dtype, device=x.device)
    log_z = torch.empty(n, dtype=torch.float64, device=x.device)
    grad = torch.empty((n, grid.d), dtype=x.dtype, device=x.device) if want_grad else None
    if n:
        _absorb_call("wiski_absorb_input_noise", grid, x.dtype, x.device, _absorb_record(x, (y, wa, wb, noise), (b, A_half, cnt, stats, err), (u, res, mean_out)),
                     _hip.dptr(xvar.contiguous()), _hip.dptr(None if gvar is None else gvar.contiguous()), _hip.dptr(pvar.contiguous()), float(sigma2),
                     _hip.dptr(omega), _hip.dptr(log_z), _hip.dptr(grad))
    return (omega, log_z, grad) if want_grad else (omega, log_z)


def count_sites(mean, pvar, counts, t, family):
    """The sites of count observations alone (``wiski_count_sites``: the device function of ``scatter_stats_count``, one wave per
    site, no scatter) against given means and variances [n]: (ytilde [n], tau [n], log_z [n] float64), tau the site precision (the
    omega of ``scatter_stats_count`` at sigma2 noise = 1)."""
    if family not in COUNT_FAMILIES:
        raise ValueError(f"count_sites: family must be one of {sorted(COUNT_FAMILIES)}, got {family!r}")
    n = mean.shape[0]
    for name, v in (("mean", mean), ("pvar", pvar), ("counts", counts), ("t", t)):
        if tuple(v.shape) != (n,) or v.dtype != mean.dtype:
            raise ValueError(f"count_sites: {name} must be [{n}] {mean.dtype}, got {tuple(v.shape)} {v.dtype}")
    ytilde = torch.empty(n, dtype=mean.dtype, device=mean.device)
    tau = torch.empty(n, dtype=mean.dtype, device=mean.device)
    log_z = torch.empty(n, dtype=torch.float64, device=mean.device)
    if n == 0:
        return ytilde, tau, log_z
    rc = _hip.fn("wiski_count_sites", mean.dtype)(_hip.dptr(mean.contiguous()), _hip.dptr(pvar.contiguous()), _hip.dptr(counts.contiguous()),
                                                  _hip.dptr(t.contiguous()), ctypes.c_int(COUNT_FAMILIES[family]), ctypes.c_int64(n), _hip.dptr(ytilde),
                                                  _hip.dptr(tau), _hip.dptr(log_z), _hip.stream_ptr(mean.device))
    _hip.check(rc, "wiski_count_sites")
    return ytilde, tau, log_z


def scatter_stats_hetero(grid, x, y, pvar, pvar2, sigma2, g0, wa, wb, noise, f_set, g_set, err, mean_out=None):
    """The heteroscedastic absorb in ONE launch (``wiski_absorb_hetero``): two single-output models on the same
    grid, f and g = log of the noise multiplier (prior mean ``g0``), each given as a set ``(b, A_half, cnt, stats, u, res)`` (res may
    be None).  Against the two posteriors before the batch -- the grid means, the posterior variances ``pvar`` (of f) and ``pvar2`` (of
    g) at x [n] -- point i enters f as y_i at noise_i e_i, e = exp(mu_g + v_g / 2), and its deflated squared residual enters g as a
    log-variance site, the target ytilde_g - g0 at noise 1 / tau.  Returns (e [n], ytilde_g [n], tau [n], log_z_g [n] float64,
    log_z_y [n] float64): a skipped noise site has tau = 0 and ytilde_g = mu_g (the point still entered f), a point with a NaN y both
    log Z = NaN and nothing anywhere, a point outside the grid zeros.  ``mean_out`` [n] receives w . u_f."""
    op = "scatter_stats_hetero"
    b, A_half, cnt, stats, u, res = f_set
    b2, A2_half, cnt2, stats2, u2, res2 = g_set
    x, n = _absorb_points(op, grid, x, u, [(("n",), dict(y=y, pvar=pvar, pvar2=pvar2, wa=wa, wb=wb, noise=noise, mean_out=mean_out), None)],
                          u_is="the grid mean of f")
    if u2 is None or tuple(u2.shape) != (grid.m,) or u2.dtype != x.dtype:
        raise ValueError(f"{op}: the second set's u must be the grid mean of g - g0 [{grid.m}] {x.dtype}")
    ytilde, tau, log_z = _site_outputs(x, (n,))
    e = torch.empty(n, dtype=x.dtype, device=x.device)
    log_zy = torch.empty(n, dtype=torch.float64, device=x.device)
    if n == 0:
        return e, ytilde, tau, log_z, log_zy
    _absorb_call("wiski_absorb_hetero", grid, x.dtype, x.device, _absorb_record(x, (y, wa, wb, noise), (b, A_half, cnt, stats, err), (u, res, mean_out)),
                 _hip.dptr(pvar.contiguous()), _hip.dptr(pvar2.contiguous()), float(sigma2), float(g0), _hip.dptr(b2), _hip.dptr(A2_half), _hip.dptr(cnt2),
                 _hip.dptr(u2), _hip.dptr(res2), _hip.dptr(stats2), _hip.dptr(e), _hip.dptr(ytilde), _hip.dptr(tau), _hip.dptr(log_z), _hip.dptr(log_zy))
    return e, ytilde, tau, log_z, log_zy


def hetero_sites(mean, pvar, rho, nu):
    """The log-variance sites alone (``wiski_hetero_sites``: the device function of ``scatter_stats_hetero``, one wave per site, no
    scatter): ``rho`` the sum of squares of ``nu`` residuals in units of the known noise, matched against N(mean, pvar) of the log
    multiplier, all [n].  Returns (ytilde [n], tau [n], log_z [n] float64)."""
    n = mean.shape[0]
    for name, v in (("mean", mean), ("pvar", pvar), ("rho", rho), ("nu", nu)):
        if tuple(v.shape) != (n,) or v.dtype != mean.dtype:
            raise ValueError(f"hetero_sites: {name} must be [{n}] {mean.dtype}, got {tuple(v.shape)} {v.dtype}")
    ytilde = torch.empty(n, dtype=mean.dtype, device=mean.device)
    tau = torch.empty(n, dtype=mean.dtype, device=mean.device)
    log_z = torch.empty(n, dtype=torch.float64, device=mean.device)
    if n == 0:
        return ytilde, tau, log_z
    rc = _hip.fn("wiski_hetero_sites", mean.dtype)(_hip.dptr(mean.contiguous()), _hip.dptr(pvar.contiguous()), _hip.dptr(rho.contiguous()),
                                                   _hip.dptr(nu.contiguous()), n, _hip.dptr(ytilde), _hip.dptr(tau), _hip.dptr(log_z),
                                                   _hip.stream_ptr(mean.device))
    _hip.check(rc, "wiski_hetero_sites")
    return ytilde, tau, log_z


LABEL_MAX_CLASSES = 16                              # WISKI_LABEL_MAX_CLASSES


def _label_classes(op, C):
    if not 2 <= C <= LABEL_MAX_CLASSES:
        raise ValueError(f"{op}: 2 .. {LABEL_MAX_CLASSES} classes, got {C}")


def scatter_stats_label(grid, x, labels, pvar, sigma2, wa, wb, noise, b, A_pack, cnt, stats, err, u, res=None, mean_out=None):
    """The categorical-observation absorb in ONE launch (``wiski_absorb_label``): point i carries the label
    ``labels_i`` in {0 .. C - 1} (in x's dtype) over the C outputs of b / cnt / u / res [C, m], A_pack [C, H, m] and stats [C, 2].  The
    multinomial probit likelihood is moment-matched against the posterior before the batch -- the grid means ``u``, the posterior
    variances ``pvar`` [C, n], the noise variances ``sigma2[c] * noise`` -- by a quadrature over the lanes of the point's wave, and
    output c takes the point as ytilde_c at noise / omega_c.  wa / wb / noise are [C, n] or [n] (shared by the outputs); ``sigma2``
    is a sequence of C positive floats.  Returns (ytilde [C, n], omega [C, n], log_z [n] float64): a skipped site has omega = 0 and
    ytilde = its predictive mean, a point with an invalid label log_z = NaN and no site, a point outside the grid zeros.
    ``mean_out`` [C, n] receives the predictive means."""
    op = "scatter_stats_label"
    x = _x2d(x, grid)
    if u is None or u.dim() != 2 or u.shape[1] != grid.m or u.dtype != x.dtype:
        raise ValueError(f"{op}: u must be the grid means [C, {grid.m}] {x.dtype}")
    C = u.shape[0]
    _label_classes(op, C)
    shared = wa.dim() == 1
    weights = ("n",) if shared else (C, "n")
    x, n = _absorb_points(op, grid, x, u, u_is=None, groups=[
        (("n",), dict(labels=labels), ()), ((C, "n"), dict(pvar=pvar, mean_out=mean_out), ("mean_out",)), (weights, dict(wa=wa, wb=wb, noise=noise), ()),
        ((C, grid.m), dict(b=b, cnt=cnt, res=res), ("res",))])
    if A_pack.dim() != 3 or A_pack.shape[0] != C or A_pack.dtype != x.dtype or tuple(stats.shape) != (C, 2) or stats.dtype != torch.float64:
        raise ValueError(f"{op}: A_pack must be [C, H, m] {x.dtype} half stencils and stats [C, 2] float64")
    sigma2 = [float(v) for v in sigma2]
    if len(sigma2) != C:
        raise ValueError(f"{op}: sigma2 must hold {C} values, got {len(sigma2)}")
    ytilde, omega, log_z = _site_outputs(x, (C, n), logz_shape=(n,))
    if n == 0:
        return ytilde, omega, log_z
    rec = _absorb_record(x, (None, wa, wb, noise), (b, A_pack, cnt, stats, err), (u, res, mean_out), nout=C, w_stride=0 if shared else n,
                         A_stride=A_pack.shape[1] * A_pack.shape[2])
    _absorb_call("wiski_absorb_label", grid, x.dtype, x.device, rec, _hip.dptr(labels.contiguous()), _hip.dptr(pvar.contiguous()),
                 (ctypes.c_double * C)(*sigma2), _hip.dptr(ytilde), _hip.dptr(omega), _hip.dptr(log_z))
    return ytilde, omega, log_z


def _label_inputs(op, mean, pvar, s):
    if mean.dim() != 2:
        raise ValueError(f"{op}: mean must be [C, n], got {tuple(mean.shape)}")
    C, n = mean.shape
    _label_classes(op, C)
    for name, v in (("pvar", pvar), ("s", s)):
        if tuple(v.shape) != (C, n) or v.dtype != mean.dtype:
            raise ValueError(f"{op}: {name} must be [{C}, {n}] {mean.dtype}, got {tuple(v.shape)} {v.dtype}")
    return C, n


def label_sites(mean, pvar, s, labels):
    """The sites of labels alone (``wiski_label_sites``: the device function of ``scatter_stats_label``, one wave per point, no
    scatter) against given class means, latent variances and noise variances [C, n]: (ytilde [C, n], tau [C, n], log_z [n] float64),
    tau the site precisions (the omega of ``scatter_stats_label`` divided by s)."""
    C, n = _label_inputs("label_sites", mean, pvar, s)
    if tuple(labels.shape) != (n,) or labels.dtype != mean.dtype:
        raise ValueError(f"label_sites: labels must be [{n}] {mean.dtype}, got {tuple(labels.shape)} {labels.dtype}")
    ytilde, tau = torch.empty_like(mean, memory_format=torch.contiguous_format), torch.empty_like(mean, memory_format=torch.contiguous_format)
    log_z = torch.empty(n, dtype=torch.float64, device=mean.device)
    if n == 0:
        return ytilde, tau, log_z
    rc = _hip.fn("wiski_label_sites", mean.dtype)(_hip.dptr(mean.contiguous()), _hip.dptr(pvar.contiguous()), _hip.dptr(s.contiguous()),
                                                  _hip.dptr(labels.contiguous()), C, n, _hip.dptr(ytilde), _hip.dptr(tau), _hip.dptr(log_z),
                                                  _hip.stream_ptr(mean.device))
    _hip.check(rc, "wiski_label_sites")
    return ytilde, tau, log_z


def label_proba(mean, pvar, s):
    """P(y = k) for every class k (``wiski_label_proba``) from class means, latent variances and noise variances [C, n]: [n, C]
    float64, each entry by its own integral -- the rows sum to 1 to quadrature error and are not normalised."""
    C, n = _label_inputs("label_proba", mean, pvar, s)
    out = torch.empty((n, C), dtype=torch.float64, device=mean.device)
    if n == 0:
        return out
    rc = _hip.fn("wiski_label_proba", mean.dtype)(_hip.dptr(mean.contiguous()), _hip.dptr(pvar.contiguous()), _hip.dptr(s.contiguous()), C, n,
                                                  _hip.dptr(out), _hip.stream_ptr(mean.device))
    _hip.check(rc, "wiski_label_proba")
    return out


class WindowRing:
    """The device-resident ring of a sliding window (``wiski_window_ring``): x [cap, d], y / wa / wb / noise [cap]
    in the working precision, and on the host ``head`` -- the slot the next entering point takes -- and ``fill``, the number of
    slots written so far (at most cap).  An empty slot holds wa = wb = 0, noise = 1; a void one (its point lay outside the grid
    when it entered) the same with x = NaN.  ``void_left`` [1] int32 counts, on the device, the void slots overwritten so far.
    ``unit`` (host, bool [cap]) is the owner's note of the slots it wrote at unit noise (the model keeps their weight sum on the host),
    ``explicit`` [cap] the device mask of the slots written with explicit noise (1, else 0) and ``explicit_host`` its host copy;
    ``mark`` writes all three.  An empty slot is in neither set."""

    def __init__(self, cap, d, dtype, device):
        cap = int(cap)
        if cap < 1:
            raise ValueError(f"WindowRing: cap must be at least 1, got {cap}")
        self.cap, self.d, self.head, self.fill = cap, int(d), 0, 0
        self.x = torch.zeros((cap, self.d), dtype=dtype, device=device)
        self.y = torch.zeros(cap, dtype=dtype, device=device)
        self.wa = torch.zeros(cap, dtype=dtype, device=device)
        self.wb = torch.zeros(cap, dtype=dtype, device=device)
        self.noise = torch.ones(cap, dtype=dtype, device=device)
        self.void_left = torch.zeros(1, dtype=torch.int32, device=device)
        self.unit = np.zeros(cap, dtype=bool)
        self.explicit = torch.zeros(cap, dtype=dtype, device=device)
        self.explicit_host = np.zeros(cap, dtype=bool)

    def tensors(self):
        return self.x, self.y, self.wa, self.wb, self.noise

    def clone(self):
        new = object.__new__(WindowRing)
        new.cap, new.d, new.head, new.fill = self.cap, self.d, self.head, self.fill
        new.x, new.y, new.wa, new.wb, new.noise = (t.clone() for t in self.tensors())
        new.void_left = self.void_left.clone()
        new.unit = self.unit.copy()
        new.explicit, new.explicit_host = self.explicit.clone(), self.explicit_host.copy()
        return new

    def to(self, device):
        new = self.clone()
        new.x, new.y, new.wa, new.wb, new.noise = (t.to(device) for t in new.tensors())
        new.void_left, new.explicit = new.void_left.to(device), new.explicit.to(device)
        return new

    def clear(self):
        """Every slot empty again."""
        self.head = self.fill = 0
        for t in (self.x, self.y, self.wa, self.wb, self.void_left):
            t.zero_()
        self.noise.fill_(1)
        self.unit[:] = False
        self.explicit.zero_()
        self.explicit_host[:] = False

    def spans(self, n):
        """The slots head .. head + n - 1 (mod cap), n <= cap, as one or two slices."""
        end = self.head + n
        return [slice(self.head, end)] if end <= self.cap else [slice(self.head, self.cap), slice(0, end - self.cap)]

    def mark(self, spans, unit):
        """Note the slots of `spans` as written at unit noise, or with explicit noise (host flags and device mask; no host read)."""
        for sl in spans:
            self.unit[sl] = unit
            self.explicit_host[sl] = not unit
            self.explicit[sl] = 0 if unit else 1

    def advance(self, n):
        self.head = (self.head + n) % self.cap
        self.fill = min(self.cap, self.fill + n)

    def order(self):
        """Slot indices of the written slots, oldest first (a host list)."""
        first = self.head if self.fill == self.cap else 0
        return [(first + i) % self.cap for i in range(self.fill)]

    def ref(self, head=None):
        return _hip.wiski_window_ring(*(t.data_ptr() for t in self.tensors()), self.cap, self.head if head is None else int(head))


def scatter_stats_window(grid, x, y, wa, wb, noise, ring, b, A_half, cnt, stats, err, u, res=None, mean_out=None):
    """The sliding-window absorb in ONE launch (``wiski_absorb_window``): the n <= ring.cap points enter
    (b, A_half, cnt, stats) -- and the carried residual ``res``, if given -- and the slots ring.head, ring.head + 1, ... (mod cap)
    of ``ring``; what those slots held leaves the statistics again, with its weights negated.  ``u`` [m]: the posterior mean on the
    grid both sweeps are taken against (any vector when neither ``res`` nor ``mean_out`` is asked for); ``mean_out`` [n] receives
    w . u of the entering points.  Advances ``ring.head`` and ``ring.fill``."""
    x, n = _absorb_points("scatter_stats_window", grid, x, u, [(("n",), dict(y=y, wa=wa, wb=wb, noise=noise, mean_out=mean_out), None)], u_is="a grid vector")
    if ring.d != grid.d or ring.x.dtype != x.dtype or ring.x.device != x.device:
        raise ValueError(f"scatter_stats_window: the ring holds {ring.d}-d {ring.x.dtype} points on {ring.x.device}")
    if n == 0:
        return
    r = ring.ref()
    _absorb_call("wiski_absorb_window", grid, x.dtype, x.device, _absorb_record(x, (y, wa, wb, noise), (b, A_half, cnt, stats, err), (u, res, mean_out)),
                 ctypes.byref(r), _hip.dptr(ring.void_left))
    ring.advance(n)


SITE_FORMS = {"interval": 1, "poisson": 2, "binomial": 3}     # WISKI_SITE_INTERVAL, _POISSON, _BINOMIAL (0: an empty slot)


class SiteRing:
    """The device-resident ring of stored sites (``wiski_site_ring``): per slot the point ``x`` [cap, d], its two
    data numbers ``d0`` / ``d1`` ((lower, upper) of an interval, (count, exposure or trials) of a count), ``noise`` / ``wa`` / ``wb``,
    the site ``ytilde`` / ``omega`` it is in the statistics with -- all [cap] in the working precision -- and ``form`` [cap] int32
    (SITE_FORMS; 0: empty).  On the host ``head``, the slot the next stored point takes, ``fill``, the number of slots written so far
    (at most cap), and ``forms``, the set of form names stored so far (which launches a sweep needs; never shrinks until clear())."""

    _REAL = ("x", "d0", "d1", "noise", "wa", "wb", "ytilde", "omega")

    def __init__(self, cap, d, dtype, device):
        cap = int(cap)
        if cap < 1:
            raise ValueError(f"SiteRing: cap must be at least 1, got {cap}")
        self.cap, self.d, self.head, self.fill, self.forms = cap, int(d), 0, 0, set()
        self.x = torch.zeros((cap, self.d), dtype=dtype, device=device)
        for k in self._REAL[1:]:
            setattr(self, k, torch.zeros(cap, dtype=dtype, device=device))
        self.noise.fill_(1)
        self.form = torch.zeros(cap, dtype=torch.int32, device=device)

    def tensors(self):
        return tuple(getattr(self, k) for k in self._REAL) + (self.form,)

    def clone(self):
        new = object.__new__(SiteRing)
        new.cap, new.d, new.head, new.fill, new.forms = self.cap, self.d, self.head, self.fill, set(self.forms)
        for k in self._REAL + ("form",):
            setattr(new, k, getattr(self, k).clone())
        return new

    def to(self, device):
        new = self.clone()
        for k in self._REAL + ("form",):
            setattr(new, k, getattr(new, k).to(device))
        return new

    def clear(self):
        """Every slot empty again."""
        self.head = self.fill = 0
        self.forms = set()
        for t in self.tensors():
            t.zero_()
        self.noise.fill_(1)

    def store(self, form, x, d0, d1, noise, wa, wb, ytilde, omega, keep=None):
        """Write the points into the slots head, head + 1, ... (mod cap) with plain index copies and advance; of more than cap
        points the last cap are stored.  ``keep`` (bool [n], device): only these are stored -- this costs one host read of their
        number.  What an overwritten slot held stays in the statistics as it was."""
        cols = [x.reshape(-1, self.d), d0, d1, noise, wa, wb, ytilde, omega]
        if keep is not None:
            idx = torch.nonzero(keep.reshape(-1)).reshape(-1)
            cols = [c[idx] for c in cols]
        n = cols[0].shape[0]
        if n > self.cap:
            cols = [c[n - self.cap:] for c in cols]
            n = self.cap
        if n == 0:
            return 0
        slots = (torch.arange(n, device=self.x.device) + self.head) % self.cap
        for k, c in zip(self._REAL, cols):
            getattr(self, k)[slots] = c.to(self.x.dtype)
        self.form[slots] = SITE_FORMS[form]
        self.forms.add(form)
        self.head = (self.head + n) % self.cap
        self.fill = min(self.cap, self.fill + n)
        return n

    def order(self):
        """Slot indices of the written slots, oldest first (a host list)."""
        first = self.head if self.fill == self.cap else 0
        return [(first + i) % self.cap for i in range(self.fill)]

    def ref(self):
        return _hip.wiski_site_ring(*(t.data_ptr() for t in self.tensors()), self.cap)


def revisit_sites(grid, ring, form, pvar, sigma2, damping, b, A_half, cnt, stats, err, u, res=None, log_z=None, change=None):
    """One expectation-propagation launch over the stored sites of one form (``wiski_absorb_revisit``): every slot
    of ``ring`` whose form is ``form`` ("interval", "poisson", "binomial") is re-matched against its cavity under the grid mean ``u``
    [m] and the posterior variance ``pvar`` [cap] of f at the slots' points, damped by ``damping`` in [0, 1], and enters
    (b, A_half, cnt, stats) -- and the carried residual ``res``, if given -- with the difference of its site; the ring's ytilde /
    omega are updated in place.  Returns (log_z [cap] float64, change [cap]): log Z of the fresh site against the cavity (NaN for a
    slot left alone) and |omega_new - omega_old| / max(omega_new, omega_old).  The slots of other forms and empty slots are not
    written: pass the pair returned by one launch on as ``log_z`` / ``change`` to the next form's launch of the same sweep."""
    if form not in SITE_FORMS:
        raise ValueError(f"revisit_sites: form must be one of {sorted(SITE_FORMS)}, got {form!r}")
    dtype, device = ring.x.dtype, ring.x.device
    if ring.d != grid.d:
        raise ValueError(f"revisit_sites: the ring holds {ring.d}-d points, the grid has {grid.d} dims")
    for name, t, dt in (("pvar", pvar, dtype), ("change", change, dtype), ("log_z", log_z, torch.float64)):
        if (t is None and name == "pvar") or (t is not None and (tuple(t.shape) != (ring.cap,) or t.dtype != dt)):
            raise ValueError(f"revisit_sites: {name} must be [{ring.cap}] {dt}, got {None if t is None else (tuple(t.shape), t.dtype)}")
    if u is None or tuple(u.shape) != (grid.m,) or u.dtype != dtype:
        raise ValueError(f"revisit_sites: u must be the grid mean [{grid.m}] {dtype}")
    if log_z is None:
        log_z = torch.full((ring.cap,), float("nan"), dtype=torch.float64, device=device)
    if change is None:
        change = torch.zeros(ring.cap, dtype=dtype, device=device)
    r = ring.ref()
    # the points are the ring's slots: the record carries the targets and the carry alone
    _absorb_call("wiski_absorb_revisit", grid, dtype, device, _absorb_record(None, (None,) * 4, (b, A_half, cnt, stats, err), (u, res, None)),
                 ctypes.byref(r), SITE_FORMS[form], _hip.dptr(pvar.contiguous()), float(sigma2), float(damping), _hip.dptr(log_z), _hip.dptr(change))
    return log_z, change


def scatter_probes(grid, x, wa, first_index, seed, P, err):
    """P [m, S] += the probe increments sum_i sqrt(wa_i) eps(first_index + i, s) w(x_i) of the points x [q, d]
    (``wiski_scatter_probes``; wa [q] or None = unit weights; the normals are a function of (seed, global point index, s):
    include/wiski.h).  One launch; a no-op for q = 0."""
    x = _x2d(x, grid)
    if P.dim() != 2 or P.shape[0] != grid.m or P.dtype != x.dtype or not P.is_contiguous():
        raise ValueError(f"scatter_probes needs contiguous probes [m = {grid.m}, S] in the points' dtype, got {tuple(P.shape)} ({P.dtype})")
    if wa is not None:
        wa = wa.contiguous()
        assert wa.shape == (x.shape[0],) and wa.dtype == x.dtype
    rc = _hip.fn("wiski_scatter_probes", x.dtype)(grid.ref, _hip.dptr(x), _hip.dptr(wa), ctypes.c_int64(x.shape[0]), ctypes.c_int64(int(first_index)),
                                                  ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ctypes.c_int32(P.shape[1]), _hip.dptr(P), _hip.dptr(err),
                                                  _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_scatter_probes")


TREND_DEGREES = {"constant": 0, "linear": 1, "quadratic": 2}


def trend_size(d, deg):
    """p: the number of monomials of total degree <= deg in d coordinates (deg 0, 1, 2)."""
    if deg not in (0, 1, 2):
        raise ValueError(f"the trend's degree must be 0, 1 or 2, got {deg!r}")
    return 1 if deg == 0 else (d + 1 if deg == 1 else (d + 1) * (d + 2) // 2)


def _trend_frame(grid, deg, center, scale, what):
    p = trend_size(grid.d, int(deg))
    for t in (center, scale):
        if t.dtype != torch.float64 or t.shape != (grid.d,) or not t.is_contiguous():
            raise ValueError(f"{what} needs the basis centre and scale as contiguous fp64 tensors [{grid.d}]")
    return p


def _same_device(what, x, **tensors):
    for name, t in tensors.items():
        if t is not None and t.device != x.device:
            raise ValueError(f"{what}: {name} lives on {t.device}, the points on {x.device}")


def scatter_trend(grid, x, wa, wby, deg, center, scale, C, G, g, err):
    """The trend's statistics of the points x [n, d] (``wiski_scatter_trend``), in one launch: C [m, p] +=
    sum_i wa_i w(x_i) h(x_i)^T (the points' dtype, trend-minor), G [p, p] += sum_i wa_i h_i h_i^T (fp64; the kernel adds to the UPPER
    triangle only: ``trend_mirror`` completes it), g [p] += sum_i wby_i h_i (fp64).  wa [n] or None = unit weights; wby [n] = wb * y.
    center / scale: fp64 [d], the normalisation of the basis.  A no-op for n = 0."""
    x = _x2d(x, grid)
    n = x.shape[0]
    p = _trend_frame(grid, deg, center, scale, "scatter_trend")
    if C.shape != (grid.m, p) or C.dtype != x.dtype or not C.is_contiguous():
        raise ValueError(f"scatter_trend needs contiguous C [m = {grid.m}, p = {p}] in the points' dtype, got {tuple(C.shape)} ({C.dtype})")
    if (G.shape != (p, p) or g.shape != (p,) or G.dtype != torch.float64 or g.dtype != torch.float64 or not G.is_contiguous()
            or not g.is_contiguous()):
        raise ValueError(f"scatter_trend needs contiguous fp64 G [{p}, {p}] and g [{p}], got {tuple(G.shape)} ({G.dtype}) and {tuple(g.shape)} ({g.dtype})")
    for name, w in (("wby", wby), ("wa", wa)):
        if w is not None and (w.shape != (n,) or w.dtype != x.dtype):
            raise ValueError(f"scatter_trend needs {name} [{n}] in the points' dtype, got {tuple(w.shape)} ({w.dtype})")
    _same_device("scatter_trend", x, wa=wa, wby=wby, center=center, scale=scale, C=C, G=G, g=g, err=err)
    wby = wby.contiguous()
    wa = None if wa is None else wa.contiguous()
    rc = _hip.fn("wiski_scatter_trend", x.dtype)(grid.ref, _hip.dptr(x), _hip.dptr(wa), _hip.dptr(wby), ctypes.c_int64(n), ctypes.c_int32(int(deg)),
                                                 _hip.dptr(center), _hip.dptr(scale), _hip.dptr(C), _hip.dptr(G), _hip.dptr(g), _hip.dptr(err),
                                                 _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_scatter_trend")


def trend_mirror(G):
    """The symmetric G of the upper triangle ``scatter_trend`` accumulates (a new tensor)."""
    U = torch.triu(G)
    return U + torch.triu(G, 1).t()


def trend_rows(grid, x, deg, center, scale, S, err, want_basis=False):
    """R* [n, p] = h(x*) - W* S of the points x [n, d] in one fused gather (``wiski_trend_rows``), S [m, p] trend-minor in the points'
    dtype; S None: R* = H*, the basis rows.  want_basis: returns (R*, H*).  Points outside the grid are flagged in err; their rows
    are h(x*)."""
    x = _x2d(x, grid)
    n = x.shape[0]
    p = _trend_frame(grid, deg, center, scale, "trend_rows")
    if S is not None and (S.shape != (grid.m, p) or S.dtype != x.dtype or not S.is_contiguous()):
        raise ValueError(f"trend_rows needs contiguous S [m = {grid.m}, p = {p}] in the points' dtype, got {tuple(S.shape)} ({S.dtype})")
    _same_device("trend_rows", x, center=center, scale=scale, S=S, err=err)
    R = torch.empty((n, p), dtype=x.dtype, device=x.device)
    H = torch.empty((n, p), dtype=x.dtype, device=x.device) if want_basis else None
    rc = _hip.fn("wiski_trend_rows", x.dtype)(grid.ref, _hip.dptr(x), ctypes.c_int64(n), ctypes.c_int32(int(deg)), _hip.dptr(center), _hip.dptr(scale),
                                              _hip.dptr(S), _hip.dptr(R), _hip.dptr(H), _hip.dptr(err), _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_trend_rows")
    return (R, H) if want_basis else R


def decay_stats(gamma, regions, stats=None, counts=None, R=None, Z=None, side=None):
    """Exponential forgetting in ONE launch (``wiski_decay_stats``): every ``(tensor, factor)`` of `regions` is scaled in
    place, ``x <- x * factor`` with the factor rounded once to the tensors' dtype (the stencil pack, b, cnt: gamma; the path probes:
    sqrt(gamma)); ``stats [out, 2]`` (fp64) gets slot 0 times gamma and slot 1 minus ``counts[o] * log(gamma)``; the carried residual
    ``R <- gamma R - (1 - gamma) Z`` (both or neither); ``side`` (a flat fp64 tensor of a few scalars) is scaled by gamma.  All tensors contiguous, on one
    device, the regions / R / Z of one dtype.  gamma = 1 launches nothing; gamma outside (0, 1] or NaN raises WiskiError.  More than 8
    regions, outputs or side scalars take one launch per 8."""
    gamma = float(gamma)
    regions = [(t, float(f)) for t, f in regions if t is not None and t.numel() > 0]
    reals = [t for t, _ in regions] + [t for t in (R, Z) if t is not None]
    if (R is None) != (Z is None) or (R is not None and (R.shape != Z.shape)):
        raise _hip.WiskiError("decay_stats: R and Z go together and have one shape")
    dtype = reals[0].dtype if reals else torch.float64
    if any(t.dtype != dtype for t in reals):
        raise _hip.WiskiError("decay_stats: the regions, R and Z must have one dtype")
    nout = 0 if stats is None else stats.shape[0]
    if stats is not None and (stats.dtype != torch.float64 or stats.dim() != 2 or stats.shape[1] != 2 or counts is None or len(counts) != nout):
        raise _hip.WiskiError("decay_stats: stats is fp64 [out, 2] with one point count per output")
    if side is not None and (side.dtype != torch.float64 or side.dim() != 1):
        raise _hip.WiskiError("decay_stats: side is a flat fp64 tensor")
    nside = 0 if side is None else side.numel()
    every = reals + [t for t in (stats, side) if t is not None]
    if not every:
        if not (0.0 < gamma <= 1.0):
            raise _hip.WiskiError("wiski_decay_stats failed: WISKI_E_BADARG")
        return
    dev = every[0].device
    f = _hip.fn("wiski_decay_stats", dtype)
    R_MAX, O_MAX = _hip.DECAY_MAX_REGIONS, _hip.DECAY_MAX_OUTPUTS
    calls = max(1, -(-len(regions) // R_MAX), -(-nout // O_MAX), -(-nside // O_MAX))
    for c in range(calls):
        plan = _hip.wiski_decay_plan()
        part = regions[c * R_MAX:(c + 1) * R_MAX]
        plan.count = len(part)
        for i, (t, fac) in enumerate(part):
            plan.ptr[i], plan.n[i], plan.factor[i] = _hip.dptr(t).value, t.numel(), fac
        o0, o1 = min(c * O_MAX, nout), min((c + 1) * O_MAX, nout)
        cnts = (ctypes.c_double * max(1, o1 - o0))(*[float(v) for v in counts[o0:o1]]) if o1 > o0 else None
        s0, s1 = min(c * O_MAX, nside), min((c + 1) * O_MAX, nside)
        first = c == 0
        rc = f(ctypes.byref(plan), ctypes.c_double(gamma), _hip.dptr(R) if first else None, _hip.dptr(Z) if first else None,
               ctypes.c_int64(R.numel() if (first and R is not None) else 0), _hip.dptr(stats[o0:o1]) if o1 > o0 else None, ctypes.c_int32(o1 - o0), cnts,
               _hip.dptr(side[s0:s1]) if s1 > s0 else None, ctypes.c_int32(s1 - s0), _hip.stream_ptr(dev))
        _hip.check(rc, "wiski_decay_stats")


def stencil_regrid_regions(old_grid, new_grid, src, dst, report=-1):
    """The regions of ``regrid_stats`` that move one stencil: the native half stencil ``[H, m] -> [H, m']`` (group 0 as rows of 4, the
    groups >= 1 as rows of 7, starting at 4 m / 4 m') or an offset-major full stencil ``[7^d, m] -> [7^d, m']``.  `report`: the slot of
    the drop report this stencil's diagonal is counted in (-1: none)."""
    R, m, m2 = old_grid.R, old_grid.m, new_grid.m
    if src.dim() != 2 or dst.shape != (src.shape[0], m2) or src.shape[1] != m:
        raise ValueError(f"stencil_regrid_regions: {tuple(src.shape)} -> {tuple(dst.shape)} is no stencil of a grid of {m} -> {m2} nodes")
    if not is_half_stencil(old_grid, src):
        return [(src, dst, R, 1, 0, report)]
    H = (R + 1) // 2
    regions = [(src.reshape(-1)[:4 * m], dst.reshape(-1)[:4 * m2], 1, 4, (R - 1) // 2, report)]
    if H > 4:
        regions.append((src.reshape(-1)[4 * m:], dst.reshape(-1)[4 * m2:], (H - 4) // 7, 7, 7 * ((R // 7 - 1) // 2 + 1), -1))
    return regions


def regrid_stats(old_grid, new_grid, below, regions):
    """Re-embed statistics on a grid grown / shifted / trimmed by whole nodes (``wiski_regrid_stats``) in ONE launch, out of
    place: `new_grid` is ``old_grid.shifted(below, above)``; every region ``(src, dst, k, w[, r0[, report]])`` holds k blocks of m nodes of
    w reals, element (c, node i, s) at ``src[c m w + i w + s]`` goes to ``dst[c m' w + i' w + s]`` and every element of dst is written
    exactly once (zero where the old grid has no such node; for a stencil region, ``r0 >= 0``: also where the entry's neighbour node is
    outside the new grid).  src and dst are contiguous ROCm tensors (or flat views) of one dtype with ``k m w`` and ``k m' w`` elements.
    ``report >= 0`` on the region that holds a stencil's diagonal asks for the drop report of that slot.  Returns ``(dropped_rows,
    dropped_mass)``: per report slot, the number of removed nodes whose ``A_ii != 0`` and the sum of those ``A_ii`` (two lists; empty
    without a report, else one host read).  Tables beyond the plan's 16 regions (or 8 report slots) take one launch per part."""
    a = [int(below)] * old_grid.d if isinstance(below, int) else [int(v) for v in below]
    if old_grid.d != new_grid.d or len(a) != old_grid.d:
        raise _hip.WiskiError("regrid_stats: the grids and `below` must have one dimension")
    regs = []
    for reg in regions:
        src, dst, k, w = reg[:4]
        r0 = int(reg[4]) if len(reg) > 4 else -1
        report = int(reg[5]) if len(reg) > 5 else -1
        k, w = int(k), int(w)
        if src.dtype != dst.dtype or src.device != dst.device or src.numel() != k * old_grid.m * w or dst.numel() != k * new_grid.m * w:
            raise _hip.WiskiError(f"regrid_stats: region of {src.numel()} -> {dst.numel()} elements ({src.dtype} -> {dst.dtype}) does not match "
                                  f"k = {k}, w = {w} on grids of {old_grid.m} -> {new_grid.m} nodes")
        regs.append((src, dst, k, w, r0, report))
    if not regs:
        return [], []
    dtype, dev = regs[0][0].dtype, regs[0][0].device
    if any(r[0].dtype != dtype for r in regs):
        raise _hip.WiskiError("regrid_stats: the regions must have one dtype")
    nrep = max(r[5] for r in regs) + 1
    record = torch.zeros((max(nrep, 1), 2), dtype=torch.float64, device=dev) if nrep > 0 else None
    f = _hip.fn("wiski_regrid_stats", dtype)
    c_below = (ctypes.c_int32 * old_grid.d)(*a)
    c_above = (ctypes.c_int32 * old_grid.d)(*[gn - go - aq for gn, go, aq in zip(new_grid.g, old_grid.g, a)])
    c_new = (ctypes.c_int32 * old_grid.d)(*new_grid.g)
    i = 0
    while i < len(regs):
        plan = _hip.wiski_regrid_plan()
        base = None                                          # first report slot of this launch
        n = 0
        while i < len(regs) and n < _hip.REGRID_MAX_REGIONS:
            src, dst, k, w, r0, report = regs[i]
            if report >= 0:
                if base is None:
                    base = report
                if not (0 <= report - base < _hip.REGRID_MAX_REPORTS):
                    break
            plan.src[n], plan.dst[n], plan.k[n], plan.w[n], plan.r0[n] = _hip.dptr(src).value, _hip.dptr(dst).value, k, w, r0
            plan.report[n] = report - base if report >= 0 else -1
            n += 1
            i += 1
        plan.count = n
        rc = f(old_grid.ref, c_below, c_above, c_new, ctypes.byref(plan), _hip.dptr(record[base:]) if base is not None else None, _hip.stream_ptr(dev))
        _hip.check(rc, "wiski_regrid_stats")
    if record is None:
        return [], []
    rec = record.tolist()
    return [int(r[0]) for r in rec], [float(r[1]) for r in rec]


def stencil_node_regions(grid, st):
    """The ``(flat tensor, k, w)`` node regions of one stencil ``[rows, m']`` in the layout of `grid` (m' = m, or n_sel for a compact one):
    the native half stencil is group 0 (k = 1, w = 4) plus the groups >= 1 (w = 7, starting at 4 m'); an offset-major one is k = 7^d, w = 1."""
    rows, mm = st.shape
    flat = st.reshape(-1)
    if not is_half_stencil(grid, st):
        return [(flat, rows, 1)]
    regions = [(flat[:4 * mm], 1, 4)]
    if rows > 4:
        regions.append((flat[4 * mm:], (rows - 4) // 7, 7))
    return regions


def _stats_regions(what, m, regions, n_src, n_dst):
    """Checked ``(src, dst, k, w, factor)`` list of the three stats_* functions; n_src / n_dst: nodes of the two sides (None: no such side)."""
    regs = []
    for reg in regions:
        src, dst, k, w = reg[:4]
        k, w = int(k), int(w)
        fac = float(reg[4]) if len(reg) > 4 else 1.0
        if k < 1 or w < 1 or k * m * w >= 2 ** 31:
            raise _hip.WiskiError(f"{what}: a region needs k, w >= 1 and k m w < 2^31, got k = {k}, w = {w}, m = {m}")
        for t, n, name in ((src, n_src, "src"), (dst, n_dst, "dst")):
            if n is not None and (t.numel() != k * n * w or not t.is_contiguous()):
                raise _hip.WiskiError(f"{what}: {name} of {t.numel()} elements is no contiguous region of k = {k} blocks of {n} nodes of w = {w}")
        if dst is not None and (src.dtype != dst.dtype or src.device != dst.device):
            raise _hip.WiskiError(f"{what}: src and dst of a region must have one dtype and device")
        regs.append((src, dst, k, w, fac))
    if regs and any(r[0].dtype != regs[0][0].dtype or r[0].device != regs[0][0].device for r in regs):
        raise _hip.WiskiError(f"{what}: the regions must have one dtype and device")
    return regs


def _stats_plans(regs):
    for i in range(0, len(regs), _hip.STATS_MAX_REGIONS):
        part = regs[i:i + _hip.STATS_MAX_REGIONS]
        plan = _hip.wiski_stats_plan()
        plan.count = len(part)
        for n, (src, dst, k, w, fac) in enumerate(part):
            plan.src[n], plan.k[n], plan.w[n], plan.factor[n] = _hip.dptr(src).value, k, w, fac
            plan.dst[n] = _hip.dptr(dst).value if dst is not None else None
        yield plan, i + len(part) >= len(regs)


def _check_nodes(what, nodes, m):
    if nodes.dtype != torch.int32 or nodes.dim() != 1 or nodes.numel() > m or not nodes.is_contiguous():
        raise _hip.WiskiError(f"{what}: nodes is a contiguous int32 vector of at most m = {m} node indices")


def stats_select(m, regions):
    """The touched nodes of a set of node regions (``wiski_stats_select``): `regions` is a list of ``(tensor, k, w)``, each k
    blocks of m nodes of w reals (element (c, node i, s) at ``c m w + i w + s``), contiguous, of one dtype and device.  Returns ``(nodes,
    n_sel)``: the ascending int32 list of the nodes at which any element of any region is not ``== 0`` (a NaN counts), and its length (the
    one host read).  ROCm tensors: flags, block counts, a one-workgroup scan and the write, four launches (more than 16 regions: one more flag
    launch per 16).  CPU tensors take a plain torch path (``any``), so that a host without a GPU can pack and merge states."""
    m = int(m)
    regs = _stats_regions("stats_select", m, [(t, None, k, w) for t, k, w in regions], m, None)
    if not regs:
        raise _hip.WiskiError("stats_select: no region")
    dtype, dev = regs[0][0].dtype, regs[0][0].device
    if not regs[0][0].is_cuda:
        on = torch.zeros(m, dtype=torch.bool)
        for src, _, k, w, _ in regs:
            on |= (src.reshape(k, m, w) != 0).any(dim=2).any(dim=0)
        nodes = on.nonzero().reshape(-1).to(torch.int32)
        return nodes, int(nodes.numel())
    f = _hip.fn("wiski_stats_select", dtype)
    nb = -(-m // 256)
    flags = torch.zeros(m, dtype=torch.int32, device=dev)
    nodes = torch.empty(m, dtype=torch.int32, device=dev)
    work = torch.empty(nb + 1, dtype=torch.int32, device=dev)      # block counts, and n_sel behind them
    for plan, is_last in _stats_plans(regs):
        rc = f(ctypes.byref(plan), ctypes.c_int64(m), _hip.dptr(flags), _hip.dptr(nodes) if is_last else None, _hip.dptr(work[nb:]) if is_last else None,
               _hip.dptr(work) if is_last else None, ctypes.c_int64(nb), _hip.stream_ptr(dev))
        _hip.check(rc, "wiski_stats_select")
    n_sel = int(work[nb].item())
    return nodes[:n_sel], n_sel


def stats_gather(m, nodes, regions, err=None):
    """``dst[c n_sel w + j w + s] = src[c m w + nodes[j] w + s]`` for every region ``(src, dst, k, w)`` in one launch per 16
    (``wiski_stats_gather``): src holds k m w elements, dst k n_sel w.  A node index outside [0, m) is skipped and sets bit 0
    of `err` (an int32 device flag).  CPU tensors: ``index_select`` (a bad index raises)."""
    m = int(m)
    _check_nodes("stats_gather", nodes, m)
    n_sel = nodes.numel()
    regs = _stats_regions("stats_gather", m, regions, m, n_sel)
    if not regs or n_sel == 0:
        return
    dtype, dev = regs[0][0].dtype, regs[0][0].device
    if not regs[0][0].is_cuda:
        idx = nodes.long()
        for src, dst, k, w, _ in regs:
            dst.reshape(k, n_sel, w).copy_(src.reshape(k, m, w).index_select(1, idx))
        return
    f = _hip.fn("wiski_stats_gather", dtype)
    for plan, _ in _stats_plans(regs):
        rc = f(ctypes.byref(plan), ctypes.c_int64(m), _hip.dptr(nodes), ctypes.c_int64(n_sel), _hip.dptr(err), _hip.stream_ptr(dev))
        _hip.check(rc, "wiski_stats_gather")


def stats_scatter_add(m, nodes, regions, err=None, src_full=False):
    """``dst[c m w + nodes[j] w + s] += f src[c n_sel w + j w + s]`` for every region ``(src, dst, k, w[, f])`` in one launch per 16
    (``wiski_stats_scatter_add``).  f is rounded once to the tensors' dtype; f = 1 is a plain add, otherwise a rounded
    product and a rounded add.  `nodes` is free of duplicates (``stats_select``'s list is), so no atomics are needed.  src_full: src is a full
    region of k m w elements, read at the index dst is written at.  A node index outside [0, m) is skipped and sets bit 0 of `err`.  CPU
    tensors: ``index_add_`` of the rounded product (a bad index raises)."""
    m = int(m)
    _check_nodes("stats_scatter_add", nodes, m)
    n_sel = nodes.numel()
    regs = _stats_regions("stats_scatter_add", m, regions, m if src_full else n_sel, m)
    if not regs or n_sel == 0:
        return
    dtype, dev = regs[0][0].dtype, regs[0][0].device
    if not regs[0][0].is_cuda:
        idx = nodes.long()
        for src, dst, k, w, fac in regs:
            s = src.reshape(k, -1, w)
            s = s.index_select(1, idx) if src_full else s
            fr = torch.tensor(fac, dtype=dtype)
            dst.reshape(k, m, w).index_add_(1, idx, s if bool(fr == 1) else s * fr)
        return
    f = _hip.fn("wiski_stats_scatter_add", dtype)
    for plan, _ in _stats_plans(regs):
        rc = f(ctypes.byref(plan), ctypes.c_int64(m), _hip.dptr(nodes), ctypes.c_int64(n_sel), ctypes.c_int32(1 if src_full else 0), _hip.dptr(err),
               _hip.stream_ptr(dev))
        _hip.check(rc, "wiski_stats_scatter_add")


def stencil_expand_add(grid, A_half, A_st):
    """A_st += expand(A_half) (delta and its mirror image); A_half is zeroed."""
    rc = _hip.fn("wiski_stencil_expand_add", A_st.dtype)(grid.ref, _hip.dptr(A_half), _hip.dptr(A_st), _hip.stream_ptr(A_st.device))
    _hip.check(rc, "wiski_stencil_expand_add")


def wt_columns(grid, x, err):
    """Dense columns of W(x)^T: [n, m]."""
    x = _x2d(x, grid)
    out = torch.zeros((x.shape[0], grid.m), dtype=x.dtype, device=x.device)
    rc = _hip.fn("wiski_wt_columns", x.dtype)(grid.ref, _hip.dptr(x), ctypes.c_int64(x.shape[0]), _hip.dptr(out), _hip.dptr(err),
                                              _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_wt_columns")
    return out


def wt_columns_jet(grid, x, err):
    """The jet rows J_c(x_p) as dense columns: [n C, m], row p C + c (C = d + 1; ``wiski_wt_columns_jet``)."""
    x = _x2d(x, grid)
    out = torch.zeros((x.shape[0] * (grid.d + 1), grid.m), dtype=x.dtype, device=x.device)
    rc = _hip.fn("wiski_wt_columns_jet", x.dtype)(grid.ref, _hip.dptr(x), ctypes.c_int64(x.shape[0]), _hip.dptr(out), _hip.dptr(err),
                                                  _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_wt_columns_jet")
    return out


def jet_quadform(grid, x, M, err):
    """out[p, c, c'] = J_c(x_p)^T M J_c'(x_p) for a dense row-major M [m, >= m] (leading dimension ``M.stride(0)``): [n, C, C],
    exactly symmetric (``wiski_jet_quadform``)."""
    x = _x2d(x, grid)
    assert M.dim() == 2 and M.shape[0] == grid.m and M.shape[1] >= grid.m and M.stride(1) == 1 and M.dtype == x.dtype
    C = grid.d + 1
    out = torch.empty((x.shape[0], C, C), dtype=x.dtype, device=x.device)
    if not M.is_cuda:
        raise _hip.WiskiError("online_gp_amd ops need ROCm device tensors (no CPU fallback)")
    rc = _hip.fn("wiski_jet_quadform", x.dtype)(grid.ref, _hip.dptr(x), ctypes.c_int64(x.shape[0]), ctypes.c_void_p(M.data_ptr()),
                                                ctypes.c_int64(M.stride(0)), _hip.dptr(out), _hip.dptr(err), _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_jet_quadform")
    return out


def gather_jet(grid, x, V, err, rows_per_point=0):
    """Value and gradient gather in one launch (``wiski_gather_jet``): out[p, j, c] = J_c(x_p) . V[j] for V [k, m] shared by all
    points (rows_per_point = 0; [n, k, C]), or J_c(x_p) . V[p B + j] for V [n B, m] (rows_per_point = B; [n, B, C])."""
    x = _x2d(x, grid)
    V = V.contiguous()
    if V.dim() == 1:
        V = V[None]
    n, B = x.shape[0], int(rows_per_point)
    assert V.shape[1] == grid.m and V.dtype == x.dtype and (B == 0 or V.shape[0] == n * B)
    k = B if B > 0 else V.shape[0]
    out = torch.empty((n, k, grid.d + 1), dtype=x.dtype, device=x.device)
    rc = _hip.fn("wiski_gather_jet", x.dtype)(grid.ref, _hip.dptr(x), ctypes.c_int64(n), _hip.dptr(V), ctypes.c_int32(max(k, 1)), ctypes.c_int32(B),
                                              _hip.dptr(out), _hip.dptr(err), _hip.stream_ptr(x.device))
    _hip.check(rc, "wiski_gather_jet")
    return out


class BoxTables:
    """Per-dimension integrated rows of B boxes (``wiski_box_tables``): ``tab`` [B, sum g_q], ``range`` int32 [B, d, 2] (the node range
    of each row's support), ``vol`` [B] (the clipped volume).  ``tables[s:e]`` is the same for a run of the boxes."""

    def __init__(self, tab, range_, vol):
        self.tab, self.range, self.vol = tab, range_, vol
        self.B = tab.shape[0]

    def __getitem__(self, sl):
        assert isinstance(sl, slice) and sl.step in (None, 1)
        return BoxTables(self.tab[sl], self.range[sl], self.vol[sl])


def box_tables(grid, lower, upper, err):
    """Tables of the box functionals c_b = int_[lower_b, upper_b] w(x) dx for bounds [B, d] (``wiski_box_tables``)."""
    lo, hi = _x2d(lower, grid), _x2d(upper, grid)
    if lo.shape != hi.shape or lo.dtype != hi.dtype or lo.device != hi.device:
        raise ValueError(f"lower {tuple(lo.shape)} {lo.dtype} and upper {tuple(hi.shape)} {hi.dtype} must match")
    B = lo.shape[0]
    tab = torch.empty((B, sum(grid.g)), dtype=lo.dtype, device=lo.device)
    rng = torch.empty((B, grid.d, 2), dtype=torch.int32, device=lo.device)
    vol = torch.empty((B,), dtype=lo.dtype, device=lo.device)
    rc = _hip.fn("wiski_box_tables", lo.dtype)(grid.ref, _hip.dptr(lo), _hip.dptr(hi), ctypes.c_int64(B), _hip.dptr(tab), _hip.dptr(rng), _hip.dptr(vol),
                                              _hip.dptr(err), _hip.stream_ptr(lo.device))
    _hip.check(rc, "wiski_box_tables")
    return BoxTables(tab, rng, vol)


def wt_columns_box(grid, tables):
    """The box functionals as dense columns: [B, m] (``wiski_wt_columns_box``)."""
    tab = tables.tab
    out = torch.zeros((tables.B, grid.m), dtype=tab.dtype, device=tab.device)
    rc = _hip.fn("wiski_wt_columns_box", tab.dtype)(grid.ref, _hip.dptr(tab), _hip.dptr(tables.range), ctypes.c_int64(tables.B), _hip.dptr(out),
                                                    _hip.stream_ptr(tab.device))
    _hip.check(rc, "wiski_wt_columns_box")
    return out


BOX_GATHER_BLOCKS = 2048      # blocks that a box gather aims for: eight per compute unit of an MI355X


def box_gather_nsplit(grid, pairs):
    """Blocks per (box, row) of ``gather_box``: enough for BOX_GATHER_BLOCKS in all, at most one per 1024 entries of a domain-sized
    support (256 lanes, four entries each) -- the host does not know the boxes' sizes, a small box leaves its extra blocks idle."""
    return max(1, min(-(-BOX_GATHER_BLOCKS // max(int(pairs), 1)), -(-grid.m // 1024)))


def gather_box(grid, tables, V, rows_per_box=0, nsplit=None):
    """``wiski_gather_box``: out[b, j] = c_b . V[j] for V [k, m] shared by all boxes (rows_per_box = 0; [B, k]), or c_b . V[b R + j] for
    V [B R, m] (rows_per_box = R; [B, R]).  nsplit: blocks per (box, row), ``box_gather_nsplit`` by default."""
    tab = tables.tab
    V = V.contiguous()
    if V.dim() == 1:
        V = V[None]
    B, R = tables.B, int(rows_per_box)
    assert V.shape[1] == grid.m and V.dtype == tab.dtype and (R == 0 or V.shape[0] == B * R)
    k = R if R > 0 else V.shape[0]
    out = torch.empty((B, k), dtype=tab.dtype, device=tab.device)
    ns = box_gather_nsplit(grid, B * k) if nsplit is None else int(nsplit)
    part = torch.empty((B * k * ns,), dtype=torch.float64, device=tab.device) if ns > 1 and B > 0 else None
    rc = _hip.fn("wiski_gather_box", tab.dtype)(grid.ref, _hip.dptr(tab), _hip.dptr(tables.range), ctypes.c_int64(B), _hip.dptr(V),
                                                ctypes.c_int32(max(k, 1)), ctypes.c_int32(R), ctypes.c_int32(ns), _hip.dptr(part), _hip.dptr(out),
                                                _hip.stream_ptr(tab.device))
    _hip.check(rc, "wiski_gather_box")
    return out


def is_half_stencil(grid, A_st):
    """True for the symmetric half-stencil layout [(R+1)/2, m], False for the full [R, m] one."""
    rows = A_st.shape[-2]
    if rows == (grid.R + 1) // 2:
        return True
    if rows == grid.R:
        return False
    raise ValueError(f"stencil with {rows} rows matches neither the full ({grid.R}) nor the half ({(grid.R + 1) // 2}) layout")


def half_stencil_from_offset_major(grid, A_om):
    """Offset-major half stencil ``A_om[oh, i] = A[i, i + off(c + oh)]`` ([(R+1)/2, m], e.g. the upper half of
    the oracle's full stencil) -> the native row-interleaved layout of wiski_scatter_stats_sym (same shape,
    different memory order: see include/wiski.h)."""
    H, m = A_om.shape
    flat = torch.empty(H * m, dtype=A_om.dtype, device=A_om.device)
    flat[:4 * m] = A_om[:4].t().reshape(-1)
    if H > 4:
        flat[4 * m:] = A_om[4:].reshape(-1, 7, m).transpose(1, 2).reshape(-1)
    return flat.view(H, m)


def half_stencil_to_offset_major(grid, A_h):
    """Inverse of :func:`half_stencil_from_offset_major`."""
    H, m = A_h.shape
    flat = A_h.reshape(-1)
    out = torch.empty((H, m), dtype=A_h.dtype, device=A_h.device)
    out[:4] = flat[:4 * m].view(m, 4).t()
    if H > 4:
        out[4:] = flat[4 * m:].view(-1, m, 7).transpose(1, 2).reshape(H - 4, m)
    return out


def stencil_spmv(grid, A_st, V, add=None, beta=1.0):
    """A @ V on the block stencil: A_st is either the full offset-major [R, m] stencil or the symmetric half
    ([(R+1)/2, m] reals in the native row-interleaved layout)."""
    V2 = V.contiguous().reshape(-1, grid.m)
    out = torch.empty_like(V2)
    cr = _hip.creal(V2.dtype)
    name = "wiski_stencil_spmv_sym" if is_half_stencil(grid, A_st) else "wiski_stencil_spmv"
    rc = _hip.fn(name, V2.dtype)(grid.ref, _hip.dptr(A_st), _hip.dptr(V2), ctypes.c_int32(V2.shape[0]),
                                 _hip.dptr(add.contiguous().reshape(-1, grid.m)) if add is not None else None, cr(beta),
                                 _hip.dptr(out), _hip.stream_ptr(V2.device))
    _hip.check(rc, name)
    return out.reshape(V.shape)


def kron_toeplitz_mm(grid, tcol, V, scale=1.0):
    V2 = V.contiguous().reshape(-1, grid.m)
    out = torch.empty_like(V2)
    tmp = torch.empty_like(V2) if grid.d > 1 else None
    cr = _hip.creal(V2.dtype)
    rc = _hip.fn("wiski_kron_toeplitz_mm", V2.dtype)(grid.ref, _hip.dptr(tcol.contiguous()), _hip.dptr(V2), ctypes.c_int32(V2.shape[0]), cr(scale),
                                                     _hip.dptr(tmp), _hip.dptr(out), _hip.stream_ptr(V2.device))
    _hip.check(rc, "wiski_kron_toeplitz_mm")
    return out.reshape(V.shape)


class PCGWorkspace:
    """Device scratch for wiski_pcg, cached per (k, max_iter)."""

    def __init__(self):
        self.buf = None

    def get(self, grid, k, max_iter, dtype, device):
        es = 4 if dtype == torch.float32 else 8
        need = int(_hip.lib().wiski_pcg_workspace_bytes(grid.ref, ctypes.c_int32(k), ctypes.c_int32(max_iter), ctypes.c_int32(es)))
        if need < 0:
            raise _hip.WiskiError("wiski_pcg_workspace_bytes: bad arguments")
        if self.buf is None or self.buf.numel() < need or self.buf.device != device:
            self.buf = torch.empty(need, dtype=torch.uint8, device=device)
        return self.buf, need


class _StreamArgs32(ctypes.Structure):
    _fields_ = [("d_A_half", ctypes.c_void_p), ("d_b", ctypes.c_void_p), ("d_cnt", ctypes.c_void_p), ("d_stats", ctypes.c_void_p),
                ("d_err", ctypes.c_void_p), ("d_U", ctypes.c_void_p), ("d_Z", ctypes.c_void_p), ("d_R", ctypes.c_void_p),
                ("d_tcol", ctypes.c_void_p), ("kscale", ctypes.c_float), ("d_evec", ctypes.c_void_p), ("d_evec2", ctypes.c_void_p),
                ("d_eval", ctypes.c_void_p), ("shift", ctypes.c_float), ("tol", ctypes.c_double), ("max_iter", ctypes.c_int32),
                ("check_every", ctypes.c_int32), ("d_work", ctypes.c_void_p), ("work_bytes", ctypes.c_int64),
                ("d_bin", ctypes.c_void_p), ("bin_bytes", ctypes.c_int64), ("shard", ctypes.c_void_p), ("two_level", ctypes.c_void_p),
                ("keep", ctypes.c_int32 * 3), ("d_tap_stage", ctypes.c_void_p)]


ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                ctypes.c_void_p)


class _Shard(ctypes.Structure):
    """include/wiski.h: wiski_shard"""
    _fields_ = [("rank", ctypes.c_int32), ("nranks", ctypes.c_int32), ("comm", ctypes.c_void_p), ("allreduce", ALLREDUCE_FN), ("ctx", ctypes.c_void_p)]


class TwoLevelStruct(ctypes.Structure):
    """include/wiski.h: wiski_twolevel"""
    _fields_ = [("r", ctypes.c_int32), ("nslab", ctypes.c_int32), ("d_mask", ctypes.c_void_p), ("d_off", ctypes.c_void_p), ("d_pos", ctypes.c_void_p),
                ("d_N", ctypes.c_void_p), ("d_cs", ctypes.c_void_p), ("d_mc", ctypes.c_void_p), ("mc_cols", ctypes.c_int32)]


def shard_groups(d, rank, nranks):
    """[g_lo, g_hi): the stencil groups rank `rank` of `nranks` owns (wiski_shard_groups; pure host arithmetic)."""
    lo, hi = ctypes.c_int32(0), ctypes.c_int32(0)
    _hip.check(_hip.lib().wiski_shard_groups(ctypes.c_int32(d), ctypes.c_int32(rank), ctypes.c_int32(nranks), ctypes.byref(lo), ctypes.byref(hi)),
               "wiski_shard_groups")
    return int(lo.value), int(hi.value)


def half_stencil_group_slices(grid, g_lo, g_hi):
    """Element ranges [(start, stop), ...] of the flat row-interleaved half stencil that hold the groups [g_lo, g_hi):
    group 0 is A_h[0 : 4 m], group g >= 1 is A_h[(7 g - 3) m : (7 g + 4) m] (include/wiski.h)."""
    m = grid.m
    out = []
    for g in range(g_lo, g_hi):
        out.append((0, 4 * m) if g == 0 else ((7 * g - 3) * m, (7 * g + 4) * m))
    return out


class _StreamArgs64(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double if t is ctypes.c_float else t) for n, t in _StreamArgs32._fields_]


class _PcgAsync(ctypes.Structure):
    _fields_ = [("state", ctypes.c_int32), ("it", ctypes.c_int32), ("seq", ctypes.c_int64), ("poll", ctypes.c_void_p),
                ("prezeroed", ctypes.c_int32), ("guard_ok", ctypes.c_int32), ("shift", ctypes.c_double),
                ("first_ok", ctypes.c_int32), ("first_ok_valid", ctypes.c_int32)]


class StreamStep:
    """Prepared call of ``wiski_stream_step`` (include/wiski.h): the model-resident pointers are marshalled once, a step only
    passes the batch.  Returns (iterations, relative residual, raw out-of-grid flag, converged)."""

    step_log = None

    def __init__(self, grid, dtype, device, A_half, b, cnt, stats, err, U, Z, R, tcol, workspace, max_iter):
        self.grid, self.dtype, self.device = grid, dtype, device
        self.keep = (A_half, b, cnt, stats, err, U, Z, R, tcol)             # the tensors behind the raw pointers
        self.args = (_StreamArgs32 if dtype == torch.float32 else _StreamArgs64)()
        a = self.args
        a.d_A_half, a.d_b, a.d_cnt, a.d_stats, a.d_err = A_half.data_ptr(), b.data_ptr(), cnt.data_ptr(), stats.data_ptr(), err.data_ptr()
        a.d_U, a.d_Z, a.d_R, a.d_tcol = U.data_ptr(), Z.data_ptr(), R.data_ptr(), tcol.data_ptr()
        buf, need = workspace.get(grid, 1, max_iter, dtype, device)
        self.keep += (buf,)
        a.d_work, a.work_bytes, a.max_iter = buf.data_ptr(), need, max_iter
        self.bin_buf = None                    # binning workspace of the owner-computes absorb: grown on demand, zeroed once
        # tap stage of the absorb (include/wiski.h: d_tap_stage): [m][4], zero between calls -- the step's own solve folds it in
        self.tap_stage = torch.zeros(grid.m * 4, dtype=dtype, device=device) if dtype == torch.float32 and grid.d == 3 else None
        a.d_tap_stage = self.tap_stage.data_ptr() if self.tap_stage is not None else None
        self.fn = _hip.fn("wiski_stream_step", dtype)
        self.it, self.herr, self.rr = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_double(0)
        self.eig_keep = None
        self.handle = _PcgAsync()              # deferred-poll state (include/wiski.h: wiski_pcg_async)
        self.resumed = ctypes.c_int32(0)
        # diagnostic, off by default: a file name here (or in StreamStep.step_log before the step is built) appends one line per call --
        # host time, the first_check passed, where the new solve's first poll was placed, what the resumed solve reported, whether the
        # speculative absorb ran (profiles/r09_poll_hindsight.txt was taken with it)
        self.step_log = StreamStep.step_log

    @property
    def pending(self):
        return self.handle.state == 1

    def __del__(self):
        try:
            if self.handle.poll:
                _hip.lib().wiski_pcg_async_free(ctypes.byref(self.handle))
        except Exception:  # noqa: BLE001
            pass

    def set_shard(self, rank, nranks, comm=None, allreduce=None):
        """Stencil-sharded step (wiski_shard): this replica owns the groups shard_groups(d, rank, nranks) of the half stencil.
        comm: an ncclComm_t handle (int) for the RCCL route; allreduce(vec, dots): a Python callable that all-reduces (SUM, in
        place) the two torch views it is given -- the views alias the solver's workspace."""
        if nranks < 1 or (nranks == 1 and not comm):   # (a single rank WITH a communicator runs the sharded path: it owns every group)
            self.args.shard = None
            self._shard = None
            return
        buf = self.keep[-1]                      # the PCG workspace tensor the device pointers of the callback point into
        base = buf.data_ptr()

        def cb(ctx, d_vec, n_vec, elem_bytes, d_dots, n_dots, stream):
            try:
                dt = torch.float32 if elem_bytes == 4 else torch.float64
                vec = buf[d_vec - base:d_vec - base + n_vec * elem_bytes].view(dt)
                dots = buf[d_dots - base:d_dots - base + n_dots * 8].view(torch.float64) if (d_dots and n_dots) else None
                allreduce(vec, dots)
                return 0
            except Exception:  # noqa: BLE001
                import traceback

                traceback.print_exc()
                return -2

        self._shard_cb = ALLREDUCE_FN(cb) if allreduce is not None else ALLREDUCE_FN()
        self._shard = _Shard(rank, nranks, comm, self._shard_cb, None)
        self.args.shard = ctypes.addressof(self._shard)

    def set_two_level(self, tl):
        """tl: a TwoLevelStruct kept alive by the caller (its d_N may be re-pointed between steps), or None."""
        self._two_level = tl
        self.args.two_level = ctypes.addressof(tl) if tl is not None else None

    def set_keep(self, keep):
        """keep: the eigenmodes per dimension the solve's preconditioner transforms (`keep_counts`), or None: all of them."""
        k = tuple(int(v) for v in keep) if keep is not None else (0, 0, 0)
        if tuple(self.args.keep) != k:
            self.args.keep[:] = k

    def set_solver(self, kscale, eig, shift, tol, check_every):
        a = self.args
        evec, evals, evec2 = (tuple(eig) + (None,))[:3]
        self.eig_keep = (evec, evals, evec2)
        a.kscale, a.shift, a.tol, a.check_every = kscale, shift, tol, check_every
        a.d_evec, a.d_eval = evec.data_ptr(), evals.data_ptr()
        a.d_evec2 = evec2.data_ptr() if evec2 is not None else None

    def __call__(self, x, y, wa, wb, noise, mean_out, carry, first_check, defer=False):
        """Without deferral: (iterations, relres, out-of-grid flag, converged) of THIS step's solve.  With `defer` (or a pending
        solve): the same four values describe the solve a previous call started (None when there was none) and the fifth
        element says whether this step's solve is now pending."""
        q = x.shape[0] if x is not None else 0
        if q >= 4096 and self.grid.d == 3 and (self.bin_buf is None or self.bin_q < q):
            f = _hip.lib().wiski_scatter_bin_bytes
            f.restype = ctypes.c_int64
            need = int(f(self.grid.ref, ctypes.c_int64(q), ctypes.c_int32(4 if self.dtype == torch.float32 else 8)))
            if need > 0:
                self.bin_buf, self.bin_q = torch.zeros(need, dtype=torch.uint8, device=self.device), q
                self.args.d_bin, self.args.bin_bytes = self.bin_buf.data_ptr(), need
        use_handle = defer or self.pending
        self.herr.value = 0
        rc = self.fn(self.grid.ref, ctypes.byref(self.args), _hip.dptr(x), _hip.dptr(y), _hip.dptr(wa), _hip.dptr(wb), _hip.dptr(noise),
                     ctypes.c_int64(q), _hip.dptr(mean_out), ctypes.c_int32(int(carry)), ctypes.c_int32(int(first_check)), ctypes.byref(self.it),
                     ctypes.byref(self.rr), ctypes.byref(self.herr), _hip.stream_ptr(self.device),
                     ctypes.byref(self.handle) if use_handle else None, ctypes.c_int32(int(defer)), ctypes.byref(self.resumed))
        if rc == -4:
            warnings.warn(f"wiski_pcg stopped at max_iter={self.args.max_iter} with relative residual {self.rr.value:.3e}", RuntimeWarning)
        elif rc != 1:
            _hip.check(rc, "wiski_stream_step")
        res = (int(self.it.value), float(self.rr.value), int(self.herr.value), rc != -4)
        if self.step_log:
            h = self.handle
            with open(self.step_log, "a") as f:
                f.write("t_us=%.1f q=%d first_check=%d placed=%d rc=%d resumed=%d iters=%d relres=%.3e guard_ok=%d first_ok=%d/%d\n" % (
                    time.perf_counter() * 1e6, q, int(first_check), h.it if use_handle else -1, rc, self.resumed.value, res[0], res[1],
                    h.guard_ok, h.first_ok, h.first_ok_valid))
        if not use_handle:
            return res
        # resumed == 2: a pending solve was finished AND this step's solve ran synchronously -- `res` describes the latter
        return (res if self.resumed.value == 1 else None), self.pending


def precond_apply(grid, eig, kscale, shift, r, two_level=None):
    """One application of the fused fp32 preconditioner to the grid vector r: (y = P r, t = Kt^-1 y, r . y) -- `precond_apply_cols` of one row."""
    Y, T, rho = precond_apply_cols(grid, eig, kscale, shift, r.reshape(1, grid.m), two_level=two_level)
    return Y.reshape(r.shape), T.reshape(r.shape), rho[0]


KEEP_EPS = 2.0 ** -30      # modes whose w = a lam / (1 + a lam) is below this pass the preconditioner untransformed (t = r, y = 0)


def keep_counts(D_host, kscale, shift, eps=KEEP_EPS):
    """Which eigenmodes the separable preconditioner has to transform (csrc/spectral_keep.h).  D_host: per-dim eigenvalues, ascending
    (``kron_eigen(..., host_out)["D"]``).  K_q = number of indices of dim q with w = a lam / (1 + a lam) > eps, a = shift,
    lam = kscale D_q[j] prod_{p != q} max D_p (the other dims at their largest eigenvalue); eigenvalues below g_q 2^-52 of the dim's
    largest are eigensolver noise and count as zero.  Returns (K, lo, hi): the counts rounded up to multiples of 4 -- or None
    where the rule keeps everything, nothing, or a dim whose size is no multiple of 4 in full -- and the interval lo < shift <= hi
    on which the unrounded counts stay what they are (so a caller recomputes only when the shift leaves it)."""
    import numpy as np

    if not (shift > 0 and kscale > 0):
        return None, 0.0, 0.0
    tau = eps / (1.0 - eps)                         # w > eps  <=>  a lam > tau
    dmax = [float(D[-1]) for D in D_host]
    if min(dmax) <= 0:
        return None, 0.0, 0.0
    K, lo, hi = [], 0.0, np.inf
    for q, D in enumerate(D_host):
        g = len(D)
        d = np.where(D < g * 2.0 ** -52 * dmax[q], 0.0, D)
        c = kscale * float(np.prod([dmax[p] for p in range(len(D_host)) if p != q]))
        first = int(np.searchsorted(d, tau / (shift * c), side="right"))        # first kept index
        K.append(g - first)
        if first < g:
            lo = max(lo, tau / (c * d[first]))
        if first > 0 and d[first - 1] > 0:
            hi = min(hi, tau / (c * d[first - 1]))
    out = []
    for q, D in enumerate(D_host):
        g, k4 = len(D), -(-K[q] // 4) * 4
        if K[q] < 1 or (k4 > g and g % 4 != 0):
            return None, lo, hi
        out.append(min(k4, g))
    if all(k == len(D) for k, D in zip(out, D_host)):
        return None, lo, hi
    return tuple(out), lo, hi


def keep_accepts(grid, keep, two_level=False):
    """Would a solve on `grid` take these kept-mode counts (wiski_precond_keep_ok: cap 24 per dim, coefficient cubes within the backward
    kernel's LDS budget)?"""
    return bool(_hip.lib().wiski_precond_keep_ok(grid.ref, (ctypes.c_int32 * 3)(*[int(v) for v in keep]), ctypes.c_int32(int(bool(two_level)))))


def precond_apply_keep(grid, eig, kscale, shift, r, keep, two_level=None):
    """`precond_apply` on the kept modes only (``wiski_precond_apply_keep_f32``); keep = None or zeros: the full transforms."""
    evec, evals, evec2 = (tuple(eig) + (None,))[:3]
    r = r.contiguous()
    m = r.numel()
    w0 = torch.empty(m, dtype=r.dtype, device=r.device)
    w1 = torch.empty(2 * m, dtype=r.dtype, device=r.device)
    y, t = torch.empty_like(r), torch.empty_like(r)
    rho = torch.zeros(1, dtype=torch.float64, device=r.device)
    kp = (ctypes.c_int32 * 3)(*([int(v) for v in keep] if keep is not None else [0, 0, 0]))
    rc = _hip.lib().wiski_precond_apply_keep_f32(grid.ref, _hip.dptr(evec), _hip.dptr(evec2), _hip.dptr(evals), ctypes.c_float(kscale), ctypes.c_float(shift),
                                                 _hip.dptr(r), _hip.dptr(w0), _hip.dptr(w1), _hip.dptr(y), _hip.dptr(t), _hip.dptr(rho),
                                                 ctypes.byref(two_level) if two_level is not None else None, kp, _hip.stream_ptr(r.device))
    _hip.check(rc, "wiski_precond_apply_keep")
    return y, t, rho[0]


def precond_apply_cols(grid, eig, kscale, shift, R, two_level=None):
    """`precond_apply` for the k rows of R [k, m] through the multi-column kernels (``wiski_precond_apply_cols``): (Y, T, rho [k])."""
    evec, evals, evec2 = (tuple(eig) + (None,))[:3]
    R = R.contiguous()
    k, m = R.shape
    w0 = torch.empty(k * m, dtype=R.dtype, device=R.device)
    w1 = torch.empty(2 * k * m, dtype=R.dtype, device=R.device)
    Y, T = torch.empty_like(R), torch.empty_like(R)
    rho = torch.zeros(k, dtype=torch.float64, device=R.device)
    rc = _hip.lib().wiski_precond_apply_cols_f32(grid.ref, _hip.dptr(evec), _hip.dptr(evec2), _hip.dptr(evals), ctypes.c_float(kscale), ctypes.c_float(shift),
                                                 _hip.dptr(R), ctypes.c_int32(k), _hip.dptr(w0), _hip.dptr(w1), _hip.dptr(Y), _hip.dptr(T), _hip.dptr(rho),
                                                 ctypes.byref(two_level) if two_level is not None else None, _hip.stream_ptr(R.device))
    _hip.check(rc, "wiski_precond_apply_cols")
    return Y, T, rho


def kron_eigen(grid, tcol, profiles=None, host_out=None, dtype=None):
    """Per-dim (generalized) eigen-decomposition of the d small symmetric-Toeplitz Kronecker
    factors (host side, fp64, O(d g^3) -- done when the hyper-parameters or the data-density
    profile change, not per streaming update).

    profiles=None:  K_q = V_q diag(lam_q) V_q^T                         -> (evec, evals)
    profiles=[t_q]: K_q = X_q D_q X_q^T with X_q^T diag(t_q) X_q = I     -> (evec = X, evals = D, evec2 = Z = diag(t) X)
    Eigenvalues are clamped >= 0.  Feeds wiski_pcg's preconditioner (K^-1 + a kron diag(t_q))^-1.
    dtype: of the returned tables (default: tcol's).  fp32 tables from fp64 columns keep the super-exponential tail of a smooth
    prior's spectrum down to the eigensolver's own noise (~1e-16 of the largest eigenvalue); columns rounded to fp32 first bury
    it under ~1e-9 of rounding noise, half of it positive -- modes that `keep_counts` would then have to keep."""
    import numpy as np

    tc = tcol.detach().to("cpu", torch.float64).numpy()
    X, Z, vals, off = [], [], [], 0
    for q, g in enumerate(grid.g):
        c = tc[off:off + g]
        idx = np.abs(np.arange(g)[:, None] - np.arange(g)[None, :])
        K = c[idx]
        if profiles is None:
            w, V = np.linalg.eigh(K)
            X.append(V.reshape(-1))
        else:
            t = np.asarray(profiles[q], dtype=np.float64)
            rt = np.sqrt(t)
            w, U = np.linalg.eigh(rt[:, None] * K * rt[None, :])
            X.append((U / rt[:, None]).reshape(-1))
            Z.append((U * rt[:, None]).reshape(-1))
        vals.append(np.clip(w, 0.0, None))
        off += g
    mk = lambda parts: torch.as_tensor(np.concatenate(parts)).to(tcol.device, dtype or tcol.dtype)
    if host_out is not None:              # fp64 host copies (per dim: eigenvectors [g, g] column = mode, eigenvalues ascending)
        host_out["X"] = [x.reshape(g, g) for x, g in zip(X, grid.g)]
        host_out["D"] = [v.copy() for v in vals]
    if profiles is None:
        return mk(X), mk(vals)
    return mk(X), mk(vals), mk(Z)


def _pcg_abi(dtype, *, grid, A, a_sym, RHS, k, tcol, kscale, evec, evec2, eval, shift, U, Z, R, warm, tol, max_iter, check_every, first_check,
             work, work_bytes, h_iters, h_relres, d_err, h_err, stream):
    """What every ``wiski_pcg*`` entry point starts with (include/wiski.h), from fields named and grouped as in the solve's record
    (csrc/pcg.h: PcgArgs) -- the one place the ABI's order is written down."""
    cr, i32, p = _hip.creal(dtype), (lambda v: ctypes.c_int32(int(v))), _hip.dptr
    return (grid.ref, p(A), p(tcol), cr(kscale), p(evec), p(evec2), p(eval), cr(shift), p(RHS), i32(k), p(U), p(Z), i32(warm), ctypes.c_double(tol),
            i32(max_iter), i32(check_every), i32(first_check), p(work), ctypes.c_int64(work_bytes), ctypes.byref(h_iters), h_relres, p(d_err),
            ctypes.byref(h_err), i32(a_sym), p(R), stream)


def pcg(grid, A_st, tcol, kscale, RHS, U=None, Z=None, warm=False, tol=1e-6, max_iter=1000, check_every=10, workspace=None,
        raise_on_fail=False, eigen=None, shift=0.0, first_check=0, err=None, inplace=False, R=None, two_level=None):
    """Solve (Kt^-1 + A) U = RHS, Kt = kscale*Kuu.  Returns (U, Z, iters, relres).
    two_level: a TwoLevelStruct (include/wiski.h: wiski_twolevel) -- the exact block on the dominant modes inside the fused
    preconditioner (``wiski_pcg_twolevel_f32``: fp32, d = 3, eigen tables given; one column, or up to ``two_level.mc_cols``
    columns when the block carries the multi-column scratch ``d_mc``; otherwise the argument is ignored).
    eigen = (evec, evals) from :func:`kron_eigen` selects the spectral
    preconditioner (Kt^-1 + shift I)^-1; otherwise Kt itself preconditions.
    R [k, m] (optional, contiguous): caller-owned residual buffer, left holding RHS - Z - A U;
    warm=2 starts from the residual already in R (see wiski.h) instead of forming A U."""
    RHS2 = RHS.contiguous().reshape(-1, grid.m)
    k = RHS2.shape[0]
    if U is None or Z is None or (not warm and not inplace):
        U = torch.empty_like(RHS2)
        Z = torch.empty_like(RHS2)
        warm = False
    if int(warm) == 2 and R is None:
        raise ValueError("warm=2 needs the carried-over residual R")
    ws = workspace if workspace is not None else PCGWorkspace()
    buf, need = ws.get(grid, k, max_iter, RHS2.dtype, RHS2.device)
    iters = ctypes.c_int32(0)
    h_err = ctypes.c_int32(0)
    relres = (ctypes.c_double * k)()
    evec, evals, evec2 = (tuple(eigen) + (None,))[:3] if eigen is not None else (None, None, None)
    common = _pcg_abi(RHS2.dtype, grid=grid, A=A_st, a_sym=is_half_stencil(grid, A_st), RHS=RHS2, k=k,
                      tcol=tcol.contiguous(), kscale=kscale, evec=evec, evec2=evec2, eval=evals, shift=shift,
                      U=U, Z=Z, R=R, warm=warm, tol=tol, max_iter=max_iter, check_every=check_every, first_check=first_check,
                      work=buf, work_bytes=need, h_iters=iters, h_relres=relres, d_err=err, h_err=h_err, stream=_hip.stream_ptr(RHS2.device))
    if two_level is not None and (k == 1 or (two_level.d_mc and k <= two_level.mc_cols)) and RHS2.dtype == torch.float32 and evec is not None:
        rc = _hip.lib().wiski_pcg_twolevel_f32(*common, None, ctypes.c_int32(0), None, ctypes.byref(two_level))
    else:
        rc = _hip.fn("wiski_pcg", RHS2.dtype)(*common)
    if rc == -4 and not raise_on_fail:
        # gpytorch emits a NumericalWarning when CG stops at max_cg_iterations; callers also see it in `relres`
        warnings.warn(f"wiski_pcg stopped at max_iter={max_iter} with relative residual {max(relres):.3e} (tolerance {tol:.1e})",
                      RuntimeWarning)
        pcg.last_converged = False
    else:
        _hip.check(rc, "wiski_pcg")
        pcg.last_converged = True
    pcg.last_err = int(h_err.value)
    return U, Z, int(iters.value), list(relres)


pcg.last_err = 0
pcg.last_converged = True


def kron_toeplitz_grad(grid, tcol, X, Y):
    """d/d tcol of sum_c X[c]^T (kron SymToeplitz(tcol)) Y[c]  -> float64 [sum g]."""
    X2 = X.contiguous().reshape(-1, grid.m)
    Y2 = Y.contiguous().reshape(-1, grid.m)
    k = X2.shape[0]
    tmp = torch.empty((2 * k, grid.m), dtype=X2.dtype, device=X2.device)
    grad = torch.zeros(sum(grid.g), dtype=torch.float64, device=X2.device)
    rc = _hip.fn("wiski_kron_toeplitz_grad", X2.dtype)(grid.ref, _hip.dptr(tcol.contiguous()), _hip.dptr(X2), _hip.dptr(Y2), ctypes.c_int32(k),
                                                       _hip.dptr(tmp), _hip.dptr(grad), _hip.stream_ptr(X2.device))
    _hip.check(rc, "wiski_kron_toeplitz_grad")
    return grad


def kron_spectral_mm(grid, eigen, V, kscale=1.0, shift=0.0, power=0.5, rpower=0.0):
    """V diag(lam^power / (1 + shift lam)^rpower) V^T applied to the columns of V ([k, m])."""
    evec, evals = eigen[0], eigen[1]
    assert len(eigen) == 2, "kron_spectral_mm needs the orthogonal eigenbasis (kron_eigen without profiles)"
    V2 = V.contiguous().reshape(-1, grid.m)
    out = torch.empty_like(V2)
    tmp = torch.empty_like(V2)
    cr = _hip.creal(V2.dtype)
    rc = _hip.fn("wiski_kron_spectral_mm", V2.dtype)(grid.ref, _hip.dptr(evec), _hip.dptr(evals), cr(kscale), cr(shift), cr(power), cr(rpower),
                                                     _hip.dptr(V2), ctypes.c_int32(V2.shape[0]), _hip.dptr(tmp), _hip.dptr(out),
                                                     _hip.stream_ptr(V2.device))
    _hip.check(rc, "wiski_kron_spectral_mm")
    return out.reshape(V.shape)


# ------------------------------------------------------------ dense (small-m) ops --
def gemm(A, B, ta=False, tb=False, alpha=1.0, beta=0.0, C=None):
    """C = alpha op(A) op(B) + beta C on the matrix cores (row-major 2-D tensors)."""
    A, B = A.contiguous(), B.contiguous()
    M = A.shape[1] if ta else A.shape[0]
    K = A.shape[0] if ta else A.shape[1]
    N = B.shape[0] if tb else B.shape[1]
    assert (B.shape[1] if tb else B.shape[0]) == K and A.dtype == B.dtype
    if C is None:
        C = torch.empty((M, N), dtype=A.dtype, device=A.device)
        beta = 0.0
    cr = _hip.creal(A.dtype)
    rc = _hip.fn("wiski_gemm", A.dtype)(ctypes.c_int32(int(ta)), ctypes.c_int32(int(tb)), ctypes.c_int32(M), ctypes.c_int32(N), ctypes.c_int32(K),
                                        cr(alpha), _hip.dptr(A), ctypes.c_int32(A.shape[1]), _hip.dptr(B), ctypes.c_int32(B.shape[1]), cr(beta),
                                        _hip.dptr(C), ctypes.c_int32(C.shape[1]), _hip.stream_ptr(A.device))
    _hip.check(rc, "wiski_gemm")
    return C


def gemm_path(M, N, K, dtype):
    """The kernel ``wiski_gemm`` takes for an M x N output over K terms (``wiski_gemm_path``; host only, launches nothing):
    0 k_gemm, 1 k_gemm32, 2 k_gemm128 on 64-tiles, 3 k_gemm128 on 128-tiles."""
    rc = _hip.lib().wiski_gemm_path(ctypes.c_int32(M), ctypes.c_int32(N), ctypes.c_int32(K), ctypes.c_int32(4 if dtype == torch.float32 else 8))
    if rc < 0:
        _hip.check(rc, "wiski_gemm_path")
    return rc


def potrf_(A, info=None):
    """In-place lower Cholesky; returns the device info flag (non-zero: not positive definite)."""
    assert A.dim() == 2 and A.shape[0] == A.shape[1] and A.is_contiguous()
    if info is None:
        info = torch.zeros(1, dtype=torch.int32, device=A.device)
    rc = _hip.fn("wiski_potrf", A.dtype)(ctypes.c_int32(A.shape[0]), _hip.dptr(A), ctypes.c_int32(A.shape[1]), _hip.dptr(info),
                                         _hip.stream_ptr(A.device))
    _hip.check(rc, "wiski_potrf")
    return info


def potrf_inverse_(A, info=None):
    """In-place lower Cholesky AND the explicit inverse of the factor (``wiski_potrf_inverse``: two launches for n <= 480).
    Returns (Linv, info)."""
    assert A.dim() == 2 and A.shape[0] == A.shape[1] and A.is_contiguous()
    if info is None:
        info = torch.zeros(1, dtype=torch.int32, device=A.device)
    X = torch.empty_like(A)
    rc = _hip.fn("wiski_potrf_inverse", A.dtype)(ctypes.c_int32(A.shape[0]), _hip.dptr(A), ctypes.c_int32(A.shape[1]), _hip.dptr(X),
                                                 ctypes.c_int32(X.shape[1]), _hip.dptr(info), _hip.stream_ptr(A.device))
    _hip.check(rc, "wiski_potrf_inverse")
    return X, info


def psd_safe_cholesky(A, jitter=None, max_tries=6):
    """Cholesky with gpytorch's jitter escalation (psd_safe_cholesky; imported by the
    reference at updated_root_lazy_tensor.py:5): try plain, then add jitter*10^i."""
    if jitter is None:
        jitter = 1e-6 if A.dtype == torch.float32 else 1e-8
    for i in range(max_tries + 1):
        L = A.clone()
        if i > 0:
            L.diagonal().add_(jitter * (10 ** (i - 1)))
        if int(potrf_(L).item()) == 0 and bool(torch.isfinite(L.diagonal()).all()):
            return L
    raise RuntimeError(f"Matrix not positive definite after repeatedly adding jitter up to {jitter * 10 ** (max_tries - 1):.1e}.")


def trsm_(L, B, trans=False):
    """In-place B <- L^-1 B (trans=False) or L^-T B (trans=True); B is [n, nrhs]."""
    assert B.dim() == 2 and B.is_contiguous() and L.is_contiguous() and L.shape[0] == B.shape[0]
    rc = _hip.fn("wiski_trsm", L.dtype)(ctypes.c_int32(int(trans)), ctypes.c_int32(L.shape[0]), ctypes.c_int32(B.shape[1]), _hip.dptr(L),
                                        ctypes.c_int32(L.shape[1]), _hip.dptr(B), ctypes.c_int32(B.shape[1]), _hip.stream_ptr(L.device))
    _hip.check(rc, "wiski_trsm")
    return B


def root_update_(L, R, V):
    """In-place rank-q update of a root / inverse-root pair (a6, URLT:69-119; wiski_root_update): on entry L L^T = A and
    R^T L = I, on return L L^T = A + V V^T and R^T L = I.  L, R [m, r], V [m, q], all contiguous."""
    assert L.dim() == 2 and R.shape == L.shape and V.dim() == 2 and V.shape[0] == L.shape[0]
    assert L.is_contiguous() and R.is_contiguous()
    V = V.contiguous()
    m, r = L.shape
    q = V.shape[1]
    n = int(_hip.lib().wiski_root_update_workspace_elems(ctypes.c_int32(m), ctypes.c_int32(r), ctypes.c_int32(q)))
    ws = torch.empty(n, dtype=L.dtype, device=L.device)
    rc = _hip.fn("wiski_root_update", L.dtype)(ctypes.c_int32(m), ctypes.c_int32(r), ctypes.c_int32(q), _hip.dptr(L), ctypes.c_int32(r), _hip.dptr(R),
                                               ctypes.c_int32(r), _hip.dptr(V), ctypes.c_int32(q), _hip.dptr(ws), ctypes.c_int64(n),
                                               _hip.stream_ptr(L.device))
    _hip.check(rc, "wiski_root_update")
    return L, R


def dense_factor(grid, A_half, eigen, kscale):
    """The dense regime's posterior factor in one C call (``wiski_dense_factor``): returns (M = (Kt^-1 + A)^-1 [m, m], C with
    I + sym(G A G) = C C^T, logdet(I + Kt A) as a 0-dim fp64 tensor, info int32[1] -- non-zero on a non-positive pivot)."""
    evec, evals = eigen[0], eigen[1]
    assert len(eigen) == 2 and is_half_stencil(grid, A_half)
    m, dt, dev = grid.m, A_half.dtype, A_half.device
    work = torch.empty(4 * m * m, dtype=dt, device=dev)
    chol = torch.empty((m, m), dtype=dt, device=dev)
    M = torch.empty((m, m), dtype=dt, device=dev)
    ld = torch.zeros(1, dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _hip.fn("wiski_dense_factor", dt)(grid.ref, _hip.dptr(A_half), _hip.dptr(evec.contiguous()), _hip.dptr(evals.contiguous()), _hip.creal(dt)(kscale),
                                           _hip.dptr(work), ctypes.c_int64(work.numel()), _hip.dptr(chol), _hip.dptr(M), _hip.dptr(ld), _hip.dptr(info),
                                           _hip.stream_ptr(dev))
    _hip.check(rc, "wiski_dense_factor")
    return M, chol, 2.0 * ld[0], info


def chol_logdet(L):
    out = torch.zeros(1, dtype=torch.float64, device=L.device)
    rc = _hip.fn("wiski_logdiag", L.dtype)(ctypes.c_int32(L.shape[0]), _hip.dptr(L), ctypes.c_int32(L.shape[1]), _hip.dptr(out),
                                           _hip.stream_ptr(L.device))
    _hip.check(rc, "wiski_logdiag")
    return 2.0 * out[0]


# ------------------------------------------------- reduced Kronecker-eigenbasis factor --
def basis_project(grid, x, V, kmax, S, scale=None, colscale=None, tcol=None, want_prior=False, err=None):
    """F = diag(scale) (W(x) B) diag(colscale), fp64 [n, r], for the tensor-product basis b_j = kron_q V_q[:, S[q, j]]
    (``wiski_basis_project``).  V: fp64 per-dim tables [g_q, kmax] concatenated; S int32 [d, r].  With `want_prior`
    also returns the prior variances w_p^T Kuu w_p (needs the fp64 Toeplitz columns `tcol`)."""
    x2 = _x2d(x, grid)
    n, r = x2.shape[0], S.shape[1]
    F = torch.empty((n, r), dtype=torch.float64, device=x2.device)
    prior = torch.empty(n, dtype=torch.float64, device=x2.device) if want_prior else None
    rc = _hip.fn("wiski_basis_project", x2.dtype)(grid.ref, _hip.dptr(x2), ctypes.c_int64(n), _hip.dptr(V), ctypes.c_int32(kmax), _hip.dptr(S),
                                                  ctypes.c_int32(r), _hip.dptr(scale), _hip.dptr(colscale), _hip.dptr(tcol), _hip.dptr(F),
                                                  ctypes.c_int64(r), _hip.dptr(prior), _hip.dptr(err), _hip.stream_ptr(x2.device))
    _hip.check(rc, "wiski_basis_project")
    return (F, prior) if want_prior else F


def basis_project_vjp(grid, x, V, kmax, S, GF, Gprior=None, scale=None, colscale=None, tcol=None):
    """Input gradient of :func:`basis_project` through F (upstream GF [n, r] fp64) and, with `Gprior` [n] (fp64; needs `tcol`), the
    prior variances: [n, d] in x's dtype (``wiski_basis_project_vjp``; `scale` is a constant)."""
    x2 = _x2d(x, grid)
    n, r = x2.shape[0], S.shape[1]
    GF = GF.to(torch.float64).contiguous()
    assert GF.shape == (n, r)
    Gprior = None if Gprior is None else Gprior.to(torch.float64).contiguous()
    gx = torch.empty((n, grid.d), dtype=x2.dtype, device=x2.device)
    rc = _hip.fn("wiski_basis_project_vjp", x2.dtype)(grid.ref, _hip.dptr(x2), ctypes.c_int64(n), _hip.dptr(V), ctypes.c_int32(kmax), _hip.dptr(S),
                                                      ctypes.c_int32(r), _hip.dptr(scale), _hip.dptr(colscale), _hip.dptr(tcol), _hip.dptr(GF),
                                                      ctypes.c_int64(r), _hip.dptr(Gprior), _hip.dptr(gx), _hip.stream_ptr(x2.device))
    _hip.check(rc, "wiski_basis_project_vjp")
    return gx


class BasisProject(torch.autograd.Function):
    """(F, prior) of :func:`basis_project` with ``want_prior``, differentiable w.r.t. the inputs x (wiski_basis_project_vjp, both
    outputs in one launch); the tables, index set and scales are constants."""

    @staticmethod
    def forward(ctx, grid, x, V, kmax, S, colscale, tcol, err):
        xd = x.detach().contiguous()
        ctx.args = (grid, V, kmax, S, colscale, tcol)
        ctx.save_for_backward(xd)
        F, prior = basis_project(grid, xd, V, kmax, S, colscale=colscale, tcol=tcol, want_prior=True, err=err)
        return F, prior

    @staticmethod
    def backward(ctx, gF, gprior):
        (xd,) = ctx.saved_tensors
        grid, V, kmax, S, colscale, tcol = ctx.args
        if gF is None:
            gF = torch.zeros((xd.shape[0], S.shape[1]), dtype=torch.float64, device=xd.device)
        gx = basis_project_vjp(grid, xd, V, kmax, S, gF, gprior, colscale=colscale, tcol=tcol)
        return None, gx, None, None, None, None, None, None


def stationary_columns(grid, kind, ell, scale):
    """``wiski_stationary_columns``: fp64 Toeplitz columns [sum g] of S * k(lag / ell) (kind 0 RBF, 1-3 Matern 1/2, 3/2, 5/2);
    ell [1] or [d] and scale [1] / None are device tensors of one dtype (fp32 / fp64) -- no host read."""
    out = torch.empty(sum(grid.g), dtype=torch.float64, device=ell.device)
    rc = _hip.fn("wiski_stationary_columns", ell.dtype)(grid.ref, ctypes.c_int32(kind), _hip.dptr(ell), ctypes.c_int32(ell.numel()),
                                                        None if scale is None else _hip.dptr(scale), _hip.dptr(out), _hip.stream_ptr(ell.device))
    _hip.check(rc, "wiski_stationary_columns")
    return out


def stationary_columns_grad(grid, kind, ell, scale, gout):
    g_ell = torch.empty_like(ell)
    g_scale = None if scale is None else torch.empty_like(scale)
    rc = _hip.fn("wiski_stationary_columns_grad", ell.dtype)(grid.ref, ctypes.c_int32(kind), _hip.dptr(ell), ctypes.c_int32(ell.numel()),
                                                             None if scale is None else _hip.dptr(scale), _hip.dptr(gout),
                                                             _hip.dptr(g_ell), None if g_scale is None else _hip.dptr(g_scale),
                                                             _hip.stream_ptr(ell.device))
    _hip.check(rc, "wiski_stationary_columns_grad")
    return g_ell, g_scale


def hyper_columns(plan, grid, kind, ell, scale, s2, s2_f64=None, tcol64=None, tcol=None):
    """``wiski_hyper_columns``: constrained values (ell, scale, s2: pre-allocated, parameter dtype) of the plan's raw parameters and, with
    `tcol64`, the Toeplitz columns (fp64 and, with `tcol`, the parameter dtype) -- one launch, no host read."""
    rc = _hip.fn("wiski_hyper_columns", ell.dtype)(ctypes.byref(plan), grid.ref, ctypes.c_int32(kind), _hip.dptr(ell), _hip.dptr(scale), _hip.dptr(s2),
                                                   _hip.dptr(s2_f64), _hip.dptr(tcol64), _hip.dptr(tcol), _hip.stream_ptr(ell.device))
    _hip.check(rc, "wiski_hyper_columns")


def hyper_mid(bMb, logdet, s2, c, ld, n_dev, out, loss_out=None):
    """``wiski_hyper_mid``: out [9] fp64 = {val, coef0..2, g = -1/n, g coef0, g coef1, loss, 1/s2}."""
    rc = _hip.fn("wiski_hyper_mid", s2.dtype)(_hip.dptr(bMb), None if logdet is None else _hip.dptr(logdet), _hip.dptr(s2), _hip.dptr(c), _hip.dptr(ld),
                                              _hip.dptr(n_dev), _hip.dptr(out), _hip.dptr(loss_out), _hip.stream_ptr(s2.device))
    _hip.check(rc, "wiski_hyper_mid")


def hyper_adam(plan, scale, s2, g_ell, g_scale, mid, g_kap, n_dev, lr, beta1, beta2, eps):
    """``wiski_hyper_adam``: chain rule to the raw parameters + torch.optim.Adam's update of the plan's parameters, in place."""
    rc = _hip.fn("wiski_hyper_adam", s2.dtype)(ctypes.byref(plan), _hip.dptr(scale), _hip.dptr(s2), _hip.dptr(g_ell), _hip.dptr(g_scale), _hip.dptr(mid),
                                               _hip.dptr(g_kap), _hip.dptr(n_dev), ctypes.c_double(lr), ctypes.c_double(beta1), ctypes.c_double(beta2),
                                               ctypes.c_double(eps), _hip.stream_ptr(s2.device))
    _hip.check(rc, "wiski_hyper_adam")


def multi_copy(pairs, scalar=None, scalar_dst=None):
    """``wiski_multi_copy_f64``: dst.copy_(src) for up to 12 (dst, src) pairs of contiguous fp64 tensors (and one scalar store) in ONE launch."""
    plan = _hip.wiski_copy_plan()
    plan.count = len(pairs)
    dev = None
    for i, (dst, src) in enumerate(pairs):
        if dst.dtype != torch.float64 or src.dtype != torch.float64 or dst.numel() != src.numel() or not dst.is_contiguous() or not src.is_contiguous():
            raise _hip.WiskiError("multi_copy: contiguous fp64 tensors of equal size")
        plan.src[i], plan.dst[i], plan.n[i] = src.data_ptr(), dst.data_ptr(), dst.numel()
        dev = dst.device
    if scalar_dst is not None:
        plan.scalar, plan.scalar_dst = float(scalar), scalar_dst.data_ptr()
        dev = scalar_dst.device
    rc = _hip.lib().wiski_multi_copy_f64(ctypes.byref(plan), _hip.stream_ptr(dev))
    _hip.check(rc, "wiski_multi_copy_f64")


def mll_value(bMb, logdet, s2, c, ld, n):
    """``wiski_mll_value``: (val, coef [3]) fp64 device scalars of one output's Woodbury MLL tail; s2 a 1-element tensor (fp32 / fp64)."""
    val = torch.empty((), dtype=torch.float64, device=bMb.device)
    coef = torch.empty(3, dtype=torch.float64, device=bMb.device)
    nd = torch.is_tensor(n)                          # the count as a device scalar (fp64): calls recorded into a captured graph
    rc = _hip.fn("wiski_mll_value", s2.dtype)(_hip.dptr(bMb), None if logdet is None else _hip.dptr(logdet), _hip.dptr(s2), _hip.dptr(c), _hip.dptr(ld),
                                              ctypes.c_double(0.0 if nd else float(n)), _hip.dptr(n) if nd else None, _hip.dptr(val), _hip.dptr(coef),
                                              _hip.stream_ptr(bMb.device))
    _hip.check(rc, "wiski_mll_value")
    return val, coef


def mll_s2_grad(g, coef, s2, n, g_kap):
    out = torch.empty_like(s2)
    nd = torch.is_tensor(n)
    rc = _hip.fn("wiski_mll_s2_grad", s2.dtype)(_hip.dptr(g), _hip.dptr(coef), _hip.dptr(s2), ctypes.c_double(0.0 if nd else float(n)),
                                                _hip.dptr(n) if nd else None, None if g_kap is None else _hip.dptr(g_kap), _hip.dptr(out),
                                                _hip.stream_ptr(s2.device))
    _hip.check(rc, "wiski_mll_s2_grad")
    return out


def gaussian_metrics(mu, var, y, add_var=None):
    """``wiski_gaussian_metrics``: device tensor [rmse, mean nll] of one batch (all arguments contiguous, one dtype)."""
    out = torch.empty(2, dtype=mu.dtype, device=mu.device)
    rc = _hip.fn("wiski_gaussian_metrics", mu.dtype)(ctypes.c_int64(mu.numel()), _hip.dptr(mu), _hip.dptr(var), _hip.dptr(y),
                                                     None if add_var is None else _hip.dptr(add_var), _hip.dptr(out), _hip.stream_ptr(mu.device))
    _hip.check(rc, "wiski_gaussian_metrics")
    return out


def basis_eig_update(g_dev, tcol64, Vin, kw, kuse, ref_Vtab=None, kref=0, resid_ok=None, niter=0):
    """``wiski_basis_eig_update``: the per-dim eigenvector tables Vin ([sum g_q * kw] fp64, row-major [g_q, kw] blocks) refined for the
    Toeplitz columns tcol64, all on the device.  Returns (Vout, ev [d, kw] descending, resid [d]).  resid_ok: the adaptive form
    (``wiski_basis_eig_update_adaptive``): Rayleigh-Ritz in the previous span first, subspace iteration only if the residual exceeds it."""
    d = g_dev.shape[0]
    Vout = torch.empty_like(Vin)
    ev = torch.empty((d, kw), dtype=torch.float64, device=Vin.device)
    resid = torch.empty(d, dtype=torch.float64, device=Vin.device)
    Tq = None if ref_Vtab is None else torch.empty((d, 32, 32), dtype=torch.float64, device=Vin.device)
    args = [ctypes.c_int32(d), _hip.dptr(g_dev), _hip.dptr(tcol64), _hip.dptr(Vin), ctypes.c_int32(kw), ctypes.c_int32(kuse), _hip.dptr(Vout), _hip.dptr(ev),
            _hip.dptr(resid), None if ref_Vtab is None else _hip.dptr(ref_Vtab), ctypes.c_int32(kref), None if Tq is None else _hip.dptr(Tq)]
    if resid_ok is None:
        rc = _hip.lib().wiski_basis_eig_update(*args, _hip.stream_ptr(Vin.device))
    else:
        rc = _hip.lib().wiski_basis_eig_update_adaptive(*args, ctypes.c_int32(int(niter)), ctypes.c_double(float(resid_ok)), _hip.stream_ptr(Vin.device))
    _hip.check(rc, "wiski_basis_eig_update")
    return (Vout, ev, resid) if ref_Vtab is None else (Vout, ev, resid, Tq)


def basis_change(g_dev, Tq, kref, ref_S, kw, S, ev, tcol64, resid, work, verdict_pinned=None):
    """``wiski_basis_change``: (TS [r_ref, r], lam [r], verdict [3]) for a device-refreshed basis; work: r + 1 zeroed doubles.
    verdict_pinned: a pinned host tensor (fp64 [3]) the kernel writes the verdict to directly (host-mapped memory: no copy launch; read it
    after an event recorded behind this call); the returned verdict is then that tensor."""
    d, r_ref = ref_S.shape
    r = S.shape[1]
    TS = torch.empty((r_ref, r), dtype=torch.float64, device=Tq.device)
    lam = torch.empty(r, dtype=torch.float64, device=Tq.device)
    if verdict_pinned is not None:
        if not verdict_pinned.is_pinned() or verdict_pinned.dtype != torch.float64 or verdict_pinned.numel() < 3:
            raise _hip.WiskiError("basis_change: verdict_pinned must be a pinned fp64 tensor of >= 3 elements")
        verdict, vptr = verdict_pinned, ctypes.c_void_p(verdict_pinned.data_ptr())
    else:
        verdict = torch.empty(3, dtype=torch.float64, device=Tq.device)
        vptr = _hip.dptr(verdict)
    rc = _hip.lib().wiski_basis_change(ctypes.c_int32(d), _hip.dptr(g_dev), ctypes.c_int32(kref), ctypes.c_int32(kw), ctypes.c_int32(r_ref),
                                       ctypes.c_int32(r), _hip.dptr(Tq), _hip.dptr(ref_S), _hip.dptr(S), _hip.dptr(ev),
                                       _hip.dptr(tcol64), _hip.dptr(resid), _hip.dptr(TS), _hip.dptr(lam), _hip.dptr(work), vptr,
                                       _hip.stream_ptr(Tq.device))
    _hip.check(rc, "wiski_basis_change")
    return TS, lam, verdict


_REFRESH_LAYOUT = {}


def factor_refresh(g_dev, tcol64, Vin, kw, kuse, ref_Vtab, kref, ref_S, S, work, verdict_pinned, G_ref, h_ref, kscale, info, resid_ok=None, verdict_event=None):
    """``wiski_factor_refresh``: the spectral factor's whole refresh after a hyper-parameter step -- eigenvector update, change of basis
    (+ verdict into pinned memory), G = T^T G_ref T, C, Cholesky + inverse, the tail products -- queued by ONE call into ONE packed buffer.
    verdict_event: a torch.cuda.Event that has been recorded at least once (its handle exists); the call records it behind the change of basis.
    Returns a dict of views: Vtab, ev [d, kw], TS, lam_kuu, G, chol, sqG, lam, sq, Linv and factor_tail's seven outputs."""
    d, r_ref = ref_S.shape
    r = S.shape[1]
    nV = Vin.numel()
    key = (d, nV, kw, r_ref, r)
    off = _REFRESH_LAYOUT.get(key)
    if off is None:
        buf = (ctypes.c_int64 * 15)()
        _hip.check(_hip.lib().wiski_factor_refresh_layout(ctypes.c_int32(d), ctypes.c_int64(nV), ctypes.c_int32(kw), ctypes.c_int32(r_ref), ctypes.c_int32(r), buf),
                   "wiski_factor_refresh_layout")
        off = _REFRESH_LAYOUT[key] = [int(v) for v in buf]
    out = torch.empty(off[14], dtype=torch.float64, device=Vin.device)
    niter, rok = (0, float(resid_ok)) if resid_ok is not None else (2, 1e300)
    rc = _hip.lib().wiski_factor_refresh(ctypes.c_int32(d), _hip.dptr(g_dev), ctypes.c_int64(nV), _hip.dptr(tcol64), _hip.dptr(Vin), ctypes.c_int32(kw),
                                         ctypes.c_int32(kuse), _hip.dptr(ref_Vtab), ctypes.c_int32(kref), ctypes.c_int32(niter), ctypes.c_double(rok),
                                         _hip.dptr(ref_S), _hip.dptr(S), ctypes.c_int32(r_ref), ctypes.c_int32(r), _hip.dptr(work),
                                         ctypes.c_void_p(verdict_pinned.data_ptr()), _hip.dptr(G_ref), _hip.dptr(h_ref), ctypes.c_double(float(kscale)),
                                         _hip.dptr(info), _hip.dptr(out), None if verdict_event is None else ctypes.c_void_p(verdict_event.cuda_event),
                                         _hip.stream_ptr(Vin.device))
    _hip.check(rc, "wiski_factor_refresh")
    t = out[off[13]:off[13] + 6 * r + 2]
    return {"Vtab": out[off[0]:off[0] + nV], "ev": out[off[1]:off[1] + d * kw].view(d, kw), "TS": out[off[4]:off[4] + r_ref * r].view(r_ref, r),
            "lam_kuu": out[off[5]:off[5] + r], "G": out[off[7]:off[7] + r * r].view(r, r), "chol": out[off[8]:off[8] + r * r].view(r, r),
            "sqG": out[off[9]:off[9] + r * r].view(r, r), "lam": out[off[10]:off[10] + r], "sq": out[off[11]:off[11] + r],
            "Linv": out[off[12]:off[12] + r * r].view(r, r),
            "tail": (t[:r], t[r:2 * r], t[2 * r:3 * r], t[3 * r:4 * r], t[4 * r:5 * r], t[5 * r], t[5 * r + 1])}


def factor_tail(TS, h_ref, sq, Linv, chol):
    """``wiski_factor_tail``: (hr, c_half, t, coef, zeta, bMb, logdet) -- views of one packed fp64 tensor -- in three launches."""
    r_ref, r = TS.shape
    out = torch.empty(6 * r + 2, dtype=torch.float64, device=TS.device)
    rc = _hip.lib().wiski_factor_tail(ctypes.c_int32(r_ref), ctypes.c_int32(r), _hip.dptr(TS), _hip.dptr(h_ref), _hip.dptr(sq), _hip.dptr(Linv),
                                      _hip.dptr(chol), _hip.dptr(out), _hip.stream_ptr(TS.device))
    _hip.check(rc, "wiski_factor_tail")
    return out[:r], out[r:2 * r], out[2 * r:3 * r], out[3 * r:4 * r], out[4 * r:5 * r], out[5 * r], out[5 * r + 1]


def woodbury_c(G, lam_kuu, kscale):
    """``wiski_woodbury_c``: (C = I + Lam^1/2 G Lam^1/2, lam = lam_kuu * kscale, sqrt(lam), Lam^1/2 G) in one launch."""
    r = G.shape[0]
    C = torch.empty_like(G)
    sqG = torch.empty_like(G)
    lam = torch.empty(r, dtype=torch.float64, device=G.device)
    sq = torch.empty(r, dtype=torch.float64, device=G.device)
    rc = _hip.lib().wiski_woodbury_c(ctypes.c_int32(r), _hip.dptr(G), _hip.dptr(lam_kuu), ctypes.c_double(float(kscale)), _hip.dptr(C), _hip.dptr(lam),
                                     _hip.dptr(sq), _hip.dptr(sqG), _hip.stream_ptr(G.device))
    _hip.check(rc, "wiski_woodbury_c")
    return C, lam, sq, sqG


def mll_weights(G, P, zeta, lam_kuu, g_b, g_ld):
    """``wiski_mll_weights``: (Wt = g_ld (G - P) + g_b zeta zeta^T, g_kap = sum_i Wt_ii lam_kuu_i); g_b, g_ld fp64 device scalars."""
    r = G.shape[0]
    Wt = torch.empty_like(G)
    g_kap = torch.empty((), dtype=torch.float64, device=G.device)
    rc = _hip.lib().wiski_mll_weights(ctypes.c_int32(r), _hip.dptr(G), _hip.dptr(P), _hip.dptr(zeta), _hip.dptr(lam_kuu), _hip.dptr(g_b), _hip.dptr(g_ld),
                                      _hip.dptr(Wt), _hip.dptr(g_kap), _hip.stream_ptr(G.device))
    _hip.check(rc, "wiski_mll_weights")
    return Wt, g_kap


def basis_lag_grad(g_dev, Vtab, kw, D, scale):
    """``wiski_basis_lag_grad``: [sum g] fp64 gradient w.r.t. the Toeplitz columns from the pair-reduced weights D [d, kw, kw]."""
    out = torch.empty(Vtab.shape[0] // kw, dtype=torch.float64, device=Vtab.device)
    on_dev = torch.is_tensor(scale)                  # a device scalar (fp64): calls recorded into a captured graph
    rc = _hip.lib().wiski_basis_lag_grad(ctypes.c_int32(g_dev.shape[0]), _hip.dptr(g_dev), ctypes.c_int32(kw), _hip.dptr(Vtab), _hip.dptr(D.contiguous()),
                                         ctypes.c_double(0.0 if on_dev else float(scale)), _hip.dptr(scale) if on_dev else None, _hip.dptr(out),
                                         _hip.stream_ptr(Vtab.device))
    _hip.check(rc, "wiski_basis_lag_grad")
    return out


def spectral_var(Y, F, prior, kscale):
    """``wiski_spectral_var``: (|Y[:, j]|^2, max(prior_j * kscale - |F[j]|^2, 0)) for Y [r, n], F [n, r] (fp64, contiguous)."""
    r, n = Y.shape
    diag = torch.empty(n, dtype=torch.float64, device=Y.device)
    tail = torch.empty(n, dtype=torch.float64, device=Y.device)
    if n == 0:
        return diag, tail
    rc = _hip.lib().wiski_spectral_var(ctypes.c_int32(n), ctypes.c_int32(r), _hip.dptr(Y), _hip.dptr(F), _hip.dptr(prior), ctypes.c_double(float(kscale)),
                                       _hip.dptr(diag), _hip.dptr(tail), _hip.stream_ptr(Y.device))
    _hip.check(rc, "wiski_spectral_var")
    return diag, tail


def spectral_evaluate(F, prior, Linv, t, kscale, s2, y, err, ws, want_moments=False):
    """``wiski_spectral_evaluate``: rmse / nll / out-of-grid flag / max |mean| (fp64 [4], on the device) of a query batch from the spectral
    factor: ONE launch for n <= 64 (and r <= 1024), else the MFMA GEMM chol^-1 F^T + one launch (``wiski_spectral_evaluate_y``); with
    `want_moments` also (mean, latent variance) in y's dtype.  ws: 200 zeroed doubles, reused."""
    n, r = F.shape
    out = torch.empty(4, dtype=torch.float64, device=F.device)
    mean = torch.empty(n, dtype=y.dtype, device=F.device) if want_moments else None
    var = torch.empty(n, dtype=y.dtype, device=F.device) if want_moments else None
    if n <= 64 and r <= 1024:
        rc = _hip.fn("wiski_spectral_evaluate", y.dtype)(ctypes.c_int32(n), ctypes.c_int32(r), _hip.dptr(F), _hip.dptr(prior), _hip.dptr(Linv),
                                                         ctypes.c_int32(Linv.shape[1]), _hip.dptr(t), ctypes.c_double(float(kscale)), _hip.dptr(s2), _hip.dptr(y),
                                                         _hip.dptr(err), _hip.dptr(ws), _hip.dptr(out), _hip.dptr(mean), _hip.dptr(var),
                                                         _hip.stream_ptr(F.device))
    else:
        Y = gemm(Linv, F, tb=True)                                                   # chol^-1 F^T  [r, n]
        rc = _hip.fn("wiski_spectral_evaluate_y", y.dtype)(ctypes.c_int32(n), ctypes.c_int32(r), _hip.dptr(Y), _hip.dptr(F), _hip.dptr(prior), _hip.dptr(t),
                                                           ctypes.c_double(float(kscale)), _hip.dptr(s2), _hip.dptr(y), _hip.dptr(err), _hip.dptr(ws),
                                                           _hip.dptr(out), _hip.dptr(mean), _hip.dptr(var), _hip.stream_ptr(F.device))
    _hip.check(rc, "wiski_spectral_evaluate")
    return (out, mean, var) if want_moments else out


def basis_pair_reduce(Wt, S, ev, kmax):
    """D [d, kmax, kmax] of ``wiski_basis_pair_reduce`` (Wt [r, r] fp64, S int32 [d, r], ev fp64 [d, kmax])."""
    d, r = S.shape
    D = torch.zeros((d, kmax, kmax), dtype=torch.float64, device=Wt.device)
    rc = _hip.lib().wiski_basis_pair_reduce(ctypes.c_int32(d), ctypes.c_int32(r), ctypes.c_int32(kmax), _hip.dptr(Wt.contiguous()), _hip.dptr(S),
                                            _hip.dptr(ev), _hip.dptr(D), _hip.stream_ptr(Wt.device))
    _hip.check(rc, "wiski_basis_pair_reduce")
    return D
