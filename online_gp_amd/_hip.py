"""ctypes binding of libwiski_hip.so (C ABI declared in include/wiski.h).

The library is built in-tree by :func:`build` (``hipcc --offload-arch=gfx950``);
there is no CPU fallback: every op raises if the extension is missing or if a
tensor is not a contiguous ROCm tensor.
"""
import ctypes
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_SO = os.path.join(_CSRC, "libwiski_hip.so")
_SOURCES = ["interp_gather.hip", "scatter_stats.hip", "solve.hip", "spectral.hip", "dense.hip", "collective.hip", "stream_step.hip", "spectral_basis.hip", "hyper_columns.hip", "two_level.hip", "hyper_step.hip", "lookahead.hip", "sample_paths.hip", "decay_stats.hip", "regrid_stats.hip", "trend.hip", "pack_stats.hip"]
_HEADERS = ["wiski_common.h", "spmv_sym_dma.h", "spmv_sym_dma_mc.h", "spmm_sym_cols.h", "spmm_sym_bcast.h", "scatter_half.h", "scatter_owner.h", "scatter_grad.h", "scatter_site.h", "scatter_robust.h", "scatter_window.h", "scatter_interval.h", "scatter_count.h", "scatter_hetero.h", "scatter_label.h", "scatter_input_noise.h", "scatter_grad_interval.h", "scatter_revisit.h", "absorb.h", "dense_small.h", "dense_coop.h",
            os.path.join("..", "..", "include", "wiski.h")]
MAX_DIM = 4

_lib = None


class WiskiError(RuntimeError):
    pass


_ERRS = {-1: "WISKI_E_BADARG", -2: "WISKI_E_LAUNCH", -3: "WISKI_E_WORKSPACE", -4: "WISKI_E_NOTCONV"}


class wiski_grid(ctypes.Structure):
    _fields_ = [
        ("d", ctypes.c_int32),
        ("g", ctypes.c_int32 * MAX_DIM),
        ("g0", ctypes.c_double * MAX_DIM),
        ("h", ctypes.c_double * MAX_DIM),
    ]


HYPER_MAX_PARAMS = 6


class wiski_hyper_param(ctypes.Structure):
    _fields_ = [
        ("raw", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p), ("step", ctypes.c_void_p),
        ("numel", ctypes.c_int32), ("step_numel", ctypes.c_int32), ("role", ctypes.c_int32), ("kind", ctypes.c_int32),
        ("lower", ctypes.c_double), ("upper", ctypes.c_double),
    ]


class wiski_hyper_plan(ctypes.Structure):
    _fields_ = [("count", ctypes.c_int32), ("reserved", ctypes.c_int32), ("p", wiski_hyper_param * HYPER_MAX_PARAMS)]


COPY_MAX_SEGMENTS = 12


class wiski_copy_plan(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p * COPY_MAX_SEGMENTS), ("dst", ctypes.c_void_p * COPY_MAX_SEGMENTS), ("n", ctypes.c_int64 * COPY_MAX_SEGMENTS),
                ("count", ctypes.c_int32), ("reserved", ctypes.c_int32), ("scalar", ctypes.c_double), ("scalar_dst", ctypes.c_void_p)]


DECAY_MAX_REGIONS = 8
DECAY_MAX_OUTPUTS = 8


class wiski_decay_plan(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p * DECAY_MAX_REGIONS), ("n", ctypes.c_int64 * DECAY_MAX_REGIONS), ("factor", ctypes.c_double * DECAY_MAX_REGIONS),
                ("count", ctypes.c_int32), ("reserved", ctypes.c_int32)]


REGRID_MAX_REGIONS = 16
REGRID_MAX_REPORTS = 8


class wiski_regrid_plan(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p * REGRID_MAX_REGIONS), ("dst", ctypes.c_void_p * REGRID_MAX_REGIONS), ("k", ctypes.c_int64 * REGRID_MAX_REGIONS),
                ("r0", ctypes.c_int64 * REGRID_MAX_REGIONS), ("w", ctypes.c_int32 * REGRID_MAX_REGIONS), ("report", ctypes.c_int32 * REGRID_MAX_REGIONS),
                ("count", ctypes.c_int32), ("reserved", ctypes.c_int32)]


STATS_MAX_REGIONS = 16


class wiski_stats_plan(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p * STATS_MAX_REGIONS), ("dst", ctypes.c_void_p * STATS_MAX_REGIONS), ("k", ctypes.c_int64 * STATS_MAX_REGIONS),
                ("w", ctypes.c_int64 * STATS_MAX_REGIONS), ("factor", ctypes.c_double * STATS_MAX_REGIONS), ("count", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class wiski_absorb_args(ctypes.Structure):
    """The absorb's full argument record (include/wiski.h); a zeroed one with the points, d_b, d_stats, d_err and nout = 1 is the plain absorb."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("d_x", "d_y", "d_wa", "d_wb", "d_noise")] + [("n", ctypes.c_int64)] + [
        ("d_b", ctypes.c_void_p), ("d_A", ctypes.c_void_p), ("half", ctypes.c_int32), ("channels", ctypes.c_int32), ("d_cnt", ctypes.c_void_p),
        ("d_stats", ctypes.c_void_p), ("d_err", ctypes.c_void_p), ("d_u", ctypes.c_void_p), ("d_res", ctypes.c_void_p), ("d_mean_out", ctypes.c_void_p),
        ("z1", ctypes.c_void_p), ("n1_bytes", ctypes.c_int64), ("z2", ctypes.c_void_p), ("n2_bytes", ctypes.c_int64),
        ("d_guard", ctypes.c_void_p), ("guard_expect", ctypes.c_int64), ("d_bin", ctypes.c_void_p), ("bin_bytes", ctypes.c_int64),
        ("g_lo", ctypes.c_int32), ("g_hi", ctypes.c_int32), ("nout", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("y_stride", ctypes.c_int64), ("w_stride", ctypes.c_int64), ("A_stride", ctypes.c_int64)]


class wiski_window_ring(ctypes.Structure):
    """The device-resident ring of a sliding-window absorb (include/wiski.h): five arrays of `cap` slots and the host-kept head."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("d_x", "d_y", "d_wa", "d_wb", "d_noise")] + [("cap", ctypes.c_int64), ("head", ctypes.c_int64)]


class wiski_site_ring(ctypes.Structure):
    """The device-resident ring of stored sites (include/wiski.h): nine arrays of `cap` slots."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("d_x", "d_d0", "d_d1", "d_noise", "d_wa", "d_wb", "d_ytilde", "d_omega", "d_form")] + [("cap", ctypes.c_int64)]


def _absorb_signatures():
    """argtypes of every entry of the absorb's observation forms (include/wiski.h), by name: pointers as c_void_p, in the order of
    the prototypes.  A form's entry is (grid, record, the form's own arguments, stream) and only the own arguments are spelt out
    here; "real" is the one scalar in the working precision (c_float / c_double by suffix).  The site-only entries take neither
    grid nor record.  lib() sets them all, so that a call with a wrong argument count or kind fails in ctypes, and
    tests/test_host.py holds the table against the header."""
    p, f64, i32, i64, cint = ctypes.c_void_p, ctypes.c_double, ctypes.c_int32, ctypes.c_int64, ctypes.c_int
    own = {
        "wiski_absorb": [],
        "wiski_absorb_robust": [p, "real", p],
        "wiski_absorb_window": [ctypes.POINTER(wiski_window_ring), p],
        "wiski_absorb_interval": [p, p, p, f64, p, p, p],
        "wiski_absorb_grad_interval": [p, p, p, f64, p, p, p],
        "wiski_absorb_count": [p, p, cint, p, f64, p, p, p],
        "wiski_absorb_revisit": [ctypes.POINTER(wiski_site_ring), cint, p, f64, f64, p, p],
        "wiski_absorb_hetero": [p, p, f64, f64] + [p] * 11,
        "wiski_absorb_label": [p, p, ctypes.POINTER(f64), p, p, p],
        "wiski_absorb_input_noise": [p, p, p, f64, p, p, p],
        "wiski_count_sites": [p] * 4 + [cint, i64] + [p] * 3,
        "wiski_hetero_sites": [p] * 4 + [i64] + [p] * 3,
        "wiski_label_sites": [p] * 4 + [i32, i64] + [p] * 3,
        "wiski_label_proba": [p] * 3 + [i32, i64, p],
    }
    record = [ctypes.POINTER(wiski_grid), ctypes.POINTER(wiski_absorb_args)]
    return {name + suf: (record if name.startswith("wiski_absorb") else []) + [real if t == "real" else t for t in args] + [p]
            for name, args in own.items() for suf, real in (("_f32", ctypes.c_float), ("_f64", f64))}


ABSORB_SIGNATURES = _absorb_signatures()


def sources():
    return [os.path.join(_CSRC, s) for s in _SOURCES if os.path.exists(os.path.join(_CSRC, s))]


_COMPILE_BYTES = 512 << 20     # memory budget of one hipcc -c (the largest source peaks at ~270 MB)


def _build_jobs(n):
    """Concurrent compiles: at most n, the CPUs this process may use (affinity, cgroup CPU quota), MAX_JOBS when set, and
    what the memory limit leaves room for (cgroup memory.max less what is in use, MemAvailable) at _COMPILE_BYTES each.
    os.cpu_count() alone over-subscribes a container that shows far more CPUs or memory than its limits allow."""
    cpus = os.cpu_count() or 1
    try:
        cpus = min(cpus, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            cpus = min(cpus, max(1, -(-int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    free = []
    try:
        lim = open("/sys/fs/cgroup/memory.max").read().strip()
        if lim != "max":
            free.append(int(lim) - int(open("/sys/fs/cgroup/memory.current").read()))
    except (OSError, ValueError):
        pass
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                free.append(int(line.split()[1]) * 1024)
    except (OSError, ValueError, IndexError):
        pass
    jobs = min(n, cpus)
    if free:
        jobs = min(jobs, min(free) // _COMPILE_BYTES)
    try:
        jobs = min(jobs, int(os.environ["MAX_JOBS"]))
    except (KeyError, ValueError):
        pass
    return max(1, jobs)


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 into csrc/libwiski_hip.so: one object per source (built concurrently, only when
    the source or a header is newer than its object), then one link.  Every output is written under a temporary name and
    renamed into place, so that a build cut short leaves no partial file that a later build would take for current."""
    from concurrent.futures import ThreadPoolExecutor

    srcs = sources()
    import glob

    hdrs = sorted(set([os.path.join(_CSRC, h) for h in _HEADERS] + glob.glob(os.path.join(_CSRC, "*.h"))))   # every header in csrc/ counts
    hdr_time = max(os.path.getmtime(h) for h in hdrs if os.path.exists(h))
    if not force and os.path.exists(_SO):
        deps = srcs + [h for h in hdrs if os.path.exists(h)]
        if all(os.path.getmtime(d_) <= os.path.getmtime(_SO) for d_ in deps):
            return _SO                               # the shipped library is current (the object cache need not exist)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(_HERE, "..", "build", "obj")
    os.makedirs(objdir, exist_ok=True)
    objs, todo = [], []
    tmp = ".%d.tmp" % os.getpid()                    # per process: two builds at once never write the same file
    for src in srcs:
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        objs.append(obj)
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), hdr_time):
            todo.append(([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", obj + tmp], obj))
    if not todo and os.path.exists(_SO) and all(os.path.getmtime(o) <= os.path.getmtime(_SO) for o in objs):
        return _SO

    def run(job):
        cmd, out = job
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        os.replace(cmd[cmd.index("-o") + 1], out)

    jobs = _build_jobs(len(todo)) if todo else 1
    if verbose:
        print(f"{len(todo)} HIP sources to compile, {jobs} at a time", flush=True)
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        list(ex.map(run, todo))
    run(([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", _SO + tmp] + objs + ["-ldl"], _SO))
    return _SO


def lib():
    global _lib
    if _lib is None:
        alt = os.environ.get("WISKI_HIP_SO")          # A/B testing of kernel variants (tools/ubench)
        if alt:
            _lib = ctypes.CDLL(alt)
            _lib.wiski_pcg_workspace_bytes.restype = ctypes.c_int64
            if hasattr(_lib, "wiski_root_update_workspace_elems"):
                _lib.wiski_root_update_workspace_elems.restype = ctypes.c_int64
            for name, sig in ABSORB_SIGNATURES.items():      # (a variant need not have every form; the ones it has take plain floats and ints)
                if hasattr(_lib, name):
                    getattr(_lib, name).argtypes = sig
            return _lib
        if not os.path.exists(_SO):
            raise WiskiError(
                f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). online_gp_amd has no CPU fallback."
            )
        _lib = ctypes.CDLL(_SO)
        _lib.wiski_pcg_workspace_bytes.restype = ctypes.c_int64
        _lib.wiski_twolevel_refresh_workspace_bytes.restype = ctypes.c_int64
        for name, sig in ABSORB_SIGNATURES.items():
            f = getattr(_lib, name)
            f.argtypes, f.restype = sig, ctypes.c_int
    if hasattr(_lib, "wiski_root_update_workspace_elems"):
        _lib.wiski_root_update_workspace_elems.restype = ctypes.c_int64
    return _lib


def check(rc, what):
    if rc != 0:
        raise WiskiError(f"{what} failed: {_ERRS.get(rc, rc)}")


def dptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise WiskiError("online_gp_amd ops need ROCm device tensors (no CPU fallback)")
    if not t.is_contiguous():
        raise WiskiError("online_gp_amd ops need contiguous tensors")
    return ctypes.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr(device=None):
    """The caller's current HIP stream on `device` (a torch.device, index or None = current device)."""
    cur = torch.cuda.current_device()
    if device is None:
        idx = cur
    elif isinstance(device, int):
        idx = device
    else:
        idx = torch.device(device).index
        if idx is None:
            idx = cur
    if idx != cur:
        # the library launches on the CURRENT HIP device; a stream of another device would make every launch fail (or hang a
        # convergence poll).  Fail loudly instead of guarding silently: the caller owns the device selection.
        raise RuntimeError(f"online_gp_amd: tensors live on cuda:{idx} but the current device is cuda:{cur}; "
                           f"call torch.cuda.set_device({idx}) (or use `with torch.cuda.device({idx}):`) around the model calls")
    if _raw_stream is not None:                      # ~0.3 us instead of ~3 us through torch.cuda.current_stream
        return ctypes.c_void_p(_raw_stream(idx))
    return ctypes.c_void_p(torch.cuda.current_stream(idx).cuda_stream)


_fn_cache = {}


def suffix(dtype):
    if dtype == torch.float32:
        return "_f32"
    if dtype == torch.float64:
        return "_f64"
    raise WiskiError(f"unsupported dtype {dtype}")


def creal(dtype):
    return ctypes.c_float if dtype == torch.float32 else ctypes.c_double


def fn(name, dtype):
    key = (name, dtype)
    f = _fn_cache.get(key)
    if f is None:
        f = _fn_cache[key] = getattr(lib(), name + suffix(dtype))
    return f
