"""Test helper: walk the tensors of a kernel cache (online_gp_amd/models/kernel_cache.py) -- for tests/test_kernel_cache_host.py and
tests/test_kernel_cache_gpu.py."""
import torch

from online_gp_amd import grid_ops
from online_gp_amd.models import kernel_cache as kc


def ring_tensors(ring):
    return list(ring.tensors()) + ([ring.void_left, ring.explicit] if isinstance(ring, grid_ops.WindowRing) else [])


def leaves(cache):
    """(name, tensor) of every tensor that owns values: the views response_cache and D_logdet are left out, the stencils, the root pairs
    and the rings' tensors are in."""
    for k, v in cache.items():
        if k in ("response_cache", "D_logdet", "_spectral"):
            continue
        if k == "WtW":
            for o, op in enumerate(kc._wtw_ops(v)):
                for name in ("stencil", "root", "inv_root"):
                    if getattr(op, name, None) is not None:
                        yield f"WtW[{o}].{name}", getattr(op, name)
        elif torch.is_tensor(v):
            yield k, v
        elif hasattr(v, "tensors"):
            for i, t in enumerate(ring_tensors(v)):
                yield f"{k}.{i}", t


def snapshot(cache):
    return {name: t.clone() for name, t in leaves(cache)}


def storages(cache):
    """The addresses of the storages behind the cache's tensors (of a view: its base's as well)."""
    ptrs = set()
    for _, t in leaves(cache):
        ptrs.add(t.untyped_storage().data_ptr())
        if t._base is not None:
            ptrs.add(t._base.data_ptr())
    return ptrs
