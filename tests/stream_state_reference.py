"""Test helper: an independent restatement of the checkpoint / merge operations of DESIGN.md 3.31 in numpy, with plain loops over regions, blocks,
slots and nodes -- for tests/test_stream_state_host.py and tests/test_stream_state_gpu.py.  It shares no code with online_gp_amd.grid_ops or
online_gp_amd.models.kernel_cache.

A region is ``(a, k, w)``: a flat array of k blocks of m nodes of w reals, element (c, node i, s) at ``c m w + i w + s``.  Arithmetic is done in
the array's own dtype, one correctly rounded operation at a time, so that a kernel that does the same operations matches bit for bit."""
import math

import numpy as np


def select(m, regions):
    """Ascending int32 list of the nodes at which any element of any region is not == 0 (a NaN is not == 0)."""
    hit = np.zeros(m, dtype=bool)
    for a, k, w in regions:                               # (block by block and slot by slot; the node axis as one array)
        for c in range(k):
            for s in range(w):
                hit |= ~(a[c * m * w + s:(c + 1) * m * w:w] == 0)
    return np.asarray([i for i in range(m) if hit[i]], dtype=np.int32)


def gather(m, nodes, a, k, w):
    """compact[c n_sel w + j w + s] = a[c m w + nodes[j] w + s]"""
    src = a.reshape(k, m, w)
    out = np.zeros((k, len(nodes), w), dtype=a.dtype)
    for j, i in enumerate(nodes):
        out[:, j, :] = src[:, int(i), :]
    return out.reshape(-1)


def scatter_add(m, nodes, dst, src, k, w, f=1.0, src_full=False):
    """A copy of dst with dst[c m w + nodes[j] w + s] += f src[c n_sel w + j w + s]: f rounded once to the dtype; f == 1 a plain add, else a
    rounded product followed by a rounded add.  src_full: src is a full region, read at nodes[j] too."""
    out = dst.copy().reshape(k, m, w)
    s = src.reshape(k, m if src_full else len(nodes), w)
    f = dst.dtype.type(f)
    for j, i in enumerate(nodes):
        row = s[:, int(i) if src_full else j, :]
        if f != 1:
            row = row * f
        out[:, int(i), :] = out[:, int(i), :] + row
    return out.reshape(-1)


# the merge rule of every leaf of a kernel cache (kernel_cache_leaves.leaves names them), weight w in (0, 1]
def merge_leaf(name, mine, other, weight, n_other):
    """What the receiver's leaf `name` holds after the other side's was merged in at `weight` (n_other: points per output the other holds)."""
    key = name.split("[")[0]
    if key in ("WtW", "interpolation_cache", "_cnt", "trend_C", "trend_G", "trend_g"):
        f = mine.dtype.type(weight)
        return mine + (other if f == 1 else other * f)
    if key == "path_probes":
        f = mine.dtype.type(math.sqrt(weight))
        return mine + (other if f == 1 else other * f)
    if key == "_stats":
        out = mine.copy()
        out[:, 0] = mine[:, 0] + other[:, 0] * np.float64(weight)
        out[:, 1] = mine[:, 1] + (other[:, 1] - (0.0 if weight == 1.0 else float(n_other) * math.log(weight)))
        return out
    if key in ("trend_center", "trend_scale"):
        return mine.copy()
    raise KeyError(name)
