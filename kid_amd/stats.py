"""Per-level ensemble statistics on the device (include/kidmp_stats.h): the moments and histograms of [ncol, nz]
CUDA tensors over the columns, per level and per ensemble group, without a download.

The five entries of kidmp_stats.h are declared here, on the object load_library() returned, the first time one of them
is needed: include/kidmp.h and its mirror in thompson.py stay what they are.  Like every device entry there is no
fallback: without the library or the device a call raises KidmpError.
"""
import ctypes as C

import numpy as np

from . import thompson as _th
from .thompson import KidmpError

MAX_FIELDS, MAX_GROUPS, MAX_BINS, NMOM = 16, 64, 64, 5        # KIDMP_STATS_* of include/kidmp_stats.h


class _StatsRequest(C.Structure):
    """kidmp_stats_request."""
    _fields_ = [("nfield", C.c_int32), ("field", C.POINTER(C.c_void_p)), ("col_stride", C.POINTER(C.c_int64)),
                ("floor", C.POINTER(C.c_double)), ("group", C.c_void_p), ("ngroup", C.c_int32), ("nbin", C.c_int32),
                ("edges", C.c_void_p)]


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_stats.h."""
    i32, i64, size, vp, rc = C.c_int32, C.c_int64, C.c_size_t, C.c_void_p, C.c_int
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    device = [vp, i64, i32, C.POINTER(_StatsRequest), vp, vp, vp, size, vp]
    return {
        "kidmp_level_stats_device": (rc, device),
        "kidmp32_level_stats_device": (rc, device),
        "kidmp_stats_workspace_bytes": (size, [i64, i32, i32, i32, i32]),
        "kidmp_stats_chunks": (i32, [i64]),
        "kidmp_stats_merge": (rc, [i64, i32, i32, dp, lp, dp, lp]),
    }


def declare(L):
    """Declare the entries of kidmp_stats.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the statistics entries declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def stats_chunks(ncol):
    """kidmp_stats_chunks: the number of column chunks a reduction of ncol columns is cut into."""
    return int(library().kidmp_stats_chunks(int(ncol)))


def stats_workspace_bytes(ncol, nz, nfield, ngroup=1, nbin=0):
    """kidmp_stats_workspace_bytes; 0 for arguments outside their ranges and for ncol == 0."""
    return int(library().kidmp_stats_workspace_bytes(int(ncol), int(nz), int(nfield), int(ngroup), int(nbin)))


def _refuse(msg):
    raise KidmpError("level_stats: " + msg)


class LevelStats:
    """The result of level_stats: count, mean, m2, min, max [ngroup, nfield, nz] (views of mom [ngroup, nfield, 5, nz]),
    hist [ngroup, nfield, nz, nbin+3] or None, names (the order of the fields) and edges (numpy [nfield, nbin+1] or None).
    An empty cell has count 0, mean 0, m2 0, min +inf, max -inf."""

    def __init__(self, names, mom, hist, edges, keep=()):
        self.names, self.mom, self.hist, self.edges = tuple(names), mom, hist, edges
        self.count, self.mean, self.m2, self.min, self.max = (mom[:, :, r, :] for r in range(NMOM))
        self._keep = keep                      # what the enqueued launches still read: lives as long as the result

    def index(self, name):
        return self.names.index(name)

    def variance(self):
        """m2 / count (the population variance); NaN where the cell is empty."""
        return self.m2 / self.count

    def percentile(self, q):
        """The q-th percentile (0 <= q <= 100) of every cell from its histogram, linear inside the bin:
        [ngroup, nfield, nz] float64.  NaN values are not counted; a rank that falls below the first or above the last
        edge gives that edge; an empty cell gives NaN."""
        import torch
        if self.hist is None:
            raise KidmpError("percentile: level_stats was called without edges")
        if not 0.0 <= float(q) <= 100.0:
            raise KidmpError("percentile: q outside [0, 100]")
        h = self.hist[..., :-1].to(torch.float64)                              # slots 0 .. nbin+1
        nbin = h.shape[-1] - 2
        e = torch.as_tensor(self.edges, dtype=torch.float64, device=h.device)[None, :, None, :]   # [1, nfield, 1, nbin+1]
        cum = torch.cumsum(h, dim=-1)
        total = cum[..., -1:]
        rank = total * (float(q) / 100.0)
        # the first occupied slot whose cumulative count reaches the rank
        slot = torch.clamp(((cum < rank) | (cum <= 0)).sum(dim=-1, keepdim=True), max=nbin + 1)
        before = torch.gather(cum - h, -1, slot)
        inside = torch.gather(h, -1, slot)
        b = torch.clamp(slot - 1, 0, nbin - 1)
        lo, hi = torch.gather(e.expand(*h.shape[:-1], -1), -1, b), torch.gather(e.expand(*h.shape[:-1], -1), -1, b + 1)
        frac = torch.where(inside > 0, (rank - before) / torch.clamp(inside, min=1.0), torch.zeros_like(rank))
        out = lo + frac * (hi - lo)
        out = torch.where(slot == 0, e[..., :1].expand_as(out), out)
        out = torch.where(slot == nbin + 1, e[..., -1:].expand_as(out), out)
        out = torch.where(total > 0, out, torch.full_like(out, float("nan")))
        return out[..., 0]

    def merge(self, other):
        """This result with `other` folded in (kidmp_stats_merge on host copies): for shards, batches and accumulation
        over time steps.  Count, min, max and the histogram of the merged result are exact; mean and m2 are Chan's
        pairwise combination.  Returns a new LevelStats on this result's device."""
        import torch
        if (self.names != other.names or tuple(self.mom.shape) != tuple(other.mom.shape)
                or (self.hist is None) != (other.hist is None)
                or (self.hist is not None and (tuple(self.hist.shape) != tuple(other.hist.shape)
                                               or not np.array_equal(self.edges, other.edges)))):
            raise KidmpError("merge: the two results differ in fields, groups, levels or edges")
        ngroup, nfield, _, nz = self.mom.shape
        nbin = 0 if self.hist is None else self.hist.shape[-1] - 3
        mom_a = np.ascontiguousarray(self.mom.detach().cpu().numpy()).copy()
        mom_b = np.ascontiguousarray(other.mom.detach().cpu().numpy())
        hist_a = hist_b = None
        if nbin:
            hist_a = np.ascontiguousarray(self.hist.detach().cpu().numpy()).copy()
            hist_b = np.ascontiguousarray(other.hist.detach().cpu().numpy())
        dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        rc = library().kidmp_stats_merge(ngroup * nfield, nz, nbin, mom_a.ctypes.data_as(dp),
                                         hist_a.ctypes.data_as(lp) if nbin else None, mom_b.ctypes.data_as(dp),
                                         hist_b.ctypes.data_as(lp) if nbin else None)
        if rc < 0:
            raise KidmpError("kidmp error %d: %s" % (rc, library().kidmp_last_error(None).decode()))
        dev = self.mom.device
        return LevelStats(self.names, torch.from_numpy(mom_a).to(dev), torch.from_numpy(hist_a).to(dev) if nbin else None, self.edges)


def _check_fields(fields):
    """(names, tensors, dtype, ncol, nz) of the `fields` argument, judged for dtype, shape and stride."""
    import torch
    if not isinstance(fields, dict) or not 1 <= len(fields) <= MAX_FIELDS:
        _refuse("fields must be a dict of 1 to %d tensors [ncol, nz]" % MAX_FIELDS)
    names, tensors = list(fields.keys()), list(fields.values())
    for k, a in zip(names, tensors):
        if not isinstance(a, torch.Tensor):
            _refuse("fields[%r] must be a torch tensor, got %s" % (k, type(a).__name__))
    q = tensors[0]
    if q.dtype not in (torch.float64, torch.float32):
        _refuse("fields must be float64 or float32 tensors, fields[%r] is %s" % (names[0], str(q.dtype).replace("torch.", "")))
    if q.dim() != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse("fields[%r] must be [ncol, nz] with nz in [2, %d], got %s" % (names[0], _th.MAX_NZ, list(q.shape)))
    for k, a in zip(names, tensors):
        if a.dtype != q.dtype:
            _refuse("all fields must be %s, fields[%r] is %s" % (str(q.dtype).replace("torch.", ""), k, str(a.dtype).replace("torch.", "")))
        if tuple(a.shape) != tuple(q.shape):
            _refuse("all fields must be %s, fields[%r] is %s" % (list(q.shape), k, list(a.shape)))
        if a.stride(1) != 1 or (a.shape[0] > 1 and a.stride(0) < a.shape[1]):
            _refuse("fields[%r]: the levels must be contiguous and the columns at least nz apart (strides %s)" % (k, list(a.stride())))
    return names, tensors, q.dtype, int(q.shape[0]), int(q.shape[1])


def _check_edges(edges, names):
    """numpy [nfield, nbin+1] of the `edges` argument (None: no histogram)."""
    if edges is None:
        return None
    if not isinstance(edges, dict) or sorted(edges.keys(), key=str) != sorted(names, key=str):
        _refuse("edges must be a dict with an entry for every field")
    rows = []
    for k in names:
        try:
            e = np.asarray(edges[k], dtype=np.float64)
        except (TypeError, ValueError):
            _refuse("edges[%r] must be a one-dimensional array of numbers" % (k,))
        if e.ndim != 1 or not 2 <= e.size <= MAX_BINS + 1:
            _refuse("edges[%r] must be one-dimensional with 2 to %d entries (1 to %d bins)" % (k, MAX_BINS + 1, MAX_BINS))
        if not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0.0):
            _refuse("edges[%r] must be finite and strictly ascending" % (k,))
        rows.append(e)
    if len({e.size for e in rows}) != 1:
        _refuse("all edges must have the same length")
    return np.ascontiguousarray(np.stack(rows))


def level_stats(mp, fields, group=None, ngroup=1, edges=None, floor=None, work=None, stream=None):
    """Moments and histograms over the columns, per level and per ensemble group (kidmp[32]_level_stats_device).

    fields   dict name -> CUDA tensor [ncol, nz] on the context's device, all float64 or all float32 (widened on load);
             the levels contiguous, the row stride taken from the tensor: a slice rates[:, r, :] needs no copy
    group    int32 CUDA tensor [ncol] of group ids, None = every column in group 0; a column whose id is outside
             [0, ngroup) is left out of everything
    edges    dict name -> ascending 1-D array of nbin+1 bin edges, one per field, all of one length; None = no histogram
    floor    dict name -> float: only values x > floor enter that field's moments (the histogram ignores it)
    work     uint8 CUDA tensor of at least stats_workspace_bytes(...) bytes, None = made here
    Returns a LevelStats.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    names, tensors, dtype, ncol, nz = _check_fields(fields)
    if isinstance(ngroup, bool) or not isinstance(ngroup, (int, np.integer)) or not 1 <= ngroup <= MAX_GROUPS:
        _refuse("ngroup must be an integer in [1, %d]" % MAX_GROUPS)
    if group is not None:
        if not isinstance(group, torch.Tensor) or group.dtype != torch.int32 or tuple(group.shape) != (ncol,) or not group.is_contiguous():
            _refuse("group must be a contiguous int32 tensor [ncol] = [%d]" % ncol)
    host_edges = _check_edges(edges, names)
    nbin = 0 if host_edges is None else host_edges.shape[1] - 1
    host_floor = None
    if floor is not None:
        if not isinstance(floor, dict) or any(k not in fields for k in floor):
            _refuse("floor must be a dict whose keys are names of fields")
        try:
            host_floor = [float(floor.get(k, -np.inf)) for k in names]
        except (TypeError, ValueError):
            _refuse("floor values must be numbers")
    for k, a in list(zip(names, tensors)) + ([("group", group)] if group is not None else []) + ([("work", work)] if work is not None else []):
        what = "fields[%r]" % (k,) if a is not group and a is not work else k
        if not isinstance(a, torch.Tensor) or not a.is_cuda:
            _refuse("%s must be a CUDA tensor" % what)
        if a.device.index != mp.device:
            _refuse("%s lives on cuda:%d but this context is bound to cuda:%d" % (what, a.device.index, mp.device))
    L = library()
    nfield = len(names)
    need = int(L.kidmp_stats_workspace_bytes(ncol, nz, nfield, int(ngroup), nbin))
    device = tensors[0].device
    if work is None:
        work = torch.empty(max(need, 8), dtype=torch.uint8, device=device)
    elif work.dtype != torch.uint8 or not work.is_contiguous() or work.numel() < need:
        _refuse("work must be a contiguous uint8 tensor of at least %d bytes" % need)
    mom = torch.empty((int(ngroup), nfield, NMOM, nz), dtype=torch.float64, device=device)
    hist = torch.empty((int(ngroup), nfield, nz, nbin + 3), dtype=torch.int64, device=device) if nbin else None
    dev_edges = torch.from_numpy(host_edges).to(device) if nbin else None
    req = _StatsRequest()
    req.nfield = nfield
    ptrs = (C.c_void_p * nfield)(*[a.data_ptr() for a in tensors])
    strides = (C.c_int64 * nfield)(*[int(a.stride(0)) if ncol > 1 else nz for a in tensors])
    req.field = C.cast(ptrs, C.POINTER(C.c_void_p))
    req.col_stride = C.cast(strides, C.POINTER(C.c_int64))
    if host_floor is not None:
        floors = (C.c_double * nfield)(*host_floor)
        req.floor = C.cast(floors, C.POINTER(C.c_double))
    req.group = group.data_ptr() if group is not None else None
    req.ngroup, req.nbin = int(ngroup), nbin
    req.edges = dev_edges.data_ptr() if nbin else None
    fn = L.kidmp_level_stats_device if dtype == torch.float64 else L.kidmp32_level_stats_device
    rc = fn(mp._h, ncol, nz, C.byref(req), mom.data_ptr(), hist.data_ptr() if nbin else None, work.data_ptr(),
            work.numel(), _th._stream(stream, tensors[0]))
    if rc < 0:
        raise KidmpError("kidmp error %d: %s" % (rc, L.kidmp_last_error(mp._h).decode()))
    return LevelStats(names, mom, hist, host_edges, keep=(work, dev_edges, group) + tuple(tensors))
