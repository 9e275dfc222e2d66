"""The per-level ensemble statistics on the MI355X (kidmp[32]_level_stats_device, kid_amd/csrc/kidmp_stats.hip) against
numpy and exact arithmetic on the host (tests/level_stats_ref.py, which states the rules): count, min, max and every
histogram slot exactly; the mean within 4 n 2**-53 max|x| of the fsum mean; M2 within 8 n kappa 2**-53 (relative) of the
exact M2.  A sum-of-squares formula misses the M2 bound on the shifted fields by 10**4 .. 10**6; Welford's update keeps
below a few per cent of either bound.  The tests print the worst ratios they met.

Shapes: the smallest that cross a wave (64 levels: also the level tile) and a chunk (C = kidmp_stats_chunks of a large
ensemble, read from the library): nz in {2, 65, 120, 256}, ncol in {1, C-1, C+1, 3C+7}, nbin in {0, 1, 64}, nfield in
{1, 3, 16}."""
import ctypes as C

import numpy as np
import pytest

import cases
import level_stats_ref as ref

pytestmark = pytest.mark.gpu

SEED = 20250611
NCOL_OF = {"1": lambda c: 1, "C-1": lambda c: c - 1, "C+1": lambda c: c + 1, "3C+7": lambda c: 3 * c + 7}
KINDS = ("dbz", "t", "lognormal", "shifted", "scaled")


def _chunks_of_a_large_ensemble():
    from kid_amd import stats_chunks
    return stats_chunks(10 ** 7)


def _edges_of(kind, nbin):
    if kind == "dbz":
        return np.linspace(-35.0, 60.0, nbin + 1)
    if kind == "t":
        return np.linspace(220.0, 280.0, nbin + 1)
    if kind == "lognormal":
        return np.logspace(-9.0, -2.0, nbin + 1)
    if kind == "shifted":
        return 2.0 ** 30 + np.linspace(-48.0, 48.0, nbin + 1)
    return 1.0e8 * (1.0 + 1.0e-3 * np.linspace(-3.0, 3.0, nbin + 1))


def _field_of(kind, ncol, nz, rng, nbin):
    """One [ncol, nz] field.  The dBZ-like one carries the awkward values: negative numbers, +-0, NaN, +-inf, values
    exactly on the first, an inner and the last edge, and values equal to its floor (-35, also its first edge)."""
    if kind == "t":
        return 250.0 + 10.0 * rng.standard_normal((ncol, nz))
    if kind == "lognormal":
        return np.exp(rng.normal(np.log(1.0e-5), 2.0, (ncol, nz)))
    if kind == "shifted":                                        # ill-conditioned: integers in [-50, 50] shifted by 2**30
        return rng.integers(-50, 51, (ncol, nz)).astype(np.float64) + 2.0 ** 30
    if kind == "scaled":                                         # ill-conditioned: 1e8 (1 + 1e-3 N(0, 1))
        return 1.0e8 * (1.0 + 1.0e-3 * rng.standard_normal((ncol, nz)))
    x = rng.uniform(-35.3, 60.0, (ncol, nz))
    e = _edges_of("dbz", max(nbin, 2))
    special = [np.nan, e[0], np.inf, e[len(e) // 2], -np.inf, e[-1], 0.0, -0.0, -35.0, np.nan, e[1]]
    flat = x.reshape(-1)
    for i, v in enumerate(special[: flat.size // 2 + 1]):
        flat[(i * 7919 + 1) % flat.size] = v
    return x


def _make(ncol, nz, nfield, nbin, seed=SEED, kinds=KINDS):
    """(fields, edges [nfield, nbin+1] or None, floors) of nfield fields that cycle through `kinds`."""
    rng = np.random.default_rng(seed + 1000 * nz + ncol)
    which = [kinds[f % len(kinds)] for f in range(nfield)]
    fields = [_field_of(k, ncol, nz, rng, nbin) for k in which]
    edges = np.stack([_edges_of(k, nbin) for k in which]) if nbin else None
    return fields, edges, [-35.0 if k == "dbz" else None for k in which]


def _run(m, fields, group=None, ngroup=1, edges=None, floors=None, dtype=np.float64, tensors=None):
    """level_stats of numpy fields (or of the CUDA `tensors` given in their place) -> the LevelStats, synchronised."""
    import torch
    names = ["f%d" % i for i in range(len(fields))]
    dev = tensors if tensors is not None else [torch.from_numpy(np.ascontiguousarray(x.astype(dtype))).to("cuda:0") for x in fields]
    r = m.level_stats(dict(zip(names, dev)), group=None if group is None else torch.from_numpy(group).to("cuda:0"), ngroup=ngroup,
                      edges=None if edges is None else dict(zip(names, edges)),
                      floor=None if floors is None else {n: f for n, f in zip(names, floors) if f is not None})
    torch.cuda.synchronize()
    return r


def _np(r):
    return r.mom.cpu().numpy(), None if r.hist is None else r.hist.cpu().numpy()


def _same_bits(a, b):
    return all((x is None and y is None) or (x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)))
               for x, y in zip(_np(a), _np(b)))


@pytest.mark.parametrize("ncol_of,nz,nfield,nbin", [("1", 2, 1, 0), ("C-1", 65, 3, 1), ("C+1", 120, 16, 64), ("3C+7", 256, 1, 64),
                                                    ("3C+7", 120, 3, 0), ("C+1", 2, 1, 64), ("1", 256, 16, 1)])
def test_shapes_against_numpy(gpu_mixed, ncol_of, nz, nfield, nbin):
    ncol = NCOL_OF[ncol_of](_chunks_of_a_large_ensemble())
    fields, edges, floors = _make(ncol, nz, nfield, nbin)
    r = _run(gpu_mixed, fields, edges=edges, floors=floors)
    assert tuple(r.count.shape) == (1, nfield, nz) and r.names == tuple("f%d" % i for i in range(nfield))
    worst = ref.check(*_np(r), fields, None, 1, edges, floors)
    print("ncol %d nz %d nfield %d nbin %d: worst mean error %.3g, worst M2 error %.3g of the bounds" % ((ncol, nz, nfield, nbin) + worst))


@pytest.mark.parametrize("ncol,nz", [(775, 65), (4099, 2)])
def test_bounds_on_every_dataset(gpu_mixed, ncol, nz):
    """T-like, lognormal, dBZ-like and the two ill-conditioned fields, with and without a histogram beside them."""
    fields, edges, floors = _make(ncol, nz, len(KINDS), 16)
    for e in (edges, None):
        worst = ref.check(*_np(_run(gpu_mixed, fields, edges=e, floors=floors)), fields, None, 1, e, floors)
        print("ncol %d nz %d: worst mean error %.3g, worst M2 error %.3g of the bounds" % ((ncol, nz) + worst))


def test_a_constant_field_has_its_value_as_mean_and_no_spread(gpu_mixed):
    x = np.full((775, 65), 0.1)
    mom, _ = _np(_run(gpu_mixed, [x, -x * 3.0e7]))
    assert np.all(mom[0, 0, 0] == 775) and np.all(mom[0, 0, 1] == 0.1) and np.all(mom[0, 1, 1] == -0.1 * 3.0e7)
    assert np.all(mom[0, :, 2] == 0.0)


def _groups(ncol, rng):
    """ngroup = 3: sizes that differ, group 1 empty, ids -1 and 3 present (left out)."""
    g = rng.choice(np.array([-1, 0, 2, 3], dtype=np.int32), size=ncol, p=[0.1, 0.5, 0.25, 0.15])
    g[:4] = (-1, 0, 2, 3)
    return g


def test_groups(gpu_mixed):
    ncol, nz = 257, 65
    fields, edges, floors = _make(ncol, nz, 3, 8)
    group = _groups(ncol, np.random.default_rng(SEED))
    r = _run(gpu_mixed, fields, group=group, ngroup=3, edges=edges, floors=floors)
    mom, hist = _np(r)
    worst = ref.check(mom, hist, fields, group, 3, edges, floors)
    print("3 groups: worst mean error %.3g, worst M2 error %.3g of the bounds" % worst)
    assert np.all(mom[1, :, 0] == 0) and np.all(mom[1, :, 1:3] == 0) and np.all(mom[1, :, 3] == np.inf) and np.all(mom[1, :, 4] == -np.inf)
    assert np.all(hist[1] == 0)
    assert hist[0].sum() == int((group == 0).sum()) * nz * 3       # the histogram counts every value of the group's columns


def test_64_groups_and_no_group(gpu_mixed):
    ncol, nz = 775, 65
    fields, edges, floors = _make(ncol, nz, 1, 1)
    group = np.random.default_rng(SEED + 1).integers(0, 64, ncol).astype(np.int32)
    ref.check(*_np(_run(gpu_mixed, fields, group=group, ngroup=64, edges=edges, floors=floors)), fields, group, 64, edges, floors)
    none = _run(gpu_mixed, fields, edges=edges, floors=floors)
    assert _same_bits(none, _run(gpu_mixed, fields, group=np.zeros(ncol, dtype=np.int32), edges=edges, floors=floors))
    two = _run(gpu_mixed, fields, ngroup=2, edges=edges, floors=floors)           # no ids: all in group 0, group 1 empty
    assert np.array_equal(_np(two)[0][0].view(np.uint64), _np(none)[0][0].view(np.uint64)) and np.all(_np(two)[1][1] == 0)


def test_a_rate_reached_through_its_column_stride(gpu_mixed):
    """rates[ncol][36][nz]: rate r is the slice rates[:, r, :], col_stride = 36 nz, beside a contiguous field."""
    import torch
    ncol, nz = 257, 120
    rng = np.random.default_rng(SEED + 2)
    rates = rng.standard_normal((ncol, 36, nz)) * 1.0e-6
    other = 250.0 + 10.0 * rng.standard_normal((ncol, nz))
    dev = torch.from_numpy(rates).to("cuda:0")
    edges = np.stack([np.linspace(-3.0e-6, 3.0e-6, 9), np.linspace(220.0, 280.0, 9)])
    for r in (0, 5, 35):
        got = _run(gpu_mixed, [None, None], edges=edges, tensors=[dev[:, r, :], torch.from_numpy(other).to("cuda:0")])
        ref.check(*_np(got), [np.ascontiguousarray(rates[:, r, :]), other], None, 1, edges, None)


def test_an_element_index_beyond_2_to_31(gpu_mixed):
    """300 columns whose stride puts the last of them past element 2**31 of a binary32 array (8.6 GB that are allocated
    and, but for the 300 x 2 values read, never touched)."""
    import torch
    ncol, nz, stride = 300, 2, 7200000
    assert (ncol - 1) * stride > 2 ** 31
    big = torch.empty(ncol * stride, dtype=torch.float32, device="cuda:0").as_strided((ncol, nz), (stride, 1))
    x = np.random.default_rng(SEED + 3).uniform(-35.3, 60.0, (ncol, nz)).astype(np.float32)
    big.copy_(torch.from_numpy(x).to("cuda:0"))
    edges = _edges_of("dbz", 19)[None]
    ref.check(*_np(_run(gpu_mixed, [None], edges=edges, tensors=[big])), [x.astype(np.float64)], None, 1, edges, None)


def test_reproducible_and_binary32_equals_widened(gpu_mixed):
    ncol, nz = 775, 120
    fields, edges, floors = _make(ncol, nz, 3, 64, kinds=("dbz", "t", "lognormal"))
    group = _groups(ncol, np.random.default_rng(SEED + 4))
    f32 = [x.astype(np.float32) for x in fields]
    a = _run(gpu_mixed, f32, group=group, ngroup=3, edges=edges, floors=floors, dtype=np.float32)
    b = _run(gpu_mixed, f32, group=group, ngroup=3, edges=edges, floors=floors, dtype=np.float32)
    wide = _run(gpu_mixed, [x.astype(np.float64) for x in f32], group=group, ngroup=3, edges=edges, floors=floors)
    assert _same_bits(a, b) and _same_bits(a, wide)
    assert _same_bits(wide, _run(gpu_mixed, [x.astype(np.float64) for x in f32], group=group, ngroup=3, edges=edges, floors=floors))
    ref.check(*_np(a), [x.astype(np.float64) for x in f32], group, 3, edges, floors)


@pytest.mark.parametrize("cut", [1, 300, 774])
def test_shards_merged_on_the_host(gpu_mixed, cut):
    ncol, nz = 775, 65
    fields, edges, floors = _make(ncol, nz, len(KINDS), 16)
    group = _groups(ncol, np.random.default_rng(SEED + 5))
    whole = _run(gpu_mixed, fields, group=group, ngroup=3, edges=edges, floors=floors)
    parts = [_run(gpu_mixed, [x[s] for x in fields], group=group[s], ngroup=3, edges=edges, floors=floors)
             for s in (slice(0, cut), slice(cut, ncol))]
    merged = parts[0].merge(parts[1])
    assert merged.mom.device == whole.mom.device
    (mom, hist), (wmom, whist) = _np(merged), _np(whole)
    for r in (0, 3, 4):
        assert np.array_equal(mom[:, :, r], wmom[:, :, r])
    assert np.array_equal(hist, whist)
    worst = ref.check(mom, hist, fields, group, 3, edges, floors)
    print("cut %d: worst mean error %.3g, worst M2 error %.3g of the bounds" % ((cut,) + worst))


def test_no_column(gpu_mixed):
    import torch
    r = gpu_mixed.level_stats({"a": torch.zeros(0, 37, dtype=torch.float64, device="cuda:0")}, ngroup=2, edges={"a": [0.0, 1.0, 2.0]})
    torch.cuda.synchronize()
    mom, hist = _np(r)
    assert np.all(mom[:, :, :3] == 0) and np.all(mom[:, :, 3] == np.inf) and np.all(mom[:, :, 4] == -np.inf) and np.all(hist == 0)
    assert np.all(np.isnan(r.percentile(50.0).cpu().numpy()))


def test_end_to_end_on_the_column_outputs(gpu_mixed):
    """256 mixed-phase columns: column_outputs, then the statistics of dBZ (5-dB bins, a floor of -35 dBZ: the CFAD) and
    re_qc over four groups, against numpy on the downloaded arrays."""
    import torch
    ncol = 256
    st = {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in cases.config3(ncol).items()}
    dbz, (re_qc, _, _) = gpu_mixed.column_outputs(st)
    group = (np.arange(ncol) % 4).astype(np.int32)
    edges = {"dbz": np.arange(-35.0, 65.0, 5.0), "re_qc": np.linspace(2.0e-6, 50.0e-6, 20)}
    r = gpu_mixed.level_stats({"dbz": dbz, "re_qc": re_qc}, group=torch.from_numpy(group).to("cuda:0"), ngroup=4, edges=edges,
                              floor={"dbz": -35.0})
    torch.cuda.synchronize()
    fields = [dbz.cpu().numpy(), re_qc.cpu().numpy()]
    assert fields[0].shape == (ncol, cases.NZ) and (fields[0] > -35.0).any()
    worst = ref.check(*_np(r), fields, group, 4, np.stack([edges["dbz"], edges["re_qc"]]), [-35.0, None])
    print("end to end: worst mean error %.3g, worst M2 error %.3g of the bounds" % worst)
    p90 = r.percentile(90.0).cpu().numpy()
    assert p90.shape == (4, 2, cases.NZ) and np.all((p90[:, 0] >= -35.0) & (p90[:, 0] <= 60.0))
    assert np.allclose(r.variance().cpu().numpy()[r.count.cpu().numpy() > 0], (r.m2 / r.count).cpu().numpy()[r.count.cpu().numpy() > 0])


def test_refusals_leave_the_outputs_untouched(gpu_mixed):
    import torch
    from kid_amd.stats import _StatsRequest, library
    L = library()
    ncol, nz, nbin = 40, 37, 4
    x = torch.zeros(ncol, nz, dtype=torch.float64, device="cuda:0")
    host = np.zeros((ncol, nz))
    edges = torch.linspace(-1.0, 1.0, nbin + 1, dtype=torch.float64, device="cuda:0")
    mom = torch.full((1, 1, 5, nz), 7.25, dtype=torch.float64, device="cuda:0")
    hist = torch.full((1, 1, nz, nbin + 3), -3, dtype=torch.int64, device="cuda:0")
    need = L.kidmp_stats_workspace_bytes(ncol, nz, 1, 1, nbin)
    assert need > 0
    work = torch.empty(need, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream

    def call(nz=nz, nfield=1, ptr=x.data_ptr(), stride=nz, nbytes=need, fn=L.kidmp_level_stats_device):
        req = _StatsRequest()
        ptrs = (C.c_void_p * 17)(*([ptr] * 17))
        strides = (C.c_int64 * 17)(*([stride] * 17))
        req.nfield, req.field, req.col_stride = nfield, C.cast(ptrs, C.POINTER(C.c_void_p)), C.cast(strides, C.POINTER(C.c_int64))
        req.ngroup, req.nbin, req.edges = 1, nbin, edges.data_ptr()
        return fn(gpu_mixed._h, ncol, nz, C.byref(req), mom.data_ptr(), hist.data_ptr(), work.data_ptr(), nbytes, s)

    for fn in (L.kidmp_level_stats_device, L.kidmp32_level_stats_device):
        for what, kw in (("a workspace that is too small", dict(nbytes=need - 1)), ("col_stride < nz", dict(stride=nz - 1)),
                         ("nz = 1", dict(nz=1)), ("nz = 257", dict(nz=257)), ("nfield = 17", dict(nfield=17)),
                         ("a host pointer as a field", dict(ptr=host.ctypes.data))):
            assert call(fn=fn, **kw) == -1, what                        # KIDMP_EINVAL
            assert L.kidmp_last_error(gpu_mixed._h)
    torch.cuda.synchronize()
    assert bool((mom == 7.25).all()) and bool((hist == -3).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((mom[0, 0, 0] == ncol).all()) and int(hist.sum()) == ncol * nz
