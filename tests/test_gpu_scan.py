"""The range-height scan on the MI355X (include/kidmp_scan.h, kidmp::k_scan) against tests/scan_ref.py, the operator
restated in numpy.  -m gpu.

Exact, bit for bit: the geometry (cell, height) over every combination of the ranges of tests/scan_cases.py; the whole
pass-through (nsub = 1: dbz, pia, dbz_att, vr) on random fields; pia and dbz_att of a vertical scan against the cloud
radar's own pia_up and dbz_up; every equality between two device results (a ray alone and in a table of 300, a repeated
call, subsets of the outputs, out= reuse, graph replay, the NaN-filled surroundings, binary32 after one rounding, the scan
inside a slab run).

Against the restatement with nsub > 1 the kernel's exp and ln are fastmath.h's and the reference's are numpy's, so the
bound is max(4 x measured, 64 ulp); MEASURED holds the largest difference in ulp (2**-52) over every case of this file on
the MI355X: dbz, dbz_att and pia as the relative difference of the reflectivity (ratio) they stand for, |d dB| ln(10)/10,
vr relative to the largest |uc*ce| + |vd*se| among the gate's samples:
    dbz 14.7    dbz_att 58.9    pia 58.9    vr 1.9
so the bounds are 64 ulp for dbz and vr and 236 ulp for dbz_att and pia (both at nsub = 9 over 1024 gates, -120 dB).
A value in dB of magnitude M is itself only known to M ln(10)/10 ulp of the reflectivity it stands for (half an ulp of
-170 dB is 4 ulp of the ratio), which is what dbz_att and pia measure at the far gates of an attenuated ray.  No gate is
left out: where the reference is `missing` or infinite the device must hold the same bits.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import scan_cases as cases
import scan_ref as ref

pytestmark = pytest.mark.gpu

ULP = 2.220446049250313e-16
# the largest differences from the restatement measured on the MI355X, in ulp (see the module docstring)
MEASURED = {"dbz": 14.7, "dbz_att": 58.9, "pia": 58.9, "vr": 1.9}
VALUES = ("dbz", "dbz_att", "pia", "vr")
A_E = 8.5e6


def bound(kind):
    return max(4.0 * MEASURED[kind], 64.0) * ULP


def _ks():
    return importlib.import_module("kid_amd.scan")


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _cfg(**kw):
    from kid_amd import ScanCfg
    return ScanCfg(**kw)


def _scan(m, fields, zf, rays, dx, nx, want=ref.NAMES, dtype=None, **cfg):
    """scan() of numpy inputs, back as numpy."""
    import torch
    dev = {k: _cu(v if dtype is None else v.astype(dtype)) for k, v in fields.items() if v is not None}
    out = m.scan(dev, _cu(zf), _cu(rays), dx, nx, _cfg(**cfg), want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(ref.bits(a), ref.bits(b))


def _assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    diff = ref.bits(got) != ref.bits(want)
    assert not diff.any(), "%s: %d of %d differ, first at %s: %r vs %r" % (what, int(diff.sum()), diff.size, np.argwhere(diff)[0],
                                                                         got[tuple(np.argwhere(diff)[0])], want[tuple(np.argwhere(diff)[0])])


def _fields(ncol, nz, nx, seed, shared=False):
    """Random fields: dbz in [-25, 65], ext in [0, 5e-4] 1/m with a fifth of the cells clear, vd in [-2, 10], u in [-25, 25]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ext = rng.uniform(0.0, 5.0e-4, (ncol, nz)) * (rng.uniform(size=(ncol, nz)) > 0.2)
    return {"dbz": rng.uniform(-25.0, 65.0, (ncol, nz)), "ext": ext, "vd": rng.uniform(-2.0, 10.0, (ncol, nz)),
            "u": rng.uniform(-25.0, 25.0, (nx if shared else ncol, nz))}


def _kw(c):
    return dict(r0=c["r0"], dr=c["dr"], ngate=c["ngate"], half_inv_ae=c["half_inv_ae"], periodic=c["periodic"])


# ---- 1. geometry, exact ----
def _check_geometry(m, c, missing):
    nz, nx = c["nz"], c["nx"]
    ncol = c["nslab"] * nx
    f = {"dbz": np.arange(ncol * nz, dtype=np.float64).reshape(ncol, nz)}     # a cell's dbz is its own flat index
    got = _scan(m, f, c["zf"], c["rays"], c["dx"], nx, want=("dbz", "dbz_att", "pia", "height", "cell"), missing=missing, **_kw(c))
    valid, inside, i, k, h = cases.reference(c)
    inside = inside & valid[:, None]
    slab = np.where(valid, c["rays"][:, 0], 0.0).astype(np.int64)[:, None]
    cell = np.where(inside, (slab * nx + i) * nz + k, -1).astype(np.int32)
    _assert_same(got["cell"], cell, c["name"] + " cell")
    _assert_same(got["height"], np.where(valid[:, None], h, np.nan), c["name"] + " height")
    miss = np.float64(missing)
    _assert_same(got["dbz"], np.where(inside, cell.astype(np.float64), miss), c["name"] + " dbz")
    _assert_same(got["dbz_att"], np.where(inside, cell.astype(np.float64), miss), c["name"] + " dbz_att")   # no ext: d - (+0.0)
    _assert_same(got["pia"], np.where(inside, 0.0, miss), c["name"] + " pia")
    return inside


@pytest.mark.parametrize("nz", cases.NZS)
def test_geometry_is_the_references_bit_for_bit(gpu_mixed, nz):
    """cell and height over every combination of nx, ngate, periodic and curvature at this nz: both slabs, elevations 0.5,
    30, 90 and 150 degrees, and the rows of which no gate is inside (a slab that is none, weights that are none, NaN and
    infinite rows, positions beyond every cell index): those hold cell = -1 and the bits of `missing`."""
    missing = np.frombuffer(np.uint64(0x7ff8dead0000beef).tobytes(), dtype=np.float64)[0]    # a NaN with a payload
    n_in = n_out = 0
    for c in cases.full(nz):
        inside = _check_geometry(gpu_mixed, c, missing)
        n_in += int(inside.sum())
        n_out += int((~inside[:8]).sum())
        if c["periodic"] == 0 and c["ngate"] >= 130 and c["nx"] <= 7:
            assert not inside[3, -1] and inside[3, 0]                    # 150 degrees leaves through the side
        if c["ngate"] == 1024:
            assert not inside[2, -1] and inside[2, 0]                    # the vertical beam leaves through the top
    assert n_in > 5000 and n_out > 5000


def test_a_gate_on_a_face_belongs_to_the_level_above_and_an_edge_to_the_cell_on_its_right(gpu_mixed):
    c = cases.on_the_face()
    inside = _check_geometry(gpu_mixed, c, -999.0)
    nz, nx = c["nz"], c["nx"]
    got = _scan(gpu_mixed, {"dbz": np.zeros((2 * nx, nz))}, c["zf"], c["rays"], c["dx"], nx, want=("cell", "height"), **_kw(c))
    g = np.arange(20)
    assert np.array_equal(got["cell"][0, :20], 2 * nz + 2 * g + 1) and (got["cell"][0, 20:] == -1).all()       # cell 2 of slab 0
    assert np.array_equal(got["cell"][1, :20], nx * nz + 2 * g + 1)                                          # cell 0 of slab 1
    assert (got["cell"][2] == -1).all() and inside[:2, :20].all()                                             # x0 = nx*dx: outside
    assert np.array_equal(got["height"][0], 125.0 + 250.0 * np.arange(24))


# ---- 2. nsub = 1, exact ----
@pytest.mark.parametrize("nz, nx, ngate, periodic, curved, shared", [(65, 7, 130, 1, 1, False), (256, 3, 1024, 1, 0, True), (2, 64, 63, 0, 1, False),
                                                                     (64, 7, 65, 0, 0, True)])
def test_pass_through_is_the_references_bit_for_bit(gpu_mixed, nz, nx, ngate, periodic, curved, shared):
    import torch
    c = cases.case(nz, nx, ngate, periodic, curved)
    ncol = c["nslab"] * nx
    f = _fields(ncol, nz, nx, seed=nz + ngate, shared=shared)
    want = ref.scan(f, c["zf"], c["rays"], c["dx"], nx, c["r0"], c["dr"], ngate, 1, c["half_inv_ae"], periodic, -999.0)
    got = _scan(gpu_mixed, f, c["zf"], c["rays"], c["dx"], nx, missing=-999.0, **_kw(c))
    for n in ref.NAMES:
        _assert_same(got[n], want[n], "%s %s" % (c["name"], n))
    hit = got["cell"] >= 0
    assert hit.sum() > 100 and (got["pia"][hit] > 0).any()
    # dbz_att is dbz - pia as one subtraction of the device's own two numbers; dbz is the field at the returned cell
    _assert_same(got["dbz_att"][hit], (got["dbz"] - got["pia"])[hit], "dbz - pia")
    taken = torch.take(_cu(f["dbz"]), _cu(np.where(hit, got["cell"], 0)).long()).cpu().numpy()
    _assert_same(got["dbz"][hit], taken[hit], "torch.take(dbz, cell)")
    # without ext, vd and u: no attenuation; vr then needs one of the two
    bare = _scan(gpu_mixed, {"dbz": f["dbz"], "vd": f["vd"]}, c["zf"], c["rays"], c["dx"], nx, want=VALUES, missing=-999.0, **_kw(c))
    only = ref.scan({"dbz": f["dbz"], "vd": f["vd"]}, c["zf"], c["rays"], c["dx"], nx, c["r0"], c["dr"], ngate, 1, c["half_inv_ae"], periodic, -999.0)
    for n in VALUES:
        _assert_same(bare[n], only[n], "%s without ext and u: %s" % (c["name"], n))
    assert (bare["pia"][hit] == 0).all() and _same(bare["dbz"], bare["dbz_att"])


# ---- 3. the vertical scan is the cloud radar's own path ----
@pytest.mark.parametrize("nz", [65, 120])
def test_vertical_scan_is_mie_radars_pia_up_and_dbz_up(gpu_mixed, nz):
    """ce = 0, se = 1, x0 at the cell centres, r0 = 0, dr = dz uniform, ngate = nz, on the mixed-phase state of
    tests/mie_radar_cases.py: a = ext*dr is mie_radar's ext*dz, the scan over the gates is its scan over the levels with
    the same carry from group to group, then the same product with 20/ln 10 and the same subtraction.  Bit for bit."""
    import torch
    from kid_amd import MieCfg
    from mie_radar_cases import CFGS, state
    m = gpu_mixed
    st, _, w, _ = state(nz)
    ncol, dz0, dx = st["t"].shape[0], 100.0, 500.0
    with m.mie_table(MieCfg(**CFGS["w"])) as table:
        rad = m.mie_radar(table, {k: _cu(v) for k, v in st.items()}, _cu(np.full(nz, dz0)), _cu(w), None, ("dbz", "ext", "vd", "pia_up", "dbz_up"))
        torch.cuda.synchronize()
    rays = np.array([[0.0, (i + 0.5) * dx, 0.0, 0.0, 1.0, 1.0] for i in range(ncol)])
    zf = _cu(dz0 * np.arange(nz + 1))
    got = m.scan({"dbz": rad["dbz"], "ext": rad["ext"], "vd": rad["vd"]}, zf, _cu(rays), dx, ncol, _cfg(r0=0.0, dr=dz0, ngate=nz), ref.NAMES)
    torch.cuda.synchronize()
    assert np.array_equal(got["cell"].cpu().numpy(), np.arange(ncol * nz, dtype=np.int32).reshape(ncol, nz))
    assert (rad["pia_up"] > 0).any() and float(rad["pia_up"].max()) > 1.0
    for a, b in (("pia", "pia_up"), ("dbz_att", "dbz_up"), ("dbz", "dbz")):
        _assert_same(got[a].cpu().numpy(), rad[b].cpu().numpy(), "%s against mie_radar's %s" % (a, b))
    # straight up the radial velocity is -vd
    _assert_same(got["vr"].cpu().numpy(), (0.0 * 0.0 - rad["vd"] * 1.0).cpu().numpy(), "vr = -vd")


# ---- 4. nsub > 1 against the restatement ----
def _rel(got, want, hits):
    """|d dB| ln(10)/10 in ulp over the gates with a finite reference; everywhere else the bits must be the reference's."""
    fin = hits & np.isfinite(want)
    _assert_same(got[~fin], want[~fin], "a gate without a finite reference")
    return np.abs(got[fin] - want[fin]).max() * ref.DB_TO_LN / ULP if fin.any() else 0.0


def _beam_case(m, nsub, nz, nx, ngate, periodic, curved, seed, bw=1.0, fields=None, missing=float("nan")):
    from kid_amd import rhi_rays
    zf = ref.stretched_faces(nz, cases.TOP)
    x0 = 0.37 * nx * cases.DX
    rays = np.concatenate([rhi_rays(s, x0, 10.0, [0.5, 3.0, 30.0, 89.5, 150.0], bw, nsub) for s in range(2)])
    f = _fields(2 * nx, nz, nx, seed) if fields is None else fields
    kw = dict(r0=cases.R0, dr=cases.DR, ngate=ngate, half_inv_ae=1.0 / (2.0 * A_E) if curved else 0.0, periodic=periodic)
    want = ref.scan(f, zf, rays, cases.DX, nx, kw["r0"], kw["dr"], ngate, nsub, kw["half_inv_ae"], periodic, missing, parts=True)
    got = _scan(m, f, zf, rays, cases.DX, nx, nsub=nsub, missing=missing, **kw)
    return got, want


def _check_beam(got, want, what):
    _assert_same(got["cell"], want["cell"], what + " cell")
    _assert_same(got["height"], want["height"], what + " height")
    hits = want["hits"]
    seen = {n: _rel(got[n], want[n], hits) for n in ("dbz", "dbz_att", "pia")}
    _assert_same(got["vr"][~hits], want["vr"][~hits], what + " vr of a gate without a sample")
    scale = want["scale"][hits]
    assert (scale > 0).all()
    seen["vr"] = (np.abs(got["vr"][hits] - want["vr"][hits]) / scale).max() / ULP
    print("%s: " % what + "  ".join("%s %.1f" % (n, seen[n]) for n in VALUES) + " ulp")
    for n in VALUES:
        assert seen[n] * ULP <= bound(n), (what, n, seen[n])
    return seen


@pytest.mark.parametrize("nsub", [3, 5, 9])
def test_beam_against_the_restatement(gpu_mixed, nsub):
    worst = {n: 0.0 for n in VALUES}
    n_hit = n_miss = n_partly = 0
    for nz, nx, ngate, periodic, curved in ((65, 7, 130, 1, 1), (64, 3, 1024, 1, 0), (256, 64, 65, 0, 1), (2, 7, 63, 0, 0)):
        got, want = _beam_case(gpu_mixed, nsub, nz, nx, ngate, periodic, curved, seed=nsub + nz)
        seen = _check_beam(got, want, "nsub %d nz %d nx %d ngate %d" % (nsub, nz, nx, ngate))
        worst = {n: max(worst[n], seen[n]) for n in VALUES}
        n_hit, n_miss = n_hit + int(want["hits"].sum()), n_miss + int((~want["hits"]).sum())
        n_partly += int(((want["cell"] < 0) & want["hits"]).sum())   # non-uniform beam filling: the centre is outside, a neighbour is not
    assert n_hit > 5000 and n_miss > 1000 and n_partly > 0
    print("nsub %d worst: " % nsub + "  ".join("%s %.1f" % (n, worst[n]) for n in VALUES))


def test_four_identical_rows_of_a_quarter_reproduce_the_single_ray(gpu_mixed):
    nz, nx, ngate = 65, 7, 130
    zf = ref.stretched_faces(nz, cases.TOP)
    one = cases.sweep_rows(nx)[:8]
    four = np.repeat(one, 4, axis=0)
    four[:, 5] = 0.25
    f = _fields(2 * nx, nz, nx, seed=4)
    kw = dict(r0=cases.R0, dr=cases.DR, ngate=ngate, periodic=1, missing=-999.0)
    a = _scan(gpu_mixed, f, zf, one, cases.DX, nx, **kw)
    b = _scan(gpu_mixed, f, zf, four, cases.DX, nx, nsub=4, **kw)
    single = ref.scan(f, zf, one, cases.DX, nx, kw["r0"], kw["dr"], ngate, 1, 0.0, 1, -999.0, parts=True)
    assert _same(a["cell"], b["cell"]) and _same(a["height"], b["height"])
    _check_beam(b, dict(single, **{n: a[n] for n in VALUES}), "4 x 0.25 against the single ray")


def test_a_constant_field_without_extinction_returns_the_constant(gpu_mixed):
    nz, nx = 64, 7
    f = {"dbz": np.full((2 * nx, nz), 37.25), "ext": np.zeros((2 * nx, nz)), "vd": np.full((2 * nx, nz), 4.5), "u": np.full((2 * nx, nz), -12.0)}
    for nsub in (3, 9):
        got, want = _beam_case(gpu_mixed, nsub, nz, nx, 130, 1, 1, seed=0, fields=f)
        hits = want["hits"]
        assert np.abs(got["dbz"][hits] - 37.25).max() * ref.DB_TO_LN <= bound("dbz")
        assert np.abs(got["dbz_att"][hits] - 37.25).max() * ref.DB_TO_LN <= bound("dbz_att")
        assert np.abs(got["pia"][hits]).max() * ref.DB_TO_LN <= bound("pia")
        _check_beam(got, want, "constant field nsub %d" % nsub)
    # one sub-ray's v = uc*ce - vd*se exactly, through the pass-through
    rows = cases.sweep_rows(nx)[:8]
    got = _scan(gpu_mixed, f, ref.stretched_faces(nz, cases.TOP), rows, cases.DX, nx, want=("vr", "cell"), r0=cases.R0, dr=cases.DR, ngate=130, periodic=1)
    v = (-12.0 * rows[:, 3] - 4.5 * rows[:, 4])[:, None] * np.ones((1, 130))
    hit = got["cell"] >= 0
    _assert_same(got["vr"][hit], v[hit], "vr = uc*ce - vd*se")


# ---- 5. invariance: every one an equality of bits ----
def _table_of_300(nx, nsub):
    from kid_amd import rhi_rays
    el = np.linspace(0.3, 179.0, 150)
    return np.concatenate([rhi_rays(s, (0.21 + 0.4 * s) * nx * cases.DX, 5.0 + s, el, 0.9, nsub) for s in range(2)])


@pytest.mark.parametrize("nsub", [1, 5])
def test_bits_do_not_depend_on_batch_position_request_repeat_or_out(gpu_mixed, nsub):
    import torch
    m = gpu_mixed
    nz, nx, ngate = 65, 7, 130
    zf = ref.stretched_faces(nz, cases.TOP)
    rays = _table_of_300(nx, nsub)
    f = _fields(2 * nx, nz, nx, seed=5)
    kw = dict(r0=cases.R0, dr=cases.DR, ngate=ngate, nsub=nsub, half_inv_ae=1.0 / (2.0 * A_E), periodic=1, missing=-999.0)
    full = _scan(m, f, zf, rays, cases.DX, nx, **kw)
    assert (full["cell"] >= 0).sum() > 10000
    again = _scan(m, f, zf, rays, cases.DX, nx, **kw)
    for n in ref.NAMES:
        _assert_same(again[n], full[n], "repeat " + n)
    for r in (0, 137, 299):                                             # alone; 137 sits in the second wave of its workgroup
        alone = _scan(m, f, zf, rays[r * nsub:(r + 1) * nsub], cases.DX, nx, **kw)
        for n in ref.NAMES:
            _assert_same(alone[n][0], full[n][r], "ray %d alone: %s" % (r, n))
    shifted = _scan(m, f, zf, rays[nsub:], cases.DX, nx, **kw)            # every ray in another wave of another workgroup
    for n in ref.NAMES:
        _assert_same(shifted[n], full[n][1:], "shifted table: " + n)
    for sub in [(n,) for n in ref.NAMES] + [("pia", "cell"), ("height", "dbz"), ("vr", "dbz_att", "pia")]:
        part = _scan(m, f, zf, rays, cases.DX, nx, want=sub, **kw)
        assert sorted(part) == sorted(sub)
        for n in sub:
            _assert_same(part[n], full[n], "subset %s: %s" % (sub, n))
    # out= rewrites an earlier result in place
    dev = {k: _cu(v) for k, v in f.items()}
    dzf, drays, cfg = _cu(zf), _cu(rays), _cfg(**kw)
    first = m.scan(dev, dzf, drays, cases.DX, nx, cfg, ref.NAMES)
    ptrs = {n: t.data_ptr() for n, t in first.items()}
    for t in first.values():
        t.fill_(7)
    before = torch.cuda.memory_allocated()
    second = m.scan(dev, dzf, drays, cases.DX, nx, cfg, ref.NAMES, out=first)
    assert torch.cuda.memory_allocated() == before
    torch.cuda.synchronize()
    assert all(second[n] is first[n] for n in ref.NAMES) and {n: t.data_ptr() for n, t in second.items()} == ptrs
    for n in ref.NAMES:
        _assert_same(second[n].cpu().numpy(), full[n], "out= " + n)


def test_the_middle_of_a_nan_filled_tensor(gpu_mixed):
    """Every output lives in the middle of a NaN-filled (cell: -7-filled) buffer; the guard zones are intact afterwards."""
    import torch
    m = gpu_mixed
    nz, nx, ngate, nsub, pad = 64, 3, 65, 3, 4096
    zf = ref.stretched_faces(nz, cases.TOP)
    rays = _table_of_300(nx, nsub)[: 13 * nsub]
    f = _fields(2 * nx, nz, nx, seed=6)
    kw = dict(r0=cases.R0, dr=cases.DR, ngate=ngate, nsub=nsub, periodic=1, missing=-999.0)
    want = _scan(m, f, zf, rays, cases.DX, nx, **kw)
    n = 13 * ngate
    bufs, out = {}, {}
    for name in ref.NAMES:
        if name == "cell":
            bufs[name] = torch.full((n + 2 * pad,), -7, dtype=torch.int32, device="cuda:0")
        else:
            bufs[name] = torch.full((n + 2 * pad,), float("nan"), dtype=torch.float64, device="cuda:0")
        out[name] = bufs[name][pad:pad + n].view(13, ngate)
    m.scan({k: _cu(v) for k, v in f.items()}, _cu(zf), _cu(rays), cases.DX, nx, _cfg(**kw), ref.NAMES, out=out)
    torch.cuda.synchronize()
    for name in ref.NAMES:
        b = bufs[name].cpu().numpy()
        guard = np.concatenate([b[:pad], b[pad + n:]])
        assert (guard == -7).all() if name == "cell" else (ref.bits(guard) == ref.bits(np.float64("nan"))[()]).all(), name
        _assert_same(b[pad:pad + n].reshape(13, ngate), want[name], "guarded " + name)


@pytest.mark.parametrize("nsub", [1, 5])
def test_binary32_entry_rounds_once(gpu_mixed, nsub):
    nz, nx, ngate = 65, 7, 130
    zf = ref.stretched_faces(nz, cases.TOP)
    rays = _table_of_300(nx, nsub)[: 40 * nsub]
    f32 = {k: v.astype(np.float32) for k, v in _fields(2 * nx, nz, nx, seed=8).items()}
    kw = dict(r0=cases.R0, dr=cases.DR, ngate=ngate, nsub=nsub, half_inv_ae=1.0 / (2.0 * A_E), periodic=0, missing=-999.25)
    wide = _scan(gpu_mixed, {k: v.astype(np.float64) for k, v in f32.items()}, zf, rays, cases.DX, nx, **kw)
    narrow = _scan(gpu_mixed, f32, zf, rays, cases.DX, nx, **kw)
    assert (wide["cell"] >= 0).sum() > 1000 and (wide["cell"] < 0).sum() > 100
    for n in ref.NAMES:
        _assert_same(narrow[n], wide[n] if n == "cell" else wide[n].astype(np.float32), "binary32 " + n)


def test_hip_graph_replay_of_one_captured_launch(gpu_mixed):
    import torch
    ks = _ks()
    m, L = gpu_mixed, ks.library()
    nz, nx, ngate, nsub = 65, 7, 130, 3
    zf = ref.stretched_faces(nz, cases.TOP)
    rays = _table_of_300(nx, nsub)[: 50 * nsub]
    f = _fields(2 * nx, nz, nx, seed=9)
    kw = dict(r0=cases.R0, dr=cases.DR, ngate=ngate, nsub=nsub, periodic=1, missing=-999.0)
    eager = _scan(m, f, zf, rays, cases.DX, nx, **kw)
    dev = {k: _cu(v) for k, v in f.items()}
    dzf, drays = _cu(zf), _cu(rays)
    out = {n: torch.full((50, ngate), -7, dtype=torch.int32 if n == "cell" else torch.float64, device="cuda:0") for n in ref.NAMES}
    o = ks._ScanOut(**{n: t.data_ptr() for n, t in out.items()})
    cfg = ks._config("scan", _cfg(**kw))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = L.kidmp_scan_device(m._h, 2, nx, nz, cases.DX, dev["dbz"].data_ptr(), dev["ext"].data_ptr(), dev["vd"].data_ptr(), dev["u"].data_ptr(), 0,
                                 dzf.data_ptr(), drays.data_ptr(), 50, C.byref(cfg), C.byref(o), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    for _ in range(2):
        for t in out.values():
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for n in ref.NAMES:
            _assert_same(out[n].cpu().numpy(), eager[n], "replay " + n)


# ---- 6. refusals ----
def test_refusals_write_nothing(gpu_mixed):
    import torch
    ks = _ks()
    L = ks.library()
    nz, nx, nslab, ngate, nray = 16, 8, 2, 32, 6
    ncol = nslab * nx
    field = torch.zeros(ncol, nz, dtype=torch.float64, device="cuda:0")
    zf = _cu(100.0 * np.arange(nz + 1))
    rays = _cu(cases.sweep_rows(nx)[:nray])
    out = torch.full((nray, ngate), -7.0, dtype=torch.float64, device="cuda:0")
    cell = torch.full((nray, ngate), -7, dtype=torch.int32, device="cuda:0")
    host = torch.zeros(ncol * nz, dtype=torch.float64)
    nan, inf = float("nan"), float("inf")
    P = dict(dbz=field.data_ptr(), ext=field.data_ptr(), vd=field.data_ptr(), u=field.data_ptr(), zf=zf.data_ptr(), rays=rays.data_ptr())

    def call(m=gpu_mixed, nslab=nslab, nx=nx, nz=nz, dx=100.0, nray=nray, names=("dbz", "vr"), cfg=True, outp=True, fn=L.kidmp_scan_device, **over):
        p = dict(P)
        c = dict(r0=0.0, dr=60.0, ngate=ngate, nsub=1, half_inv_ae=0.0, periodic=0, missing=-5.0)
        for k in list(over):
            if k in c:
                c[k] = over.pop(k)
        p.update(over)
        o = ks._ScanOut(**{n: (cell if n == "cell" else out).data_ptr() for n in names})
        return fn(m._h if m is not None else None, nslab, nx, nz, dx, p["dbz"], p["ext"], p["vd"], p["u"], 0, p["zf"], p["rays"], nray,
                  C.byref(ks._ScanCfg(*[c[k] for k, _ in ks._ScanCfg._fields_])) if cfg else None, C.byref(o) if outp else None, None)

    refused = [dict(nx=0), dict(nx=-3), dict(nz=1), dict(nz=257), dict(nslab=-1), dict(nslab=2 ** 31, nx=1), dict(nslab=2 ** 28, nx=8), dict(nray=-1),
               dict(ngate=0), dict(ngate=1025), dict(nsub=0), dict(nsub=10), dict(dx=0.0), dict(dx=-1.0), dict(dx=nan), dict(dx=inf), dict(dr=0.0),
               dict(dr=-60.0), dict(dr=nan), dict(dr=inf), dict(r0=-1.0), dict(r0=nan), dict(half_inv_ae=nan), dict(half_inv_ae=inf), dict(dbz=None),
               dict(zf=None), dict(rays=None), dict(cfg=False), dict(outp=False), dict(names=()), dict(names=("vr",), vd=None, u=None),
               dict(names=("cell",), nslab=2 ** 27, nx=8, nz=16), dict(dbz=host.data_ptr()), dict(ext=host.data_ptr()), dict(vd=host.data_ptr()),
               dict(u=host.data_ptr()), dict(zf=host.data_ptr()), dict(rays=host.data_ptr())]
    for kw in refused:
        for fn in (L.kidmp_scan_device, L.kidmp32_scan_device):
            assert call(fn=fn, **kw) == -1, kw
            assert L.kidmp_last_error(gpu_mixed._h), kw
    assert call(m=None) == -5 and call(nray=0) == 0 and call(nslab=0) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all() and (cell.cpu().numpy() == -7).all()
    assert call(ext=None, vd=None, names=("dbz", "vr", "cell")) == 0 and call(u=None, names=("vr",)) == 0 and call(names=("height",)) == 0
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()).all() and (cell.cpu().numpy() >= -1).all()
    from kid_amd import KidmpError
    with pytest.raises(KidmpError, match="vr needs"):
        gpu_mixed.scan({"dbz": field}, zf, rays, 100.0, nx, _cfg(dr=60.0, ngate=ngate), want=("vr",))


# ---- 7. inside a run ----
def test_scan_from_on_step_of_a_slab_run_equals_a_scan_of_the_final_fields(gpu_mixed):
    """kid_run_slab on nx = 8, nz = 16, two steps; on_step forms t and calls reflectivity, then scan, on the run's stream
    without a synchronisation, rewriting one result.  What the last step left equals a scan of the cloned final fields."""
    import torch
    import cases as col
    from kid_amd import rhi_rays, streamfunction_flow
    m = gpu_mixed
    P0, R_ON_CP, DT = 1.0e5, 287.058 / 1005.0, 10.0
    nx, nz, nsub = 8, 16, 3
    lev = np.arange(nz) * (col.NZ // nz)
    st = {k: np.ascontiguousarray(v[:, lev]) for k, v in col.config3(nx).items()}
    exner = (st["p"] / P0) ** R_ON_CP
    state = {k: _cu(st[k]) for k in ("qv", "qc", "qr", "nr", "qi", "ni", "qs", "qg")}
    state["theta"] = _cu(st["t"] / exner)
    dz = np.ascontiguousarray(st["dz"][0])
    rho = 0.622 * st["p"][0] / (287.04 * st["t"][0] * (st["qv"][0] + 0.622))
    dx = 4.0 * float(dz.mean())
    x = (np.arange(nx) / float(nx))[:, None]
    psi = 0.02 * rho.mean() * dx * np.sin(2.0 * np.pi * x + 0.4) * np.sin(np.pi * np.arange(nz + 1) / float(nz))[None, :]
    drho, ddz, dex, dp = _cu(rho), _cu(dz), _cu(exner), _cu(st["p"])
    du, dw = streamfunction_flow(_cu(psi), drho, ddz, dx, nx=nx)
    zf = _cu(np.concatenate([[0.0], np.cumsum(dz)]))
    rays = _cu(rhi_rays(0, 0.3 * nx * dx, 0.0, [2.0, 20.0, 60.0, 90.0, 140.0], 1.0, nsub))
    cfg = _cfg(r0=0.0, dr=float(dz.sum()) / 50.0, ngate=65, nsub=nsub, periodic=True, missing=-999.0)
    want = ("dbz", "dbz_att", "vr", "height", "cell")
    dbz = torch.empty(nx, nz, dtype=torch.float64, device="cuda:0")
    res = {n: torch.full((5, 65), -7, dtype=torch.int32 if n == "cell" else torch.float64, device="cuda:0") for n in want}
    calls = []

    def observe(s):
        refl = {"t": s["theta"] * dex, "p": dp, "qv": s["qv"], "qr": s["qr"], "nr": s["nr"], "qs": s["qs"], "qg": s["qg"]}
        m.reflectivity(refl, out=dbz)
        return m.scan({"dbz": dbz, "u": du}, zf, rays, dx, nx, cfg, want, out=res)

    def on_step(step, s, mphys):
        r = observe(s)
        assert all(r[n] is res[n] for n in want)
        calls.append(step)

    out, _, courant = m.kid_run_slab(state, 2, DT, P0, R_ON_CP, dex, ddz, drho, dx, nx, du, dw, on_step=on_step)
    torch.cuda.synchronize()
    assert calls == [0, 1] and float(courant.max()) < 1.0
    in_run = {n: t.cpu().numpy().copy() for n, t in res.items()}
    final = {k: v.clone() for k, v in out.items()}
    res = {n: torch.empty_like(t) for n, t in res.items()}
    after = observe(final)
    torch.cuda.synchronize()
    for n in want:
        _assert_same(in_run[n], after[n].cpu().numpy(), "in the run against afterwards: " + n)
    assert (in_run["cell"] >= 0).sum() > 50 and np.isfinite(in_run["dbz"][in_run["cell"] >= 0]).all()
