"""The multi-channel entries (include/kidmp_multichannel.h, kid_amd/multichannel.py) without a GPU: the eight entries and
kidmp_multichannel_tile exist in the built library and in the new header only, kid_amd/multichannel.py declares them as the
header has them, the header compiles as C99 and C++11, a missing context is refused, the tile is a count of channels, and
the wrappers refuse wrong input before the library is reached."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_mie_abi as tma
import test_radiometer_abi as tra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_multichannel.h")
ENTRIES = tuple("%s_%s_multi_%s" % (p, k, e) for k in ("radiometer", "mie_radar") for p in ("kidmp", "kidmp32") for e in ("device", "host"))
SYMBOLS = ENTRIES + ("kidmp_multichannel_tile",)
EINVAL, ESTATE = -1, -5


def test_symbols_are_exported_and_prototyped_in_the_new_header_only():
    lib = os.path.join(ROOT, "kid_amd", "libkidmp.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(lib)
    assert len(ENTRIES) == 8 and sorted(tra._prototypes(HEADER)) == sorted(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    raw = open(HEADER).read()
    assert '#include "kidmp_radiometer.h"' in raw and int(re.search(r"#define KIDMP_MAX_CHANNELS (\d+)", raw).group(1)) == 16
    inc = os.path.join(ROOT, "include")
    for other in sorted(os.listdir(inc)):
        if other.endswith(".h") and other != "kidmp_multichannel.h":
            assert not set(SYMBOLS) & set(tra._prototypes(os.path.join(inc, other))), other


def test_the_python_declarations_match_the_header():
    import kid_amd
    import kid_amd.mie as km
    import kid_amd.multichannel as kmc
    import kid_amd.radiometer as kr
    import kid_amd.thompson as th
    declared = kmc.declare(tma._Stub()).entries
    protos = tra._prototypes(HEADER)
    assert sorted(declared) == sorted(protos) == sorted(kmc._declarations())
    wrong = []
    for name, (ret, params) in sorted(protos.items()):
        e = declared[name]
        if len(e.argtypes) != len(params):
            wrong.append("%s: %d arguments declared, the header has %d" % (name, len(e.argtypes), len(params)))
            continue
        for i, (p, t) in enumerate(zip(params, e.argtypes)):
            ok = tma._is_pointer(t) if "*" in p else t in tma.SCALARS[re.sub(r"\bconst\b", "", p).split()[0]]
            if not ok:
                wrong.append("%s: argument %d is `%s`, declared %s" % (name, i, p, getattr(t, "__name__", t)))
        if e.restype not in tma.SCALARS[ret]:
            wrong.append("%s: returns `%s`, declared %s" % (name, ret, getattr(e.restype, "__name__", e.restype)))
    assert not wrong, "\n".join(wrong)
    for other in (th, km, kr):
        assert not set(SYMBOLS) & set(other._declarations())
    assert kmc.MAX_CHANNELS == kid_amd.MAX_CHANNELS == 16
    for name in ("radiometer_multi", "radiometer_multi_host", "mie_radar_multi", "mie_radar_multi_host", "multichannel_tile"):
        assert getattr(kid_amd, name) is getattr(kmc, name)
        assert name == "multichannel_tile" or callable(getattr(kid_amd.ThompsonMP, name))


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_multichannel.h"\n'
                   "int use(kidmp_ctx *c, const double *a, const float *b, const kidmp_radiometer_table *const *rt, const kidmp_mie_table *const *mt,\n"
                   "        const kidmp_radiometer_cfg *q, kidmp_radiometer_out *ro, kidmp32_radiometer_out *ro32, kidmp_mie_out *mo, kidmp32_mie_out *mo32)\n"
                   "{ int n = kidmp_multichannel_tile(0, 120) + kidmp_multichannel_tile(1, 120);\n"
                   "  n += kidmp_radiometer_multi_device(c, rt, 2, q, 1, 2, a, a, a, a, a, a, a, a, a, 0, a, 0, 2, a, ro, 0);\n"
                   "  n += kidmp32_radiometer_multi_device(c, rt, 2, q, 1, 2, b, b, b, b, b, b, b, b, b, 0, b, 0, 2, b, ro32, 0);\n"
                   "  n += kidmp_radiometer_multi_host(c, rt, 2, q, 1, 2, a, a, a, a, a, a, a, a, a, 0, a, 0, 2, a, ro);\n"
                   "  n += kidmp32_radiometer_multi_host(c, rt, 2, q, 1, 2, b, b, b, b, b, b, b, b, b, 0, b, 0, 2, b, ro32);\n"
                   "  n += kidmp_mie_radar_multi_device(c, mt, 2, 1, 2, a, a, a, a, a, a, a, a, a, 0, a, a, 0, 2, mo, 0);\n"
                   "  n += kidmp32_mie_radar_multi_device(c, mt, 2, 1, 2, b, b, b, b, b, b, b, b, b, 0, b, b, 0, 2, mo32, 0);\n"
                   "  n += kidmp_mie_radar_multi_host(c, mt, 2, 1, 2, a, a, a, a, a, a, a, a, a, 0, a, a, 0, 2, mo);\n"
                   "  n += kidmp32_mie_radar_multi_host(c, mt, 2, 1, 2, b, b, b, b, b, b, b, b, b, 0, b, b, 0, 2, mo32);\n"
                   "  return n + KIDMP_MAX_CHANNELS; }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context_and_the_tile_is_a_count():
    from kid_amd import multichannel_tile
    from kid_amd.mie import _MieOut
    from kid_amd.multichannel import library
    from kid_amd.radiometer import _RadiometerOut
    L = library()
    ro, mo = _RadiometerOut(), _MieOut()
    handles = (C.c_void_p * 2)(None, None)
    rad = [None, handles, 2, None, 4, 120] + [None] * 8 + [None, 0, None, 0, 0, None, C.byref(ro)]
    mie = [None, handles, 2, 4, 120] + [None] * 8 + [None, 0, None, None, 0, 0, C.byref(mo)]
    for p in ("kidmp", "kidmp32"):
        assert getattr(L, p + "_radiometer_multi_host")(*rad) == ESTATE and getattr(L, p + "_radiometer_multi_device")(*rad, None) == ESTATE
        assert getattr(L, p + "_mie_radar_multi_host")(*mie) == ESTATE and getattr(L, p + "_mie_radar_multi_device")(*mie, None) == ESTATE
    for which in ("radiometer", "radar"):
        tiles = [multichannel_tile(which, nz) for nz in (2, 64, 65, 128, 129, 256)]
        print(which, tiles)
        assert all(isinstance(t, int) and 1 <= t <= 16 for t in tiles)
        assert tiles[0] == tiles[1] and tiles[2] == tiles[3] and tiles[4] == multichannel_tile(which, 192)   # one tile per number of level groups
        assert multichannel_tile(("radiometer", "radar").index(which), 120) == multichannel_tile(which, 120)
    assert L.kidmp_multichannel_tile(2, 120) == 0 and L.kidmp_multichannel_tile(-1, 120) == 0
    assert L.kidmp_multichannel_tile(0, 0) == 0 and L.kidmp_multichannel_tile(1, 257) == 0


def test_wrappers_reject_bad_arguments_before_the_library(monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import RADIOMETER_INPUTS, MieTable, RadiometerCfg, RadiometerTable, multichannel_tile
    N, NZ = 4, 30
    good = lambda: {k: np.zeros((N, NZ)) for k in RADIOMETER_INPUTS}   # noqa: E731
    m = tma._bare()
    rt, mt = [tra._fake_table(m) for _ in range(3)], [tma._fake_table(m) for _ in range(3)]
    monkeypatch.setattr(th, "load_library", lambda *a: tma._NoLibrary())
    monkeypatch.setattr(RadiometerTable, "close", lambda self: None)
    monkeypatch.setattr(MieTable, "close", lambda self: None)
    dz = np.ones(NZ)
    r = RadiometerCfg()
    tables = [[], rt * 6, rt[0], None, "tables", [rt[0], None, rt[2]], [rt[0], mt[1], rt[2]], [rt[0], tra._fake_table(tma._bare()), rt[2]]]
    for ts in tables:
        with pytest.raises(th.KidmpError, match="radiometer_multi_host"):
            m.radiometer_multi_host(ts, good(), dz)
    for ts in ([], mt * 6, mt[0], [mt[0], None, mt[2]], [mt[0], rt[1], mt[2]], [mt[0], tma._fake_table(tma._bare()), mt[2]]):
        with pytest.raises(th.KidmpError, match="mie_radar_multi_host"):
            m.mie_radar_multi_host(ts, good(), dz)
    cases = [
        ([np.zeros((N, NZ))], {}), ({k: np.zeros((N, 1)) for k in RADIOMETER_INPUTS}, {}), ({k: v for k, v in good().items() if k != "qr"}, dict(dz=dz)),
        (good(), dict(dz=dz, want=("tb_toa", "tb"))), (good(), dict(dz=dz, want=())), (good(), dict(want=("tb_toa",))), (good(), dict(dz=np.ones(NZ + 1))),
        (good(), dict(dz=dz, k_gas=np.ones((NZ, N)))), (good(), dict(dz=dz, k_gas=np.ones((2, NZ)))), (good(), dict(dz=dz, k_gas=np.ones((3, N, NZ + 1)))),
        (good(), dict(dz=dz, k_gas=np.ones((3, N + 1, NZ)))), (good(), dict(dz=dz, k_gas=[1.0] * NZ)), (good(), dict(dz=dz, k_gas=np.ones((3, NZ), dtype=np.float32))),
        (good(), dict(dz=dz, t_sfc=np.ones(NZ))), (good(), dict(dz=dz, out={"tb_toa": np.zeros(N)})), (good(), dict(dz=dz, out={"tb_toa": np.zeros((2, N))})),
        (good(), dict(dz=dz, want=("tb_up",), out={"tb_up": np.zeros((N, NZ))})),
        (good(), dict(dz=dz, rcfgs=[r, r])), (good(), dict(dz=dz, rcfgs=[r] * 4)), (good(), dict(dz=dz, rcfgs=dict(mu=1.0))),
        (good(), dict(dz=dz, rcfgs=[r, r, RadiometerCfg(mu=0.0)])), (good(), dict(dz=dz, rcfgs=[r, r, RadiometerCfg(emissivity=1.1)])),
        (good(), dict(dz=dz, rcfgs=RadiometerCfg(t_cosmic=-1.0))), (good(), dict(dz=dz, rcfgs=[r, None, "r"])),
    ]
    for st, kw in cases:
        with pytest.raises(th.KidmpError, match="radiometer_multi_host"):
            m.radiometer_multi_host(rt, st, **kw)
    for kw in (dict(want=("dbz_up",)), dict(dz=dz, want=("dbz", "z")), dict(dz=dz, k_gas=np.ones((2, NZ))), dict(dz=dz, w=np.ones(NZ)),
               dict(dz=dz, out={"dbz": np.zeros((N, NZ))}), dict(dz=dz, want=("pia_total",), out={"pia_total": np.zeros((3, N, NZ))})):
        with pytest.raises(th.KidmpError, match="mie_radar_multi_host"):
            m.mie_radar_multi_host(mt, good(), **kw)
    import torch
    with pytest.raises(th.KidmpError, match="radiometer_multi"):
        m.radiometer_multi(rt, {k: torch.zeros(N, NZ, dtype=torch.float64) for k in RADIOMETER_INPUTS}, torch.ones(NZ, dtype=torch.float64))   # host memory
    with pytest.raises(th.KidmpError, match="mie_radar_multi"):
        m.mie_radar_multi(mt, good(), dz)
    for which, nz in (("imager", 120), (2, 120), ("radar", 0), ("radar", 257), (0, 12.5)):
        with pytest.raises(th.KidmpError, match="multichannel_tile"):
            multichannel_tile(which, nz)
