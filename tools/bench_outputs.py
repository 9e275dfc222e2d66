#!/usr/bin/env python
"""tools/bench_outputs.py -- time the column outputs (calc_effectRad + calc_refl10cm) on one MI355X: the fused
kidmp::k_column_outputs against the two launches that return the same four arrays.

Workload: BASELINE config 3 (10^5 mixed-phase columns x 120 levels, fp64) after one column step, state in HBM.
All variants run in ONE process, warmed up, alternating in blocks of --block launches, --blocks times each (200 launches
each by default); a block is timed with device events around it.  Variants:
  a_reflectivity     kidmp_reflectivity_device
  b_radii            kidmp_effective_radii_device on preset-filled arrays (INOUT; the fills are NOT in this time)
  b_fills            the three preset fills that (b) needs before every call, timed on their own
  c_all              kidmp_column_outputs_device, dbz + radii: one launch of k_column_outputs
  c_dbz, c_radii     kidmp_column_outputs_device with dbz alone / the radii alone
Prints ONE JSON line per process start: per variant ms_min / ms_mean over the blocks and the algorithmic bytes per column,
a_plus_b (the yardstick for c_all), the compiler's resource usage of the instantiations
(-Rpass-analysis=kernel-resource-usage with the library's own flags) and, unless --no-host, host_entry: ms of
kidmp_batch_step_host_out (all four) against kidmp_batch_step_host_refl and kidmp_batch_step_host_diag on the same 10^5
page-locked host columns (median of --host-reps alternating calls).
--starts N repeats the whole measurement from N fresh child processes, one line each, so that the spread between process
starts is on record.  Kernel times for the record come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/bench_outputs.py --no-host` run.
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NZ = 120
PROFILE = NZ * 8                         # bytes of one binary64 profile of a column
# profiles read + written per column by each variant in a context that is not aerosol-aware (nc is handed over but not read)
ALGO_PROFILES = {"a_reflectivity": 7 + 1,        # t p qv qr nr qs qg -> dbz
                 "b_radii": 7 + 3,               # t p qv qc qi ni qs -> re_qc re_qi re_qs (conditional stores, no read)
                 "b_fills": 3,
                 "c_all": 10 + 4,                # t p qv qc qi ni qr nr qs qg -> dbz re_qc re_qi re_qs
                 "c_dbz": 7 + 1, "c_radii": 7 + 3}
HBM_PEAK = 8.0e12
KERNELS = {"k_reflectivity<double,2>": ("thompson_reflectivity.hip", "k_reflectivityIdLi2E"),
           "k_column_outputs<double,2>": ("thompson_reflectivity.hip", "k_column_outputsIdLi2E"),
           "k_effective_radii<double,keep>": ("kidmp_diag.hip", "k_effective_radiiIdLb1E"),
           "k_effective_radii<double,preset>": ("kidmp_diag.hip", "k_effective_radiiIdLb0E")}


def resource_usage():
    """VGPRs / SGPRs / scratch / occupancy of the fp64 nz <= 128 instantiations as the compiler reports them."""
    csrc = os.path.join(ROOT, "kid_amd", "csrc")
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
             "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
    res = {}
    for src in sorted({v[0] for v in KERNELS.values()}):
        with tempfile.TemporaryDirectory() as d:
            r = subprocess.run(["hipcc"] + flags + ["-c", os.path.join(csrc, src), "-o", os.path.join(d, "r.o")],
                               capture_output=True, text=True, cwd=csrc)
        cur = None
        for line in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = next((k for k, (s, tag) in KERNELS.items() if s == src and tag in m.group(1)), None)
                continue
            if cur:
                for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"),
                                 ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                                 ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"),
                                 ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)")):
                    mm = re.search(pat, line)
                    if mm:
                        res.setdefault(cur, {})[key] = int(mm.group(1))
        if r.returncode != 0:
            res["error"] = "hipcc rc=%d on %s" % (r.returncode, src)
    return res


def measure(a):
    import numpy as np
    import torch
    import cases
    from kid_amd import STATE_NAMES, ThompsonMP, load_library
    from kid_amd.thompson import _Outputs, host_pinned_copy

    if not torch.cuda.is_available():
        sys.exit("bench_outputs: no GPU visible (this measurement has no CPU path)")
    L = load_library()
    m = ThompsonMP(iiwarm=False, device=0)
    st0 = cases.config3(a.ncol)
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in st0.items()}
    ppt = torch.zeros(a.ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                 # config 3 after one step
    s = torch.cuda.current_stream().cuda_stream
    ptr = lambda k: dev[k].data_ptr()            # noqa: E731
    new = lambda: torch.empty_like(dev["t"])     # noqa: E731
    dbz_a, dbz_c, dbz_d = new(), new(), new()
    re_b, re_c, re_r = [new() for _ in range(3)], [new() for _ in range(3)], [new() for _ in range(3)]
    presets = (2.49e-6, 4.99e-6, 9.99e-6)
    state11 = [ptr(k) for k in m.OUTPUT_NAMES]
    o_all = _Outputs(dbz_c.data_ptr(), *[x.data_ptr() for x in re_c])
    o_dbz = _Outputs(dbz_d.data_ptr(), None, None, None)
    o_rad = _Outputs(None, *[x.data_ptr() for x in re_r])

    def check(rc):
        if rc != 0:
            sys.exit("bench_outputs: entry failed (%d): %s" % (rc, L.kidmp_last_error(m._h).decode()))

    def fills():
        for x, v in zip(re_b, presets):
            x.fill_(v)
    variants = {
        "a_reflectivity": lambda: check(L.kidmp_reflectivity_device(m._h, a.ncol, NZ, *[ptr(k) for k in m.REFL_NAMES], dbz_a.data_ptr(), s)),
        "b_radii": lambda: check(L.kidmp_effective_radii_device(m._h, a.ncol * NZ, *[ptr(k) for k in m.RADII_NAMES], *[x.data_ptr() for x in re_b], s)),
        "b_fills": fills,
        "c_all": lambda: check(L.kidmp_column_outputs_device(m._h, a.ncol, NZ, *state11, C.byref(o_all), s)),
        "c_dbz": lambda: check(L.kidmp_column_outputs_device(m._h, a.ncol, NZ, *state11, C.byref(o_dbz), s)),
        "c_radii": lambda: check(L.kidmp_column_outputs_device(m._h, a.ncol, NZ, *state11, C.byref(o_rad), s)),
    }
    fills()
    for _ in range(a.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    fills()
    blocks = {k: [] for k in variants}
    for _ in range(a.blocks):                    # alternating: a block of every variant, then the next round
        for name, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.block):
                f()
            e1.record()
            e1.synchronize()
            blocks[name].append(e0.elapsed_time(e1) / a.block)
    torch.cuda.synchronize()
    # the fused launch returns what the two return (b started from the presets)
    fills()
    variants["b_radii"]()
    torch.cuda.synchronize()
    same = bool(torch.equal(dbz_a, dbz_c) and torch.equal(dbz_a, dbz_d)
                and all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(re_b, re_c, re_r)))
    res = {"metric": "column outputs fp64, config3 after one step", "ncol": a.ncol, "nz": NZ, "pid": os.getpid(),
           "launches_per_variant": a.block * a.blocks, "block": a.block, "blocks": a.blocks, "warmup": a.warmup,
           "bitwise_equal_outputs": same, "variants": {}}
    for name, t in blocks.items():
        nbytes = ALGO_PROFILES[name] * PROFILE
        res["variants"][name] = {"ms_min": round(min(t), 5), "ms_mean": round(sum(t) / len(t), 5), "ms_max": round(max(t), 5),
                                 "algo_bytes_per_col": nbytes,
                                 "achieved_TBps_at_min": round(nbytes * a.ncol / (min(t) * 1e-3) / 1e12, 4),
                                 "hbm_floor_ms": round(nbytes * a.ncol / HBM_PEAK * 1e3, 4)}
    v = res["variants"]
    res["a_plus_b"] = {"ms_min": round(v["a_reflectivity"]["ms_min"] + v["b_radii"]["ms_min"], 5),
                       "ms_mean": round(v["a_reflectivity"]["ms_mean"] + v["b_radii"]["ms_mean"], 5),
                       "algo_bytes_per_col": v["a_reflectivity"]["algo_bytes_per_col"] + v["b_radii"]["algo_bytes_per_col"]}
    res["c_all_over_a_plus_b"] = {"min": round(v["c_all"]["ms_min"] / res["a_plus_b"]["ms_min"], 4),
                                  "mean": round(v["c_all"]["ms_mean"] / res["a_plus_b"]["ms_mean"], 4)}
    res["kernel"] = resource_usage()
    res["device"] = torch.cuda.get_device_name(0)
    del dev, ppt, dbz_a, dbz_c, dbz_d, re_b, re_c, re_r
    torch.cuda.empty_cache()

    if not a.no_host:
        ncol = a.ncol
        dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        base = {k: host_pinned_copy(np.ascontiguousarray(x)) for k, x in st0.items()}
        work = {k: host_pinned_copy(x) for k, x in base.items()}
        pp = host_pinned_copy(np.zeros((ncol, 4)))
        ns = host_pinned_copy(np.zeros((ncol, 4), dtype=np.int32))
        outs = [host_pinned_copy(np.zeros((ncol, NZ))) for _ in range(4)]
        o = _Outputs(*[x.ctypes.data for x in outs])
        names = STATE_NAMES + ("p", "w", "dz")

        def call(which):
            for k in base:
                work[k][...] = base[k]
            args = [m._h, ncol, NZ, 10.0] + [dp(work[k]) for k in names] + [dp(pp), None, ns.ctypes.data_as(C.POINTER(C.c_int32))]
            t0 = time.perf_counter()
            if which == "out":
                rc = L.kidmp_batch_step_host_out(*args, C.byref(o))
            elif which == "refl":
                rc = L.kidmp_batch_step_host_refl(*args, dp(outs[0]))
            else:
                rc = L.kidmp_batch_step_host_diag(*args)
            t1 = time.perf_counter()
            check(rc)
            return (t1 - t0) * 1e3
        for w in ("diag", "refl", "out"):
            call(w)                              # warm-up (staging allocation)
        t = {"diag": [], "refl": [], "out": []}
        for _ in range(a.host_reps):
            for w in t:
                t[w].append(call(w))
        md, mr, mo = (float(np.median(t[w])) for w in ("diag", "refl", "out"))
        res["host_entry"] = {"ncol": ncol, "diag_ms": round(md, 3), "refl_ms": round(mr, 3), "out_ms": round(mo, 3),
                             "refl_minus_diag_ms": round(mr - md, 3), "out_minus_diag_ms": round(mo - md, 3),
                             "reps": a.host_reps, "pinned": True}
    print(json.dumps(res), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--starts", type=int, default=1, help="repeat from this many fresh child processes")
    a = ap.parse_args()
    if a.starts > 1:
        argv = ["--ncol", str(a.ncol), "--warmup", str(a.warmup), "--block", str(a.block), "--blocks", str(a.blocks),
                "--host-reps", str(a.host_reps)] + (["--no-host"] if a.no_host else [])
        for _ in range(a.starts):
            subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, check=True)
        return
    measure(a)


if __name__ == "__main__":
    main()
