#!/usr/bin/env python
"""tools/bench_reflectivity.py -- time the calc_refl10cm kernel (kid_amd/csrc/thompson_reflectivity.hip) on one MI355X.

Workload: BASELINE config 3 (10^5 mixed-phase columns x 120 levels, fp64) after one column step, state in HBM.
Prints ONE JSON line:
  ms_per_call        device-event time of one kidmp_reflectivity_device launch, mean over --iters launches after --warmup
  algo_bytes_per_col 7 680 B: 7 profiles read (t, p, qv, qr, nr, qs, qg) + 1 written (dbz), 120 levels x 8 B
  achieved_TBps, hbm_frac   algorithmic bytes / time, and that over 8 TB/s
  kernel             -Rpass-analysis=kernel-resource-usage of the nz <= 128 fp64 instance (VGPRs, SGPRs, scratch, occupancy),
                     from a compile of the kernel source with the library's own flags
  host_entry         unless --no-host: ms of kidmp_batch_step_host_refl vs kidmp_batch_step_host_diag on the same 10^5
                     page-locked host columns (median of --host-reps alternating calls), and the difference
Kernel time for the record comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_reflectivity.py
--no-host` run (the kernel is listed as kidmp::k_reflectivity<double, 2>).
"""
import argparse
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
ALGO_BYTES_PER_COL = 8 * NZ * 8          # 7 profiles in + 1 out, binary64
HBM_PEAK = 8.0e12


def resource_usage():
    """VGPRs / SGPRs / scratch / occupancy of k_reflectivity<double, 2> as the compiler reports them."""
    csrc = os.path.join(ROOT, "kid_amd", "csrc")
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
             "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["hipcc"] + flags + ["-c", os.path.join(csrc, "thompson_reflectivity.hip"), "-o",
                                                os.path.join(d, "r.o")], capture_output=True, text=True, cwd=csrc)
    out, cur, res = r.stderr, None, {}
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        if cur and "k_reflectivityIdLi2E" in cur:
            for key, pat in (("vgpr", r"VGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"),
                             ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"),
                             ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)")):
                mm = re.search(pat, line)
                if mm:
                    res[key] = int(mm.group(1))
    if not res:
        res["error"] = "no resource remarks (hipcc rc=%d)" % r.returncode
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    import cases
    from kid_amd import STATE_NAMES, ThompsonMP
    from kid_amd.thompson import host_pinned_copy

    if not torch.cuda.is_available():
        sys.exit("bench_reflectivity: no GPU visible (this measurement has no CPU path)")
    m = ThompsonMP(iiwarm=False, device=0)
    st0 = cases.config3(a.ncol)
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in st0.items()}
    ppt = torch.zeros(a.ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                 # config 3 after one step
    out = torch.empty_like(dev["t"])
    for _ in range(a.warmup):
        m.reflectivity(dev, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        m.reflectivity(dev, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    dbz = out.cpu().numpy()
    res = {
        "metric": "calc_refl10cm fp64, config3 after one step", "ncol": a.ncol, "nz": NZ,
        "ms_per_call": round(ms, 5), "iters": a.iters, "warmup": a.warmup,
        "algo_bytes_per_col": ALGO_BYTES_PER_COL,
        "achieved_TBps": round(ALGO_BYTES_PER_COL * a.ncol / (ms * 1e-3) / 1e12, 4),
        "hbm_frac": round(ALGO_BYTES_PER_COL * a.ncol / (ms * 1e-3) / HBM_PEAK, 4),
        "hbm_floor_ms": round(ALGO_BYTES_PER_COL * a.ncol / HBM_PEAK * 1e3, 4),
        "dbz_min_max": [round(float(dbz.min()), 3), round(float(dbz.max()), 3)],
        "kernel": resource_usage(),
        "device": torch.cuda.get_device_name(0),
    }
    del dev, out, ppt
    torch.cuda.empty_cache()

    if not a.no_host:
        from kid_amd import load_library
        import ctypes as C
        L = load_library()
        ncol = a.ncol
        dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        base = {k: host_pinned_copy(np.ascontiguousarray(v)) for k, v in st0.items()}
        work = {k: host_pinned_copy(v) for k, v in base.items()}
        pp = host_pinned_copy(np.zeros((ncol, 4)))
        ns = host_pinned_copy(np.zeros((ncol, 4), dtype=np.int32))
        dbz = host_pinned_copy(np.zeros((ncol, NZ)))
        names = STATE_NAMES + ("p", "w", "dz")

        def call(refl):
            for k in base:
                work[k][...] = base[k]
            args = [m._h, ncol, NZ, 10.0] + [dp(work[k]) for k in names] + [dp(pp), None,
                                                                             ns.ctypes.data_as(C.POINTER(C.c_int32))]
            t0 = time.perf_counter()
            rc = L.kidmp_batch_step_host_refl(*args, dp(dbz)) if refl else L.kidmp_batch_step_host_diag(*args)
            t1 = time.perf_counter()
            if rc != 0:
                sys.exit("bench_reflectivity: host entry failed (%d)" % rc)
            return (t1 - t0) * 1e3
        call(False), call(True)                     # warm-up (staging allocation)
        td, tr = [], []
        for _ in range(a.host_reps):
            td.append(call(False))
            tr.append(call(True))
        md, mr = float(np.median(td)), float(np.median(tr))
        res["host_entry"] = {"ncol": ncol, "diag_ms": round(md, 3), "refl_ms": round(mr, 3),
                             "refl_minus_diag_ms": round(mr - md, 3), "reps": a.host_reps, "pinned": True}
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    main()
