#!/usr/bin/env python
"""tools/bench_kid_advect.py -- time the kinematic entries (include/kidmp_kinematic.h: one launch of kidmp::k_kid_advect,
one of kidmp::k_kid_update) on one MI355X beside the adapter they feed and a torch composite of the same numbers.

Workloads: 10^5 and 10^4 mixed-phase columns x 120 levels (BASELINE config 3) in KiD's theta form, fp64, state in HBM,
per-column w of both signs at Courant <= 0.64.  All variants run in ONE process, warmed up, taking turns launch by launch;
every launch is timed with device events of its own and the median of --reps (30) launches is reported with the minimum
and maximum beside it.  Variants:
  advect_sum     advect(want="sum") with courant: what a run step calls
  advect_adv_div advect(want=("adv", "div"))
  update         update(state, dt, sum, mphys)
  kid_interface  the adapter alone on the same state (adv = sum)
  run_step       one full step of run(): advect, kid_interface, update, the ppt accumulation
  composite      the same `sum` of the nine fields from torch operations on the device tensors (checked against advect once)
The state is put back before every launch that changes it (outside the timed span).  Algorithmic bytes per column: advect
reads nine profiles and writes nine per requested output; update reads 27 and writes nine; their share of 8 TB/s is
printed.  Prints one line per variant and workload and ONE JSON line at the end; the lines also go to --out
(profiles/r15_kid_advect.txt) under a header with the date and the library's fingerprint."""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NZ = 120
HBM_PEAK = 8.0e12
P0, R_ON_CP, DT = 1.0e5, 287.058 / 1005.0, 10.0


def torch_composite(state, w, rho, dz, dt):
    """tests/kid_advect_ref.py in torch, on device tensors: `sum` of every member of `state`."""
    import torch
    nz = rho.shape[0]
    rf = torch.cat([rho[:1], 0.5 * (rho[:-1] + rho[1:]), rho[-1:]])
    M = rf[None, :] * w
    up = w[:, 1:nz] >= 0
    c = (w[:, 1:nz].abs() * dt) / torch.where(up, dz[None, :-1], dz[None, 1:])
    hc = 0.5 * (1.0 - c)
    den = (rho * dz)[None, :]
    dM = (M[:, 1:] - M[:, :-1]) / den
    f = torch.arange(1, nz, device=w.device)[None, :]
    inside = torch.where(up, f >= 2, f + 1 < nz)
    out = {}
    for k, q in state.items():
        pad = torch.nn.functional.pad(q, (2, 1))                     # pad[:, i + 2] = q[:, i]
        qm1, q0, qm2, qp1 = pad[:, 2:nz + 1], pad[:, 3:nz + 2], pad[:, 1:nz], pad[:, 4:nz + 3]      # of faces 1 .. nz-1
        qu, qd, quu = torch.where(up, qm1, q0), torch.where(up, q0, qm1), torch.where(up, qm2, qp1)
        dq, b = qd - qu, qu - quu
        bd = b * dq
        s = torch.where(inside & (bd > 0), (2.0 * bd) / torch.where(bd > 0, b + dq, torch.ones_like(bd)), torch.zeros_like(bd))
        qf = torch.cat([q[:, :1], qu + hc * s, q[:, -1:]], 1)
        F = M * qf
        out[k] = -((F[:, 1:] - F[:, :-1]) / den) + q * dM
    return out


def measure(a, ncol, lines):
    import numpy as np
    import torch
    import cases
    from kid_amd import KID_FIELDS, ThompsonMP

    def say(s):
        print(s)
        lines.append(s)

    m = ThompsonMP(iiwarm=False, device=0)
    st = cases.config3(ncol)
    exner = (st["p"] / P0) ** R_ON_CP
    F = {k: st[k] for k in KID_FIELDS[1:]}
    F["theta"] = st["t"] / exner
    rho = 0.622 * st["p"][0] / (287.04 * st["t"][0] * (st["qv"][0] + 0.622))
    rng = np.random.Generator(np.random.PCG64(15))
    f = np.arange(NZ + 1) / float(NZ)
    w = rng.uniform(0.3, 1.0, (ncol, 1)) * 8.0 * np.sin(np.pi * f * rng.integers(1, 3, (ncol, 1)))[:, :]
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")   # noqa: E731
    first = {k: cu(F[k]) for k in KID_FIELDS}
    state = {k: v.clone() for k, v in first.items()}
    dw, drho, ddz, dex = cu(w), cu(rho), cu(st["dz"][0]), cu(exner)

    def restore():
        for k in KID_FIELDS:
            state[k].copy_(first[k])

    o_sum = m.kid_advect(state, dw, drho, ddz, DT, want="sum", courant=True)
    o_ad = m.kid_advect(state, dw, drho, ddz, DT, want=("adv", "div"))
    work = m.kid_workspace(ncol, NZ, torch.float64)
    mphys = m.kid_interface(state, DT, P0, R_ON_CP, dex, ddz, adv=o_sum["sum"], work=work)
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")

    def run_step():
        m.kid_advect(state, dw, drho, ddz, DT, want="sum", courant=True, out=o_sum)
        m.kid_interface(state, DT, P0, R_ON_CP, dex, ddz, adv=o_sum["sum"], work=work, out=mphys)
        m.kid_update(state, DT, o_sum["sum"], mphys)
        ppt.add_(mphys["ppt"])

    # name -> (call, algorithmic profiles per column or None, changes the state)
    variants = {
        "advect_sum": (lambda: m.kid_advect(state, dw, drho, ddz, DT, want="sum", courant=True, out=o_sum), 18, False),
        "advect_adv_div": (lambda: m.kid_advect(state, dw, drho, ddz, DT, want=("adv", "div"), out=o_ad), 27, False),
        "update": (lambda: m.kid_update(state, DT, o_sum["sum"], mphys), 36, True),
        "kid_interface": (lambda: m.kid_interface(state, DT, P0, R_ON_CP, dex, ddz, adv=o_sum["sum"], work=work, out=mphys), None, False),
        "run_step": (run_step, None, True),
        "composite": (lambda: torch_composite(state, dw, drho, ddz, DT), None, False),
    }
    comp = torch_composite(state, dw, drho, ddz, DT)
    diff = {k: float((o_sum["sum"][k] - comp[k]).abs().max() / o_sum["sum"][k].abs().max().clamp(min=1e-300)) for k in KID_FIELDS}
    say("ncol=%-6d composite - advect_sum, max |difference| / max |profile|: %s   courant max %.3f"
        % (ncol, "  ".join("%s %.1e" % kv for kv in diff.items()), float(o_sum["courant"].max())))
    for _ in range(a.warmup):
        for fn, _n, _c in variants.values():
            fn()
    restore()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, (fn, _n, changes) in variants.items():
            if changes:
                restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"ncol": ncol, "nz": NZ, "reps": a.reps, "composite_max_diff_over_max": max(diff.values())}
    for k, t in times.items():
        res[k] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
        nprof = variants[k][1]
        extra = ""
        if nprof is not None:
            res[k]["algo_bytes_per_column"] = nprof * NZ * 8
            res[k]["share_of_8TBs"] = res[k]["algo_bytes_per_column"] * ncol / (res[k]["ms_median"] * 1e-3) / HBM_PEAK
            extra = "   %6d B/column -> %5.1f %% of 8 TB/s" % (res[k]["algo_bytes_per_column"], 100.0 * res[k]["share_of_8TBs"])
        say("ncol=%-6d %-14s median %8.4f ms   min %8.4f   max %8.4f%s" % (ncol, k, res[k]["ms_median"], min(t), max(t), extra))
    ms = {k: res[k]["ms_median"] for k in variants}
    res["advect_sum_over_composite"] = ms["advect_sum"] / ms["composite"]
    res["kinematic_share_of_run_step"] = (ms["run_step"] - ms["kid_interface"]) / ms["run_step"]
    say("ncol=%-6d advect_sum %.3fx composite; a run step is %.4f ms, of which advection + update + accumulation add %.1f %% over "
        "kid_interface alone (%.4f ms)" % (ncol, res["advect_sum_over_composite"], ms["run_step"],
                                           100.0 * res["kinematic_share_of_run_step"], ms["kid_interface"]))
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ncols", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--lib", default=None, help="another build of the library (an A/B of the kernel)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_kid_advect.txt"))
    a = ap.parse_args()
    import torch
    import kid_amd
    if not torch.cuda.is_available():
        sys.exit("bench_kid_advect: no GPU visible (this measurement has no CPU path)")
    if a.lib:
        kid_amd.load_library(a.lib)
    m = kid_amd.ThompsonMP(iiwarm=True, device=0)
    lines = ["# tools/bench_kid_advect.py  %s  %s%s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0),
                                                         "  --lib " + a.lib if a.lib else ""),
             "# fingerprint: %s" % m.kernel_fingerprint()]
    m.close()
    results = [measure(a, n, lines) for n in a.ncols]
    lines.append(json.dumps({"bench": "kid_advect", "device": torch.cuda.get_device_name(0), "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
