#!/usr/bin/env python
"""tools/bench_column_summary.py -- time the per-column summary (kidmp_column_summary_device, one launch of
kidmp::k_column_summary) on one MI355X against the other ways to the same 15 numbers per column.

Workloads: BASELINE config 3 (10^5 mixed-phase columns x 120 levels) and config 2 (10^4 warm columns x 120 levels), fp64,
after one column step, state in HBM, a mixed-phase context for both (all ten input profiles present) and the state's own
[ncol, nz] dz.  All variants run in ONE process, warmed up, taking turns launch by launch; every launch is timed with device
events of its own and the median of --reps (30) launches is reported with the minimum and maximum beside it.  Variants:
  summary        kidmp_column_summary_device
  a_outputs      kidmp_column_outputs_device, dbz + radii: the four profiles a composite would start from, nothing reduced
  b_composite    a_outputs followed by the torch reductions that form the same 15 numbers (checked against `summary` once)
  c_download     the ten input profiles and dz copied to page-locked host memory (what a host-side reduction needs first)
Algorithmic bytes per column of `summary`: (input profiles present + dz) * nz * 8 + 128; its share of 8 TB/s is printed.
Prints one line per variant and workload and ONE JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NZ = 120
HBM_PEAK = 8.0e12
R_GAS = 287.04
RE_QC_PRESET = 2.49e-6


def torch_composite(m, dev, dz, cfg):
    """The 15 numbers from column_outputs and torch reductions: [ncol, 16] float64."""
    import torch
    dbz_echo, q_cloud, t_freeze = cfg
    dbz, (re_qc, _, _) = m.column_outputs(dev, dbz=True, radii=True)
    qv = torch.clamp(dev["qv"], min=1e-10)
    rho = 0.622 * dev["p"] / (R_GAS * dev["t"] * (qv + 0.622))
    cw = rho * dev["qc"] * dz
    out = torch.zeros((dbz.shape[0], 16), dtype=torch.float64, device=dbz.device)
    out[:, 0] = (rho * qv * dz).sum(1)
    out[:, 1] = cw.sum(1)
    for s, k in ((2, "qr"), (3, "qi"), (4, "qs"), (5, "qg")):
        out[:, s] = (rho * dev[k] * dz).sum(1)
    out[:, 6] = torch.where(re_qc != RE_QC_PRESET, 1.5 * cw / (1000.0 * re_qc), torch.zeros_like(cw)).sum(1)
    top = torch.cumsum(dz, 1)
    bottom, mid = top - dz, top - 0.5 * dz
    nan = torch.full_like(out[:, 0], float("nan"))
    k = torch.arange(dbz.shape[1], device=dbz.device)[None, :]
    nz = dbz.shape[1]

    def lowest(mask, z):
        idx = torch.where(mask, k, nz).min(1).values
        return torch.where(idx < nz, z.gather(1, idx.clamp(max=nz - 1)[:, None])[:, 0], nan)

    def highest(mask, z):
        idx = torch.where(mask, k, -1).max(1).values
        return torch.where(idx >= 0, z.gather(1, idx.clamp(min=0)[:, None])[:, 0], nan)

    mx = dbz.max(1).values
    out[:, 7] = mx
    out[:, 8] = lowest(dbz == mx[:, None], mid)
    out[:, 9] = highest(dbz >= dbz_echo, top)
    out[:, 10] = dbz[:, 0]
    cloudy = dev["qc"] + dev["qi"] > q_cloud
    out[:, 11] = lowest(cloudy, bottom)
    out[:, 12] = highest(cloudy, top)
    out[:, 13] = cloudy.sum(1).to(torch.float64)
    out[:, 14] = lowest(dev["t"] < t_freeze, mid)
    return out


def measure(a, name, state, ncol):
    import numpy as np
    import torch
    from kid_amd import SUMMARY_INPUTS, ThompsonMP
    from kid_amd.summary import DEFAULT_CFG

    m = ThompsonMP(iiwarm=False, device=0)
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in state.items()}
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                 # the state after one step
    dz = dev["dz"]
    ins = {k: dev[k] for k in SUMMARY_INPUTS}
    out = torch.empty((ncol, 16), dtype=torch.float64, device="cuda:0")
    pinned = {k: torch.empty(v.shape, dtype=v.dtype).pin_memory() for k, v in list(ins.items()) + [("dz", dz)]}

    def download():
        for k, h in pinned.items():
            h.copy_(dz if k == "dz" else ins[k], non_blocking=True)

    variants = {
        "summary": lambda: m.column_summary(ins, dz, out=out),
        "a_outputs": lambda: m.column_outputs(dev, dbz=True, radii=True),
        "b_composite": lambda: torch_composite(m, dev, dz, DEFAULT_CFG),
        "c_download": download,
    }
    # the composite forms the same numbers (to rounding: its sums run in torch's order)
    got, comp = m.column_summary(ins, dz).cpu().numpy(), torch_composite(m, dev, dz, DEFAULT_CFG).cpu().numpy()
    same_nan = bool(np.array_equal(np.isnan(got), np.isnan(comp)))
    rel = float(np.nanmax(np.abs(got - comp) / np.maximum(np.abs(got), 1e-300)))
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    nprof = len(SUMMARY_INPUTS) + 1
    algo_bytes = nprof * NZ * 8 + 128
    res = {"workload": name, "ncol": ncol, "nz": NZ, "reps": a.reps, "composite_same_nan": same_nan, "composite_max_rel_diff": rel,
           "summary_algo_bytes_per_column": algo_bytes}
    for k, t in times.items():
        res[k] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
        print("%-8s ncol=%-6d %-12s median %8.4f ms   min %8.4f   max %8.4f" % (name, ncol, k, res[k]["ms_median"], min(t), max(t)))
    ms = res["summary"]["ms_median"]
    res["summary_share_of_8TBs"] = algo_bytes * ncol / (ms * 1e-3) / HBM_PEAK
    res["summary_columns_per_s"] = ncol / (ms * 1e-3)
    print("%-8s summary: %d algorithmic bytes per column -> %.1f %% of 8 TB/s, %.3g columns/s; %.2fx a_outputs, %.2fx b_composite, "
          "%.2fx c_download; composite agrees to %.1e relative, NaNs alike: %s"
          % (name, algo_bytes, 100.0 * res["summary_share_of_8TBs"], res["summary_columns_per_s"], ms / res["a_outputs"]["ms_median"],
             ms / res["b_composite"]["ms_median"], ms / res["c_download"]["ms_median"], rel, same_nan))
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ncol3", type=int, default=100000)
    ap.add_argument("--ncol2", type=int, default=10000)
    a = ap.parse_args()
    import torch
    import cases
    if not torch.cuda.is_available():
        sys.exit("bench_column_summary: no GPU visible (this measurement has no CPU path)")
    results = [measure(a, "config3", cases.config3(a.ncol3), a.ncol3), measure(a, "config2", cases.config2(a.ncol2), a.ncol2)]
    print(json.dumps({"bench": "column_summary", "device": torch.cuda.get_device_name(0), "results": results}))


if __name__ == "__main__":
    main()
