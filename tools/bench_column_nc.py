#!/usr/bin/env python
"""tools/bench_column_nc.py -- what a droplet number per column (kidmp_set_column_nc) costs on one MI355X.

Workloads: BASELINE config 2 (10^4 warm-rain columns) and config 3 (10^5 mixed-phase columns), 120 levels, fp64, at
bench.py's sizes, state in HBM.  Per workload, in ONE process:
  plain     kidmp_batch_step_device with nothing bound: thompson_column_step<..., NCCOL = false>
  nccol     the same call with a UNIFORM array equal to the context's set_Nc bound: the NCCOL = true instantiation doing
            identical physics (the end states are compared bit for bit)
  ensemble  a 7-value log-spaced ensemble, 25 ... 1600 cm**-3, cycling by column index: every workgroup of 4 columns holds
            4 different values (different physics: reported, not compared)
The variants alternate in blocks of --block steps, --blocks times each; before every block the state is put back to the
same initial columns (untimed), so all variants step the same inputs; a block is timed with device events around it.
Prints one JSON line and writes a readable report (--out, default profiles/r07_column_nc.txt).  No threshold is applied:
the figures are for the record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = {"config2": 10000, "config3": 100000}            # bench.py's DEFAULT_NCOL
ENSEMBLE = (25.0, 50.0, 100.0, 200.0, 400.0, 800.0, 1600.0)


def measure(name, a):
    import numpy as np
    import torch
    import cases
    from kid_amd import ThompsonMP

    ncol = a.ncol or SIZES[name]
    iiwarm = name == "config2"
    st0 = cases.config2(ncol) if iiwarm else cases.config3(ncol)
    m = ThompsonMP(iiwarm=iiwarm, device=0)
    init = {k: torch.from_numpy(v).to("cuda:0") for k, v in st0.items()}
    dev = {k: v.clone() for k, v in init.items()}
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")
    bind = {"plain": None, "nccol": np.full(ncol, 100.0),
            "ensemble": np.array([ENSEMBLE[c % len(ENSEMBLE)] for c in range(ncol)])}

    def reset():
        for k in dev:
            dev[k].copy_(init[k])
        ppt.zero_()

    def block(variant, steps):
        m.set_column_nc(bind[variant])               # allocates and synchronises: outside the timed region
        reset()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            m.batch_step(dev, 10.0, ppt)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    for v in bind:
        block(v, a.warmup)
    times = {v: [] for v in bind}
    end = {}
    for _ in range(a.blocks):                        # alternating: a block of every variant, then the next round
        for v in bind:
            times[v].append(block(v, a.block))
            if v not in end:
                end[v] = ({k: t.clone() for k, t in dev.items()}, ppt.clone())
    same = bool(all(torch.equal(end["plain"][0][k], end["nccol"][0][k]) for k in dev)
                and torch.equal(end["plain"][1], end["nccol"][1]))
    rain = end["ensemble"][1][:, 0].cpu().numpy()
    members = {("%g" % v): float(rain[i::len(ENSEMBLE)].mean()) for i, v in enumerate(ENSEMBLE)}
    m.set_column_nc(None)
    m.close()
    res = {"workload": name, "ncol": ncol, "nz": cases.NZ, "steps_per_block": a.block, "blocks": a.blocks,
           "warmup_steps": a.warmup, "plain_equals_uniform_nccol_bitwise": same, "variants": {},
           "ensemble_mean_surface_rain_by_set_Nc": members}
    for v, t in times.items():
        res["variants"][v] = {"ms_per_step_blocks": [round(x, 5) for x in t], "ms_min": round(min(t), 5),
                              "ms_median": round(float(np.median(t)), 5), "ms_max": round(max(t), 5),
                              "spread_rel": round((max(t) - min(t)) / float(np.median(t)), 5),
                              "column_steps_per_s_at_median": round(ncol / (float(np.median(t)) * 1e-3), 1)}
    p = res["variants"]["plain"]
    for v in ("nccol", "ensemble"):
        res["variants"][v]["over_plain_median"] = round(res["variants"][v]["ms_median"] / p["ms_median"], 5)
        res["variants"][v]["over_plain_min"] = round(res["variants"][v]["ms_min"] / p["ms_min"], 5)
    return res


def report(results, device):
    lines = ["droplet number per column (kidmp_set_column_nc): cost of the NCCOL instantiations, fp64, nz = 120",
             "device: %s" % device,
             "variants alternate in one process, every block starts from the same columns; ms per step over the blocks", ""]
    for r in results:
        lines.append("%s, %d columns, %d blocks of %d steps per variant; plain == uniform nccol bit for bit: %s"
                     % (r["workload"], r["ncol"], r["blocks"], r["steps_per_block"], r["plain_equals_uniform_nccol_bitwise"]))
        lines.append("  %-9s %10s %10s %10s %8s %12s" % ("variant", "min", "median", "max", "spread", "over plain"))
        for v, x in r["variants"].items():
            lines.append("  %-9s %10.5f %10.5f %10.5f %7.2f%% %12s"
                         % (v, x["ms_min"], x["ms_median"], x["ms_max"], 100 * x["spread_rel"],
                            "%.4f" % x["over_plain_median"] if "over_plain_median" in x else "1"))
        lines.append("  ensemble, mean surface rain after the block by set_Nc (cm**-3): "
                     + ", ".join("%s: %.4e" % kv for kv in r["ensemble_mean_surface_rain_by_set_Nc"].items()))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="config2,config3")
    ap.add_argument("--ncol", type=int, default=0, help="columns (default: bench.py's size of the workload)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_column_nc.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_column_nc: no GPU visible (this measurement has no CPU path)")
    results = [measure(w, a) for w in a.workloads.split(",")]
    print(json.dumps({"metric": "per-column droplet number, NCCOL against the plain kernel", "results": results}), flush=True)
    text = report(results, torch.cuda.get_device_name(0))
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
