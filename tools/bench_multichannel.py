#!/usr/bin/env python
"""tools/bench_multichannel.py -- time the multi-channel radiometer and cloud radar (include/kidmp_multichannel.h, one
launch of kidmp::k_radiometer_multi / k_mie_radar_multi for nch channels) on one MI355X against a loop of nch launches of
the single-channel entries on the same state, in the same process.

Workload, fp64, state in HBM, 10^5 and 10^4 columns x 120 levels: mixed-phase BASELINE config 3 after one column step (the
state of tools/bench_radiometer.py) with dz = 100 m, the sixteen illustrative configurations of tests/multichannel_cases.py
on the scheme's own 100 bins per species (300 bins), a closure per channel.  All variants take turns launch by launch,
warmed up; every call (one multi-channel launch, or the whole loop of nch single launches) is timed with device events of
its own and the median of --reps (30) is reported with the minimum and maximum.  Groups of variants:
  rad_toa     radiometer, tb_toa alone, nch in 1 2 4 8 13 16
  rad_optics  radiometer, k_abs and k_bsc alone, the same nch
  rad_all     radiometer, all nine outputs, nch in 1 2 4
  radar_dbz   mie_radar, dbz alone, nch in 1 2 3
  radar_all   mie_radar, all fourteen outputs, nch in 1 2 3
Per group and nch: multi, loop and the ratio loop/multi (above 1: the multi-channel call is faster); at nch = 1 the loop is
the single-channel entry itself.  Prints one line per measurement, the tile per kind, the --fingerprint line (registers per
instantiation, as the build reported them) and ONE JSON line at the end; the lines also go to --out."""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NZ = 120
GROUPS = {"rad_toa": (1, 2, 4, 8, 13, 16), "rad_optics": (1, 2, 4, 8, 13, 16), "rad_all": (1, 2, 4), "radar_dbz": (1, 2, 3), "radar_all": (1, 2, 3)}


def measure(a, ncol, lines):
    import torch
    import cases
    import multichannel_cases as mcc
    from kid_amd import MIE_INPUTS, MIE_NAMES, RADIOMETER_NAMES, MieCfg, RadiometerCfg, ThompsonMP

    def say(s):
        print(s, flush=True)
        lines.append(s)

    m = ThompsonMP(iiwarm=False, device=0)
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in cases.config3(ncol).items()}
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                     # the state after one step
    ins = {k: dev[k] for k in MIE_INPUTS}
    dz = torch.full((NZ,), 100.0, dtype=torch.float64, device="cuda:0")
    cfgs = [MieCfg(**kw) for kw in mcc.configs()]
    rad = [m.radiometer_table(c) for c in cfgs]
    mie = [m.mie_table(c) for c in cfgs[:max(GROUPS["radar_all"])]]
    rcfgs = [RadiometerCfg(**kw) for kw in mcc.rcfgs()]
    want = {"rad_toa": ("tb_toa",), "rad_optics": ("k_abs", "k_bsc"), "rad_all": RADIOMETER_NAMES, "radar_dbz": ("dbz",), "radar_all": MIE_NAMES}

    def multi(g, n):
        if g.startswith("rad_"):
            return lambda: m.radiometer_multi(rad[:n], ins, None if g == "rad_optics" else dz, rcfgs=rcfgs[:n], want=want[g])
        return lambda: m.mie_radar_multi(mie[:n], ins, dz if g == "radar_all" else None, want=want[g])

    def loop(g, n):
        if g.startswith("rad_"):
            return lambda: [m.radiometer(rad[c], ins, None if g == "rad_optics" else dz, rcfg=rcfgs[c], want=want[g]) for c in range(n)]
        return lambda: [m.mie_radar(mie[c], ins, dz if g == "radar_all" else None, want=want[g]) for c in range(n)]

    variants = {}
    for g in a.groups:
        for n in GROUPS[g]:
            variants[(g, n, "multi")], variants[(g, n, "loop")] = multi(g, n), loop(g, n)
    # the two sides give the same bits: checked once per group at its largest nch
    for g in a.groups:
        n = max(GROUPS[g])
        got, ref = variants[(g, n, "multi")](), variants[(g, n, "loop")]()
        same = all(torch.equal(got[k][c].view(torch.int64), ref[c][k].view(torch.int64)) for k in got for c in range(n))
        say("ncol=%-6d %-10s nch=%-2d multi == loop, bit for bit: %s" % (ncol, g, n, same))
        del got, ref
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
    res = {"ncol": ncol, "nz": NZ, "reps": a.reps, "rows": []}
    for g in a.groups:
        for n in GROUPS[g]:
            tm, tl = times[(g, n, "multi")], times[(g, n, "loop")]
            row = {"group": g, "nch": n, "multi_ms": statistics.median(tm), "multi_min": min(tm), "multi_max": max(tm),
                   "loop_ms": statistics.median(tl), "loop_min": min(tl), "loop_max": max(tl)}
            row["loop/multi"] = row["loop_ms"] / row["multi_ms"]
            res["rows"].append(row)
            say("ncol=%-6d %-10s nch=%-2d multi %9.4f ms (%9.4f .. %9.4f)   loop %9.4f ms (%9.4f .. %9.4f)   loop/multi %6.3f%s" % (
                ncol, g, n, row["multi_ms"], min(tm), max(tm), row["loop_ms"], min(tl), max(tl), row["loop/multi"],
                "" if row["loop/multi"] > 1.0 else "   <-- not faster than the loop"))
    for t in rad + mie:
        t.close()
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ncols", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--groups", nargs="+", default=list(GROUPS), choices=list(GROUPS))
    ap.add_argument("--lib", default=None, help="another build of libkidmp.so to measure (a tile candidate)")
    ap.add_argument("--fingerprint", default="", help="the fingerprint line to record: registers and tile per instantiation, as the build reported them")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_multichannel.txt"))
    a = ap.parse_args()
    import torch
    import kid_amd
    from kid_amd import multichannel_tile
    if not torch.cuda.is_available():
        sys.exit("bench_multichannel: no GPU visible (this measurement has no CPU path)")
    if a.lib:
        kid_amd.load_library(a.lib)
    lines = ["# tools/bench_multichannel.py  %s  %s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0))]
    tiles = {k: multichannel_tile(k, NZ) for k in ("radiometer", "radar")}
    lines.append("tile at nz = %d: radiometer %d, radar %d" % (NZ, tiles["radiometer"], tiles["radar"]))
    print(lines[-1])
    results = [measure(a, n, lines) for n in a.ncols]
    if a.fingerprint:
        lines.append("fingerprint: " + a.fingerprint)
        print(lines[-1])
    lines.append(json.dumps({"bench": "multichannel", "device": torch.cuda.get_device_name(0), "tiles": tiles, "fingerprint": a.fingerprint,
                             "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
