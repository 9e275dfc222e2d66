#!/usr/bin/env python
"""tools/bench_radiometer.py -- time the radiometer (kidmp_radiometer_device, one launch of kidmp::k_radiometer) on one
MI355X beside the cloud radar's dbz of the same state in the same context and a torch composite of the same numbers.

Workload, fp64, state in HBM, 10^5 and 10^4 columns x 120 levels: mixed-phase BASELINE config 3 after one column step (the
state of tools/bench_mie_radar.py) with dz = 100 m, tables at 3.19 mm on the scheme's own 100 bins per species (300 bins).
All variants run in ONE process, warmed up, taking turns launch by launch; every launch is timed with device events of its
own and the median of --reps (30) launches is reported with the minimum and maximum beside it.  Variants:
  rad_all        radiometer, all nine outputs
  rad_toa        radiometer, tb_toa alone (the optics, the layers and both scans; one store per column)
  rad_optics     radiometer, k_abs and k_bsc alone (no layer, no scan)
  mie_dbz        mie_radar, dbz alone, on the same state: the nearest older kernel (five sums per bin against three)
  composite      k_abs, k_bsc, refl, trans, tb_toa and tb_ground from torch operations on the device tensors: the load over
                 [ncol, nz], the three sums as [columns, nz, bins] tensors in chunks of columns, and a sequential adding
                 loop over the levels at the Python level (checked against rad_all once); timed --composite-reps times
rad_all - rad_optics is what the layers and the scans cost.  Prints one line per variant, the fingerprint line (registers
per number of level groups, LDS, scratch; read from the library with --fingerprint, else left to the caller) and ONE JSON
line at the end; the lines also go to --out (profiles/r25_radiometer.txt) under a header with the date."""
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
COL_CHUNK = 2048
# illustrative permittivities near 94 GHz (tests/test_gpu_mie_radar.py)
CFG = dict(wavelength=3.19e-3, eps_w=complex(7.7, 14.2), eps_i=complex(3.17, 0.01), rho_w=1000.0, rho_i=917.0, kw2=0.75)
RCFG = dict(mu=0.6, emissivity=0.85, t_cosmic=2.725)


def torch_composite(c, dev, table, kc, rho_w, dz):
    """tests/radiometer_ref.py in torch, on device tensors [ncol, nz], with sequential adding from both ends."""
    import torch
    import refl_oracle as ro
    from bench_mie_radar import torch_load
    mu, em, tc = RCFG["mu"], RCFG["emissivity"], RCFG["t_cosmic"]
    names = ("k_abs", "k_bsc", "refl", "trans")
    out = {n: torch.empty_like(dev["t"]) for n in names}
    out["tb_toa"], out["tb_ground"] = torch.empty_like(dev["t"][:, 0]), torch.empty_like(dev["t"][:, 0])
    ncol, nz = dev["t"].shape

    def combine(A, B):
        d = 1.0 - A[0] * B[1]
        return (B[0] + B[2] * B[2] * A[0] / d, A[1] + A[2] * A[2] * B[1] / d, A[2] * B[2] / d, B[3] + B[2] * (A[3] + A[0] * B[4]) / d,
                A[4] + A[2] * (B[4] + B[1] * A[3]) / d)

    for lo in range(0, ncol, COL_CHUNK):
        d = {k: v[lo:lo + COL_CHUNK] for k, v in dev.items()}
        rho, species, density = torch_load(c, d)
        kabs, kbsc = torch.zeros_like(rho), torch.zeros_like(rho)
        for x, (has, _, rq) in species.items():
            D, dD, rows = table[x]
            n = torch.where(has[..., None], density(x, D, dD), 0.0)
            A, S, M = ((n * rows[i]).sum(dim=2) for i in range(3))
            ok = has & (M > 0)
            kabs = kabs + torch.where(ok, rq * A / M, 0.0)
            kbsc = kbsc + torch.where(ok, rq * S / M, 0.0)
        kabs = torch.where(d["qc"] > ro.R1, kabs + kc * (rho * d["qc"] / rho_w), kabs)
        ta, b = kabs * dz, kbsc * dz
        x = torch.sqrt(ta * (ta + 2.0 * b))
        e, f = torch.exp(-x / mu), -torch.expm1(-x / mu)
        S = torch.where(ta > 0, (ta + b) + x, 1.0)
        G, H = b / S, (ta + x) / S
        p, q = H + G * f, 1.0 + G * e
        gen, cb = ta > 0, b / mu
        R = torch.where(gen, G * f * (1.0 + e) / (p * q), cb / (1.0 + cb))
        T = torch.where(gen, H * (1.0 + G) * e / (p * q), 1.0 / (1.0 + cb))
        E = torch.where(gen, H * f / q, 0.0) * d["t"]
        one, zero = torch.ones_like(R[:, 0]), torch.zeros_like(R[:, 0])
        down = (zero, zero, one, zero, zero)                                        # the stack above, from the top down
        for k in range(nz - 1, -1, -1):
            down = combine((R[:, k], R[:, k], T[:, k], E[:, k], E[:, k]), down)
        up = (zero, zero, one, zero, zero)                                          # the stack below, from the surface up
        for k in range(nz):
            up = combine(up, (R[:, k], R[:, k], T[:, k], E[:, k], E[:, k]))
        ts, rs = d["t"][:, 0], 1.0 - em
        sl = slice(lo, lo + COL_CHUNK)
        out["tb_ground"][sl] = ((down[4] + down[2] * tc) + down[1] * (em * ts)) / (1.0 - rs * down[1])
        ds = 1.0 - rs * up[1]
        out["tb_toa"][sl] = (up[3] + up[2] * (em * ts + rs * up[4]) / ds) + (up[0] + up[2] * up[2] * rs / ds) * tc
        for n, v in zip(names, (kabs, kbsc, R, T)):
            out[n][sl] = v
    return out


def measure(a, c, ncol, lines):
    import torch
    import cases
    import mie_radar_ref as ref
    from kid_amd import MIE_INPUTS, RADIOMETER_NAMES, MieCfg, RadiometerCfg, ThompsonMP

    def say(s):
        print(s)
        lines.append(s)

    m = ThompsonMP(iiwarm=False, device=0)
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in cases.config3(ncol).items()}
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                     # the state after one step
    ins = {k: dev[k] for k in MIE_INPUTS}
    dz = torch.full((NZ,), 100.0, dtype=torch.float64, device="cuda:0")
    table, mie = m.radiometer_table(MieCfg(**CFG)), m.mie_table(MieCfg(**CFG))
    rows = {x: tuple(torch.from_numpy(g).to("cuda:0") for g in table.get(x)) for x in ref.SPECIES}
    kc = ref.cloud_factor(ref.cfg_of(**CFG))
    r = RadiometerCfg(**RCFG)
    variants = {
        "rad_all": lambda: m.radiometer(table, ins, dz, rcfg=r, want=RADIOMETER_NAMES),
        "rad_toa": lambda: m.radiometer(table, ins, dz, rcfg=r, want=("tb_toa",)),
        "rad_optics": lambda: m.radiometer(table, ins, rcfg=r, want=("k_abs", "k_bsc")),
        "mie_dbz": lambda: m.mie_radar(mie, ins, want=("dbz",)),
        "composite": lambda: torch_composite(c, ins, rows, kc, CFG["rho_w"], dz),
    }
    got, comp = variants["rad_all"](), variants["composite"]()
    diff = {n: float(((got[n] - comp[n]).abs() / comp[n].abs().clamp(min=1e-300)).max()) for n in comp}
    say("ncol=%-6d tb_toa %.2f .. %.2f K   tb_ground %.2f .. %.2f K   tau_abs up to %.2f" % (
        ncol, float(got["tb_toa"].min()), float(got["tb_toa"].max()), float(got["tb_ground"].min()), float(got["tb_ground"].max()),
        float(got["tau_abs"].max())))
    say("ncol=%-6d composite - rad_all, max relative |difference|: %s" % (ncol, "  ".join("%s %.1e" % kv for kv in diff.items())))
    for _ in range(a.warmup):
        for k, fn in variants.items():
            if k != "composite":
                fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for i in range(a.reps):
        for k, fn in variants.items():
            if k == "composite" and i >= a.composite_reps:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"ncol": ncol, "nz": NZ, "reps": a.reps, "composite_reps": a.composite_reps, "composite_max_diff": diff}
    for k, t in times.items():
        res[k] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
        say("ncol=%-6d %-12s median %9.4f ms   min %9.4f   max %9.4f   (%d launches)" % (ncol, k, res[k]["ms_median"], min(t), max(t), len(t)))
    ms = {k: res[k]["ms_median"] for k in variants}
    res["ratios"] = {"rad_all/mie_dbz": ms["rad_all"] / ms["mie_dbz"], "rad_toa/mie_dbz": ms["rad_toa"] / ms["mie_dbz"],
                     "rad_optics/mie_dbz": ms["rad_optics"] / ms["mie_dbz"], "rad_all/rad_optics": ms["rad_all"] / ms["rad_optics"],
                     "composite/rad_all": ms["composite"] / ms["rad_all"]}
    say("ncol=%-6d ratios: %s" % (ncol, "  ".join("%s %.3f" % kv for kv in res["ratios"].items())))
    table.close()
    mie.close()
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--composite-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ncols", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--fingerprint", default="", help="the fingerprint line to record: registers per NJ, LDS, scratch, as the build reported them")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_radiometer.txt"))
    a = ap.parse_args()
    import torch
    import doppler_ref as ref
    from oracle.oracle import Oracle
    if not torch.cuda.is_available():
        sys.exit("bench_radiometer: no GPU visible (this measurement has no CPU path)")
    o = Oracle(iiwarm=True)
    c = ref.constants(o)
    o.close()
    lines = ["# tools/bench_radiometer.py  %s  %s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0))]
    results = [measure(a, c, n, lines) for n in a.ncols]
    if a.fingerprint:
        lines.append("fingerprint k_radiometer<double, NJ>: " + a.fingerprint)
        print(lines[-1])
    lines.append(json.dumps({"bench": "radiometer", "device": torch.cuda.get_device_name(0), "fingerprint": a.fingerprint, "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
