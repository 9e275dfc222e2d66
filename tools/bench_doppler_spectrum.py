#!/usr/bin/env python
"""tools/bench_doppler_spectrum.py -- time the Doppler spectrum (kidmp_doppler_spectrum_device, one launch of
kidmp::k_doppler_spectrum) on one MI355X beside the store roofline, beside what the library offered before it
(size_spectra of rain, snow and graupel plus doppler_moments on the same state), and beside a torch composite that
scatters the same bins.

Workloads: 10^4 and 10^3 mixed-phase columns x 120 levels (BASELINE config 3), fp64, after one column step, state in HBM,
the scheme's own 100 bins per species, the velocity grid -2 .. 14 m s-1 in nv = 64 and 256 bins, w of the case.  All
variants run in ONE process, warmed up, taking turns launch by launch, into tensors allocated beforehand; every launch is
timed with device events of its own and the median of --reps (30) launches is reported with the minimum and maximum.
Variants, per nv:
  total           the total spectrum alone
  all4            total, rain, snow and graupel (four passes inside the one launch)
  spectra+moments size_spectra(r, s, g) followed by doppler_moments: the two launches a caller had before
  composite       the total spectrum from torch operations: z_b and the positions of all bins of a species at once,
                  scatter_add along the bin axis (the level factors come from tests/doppler_spectrum_ref.py, formed on the
                  host beforehand and not timed); its distance from the kernel's spectrum is printed
Store roofline of a spectrum: nv * nz * 8 B per spectrum and column at 8 TB/s; the share of it is printed.  Prints one
line per variant and workload and ONE JSON line at the end; the lines also go to --out (profiles/r20_doppler_spectrum.txt)
under a header with the date and the library's fingerprint.  --lib names another build of the library (a tile variant)."""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NZ, NB = 120, 100
HBM_PEAK = 8.0e12
V0, VSPAN = -2.0, 16.0


def torch_composite(lv, grids, w, v0, dv, nv):
    """The total spectrum [ncol, nv, nz] with below and above from the level factors `lv` (tensors [ncol, nz]) and the
    grids: the formulas of include/kidmp_dspectrum.h, every bin of a species at once, scatter_add over the slots."""
    import torch
    import doppler_ref as dr
    import doppler_spectrum_ref as r

    def exp_neg(x):
        return torch.where(x <= r.EXP_MAX, torch.exp(-torch.clamp(x, max=r.EXP_MAX)), torch.zeros_like(x))

    ncol, nz = w.shape
    S = torch.zeros((ncol, nv + 2, nz), dtype=torch.float64, device=w.device)
    idv = 1.0 / dv
    for x in "rsg":
        D, dD = grids[x][0][None, :, None], grids[x][1][None, :, None]
        p = {k: v[:, None, :] for k, v in lv[x].items()}
        if x == "s":
            z = (p["zs"] * (dr.Kap0 * exp_neg(p["x0"] * D) + (p["k1"] * D ** dr.mu_s) * exp_neg(p["x1"] * D))) * (D ** 4 * dD)
            vfac = dr.av_s * D ** dr.bv_s * exp_neg(dr.fv_s * D)
        else:
            z = (p["A"] * exp_neg(p["lam"] * D)) * (D ** 6 * dD)
            vfac = dr.av_r * D * exp_neg(dr.fv_r * D) if x == "r" else dr.av_g * D ** dr.bv_g
        z = torch.where(p["present"], z, torch.zeros_like(z))
        pos = ((lv["rhof"][:, None, :] * vfac - w[:, None, :]) - v0) * idv
        q = torch.where(pos >= -1.0, torch.clamp(pos, max=float(nv)), torch.full_like(pos, -1.0))
        j = torch.clamp(torch.floor(q), max=nv - 1.0)
        f = q - j
        j = j.long() + 1
        S.scatter_add_(1, j, (1.0 - f) * z)
        S.scatter_add_(1, j + 1, f * z)
    return S


def measure(a, ncol, lines):
    import numpy as np
    import torch
    import cases
    import doppler_ref as dref
    import doppler_spectrum_ref as ref
    from kid_amd import DOPPLER_NAMES, DSPECTRUM_INPUTS, SPECTRA_INPUTS, ThompsonMP, default_grid
    from oracle.oracle import Oracle

    def say(s):
        print(s)
        lines.append(s)

    m = ThompsonMP(iiwarm=False, device=0)
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in cases.config3(ncol).items()}
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                 # the state after one step
    ins = {k: dev[k] for k in DSPECTRUM_INPUTS}
    sins = {k: dev[k] for k in SPECTRA_INPUTS}
    w = dev["w"]
    grids = {x: tuple(torch.from_numpy(g).to("cuda:0") for g in default_grid(m, x)) for x in "rsg"}
    o = Oracle(iiwarm=True)
    consts = dref.constants(o)
    o.close()
    lv_np = ref.levels(consts, {k: ins[k].cpu().numpy() for k in DSPECTRUM_INPUTS})
    up = lambda v: torch.from_numpy(np.ascontiguousarray(np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0))).to("cuda:0")   # noqa: E731
    lv = {"rhof": up(lv_np["rhof"])}
    for x in "rsg":
        lv[x] = {k: up(v) for k, v in lv_np[x].items() if k not in ("ze", "Mrat", "present")}
        lv[x]["present"] = torch.from_numpy(np.ascontiguousarray(lv_np[x]["present"])).to("cuda:0")
    sp_out = {x: torch.empty((ncol, NB, NZ), dtype=torch.float64, device="cuda:0") for x in "rsg"}
    results = []
    for nv in a.nvs:
        dv = VSPAN / nv
        names = ("total", "rain", "snow", "graupel")
        out = {n: torch.empty((ncol, nv, NZ), dtype=torch.float64, device="cuda:0") for n in names}

        def before():
            m.size_spectra(sins, ("r", "s", "g"), out=sp_out)
            return m.doppler_moments(ins, w, DOPPLER_NAMES)

        variants = {
            "total": (lambda: m.doppler_spectrum(ins, V0, dv, nv, w, want=("total",), out=out), 1),
            "all4": (lambda: m.doppler_spectrum(ins, V0, dv, nv, w, want=names, out=out), 4),
            "spectra+moments": (before, 0),
            "composite": (lambda: torch_composite(lv, grids, w, V0, dv, nv), 1),
        }
        got = m.doppler_spectrum(ins, V0, dv, nv, w, want=("total", "below", "above"))
        comp = torch_composite(lv, grids, w, V0, dv, nv)
        scale = (got["total"].sum(dim=1) + got["below"] + got["above"]).clamp(min=1e-300)[:, None, :]
        full = torch.cat([got["below"][:, None, :], got["total"], got["above"][:, None, :]], dim=1)
        diff = float(((full - comp).abs() / scale).max())
        say("ncol=%-6d nv=%-3d composite - total, max |difference| / (the level's summed echo): %.1e" % (ncol, nv, diff))
        del got, comp, full, scale
        for _ in range(a.warmup):
            for fn, _n in variants.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, (fn, _n) in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
                del r
        res = {"ncol": ncol, "nz": NZ, "nb": NB, "nv": nv, "reps": a.reps, "composite_max_diff_over_level_echo": diff}
        for k, t in times.items():
            res[k] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
            nspec = variants[k][1]
            extra = ""
            if nspec:
                res[k]["store_bytes_per_column"] = nspec * nv * NZ * 8
                res[k]["roofline_ms"] = res[k]["store_bytes_per_column"] * ncol / HBM_PEAK * 1e3
                res[k]["share_of_8TBs"] = res[k]["roofline_ms"] / res[k]["ms_median"]
                extra = "   %7d B/column stored -> roofline %7.4f ms, %5.1f %% of 8 TB/s" % (res[k]["store_bytes_per_column"], res[k]["roofline_ms"],
                                                                                           100.0 * res[k]["share_of_8TBs"])
            say("ncol=%-6d nv=%-3d %-15s median %9.4f ms   min %9.4f   max %9.4f%s" % (ncol, nv, k, res[k]["ms_median"], min(t), max(t), extra))
        ms = {k: res[k]["ms_median"] for k in variants}
        say("ncol=%-6d nv=%-3d total %.3fx composite, %.3fx spectra+moments; all4 %.2fx total"
            % (ncol, nv, ms["total"] / ms["composite"], ms["total"] / ms["spectra+moments"], ms["all4"] / ms["total"]))
        results.append(res)
        del out
    m.close()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ncols", type=int, nargs="+", default=[10000, 1000])
    ap.add_argument("--nvs", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--lib", default=None, help="another build of libkidmp.so (a tile variant)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_doppler_spectrum.txt"))
    a = ap.parse_args()
    import torch
    import kid_amd
    if not torch.cuda.is_available():
        sys.exit("bench_doppler_spectrum: no GPU visible (this measurement has no CPU path)")
    if a.lib:
        kid_amd.load_library(a.lib)
    m = kid_amd.ThompsonMP(iiwarm=True, device=0)
    lines = ["# tools/bench_doppler_spectrum.py  %s  %s%s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0),
                                                             "  --lib %s" % os.path.basename(a.lib) if a.lib else ""),
             "# fingerprint: %s" % m.kernel_fingerprint()]
    m.close()
    results = []
    for n in a.ncols:
        results += measure(a, n, lines)
    lines.append(json.dumps({"bench": "doppler_spectrum", "device": torch.cuda.get_device_name(0), "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
