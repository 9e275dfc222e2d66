#!/usr/bin/env python
"""tools/bench_bright_band.py -- time the bright band (kidmp_bright_band_device, one launch of kidmp::k_bright_band) on one
MI355X beside the reflectivity of the same state in the same context and a torch composite of the same numbers.

Workloads, fp64, state in HBM, 10^5 and 10^4 columns x 120 levels each:
  config3   mixed-phase BASELINE config 3 after one column step: the state of tools/bench_doppler.py
  cold      the same state with t capped at 273.0 K: no column has a melting level
  built     the hand-built melting columns of tests/bright_band_cases.py, every kind in turn
All variants run in ONE process, warmed up, taking turns launch by launch; every launch is timed with device events of its
own and the median of --reps (30) launches is reported with the minimum and maximum beside it.  Variants:
  bb_dbz        bright_band, dbz alone
  bb_all        bright_band, all eight outputs
  reflectivity  kidmp_reflectivity_device on the same state: the dry calc_refl10cm
  composite     the eight outputs from torch operations on the device tensors: the load and the melting level over
                [ncol, nz], the quadrature over the gathered active (level, species) pairs as [pairs, bins] tensors with
                torch's complex arithmetic (checked against bb_all once)
The mean number of active (level, species) pairs per column is printed for every workload.  Prints one line per variant
and workload and ONE JSON line at the end; the lines also go to --out (profiles/r23_bright_band.txt) under a header with
the date."""
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
PAIR_CHUNK = 1 << 18


def torch_composite(c, dev, grids, cfg):
    """tests/bright_band_ref.py in torch, on device tensors [ncol, nz]: the eight outputs."""
    import torch
    import bright_band_ref as b
    import doppler_ref as r
    import refl_oracle as ro
    t, p = dev["t"], dev["p"]
    ncol, nz = t.shape
    qv = torch.clamp(dev["qv"], min=1e-10)
    rho = 0.622 * p / (ro.R * t * (qv + 0.622))
    tiny = torch.full_like(t, 1.e-22)
    pr, ps, pg = dev["qr"] > ro.R1, dev["qs"] > ro.R2, dev["qg"] > ro.R2
    rr = torch.where(pr, dev["qr"] * rho, ro.R1)
    nr = torch.where(pr, torch.clamp(dev["nr"] * rho, min=ro.R2), ro.R1)
    lamr = (ro.am_r * c["crg"][2] * c["org2"] * nr / rr) ** (1. / 3.)
    mvd_r = torch.where(pr, 3.672 / lamr, 50.E-6)
    ze_r = torch.where(pr, nr * c["org2"] * lamr * c["crg"][3] / lamr ** 7, tiny)
    rs = torch.where(ps, dev["qs"] * rho, ro.R1)
    tc0 = torch.clamp(t - 273.15, max=-0.1)
    fit = lambda a, x: (a[0] + a[1] * tc0 + a[2] * x + a[3] * tc0 * x + a[4] * tc0 * tc0 + a[5] * x * x + a[6] * tc0 * tc0 * x   # noqa: E731
                        + a[7] * tc0 * x * x + a[8] * tc0 * tc0 * tc0 + a[9] * x * x * x)
    smob = rs * c["oams"]
    moment = lambda x: 10.0 ** fit(ro.sa, x) * smob ** fit(ro.sb, x)   # noqa: E731
    ze_s = torch.where(ps, (0.176 / 0.93) * (6.0 / ro.PI) * (6.0 / ro.PI) * (ro.am_s / 900.0) * (ro.am_s / 900.0) * moment(c["cse"][2]), tiny)
    rg = torch.where(pg, dev["qg"] * rho, ro.R1)
    slw = (t < 270.65) & pr & (mvd_r > 100.E-6)
    xslw1 = torch.where(slw, 4.01 + torch.log10(mvd_r), 0.01)
    ygra1 = 4.31 + torch.log10(torch.clamp(rg, min=5.E-5))
    zans1 = 3.1 + (100. / (300. * xslw1 * ygra1 / (10. / xslw1 + 1. + 0.25 * ygra1) + 30. + 10. * ygra1))
    n0 = torch.clamp(10. ** zans1, min=ro.gonv_min, max=ro.gonv_max)
    n0 = torch.flip(torch.cummin(torch.flip(n0, [1]), 1).values, [1])
    lam_exp = (n0 * ro.am_g * c["cgg"][0] / rg) ** 0.25
    lamg = lam_exp * (c["cgg"][2] * c["ogg2"] * c["ogg1"]) ** c["obmg"]
    N0_g = n0 / (c["cgg"][1] * lam_exp) * lamg
    ze_g = torch.where(pg, (0.176 / 0.93) * (6.0 / ro.PI) * (6.0 / ro.PI) * (ro.am_g / 900.0) * (ro.am_g / 900.0)
                       * N0_g * c["cgg"][3] * (1. / lamg) ** 7, tiny)
    # the melting level and the melt fractions
    kk = torch.arange(nz, device=t.device)
    hit = (t[:, :-1] > 273.15) & pr[:, :-1] & (ps | pg)[:, 1:]
    top = torch.where(hit, kk[None, :-1], -1).max(dim=1).values
    k0 = torch.where(top >= 0, top + 1, -1)
    at = k0.clamp(min=0)[:, None]
    below = (k0[:, None] >= 0) & (kk[None, :] < k0[:, None])

    def fraction(has, content):
        act = below & has & has.gather(1, at)
        fm = torch.clamp(1.0 - content / content.gather(1, at), min=0.05, max=0.99)
        return torch.where(act, fm, 0.0), act

    fm_s, act_s = fraction(ps, rs)
    fm_g, act_g = fraction(pg, rg)
    ew, ki = complex(cfg["eps_w"]), b.k_ice(cfg)

    def chunk(x, ci, ki_, fm, D, dD, e):
        f = fm[ci, ki_][:, None]
        D, dD = D[None, :], dD[None, :]
        if x == "s":
            ratio = (smob / moment(c["cse"][0]))[ci, ki_][:, None]
            n = smob[ci, ki_][:, None] * ratio ** 3 * (r.Kap0 * torch.exp(-ratio * r.Lam0 * D)
                                                       + r.Kap1 * ratio ** r.mu_s * D ** r.mu_s * torch.exp(-ratio * r.Lam1 * D)) * dD
            m = ro.am_s * D * D
        else:
            n = N0_g[ci, ki_][:, None] * torch.exp(-lamg[ci, ki_][:, None] * D) * dD
            m = ro.am_g * D * D * D
        Vi0 = m / cfg["rho_i"]
        Ve = torch.maximum((ro.PI / 6.0) * D * D * D, Vi0)
        Vi, Vw, Va = (1.0 - f) * Vi0, f * m / cfg["rho_w"], (1.0 - f) * (Ve - Vi0)
        core = Vi + Va
        V = core + Vw
        Kc = Vi / core * ki
        eps_c = (1.0 + 2.0 * Kc) / (1.0 - Kc)
        if cfg["topology"] == b.WATER_MATRIX:
            gb = core / V * (eps_c - ew) / (eps_c + 2.0 * ew)
            eps_p = ew * (1.0 + 2.0 * gb) / (1.0 - gb)
        else:
            gb = Vw / V * (ew - eps_c) / (ew + 2.0 * eps_c)
            eps_p = eps_c * (1.0 + 2.0 * gb) / (1.0 - gb)
        s = ((eps_p - 1.0) / (eps_p + 2.0)).abs() ** 2 * V * V
        s0 = ki * ki * Vi0 * Vi0
        e[ci, ki_] = (n * s).sum(dim=1) / (n * s0).sum(dim=1)

    def enhancement(x, act, fm, D, dD):
        e = torch.ones_like(t)
        ci, ki_ = torch.nonzero(act, as_tuple=True)
        if ci.numel() == 0:
            return e
        for lo in range(0, ci.numel(), PAIR_CHUNK):                  # bounded temporaries: [PAIR_CHUNK, bins]
            chunk(x, ci[lo:lo + PAIR_CHUNK], ki_[lo:lo + PAIR_CHUNK], fm, D, dD, e)
        return e

    e_s = enhancement("s", act_s, fm_s, *grids["s"])
    e_g = enhancement("g", act_g, fm_g, *grids["g"])
    zs, zg = ze_s * e_s, ze_g * e_g
    dbz_of = lambda ze: 10. * torch.log10(ze * 1.e18)   # noqa: E731
    return dict(dbz=dbz_of(ze_r + zs + zg), dbz_s=dbz_of(zs), dbz_g=dbz_of(zg), enh_s=e_s, enh_g=e_g, fmelt_s=fm_s, fmelt_g=fm_g,
                k0=k0.to(torch.int32))


def states(m, ncol):
    """workload -> the device state."""
    import numpy as np
    import torch
    import bright_band_cases as bc
    import cases
    from kid_amd import BRIGHTBAND_INPUTS
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in cases.config3(ncol).items()}
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                 # the state after one step
    config3 = {k: dev[k] for k in BRIGHTBAND_INPUTS}
    cold = dict(config3, t=torch.clamp(config3["t"], max=273.0).contiguous())
    few, _ = bc.batch(NZ, 9 * 64, 23)
    rep = np.arange(ncol) % (9 * 64)
    built = {k: torch.from_numpy(np.ascontiguousarray(few[k][rep])).to("cuda:0") for k in BRIGHTBAND_INPUTS}
    return {"config3": config3, "cold": cold, "built": built}


def measure(a, c, ncol, lines):
    import torch
    import bright_band_ref as b
    from kid_amd import BRIGHTBAND_NAMES, ThompsonMP, default_grid

    def say(s):
        print(s)
        lines.append(s)

    m = ThompsonMP(iiwarm=False, device=0)
    grids = {x: tuple(torch.from_numpy(g).to("cuda:0") for g in default_grid(m, x)) for x in b.SPECIES}
    cfg = b.default_cfg()
    out = []
    for name, ins in states(m, ncol).items():
        variants = {
            "bb_dbz": lambda: m.bright_band(ins, want=("dbz",)),
            "bb_all": lambda: m.bright_band(ins, want=BRIGHTBAND_NAMES),
            "reflectivity": lambda: m.reflectivity(ins),
            "composite": lambda: torch_composite(c, ins, grids, cfg),
        }
        got, comp = variants["bb_all"](), variants["composite"]()
        pairs = float(((got["fmelt_s"] > 0).sum() + (got["fmelt_g"] > 0).sum()).item()) / ncol
        melting = float((got["k0"] >= 0).sum().item()) / ncol
        diff = {n: float((got[n] - comp[n]).abs().max() / (1.0 if n.startswith("dbz") or n == "k0" else got[n].abs().max().clamp(min=1e-300)))
                for n in BRIGHTBAND_NAMES}
        say("ncol=%-6d %-8s active pairs per column %.3f, columns with a melting level %.3f" % (ncol, name, pairs, melting))
        say("ncol=%-6d %-8s composite - bb_all, max |difference| (dbz*: dB; k0: levels; else / max |profile|): %s"
            % (ncol, name, "  ".join("%s %.1e" % (n, d) for n, d in diff.items())))
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
        res = {"ncol": ncol, "nz": NZ, "workload": name, "reps": a.reps, "pairs_per_column": pairs, "melting_columns": melting,
               "composite_max_diff": diff}
        for k, t in times.items():
            res[k] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
            say("ncol=%-6d %-8s %-12s median %8.4f ms   min %8.4f   max %8.4f" % (ncol, name, k, res[k]["ms_median"], min(t), max(t)))
        ms = {k: res[k]["ms_median"] for k in variants}
        res["ratios"] = {"bb_dbz/reflectivity": ms["bb_dbz"] / ms["reflectivity"], "bb_all/reflectivity": ms["bb_all"] / ms["reflectivity"],
                         "bb_dbz/composite": ms["bb_dbz"] / ms["composite"], "bb_all/composite": ms["bb_all"] / ms["composite"]}
        say("ncol=%-6d %-8s ratios: %s" % (ncol, name, "  ".join("%s %.3f" % kv for kv in res["ratios"].items())))
        out.append(res)
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ncols", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_bright_band.txt"))
    a = ap.parse_args()
    import torch
    import doppler_ref as ref
    from oracle.oracle import Oracle
    if not torch.cuda.is_available():
        sys.exit("bench_bright_band: no GPU visible (this measurement has no CPU path)")
    o = Oracle(iiwarm=True)
    c = ref.constants(o)
    o.close()
    lines = ["# tools/bench_bright_band.py  %s  %s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0))]
    results = [r for n in a.ncols for r in measure(a, c, n, lines)]
    lines.append(json.dumps({"bench": "bright_band", "device": torch.cuda.get_device_name(0), "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
