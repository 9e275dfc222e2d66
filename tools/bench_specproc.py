#!/usr/bin/env python
"""tools/bench_specproc.py -- time the spectrum processor (include/kidmp_specproc.h: one launch of
kidmp::k_spectrum_process) on one MI355X beside a device copy of the spectrum, a torch composite that forms the same
numbers and the doppler_spectrum launch that made the input.

State: 10^4 mixed-phase columns x 120 levels (BASELINE config 3), fp64 in HBM; the input is doppler_spectrum's `total` on
64 and on 256 velocity bins over -1 .. 15 m/s.  The broadening has sigma/dv = 0, 2 and 8 at every level (cut = 4: H = 0, 8
and 32), the noise is 1e-3 of each level's largest bin, snr_min = 1.  All variants run in ONE process, warmed up, taking
turns launch by launch; every launch is timed with device events of its own and the median of --reps (30) launches is
reported with the minimum and maximum beside it.  Variants, per number of bins and width:
  all        every output: the broadened spectrum, what left the grid and the moments
  moments    the eight moments alone: no spectrum is stored
  composite  the outputs of `all` from torch operations on the device tensors: an unfold of the padded spectrum against the
             per-level weight rows, a mask and reductions, in chunks of columns so that the unfolded product stays under
             1 GiB; checked against the kernel once
and per number of bins:
  copy       a device copy of the spectrum: the floor of any kernel that reads and writes it once
  dspectrum  the doppler_spectrum launch that made the input
The compulsory traffic is 16 nv bytes per level with the spectrum stored and 8 nv without; the fraction of 8 TB/s on those
bytes is printed beside each time.  Prints one line per variant and ONE JSON line at the end; the lines also go to --out
(profiles/r29_specproc.txt) under a header with the date and the library's fingerprint."""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NZ, CUT, SNR = 120, 4.0, 1.0
V_LO, V_HI = -1.0, 15.0
PEAK = 8.0e12                                                   # bytes per second


def torch_composite(x, v0, dv, s, noise, chunk):
    """The eleven outputs from torch operations; x [ncol, nv, nz], s = sigma/dv [nz] (all zero: no broadening), noise
    [ncol, nz]."""
    import math
    import torch
    ncol, nv, nz = x.shape
    H = int(math.ceil(CUT * float(s.max()))) if float(s.max()) > 0 else 0
    v = v0 + dv * torch.arange(nv, dtype=torch.float64, device=x.device)
    out = {n: [] for n in ("spec", "lost_below", "lost_above", "dbz", "vm", "sw", "skew", "kurt", "v_lo", "v_hi", "nbins")}
    if H > 0:
        d = torch.arange(-H, H + 1, dtype=torch.float64, device=x.device)
        g = torch.exp(-0.5 * (d[None, :] / s[:, None]) ** 2)                       # [nz, 2H+1]
        w = g / g.sum(1, keepdim=True)
        tail = torch.flip(torch.cumsum(torch.flip(w[:, H + 1:], [1]), 1), [1])     # T_m/G for m = 1 .. H
    for c0 in range(0, ncol, chunk):
        xc = x[c0:c0 + chunk]
        if H > 0:
            pad = torch.nn.functional.pad(xc, (0, 0, H, H))
            B = torch.einsum("cvzk,zk->cvz", pad.unfold(1, 2 * H + 1, 1), w)
            nb = min(H, nv)
            out["lost_below"].append(torch.einsum("cmz,zm->cz", xc[:, :nb, :], tail[:, :nb]))
            out["lost_above"].append(torch.einsum("cmz,zm->cz", xc[:, nv - nb:, :], torch.flip(tail[:, :nb], [1])))
        else:
            B = xc.clone()
            out["lost_below"].append(torch.zeros_like(xc[:, 0, :]))
            out["lost_above"].append(torch.zeros_like(xc[:, 0, :]))
        det = B > (SNR * noise[c0:c0 + chunk])[:, None, :]
        Bd = torch.where(det, B, torch.zeros_like(B))
        z = Bd.sum(1)
        some = z > 0
        zs = torch.where(some, z, torch.ones_like(z))
        vm = (Bd * v[None, :, None]).sum(1) / zs
        e = v[None, :, None] - vm[:, None, :]
        c2, c3, c4 = (Bd * e ** 2).sum(1) / zs, (Bd * e ** 3).sum(1) / zs, (Bd * e ** 4).sum(1) / zs
        sw = torch.sqrt(torch.clamp(c2, min=0.0))
        s1 = torch.where(sw > 0, sw, torch.ones_like(sw))
        vv = v[None, :, None].expand_as(B)
        out["spec"].append(B)
        out["dbz"].append(torch.where(some, 10.0 * torch.log10(torch.clamp(z, min=1e-22) * 1e18), torch.full_like(z, -40.0)))
        out["vm"].append(vm)
        out["sw"].append(sw)
        out["skew"].append(torch.where(sw > 0, c3 / s1 ** 3, torch.zeros_like(sw)))
        out["kurt"].append(torch.where(sw > 0, c4 / s1 ** 4, torch.zeros_like(sw)))
        out["v_lo"].append(torch.where(some, torch.where(det, vv, torch.full_like(vv, float("inf"))).amin(1), torch.zeros_like(z)))
        out["v_hi"].append(torch.where(some, torch.where(det, vv, torch.full_like(vv, float("-inf"))).amax(1), torch.zeros_like(z)))
        out["nbins"].append(det.sum(1).int())
    return {n: torch.cat(t) for n, t in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ncol", type=int, default=10000)
    ap.add_argument("--no-composite", action="store_true", help="leave the torch composite out (an A/B of the kernel)")
    ap.add_argument("--lib", default=None, help="another build of the library (an A/B of the kernel)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_specproc.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import kid_amd
    if not torch.cuda.is_available():
        sys.exit("bench_specproc: no GPU visible (this measurement has no CPU path)")
    if a.lib:
        kid_amd.load_library(a.lib)
    import cases
    from kid_amd import SPECPROC_NAMES, SpecCfg, ThompsonMP
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    m = ThompsonMP(iiwarm=False, device=0)
    say("# tools/bench_specproc.py  %s  %s%s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0), "  --lib " + a.lib if a.lib else ""))
    say("# fingerprint: %s" % m.kernel_fingerprint())
    ncol = a.ncol
    cu = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")   # noqa: E731
    st = cases.config3(ncol)
    dev = {k: cu(st[k]) for k in ("t", "p", "qv", "qr", "nr", "qs", "qg")}
    cfg = SpecCfg(cut=CUT, snr_min=SNR)
    moments = SPECPROC_NAMES[3:]
    say("%d columns x %d levels; velocity grid %.0f .. %.0f m/s; cut %.0f, snr_min %.0f, noise 1e-3 of each level's largest bin" % (ncol, NZ, V_LO, V_HI, CUT, SNR))
    variants, nbytes, results = {}, {}, {}
    for nv in (64, 256):
        dv = (V_HI - V_LO) / nv
        v0 = V_LO + 0.5 * dv
        spec = m.doppler_spectrum(dev, v0, dv, nv, want=("total",))
        x = spec["total"]
        noise = (1e-3 * x.amax(1)).contiguous()
        copy = torch.empty_like(x)
        levels = ncol * NZ
        variants["nv%d_copy" % nv] = (lambda x=x, copy=copy: copy.copy_(x))
        variants["nv%d_dspectrum" % nv] = (lambda v0=v0, dv=dv, nv=nv, spec=spec: m.doppler_spectrum(dev, v0, dv, nv, want=("total",), out=spec))
        nbytes["nv%d_copy" % nv] = 16 * nv * levels
        for ratio in (0, 2, 8):
            sigma = torch.full((NZ,), ratio * dv, dtype=torch.float64, device="cuda:0") if ratio else None
            s = torch.full((NZ,), float(ratio), dtype=torch.float64, device="cuda:0")
            H = int(np.ceil(CUT * ratio))
            chunk = max(1, min(ncol, (1 << 30) // (8 * nv * NZ * (2 * H + 1))))
            key = "nv%d_s%d" % (nv, ratio)
            full = m.spectrum_process(x, v0, dv, sigma, noise, cfg, SPECPROC_NAMES)
            mom = m.spectrum_process(x, v0, dv, sigma, noise, cfg, moments)
            variants[key + "_all"] = (lambda x=x, v0=v0, dv=dv, sigma=sigma, noise=noise, full=full:
                                      m.spectrum_process(x, v0, dv, sigma, noise, cfg, SPECPROC_NAMES, out=full))
            variants[key + "_moments"] = (lambda x=x, v0=v0, dv=dv, sigma=sigma, noise=noise, mom=mom:
                                          m.spectrum_process(x, v0, dv, sigma, noise, cfg, moments, out=mom))
            nbytes[key + "_all"] = nbytes[key + "_composite"] = 16 * nv * levels
            nbytes[key + "_moments"] = 8 * nv * levels
            if a.no_composite:
                continue
            variants[key + "_composite"] = (lambda x=x, v0=v0, dv=dv, s=s, noise=noise, chunk=chunk: torch_composite(x, v0, dv, s, noise, chunk))
            # the composite against the kernel, once
            comp = torch_composite(x, v0, dv, s, noise, chunk)
            torch.cuda.synchronize()
            total = x.sum(1)
            echo = total > 0
            rel = lambda p, q, scale: float(torch.where(echo, (p - q).abs() / scale, torch.zeros_like(p)).max())   # noqa: E731
            tot1 = torch.where(echo, total, torch.ones_like(total))
            worst = {"spec": float(torch.where(echo[:, None, :], (full["spec"] - comp["spec"]).abs() / tot1[:, None, :], torch.zeros_like(x)).max())}
            for n in ("lost_below", "lost_above"):
                worst[n] = rel(full[n], comp[n], tot1)
            worst["dbz"] = rel(full["dbz"], comp["dbz"], 1.0)
            for n in ("vm", "sw", "v_lo", "v_hi"):
                worst[n] = rel(full[n], comp[n], torch.clamp(comp[n].abs(), min=dv))
            for n in ("skew", "kurt"):
                worst[n] = rel(full[n], comp[n], torch.clamp(comp[n].abs(), min=1.0))
            worst["nbins_differ"] = int((full["nbins"] != comp["nbins"]).sum())
            results[key + "_check"] = dict(worst, levels_with_echo=float(echo.double().mean()), mean_bins_detected=float(full["nbins"].double().mean()))
            say("%s (H = %d) composite against the kernel: %.1f %% of the levels hold an echo, %.1f bins detected on average; largest difference %s; "
                "nbins differs at %d levels (a bin within rounding of its threshold)"
                % (key, H, 100.0 * float(echo.double().mean()), float(full["nbins"].double().mean()),
                   "  ".join("%s %.1e" % (n, worst[n]) for n in worst if n != "nbins_differ"), worst["nbins_differ"]))
            del comp
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
    for k, t in times.items():
        med = statistics.median(t)
        results[k] = {"ms_median": med, "ms_min": min(t), "ms_max": max(t)}
        extra = ""
        if k in nbytes:
            results[k]["compulsory_bytes"] = nbytes[k]
            results[k]["fraction_of_8TBs"] = nbytes[k] / (med * 1e-3) / PEAK
            extra = "   %6.1f MB compulsory -> %5.1f %% of 8 TB/s" % (nbytes[k] * 1e-6, 100.0 * results[k]["fraction_of_8TBs"])
        say("%-22s median %9.4f ms   min %9.4f   max %9.4f%s" % (k, med, min(t), max(t), extra))
    for nv in (64, 256):
        for ratio in (0, 2, 8):
            key = "nv%d_s%d" % (nv, ratio)
            r = {k: results[key + "_" + k]["ms_median"] if key + "_" + k in results else float("nan") for k in ("all", "moments", "composite")}
            results[key + "_kernel_over_composite"] = r["all"] / r["composite"]
            results[key + "_kernel_over_copy"] = r["all"] / results["nv%d_copy" % nv]["ms_median"]
            say("%s: all outputs take %.3f of the composite's time, %.2f of the copy's and %.2f of the doppler_spectrum launch's; the moments alone %.2f "
                "of all outputs" % (key, results[key + "_kernel_over_composite"], results[key + "_kernel_over_copy"],
                                    r["all"] / results["nv%d_dspectrum" % nv]["ms_median"], r["moments"] / r["all"]))
    m.close()
    lines.append(json.dumps({"bench": "specproc", "device": torch.cuda.get_device_name(0), "ncol": ncol, "nz": NZ, "reps": a.reps, "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
