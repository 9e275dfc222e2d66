#!/usr/bin/env python
"""tools/bench_scan.py -- time the range-height scan (include/kidmp_scan.h: one launch of kidmp::k_scan) on one MI355X
beside a torch composite that forms the same numbers and the cloud-radar launch that made the fields.

State: the slab benchmark's, 10^5 mixed-phase columns x 120 levels (BASELINE config 3) as 100 slabs of 1 000 cells, fp64 in
HBM; dbz, ext and vd are mie_radar's at 3.19 mm (the illustrative W-band permittivities of tests/mie_radar_cases.py), u a
smooth flow of both signs.  Scan: one radar per slab at a tenth of its width, 90 elevations 0.5, 1.5 .. 89.5 degrees, 512
gates of 60 m, periodic in x, an earth of effective radius 8.5e6 m; with nsub = 5 a beam of one degree.  All variants run
in ONE process, warmed up, taking turns launch by launch; every launch is timed with device events of its own and the
median of --reps (30) launches is reported with the minimum and maximum beside it.  Variants, for nsub = 1 and nsub = 5:
  all        every output of the 90-elevation sweep
  cell       `cell` alone: the geometry without a gather
  low        every output, 90 elevations from 0.5 to 9.5 degrees: the 64 gates of a wave spread over eight columns
  high       every output, 90 elevations from 60.5 to 89.5 degrees: the gates of a wave sit in one or two columns
  composite  the outputs of `all` from torch operations on the device tensors (index arithmetic, gathers, cumsum, exp and
             log sums), checked against the kernel once: the largest difference is printed in the units of
             tests/test_gpu_scan.py beside that file's bound
  transpose_dbz  for scale, ONE of the four fields copied to [nz, ncol]: what a transposed staging would pay per field
             and call before the first gather
  mie_radar  for scale, the launch that made dbz, ext and vd
A sample is one gate of one sub-ray.  Prints one line per variant and ONE JSON line at the end; the lines also go to --out
(profiles/r28_scan.txt) under a header with the date and the library's fingerprint."""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NZ, NGATE, DR, A_E = 120, 512, 60.0, 8.5e6
LN10 = 2.302585092994045684
ULP = 2.220446049250313e-16


def torch_composite(f, zf, rays, dx, nx, nslab, nsub, hae, missing):
    """The six outputs from torch operations; f: dbz, ext, vd, u [ncol, nz]; periodic in x."""
    import torch
    nz = zf.shape[0] - 1
    R = rays.view(-1, nsub, 6)
    slab, x0, z0, ce, se, wgt = (R[:, :, c:c + 1] for c in range(6))
    g = torch.arange(NGATE, dtype=torch.float64, device=zf.device)
    r = (g + 0.5) * DR
    s = r * ce
    x = x0 + s
    h = (z0 + r * se) + (s * s) * hae
    xi = torch.floor(x / torch.full((), dx, dtype=torch.float64, device=zf.device))
    i = torch.remainder(xi, float(nx))
    k = torch.searchsorted(zf, h.contiguous(), right=True) - 1
    valid = (slab >= 0) & (slab < nslab) & (wgt > 0)
    inside = valid & (h >= zf[0]) & (h < zf[nz])
    col = (slab * nx + i).long()
    idx = torch.where(inside, col * nz + k, torch.zeros_like(k))
    right = torch.where(inside, (col - i.long() + torch.remainder(i + 1.0, float(nx)).long()) * nz + k, torch.zeros_like(k))
    zero = torch.zeros((), dtype=torch.float64, device=zf.device)
    d = torch.take(f["dbz"], idx)
    a = torch.where(inside, torch.take(f["ext"], idx) * DR, zero)
    v = 0.5 * (torch.take(f["u"], idx) + torch.take(f["u"], right)) * ce - torch.take(f["vd"], idx) * se
    tau = (torch.cumsum(a, -1) - a) + 0.5 * a
    p = (20.0 / LN10) * tau
    e = d - p
    c = nsub // 2
    hits = inside.any(1)
    if nsub == 1:
        vals = [d[:, 0], e[:, 0], p[:, 0], v[:, 0]]
    else:
        w = torch.where(inside, wgt.expand_as(d), zero)
        za = w * torch.exp((LN10 / 10.0) * e)
        W, Sa = w.sum(1), za.sum(1)
        o_dbz = (10.0 / LN10) * torch.log((w * torch.exp((LN10 / 10.0) * d)).sum(1) / W)
        o_att = (10.0 / LN10) * torch.log(Sa / W)
        vals = [o_dbz, o_att, o_dbz - o_att, (za * v).sum(1) / Sa]
    miss = torch.full((), missing, dtype=torch.float64, device=zf.device)
    out = {n: torch.where(hits, t, miss) for n, t in zip(("dbz", "dbz_att", "pia", "vr"), vals)}
    out["height"] = h[:, c]
    out["cell"] = torch.where(inside[:, c], idx[:, c], torch.full_like(idx[:, c], -1)).int()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nslab", type=int, default=100)
    ap.add_argument("--nx", type=int, default=1000)
    ap.add_argument("--lib", default=None, help="another build of the library (an A/B of the kernel)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_scan.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import kid_amd
    if not torch.cuda.is_available():
        sys.exit("bench_scan: no GPU visible (this measurement has no CPU path)")
    if a.lib:
        kid_amd.load_library(a.lib)
    import cases
    from mie_radar_cases import CFGS
    from test_gpu_scan import MEASURED, bound
    from kid_amd import MieCfg, ScanCfg, ThompsonMP, rhi_rays
    lines = []

    def say(s):
        print(s)
        lines.append(s)

    m = ThompsonMP(iiwarm=False, device=0)
    say("# tools/bench_scan.py  %s  %s%s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0), "  --lib " + a.lib if a.lib else ""))
    say("# fingerprint: %s" % m.kernel_fingerprint())
    nx, nslab = a.nx, a.nslab
    ncol = nx * nslab
    cu = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")   # noqa: E731
    st = cases.config3(ncol)
    dz = st["dz"][0]
    dx = 4.0 * float(dz.mean())
    zf = cu(np.concatenate([[0.0], np.cumsum(dz)]))
    dev = {k: cu(st[k]) for k in ("t", "p", "qv", "qc", "qr", "nr", "qs", "qg")}
    ddz, dw = cu(dz), cu(st["w"])
    table = m.mie_table(MieCfg(**CFGS["w"]))
    rad = m.mie_radar(table, dev, ddz, dw, None, ("dbz", "ext", "vd"))
    xs = (np.arange(nx) / float(nx))[None, :, None]
    zs = (np.arange(NZ) / float(NZ))[None, None, :]
    amp = np.linspace(6.0, 14.0, nslab)[:, None, None]
    f = {"dbz": rad["dbz"], "ext": rad["ext"], "vd": rad["vd"],
         "u": cu((amp * np.sin(2.0 * np.pi * 3.0 * xs + 0.4) * np.cos(np.pi * zs)).reshape(ncol, NZ))}
    hae = 1.0 / (2.0 * A_E)
    el_all = 0.5 + np.arange(90.0)
    sweeps = {"all": el_all, "low": np.linspace(0.5, 9.5, 90), "high": np.linspace(60.5, 89.5, 90)}   # 90 rays each: equal launches
    say("%d slabs x %d cells x %d levels, dx %.0f m, top %.0f m; %d gates of %.0f m; dbz %.1f .. %.1f, ext max %.2e 1/m, two-way path up to %.0f dB"
        % (nslab, nx, NZ, dx, float(zf[-1]), NGATE, DR, float(f["dbz"].min()), float(f["dbz"].max()), float(f["ext"].max()),
           float((20.0 / LN10) * (f["ext"] * ddz).sum(1).max())))
    variants, samples, results = {}, {}, {}
    for nsub in (1, 5):
        cfg = ScanCfg(r0=0.0, dr=DR, ngate=NGATE, nsub=nsub, half_inv_ae=hae, periodic=True, missing=-999.0)
        rays = {k: cu(np.concatenate([rhi_rays(s, 0.1 * nx * dx, 2.0, el, 1.0, nsub) for s in range(nslab)])) for k, el in sweeps.items()}
        outs = {k: m.scan(f, zf, rays[k], dx, nx, cfg, kid_amd.SCAN_NAMES) for k in sweeps}
        cell = m.scan(f, zf, rays["all"], dx, nx, cfg, ("cell",))
        for k in sweeps:
            variants["nsub%d_%s" % (nsub, k)] = (lambda k=k, cfg=cfg, rays=rays, outs=outs: m.scan(f, zf, rays[k], dx, nx, cfg, kid_amd.SCAN_NAMES, out=outs[k]))
            samples["nsub%d_%s" % (nsub, k)] = nslab * len(sweeps[k]) * NGATE * nsub
        variants["nsub%d_cell" % nsub] = (lambda cfg=cfg, rays=rays, cell=cell: m.scan(f, zf, rays["all"], dx, nx, cfg, ("cell",), out=cell))
        variants["nsub%d_composite" % nsub] = (lambda nsub=nsub, rays=rays: torch_composite(f, zf, rays["all"], dx, nx, nslab, nsub, hae, -999.0))
        samples["nsub%d_cell" % nsub] = samples["nsub%d_composite" % nsub] = samples["nsub%d_all" % nsub]
        # the composite against the kernel, once
        comp = torch_composite(f, zf, rays["all"], dx, nx, nslab, nsub, hae, -999.0)
        torch.cuda.synchronize()
        k_out = outs["all"]
        hit = (k_out["dbz"] != -999.0) & (comp["dbz"] != -999.0)
        same_cells = bool((k_out["cell"] == comp["cell"]).all()) and bool((k_out["height"] == comp["height"]).all())
        def apart(n, scale=None):                                     # over the gates where both hold a finite number
            fin = hit & torch.isfinite(k_out[n]) & torch.isfinite(comp[n])
            d = torch.where(fin, (k_out[n] - comp[n]).abs() / (1.0 if scale is None else scale), torch.zeros_like(comp[n]))
            return float(d.max()), int((hit & (torch.isfinite(k_out[n]) != torch.isfinite(comp[n]))).sum())

        worst, odd = {}, 0
        for n in ("dbz", "dbz_att", "pia"):
            w, o = apart(n)
            worst[n], odd = w * (LN10 / 10.0) / ULP, odd + o
        w, o = apart("vr", 1.0 + k_out["vr"].abs())
        worst["vr"], odd = w / ULP, odd + o
        inside = float(hit.double().mean())
        results["nsub%d_check" % nsub] = dict(worst, cell_and_height_equal=same_cells, gates_with_a_sample=inside, finite_on_one_side_only=odd)
        say("nsub=%d composite against the kernel: cell and height equal: %s; %.1f %% of the gates have a sample; largest difference in ulp of the "
            "reflectivity ratio (vr: of 1 + |vr|): %s; %d values finite on one side only   [the tests' bound for equal sums: %s; cumsum adds the %d "
            "terms of a path in another order than the kernel's scan, which allows dbz_att, pia and the weights of vr (ngate + 4)/2 ulp of the "
            "largest path's ratio on top: %.0f]"
            % (nsub, same_cells, 100.0 * inside, "  ".join("%s %.1f" % kv for kv in worst.items()), odd,
               "  ".join("%s %.0f" % (n, bound(n) / ULP) for n in MEASURED), NGATE,
               0.5 * (NGATE + 4) * float(torch.where(hit, k_out["pia"], torch.zeros_like(k_out["pia"])).max()) * (LN10 / 10.0)))
    want3 = {n: rad[n] for n in ("dbz", "ext", "vd")}
    variants["transpose_dbz"] = lambda: f["dbz"].t().contiguous()
    variants["mie_radar"] = lambda: m.mie_radar(table, dev, ddz, dw, None, ("dbz", "ext", "vd"), out=want3)
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
        if k in samples:
            results[k]["samples"] = samples[k]
            results[k]["samples_per_s"] = samples[k] / (med * 1e-3)
            extra = "   %9d samples -> %7.2f G samples/s" % (samples[k], results[k]["samples_per_s"] * 1e-9)
        say("%-16s median %8.4f ms   min %8.4f   max %8.4f%s" % (k, med, min(t), max(t), extra))
    for nsub in (1, 5):
        r = {k: results["nsub%d_%s" % (nsub, k)] for k in ("all", "cell", "low", "high", "composite")}
        results["nsub%d_kernel_over_composite" % nsub] = r["all"]["ms_median"] / r["composite"]["ms_median"]
        results["nsub%d_low_over_high_per_sample" % nsub] = r["high"]["samples_per_s"] / r["low"]["samples_per_s"]
        say("nsub=%d: the kernel takes %.3f of the composite's time and %.2f of the mie_radar launch's; `cell` alone %.2f of all outputs; a sample below "
            "10 degrees costs %.2f times one above 60 degrees"
            % (nsub, results["nsub%d_kernel_over_composite" % nsub], r["all"]["ms_median"] / results["mie_radar"]["ms_median"],
               r["cell"]["ms_median"] / r["all"]["ms_median"], results["nsub%d_low_over_high_per_sample" % nsub]))
    table.close()
    m.close()
    lines.append(json.dumps({"bench": "scan", "device": torch.cuda.get_device_name(0), "nslab": nslab, "nx": nx, "nz": NZ, "ngate": NGATE,
                             "reps": a.reps, "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
