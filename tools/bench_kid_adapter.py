#!/usr/bin/env python
"""tools/bench_kid_adapter.py -- what the KiD adapter on the device (kidmp_kid_interface_*) costs on one MI355X.

Workloads: BASELINE config 3 (10^5 mixed-phase columns) and config 2 (10^4 warm-rain columns), 120 levels, fp64, in
theta-form with kat_b's Exner recipe and a smooth forcing, measured in ONE process:
  device   ms per kid_interface call with both forcings, with adv only and with none; ms per gather alone
           (kidmp_kid_gather_device); ms per batch_step on the gathered columns (put back before every launch, untimed).
           Every launch is timed with device events; the figure is the median of --launches launches after --warmup.
           The back-out is what remains: call - gather - step (derived, not timed on its own).
           Bytes the two kernels must move, counted per present array, against 8 TB/s.
  host     kid_interface_host against batch_step_host fed by the same gather and back-out done in numpy (wall clock,
           page-locked arrays, median of --host-reps calls)
  fortran  kid_devadapter_driver at nx = 5*10^4 mixed phase, diagnostics off, 16 threads: column-steps/s with
           l_device_adapter off and on (two child processes)
Prints one JSON line and writes a readable report (--out, default profiles/r08_kid_adapter.txt); every line of the
report carries the kernel fingerprint.  No threshold is applied: the figures are for the record."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = {"config3": 100000, "config2": 10000}            # bench.py's DEFAULT_NCOL
P0, R_ON_CP, DT = 1.0e5, 287.058 / 1005.0, 10.0
FIELDS = ("theta", "qv", "qc", "qr", "nr", "qi", "ni", "qs", "qg")
HBM_PEAK = 8.0e12


def kid_fields(st):
    """theta-form fields of a cases.py batch, an advective and a divergence forcing for every field."""
    import numpy as np
    ncol, nz = st["qv"].shape
    exner = (st["p"] / P0) ** R_ON_CP
    F = {k: st[k] for k in FIELDS[1:]}
    F["theta"] = st["t"] / exner
    wave = np.sin(2.0 * np.pi * (1.5 * np.linspace(0.0, 1.0, nz)[None, :] + 0.013 * np.arange(ncol)[:, None]))
    adv = {k: np.ascontiguousarray(1e-4 * F[k] * wave) for k in FIELDS}
    div = {k: np.ascontiguousarray(-2e-5 * F[k]) for k in FIELDS}
    adv["theta"] = np.ascontiguousarray(2e-3 * wave)
    F = {k: np.ascontiguousarray(F[k]) for k in FIELDS}
    return F, adv, div, np.ascontiguousarray(exner), np.ascontiguousarray(st["dz"][0])


def median_ms(fn, launches, warmup, before=None):
    import numpy as np
    import torch
    t = []
    for i in range(warmup + launches):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            t.append(e0.elapsed_time(e1))
    return float(np.median(t))


def measure(name, a):
    import numpy as np
    import torch
    import cases
    from kid_amd import ThompsonMP
    from kid_amd.thompson import host_pinned_copy

    ncol = a.ncol or SIZES[name]
    iiwarm = name == "config2"
    nf = 5 if iiwarm else 9
    st0 = cases.config2(ncol) if iiwarm else cases.config3(ncol)
    nz = st0["qv"].shape[1]
    F, adv, div, exner, dz = kid_fields(st0)
    if iiwarm:
        F, adv, div = ({k: d[k] for k in FIELDS[:5]} for d in (F, adv, div))
    m = ThompsonMP(iiwarm=iiwarm, device=0)
    dev = lambda d: {k: torch.from_numpy(v).to("cuda:0") for k, v in d.items()}   # noqa: E731
    dF, dadv, ddiv = dev(F), dev(adv), dev(div)
    dex, ddz = torch.from_numpy(exner).to("cuda:0"), torch.from_numpy(dz).to("cuda:0")
    work = m.kid_workspace(ncol, nz, np.float64)
    res = {"workload": name, "ncol": ncol, "nz": nz, "fingerprint": m.kernel_fingerprint(), "launches": a.launches, "device": {}}
    out = m.kid_interface(dF, DT, P0, R_ON_CP, dex, ddz, adv=dadv, div=ddiv, work=work)
    prof = ncol * nz * 8
    for label, kw in (("both", dict(adv=dadv, div=ddiv)), ("adv", dict(adv=dadv)), ("none", {})):
        call = median_ms(lambda: m.kid_interface(dF, DT, P0, R_ON_CP, dex, ddz, work=work, out=out, **kw), a.launches, a.warmup)
        gather = median_ms(lambda: m.kid_interface(dF, DT, P0, R_ON_CP, dex, ddz, work=work, out=out, gather_only=True, **kw),
                           a.launches, a.warmup)
        # the step on exactly these gathered columns, put back before every launch
        m.kid_interface(dF, DT, P0, R_ON_CP, dex, ddz, work=work, out=out, gather_only=True, **kw)
        views = m.kid_workspace_views(work, ncol, nz, np.float64)
        init = {k: v.clone() for k, v in views.items()}
        ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")

        def put_back():
            for k in views:
                views[k].copy_(init[k])
            ppt.zero_()
        step = median_ms(lambda: m.batch_step(views, DT, ppt), a.launches, a.warmup, before=put_back)
        nforce = len(kw)
        b_gather = (nf * (1 + nforce) + 1 + 15) * prof
        b_backout = (nf * (2 + nforce) + 1 + nf) * prof
        backout = call - gather - step
        res["device"][label] = {
            "ms_call": round(call, 5), "ms_gather": round(gather, 5), "ms_step": round(step, 5), "ms_backout_derived": round(backout, 5),
            "call_over_step": round(call / step, 4), "column_steps_per_s": round(ncol / (call * 1e-3), 1),
            "gather_bytes": b_gather, "gather_TBps": round(b_gather / (gather * 1e-3) / 1e12, 4),
            "gather_frac_of_8TBps": round(b_gather / (gather * 1e-3) / HBM_PEAK, 4),
            "backout_bytes": b_backout, "backout_TBps_derived": round(b_backout / (max(backout, 1e-6) * 1e-3) / 1e12, 4),
            "backout_frac_of_8TBps_derived": round(b_backout / (max(backout, 1e-6) * 1e-3) / HBM_PEAK, 4)}
    # ---- host entry against the numpy adapter around batch_step_host ----
    pin = lambda d: {k: host_pinned_copy(v) for k, v in d.items()}   # noqa: E731
    hF, hadv, hdiv, hex_, hdz = pin(F), pin(adv), pin(div), host_pinned_copy(exner), host_pinned_copy(dz)
    names = {"theta": "t"}
    buf = {k: host_pinned_copy(st0[k]) for k in ("qv", "qc", "qr", "nr", "t", "p", "dz") + (() if iiwarm else ("qi", "ni", "qs", "qg"))}

    def numpy_adapter():
        for k in F:
            buf[names.get(k, k)][...] = hF[k] + (hadv[k] + hdiv[k]) * DT
        buf["t"] *= hex_
        buf["p"][...] = P0 * hex_ ** (1.0 / R_ON_CP)
        buf["dz"][...] = hdz
        ppt, _ = m.batch_step_host(buf, DT)
        tend = {k: (buf[names.get(k, k)] / (hex_ if k == "theta" else 1.0) - hF[k]) / DT - (hadv[k] + hdiv[k]) for k in F}
        return tend, ppt

    def wall(fn):
        t = []
        for i in range(1 + a.host_reps):
            t0 = time.perf_counter()
            fn()
            if i:
                t.append(time.perf_counter() - t0)
        return float(np.median(t)) * 1e3
    t_host = wall(lambda: m.kid_interface_host(hF, DT, P0, R_ON_CP, hex_, hdz, adv=hadv, div=hdiv))
    t_numpy = wall(numpy_adapter)
    res["host"] = {"ms_kid_interface_host": round(t_host, 3), "ms_numpy_adapter_plus_batch_step_host": round(t_numpy, 3),
                   "column_steps_per_s_kid_interface_host": round(ncol / (t_host * 1e-3), 1),
                   "column_steps_per_s_numpy_adapter": round(ncol / (t_numpy * 1e-3), 1), "reps": a.host_reps}
    m.close()
    return res


def fortran_rates(a):
    exe = os.path.join(ROOT, "kid_amd", "fortran", "build", "kid_devadapter_driver")
    if not os.path.exists(exe):
        return {"error": "kid_devadapter_driver not built"}
    out = {"nx": a.fortran_nx, "steps": a.fortran_steps, "threads": 16}
    for sw in ("0", "1"):
        r = subprocess.run([exe, str(a.fortran_nx), str(a.fortran_steps), "mixed", "adapter=" + sw, "rates=0", "forcing=1", "time=1"],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="16"))
        rate = [float(line.split()[3]) for line in r.stdout.splitlines() if line.startswith("TIME")]
        out["switch_" + ("on" if sw == "1" else "off")] = rate[0] if r.returncode == 0 and rate else "failed: " + (r.stdout + r.stderr)[-300:]
    return out


def report(results, fortran, device):
    fp = results[0]["fingerprint"]
    lines = ["KiD adapter on the device (kidmp_kid_interface_*): fp64, nz = 120, device %s" % device,
             "median of %d launches, device events around every launch; back-out = call - gather - step (derived)" % results[0]["launches"]]
    for r in results:
        for label, x in r["device"].items():
            lines.append("%s %d columns, forcing %-4s: call %.4f ms, gather %.4f ms, step %.4f ms, back-out %.4f ms; call/step %.3f; "
                         "%.3e column-steps/s; gather %.0f MB at %.2f TB/s (%.0f%% of 8 TB/s), back-out %.0f MB at %.2f TB/s (%.0f%%)"
                         % (r["workload"], r["ncol"], label, x["ms_call"], x["ms_gather"], x["ms_step"], x["ms_backout_derived"],
                            x["call_over_step"], x["column_steps_per_s"], x["gather_bytes"] / 1e6, x["gather_TBps"],
                            100 * x["gather_frac_of_8TBps"], x["backout_bytes"] / 1e6, x["backout_TBps_derived"],
                            100 * x["backout_frac_of_8TBps_derived"]))
        h = r["host"]
        lines.append("%s %d columns, host arrays (page-locked, both forcings): kid_interface_host %.2f ms (%.3e column-steps/s), "
                     "numpy gather + batch_step_host + numpy back-out %.2f ms (%.3e column-steps/s)"
                     % (r["workload"], r["ncol"], h["ms_kid_interface_host"], h["column_steps_per_s_kid_interface_host"],
                        h["ms_numpy_adapter_plus_batch_step_host"], h["column_steps_per_s_numpy_adapter"]))
    if fortran is not None:
        lines.append("Fortran drop-in, nx = %s mixed phase, forcing on, diagnostics off, %s threads, %s steps: "
                     "l_device_adapter off %s column-steps/s, on %s column-steps/s"
                     % (fortran.get("nx"), fortran.get("threads"), fortran.get("steps"),
                        *[("%.4e" % fortran[k]) if isinstance(fortran.get(k), float) else str(fortran.get(k)) for k in ("switch_off", "switch_on")]))
    return "\n".join("%s  [%s]" % (ln, fp) for ln in lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="config3,config2")
    ap.add_argument("--ncol", type=int, default=0, help="columns (default: bench.py's size of the workload)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--fortran-nx", type=int, default=50000)
    ap.add_argument("--fortran-steps", type=int, default=20)
    ap.add_argument("--no-fortran", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_kid_adapter.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_kid_adapter: no GPU visible (this measurement has no CPU path)")
    if a.launches < 20:
        sys.exit("bench_kid_adapter: at least 20 launches")
    results = [measure(w, a) for w in a.workloads.split(",")]
    fortran = None if a.no_fortran else fortran_rates(a)
    print(json.dumps({"metric": "KiD adapter on the device", "results": results, "fortran": fortran}), flush=True)
    text = report(results, fortran, torch.cuda.get_device_name(0))
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
