#!/usr/bin/env python
"""tools/bench_kid_ultimate.py -- time the two advection schemes of include/kidmp_advection.h (van Leer and ULTIMATE
QUICKEST: the two instantiations of kidmp::k_kid_advect and kidmp::k_kid_advect_slab) against one another on one MI355X.

Workloads: 10^5 and 10^4 mixed-phase columns x 120 levels (BASELINE config 3) in KiD's theta form, fp64, state in HBM; the
1-D cases with the per-column w of tools/bench_kid_advect.py (Courant <= 0.64), the slab cases as --nx (1000) cells per
slab, i.e. 100 and 10 periodic slabs, with the stream-function flow of tools/bench_kid_slab.py (unsplit courant 0.5).  Both
schemes run in ONE process on the same state and the same context, taking turns launch by launch (the scheme is set before
the timed span); every launch is timed with device events of its own and the median of --reps (30) launches after --warmup
is reported with the minimum and maximum beside it.  Cases, for each scheme:
  advect_sum       advect(want="sum") with courant: what a run step calls          (17 280 algorithmic B/column)
  advect_adv_div   advect(want=("adv", "div"))                                     (25 920 B/column)
  run_step         one full step of kid_run: advect, kid_interface, update, the ppt accumulation
  advect_slab_sum  advect_slab(want="sum") with courant                            (19 200 B/column)
  run_slab_step    one full step of kid_run_slab
The state is put back before every launch that changes it (outside the timed span).  The ULTIMATE / van Leer ratio of every
case and the achieved share of 8 TB/s on the algorithmic bytes are printed.

--parent-lib PATH (a build of the parent commit's library) adds an A/B of the van Leer path: tools/bench_kid_advect.py and
tools/bench_kid_slab.py are run as child processes, in turn with --lib PATH and with this tree's library, --ab-rounds (2)
times each, and the medians of advect_sum and advect_slab_sum of every run are printed with their spread.

Prints one line per case and workload and ONE JSON line at the end; the lines also go to --out under a header with the
date and the library's fingerprint."""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NZ = 120
HBM_PEAK = 8.0e12
P0, R_ON_CP, DT = 1.0e5, 287.058 / 1005.0, 10.0
SCHEMES = ("vanleer", "ultimate")


def kid_state(ncol):
    """config 3 in KiD's theta form: (fields, exner, rho, dz) as numpy arrays."""
    import cases
    from kid_amd import KID_FIELDS
    st = cases.config3(ncol)
    exner = (st["p"] / P0) ** R_ON_CP
    F = {k: st[k] for k in KID_FIELDS[1:]}
    F["theta"] = st["t"] / exner
    rho = 0.622 * st["p"][0] / (287.04 * st["t"][0] * (st["qv"][0] + 0.622))
    return F, exner, rho, st["dz"][0]


def time_variants(m, variants, restore, reps, warmup):
    """variants: name -> (scheme, call, changes the state).  Median / min / max of `reps` launches each, taking turns."""
    import torch
    for _ in range(warmup):
        for scheme, fn, _c in variants.values():
            m.set_advection(scheme)
            fn()
    restore()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, (scheme, fn, changes) in variants.items():
            if changes:
                restore()
            m.set_advection(scheme)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    m.set_advection("vanleer")
    return {k: {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)} for k, t in times.items()}


def report(say, res, ncol, cases_bytes):
    """Lines of one workload: every case under both schemes, the share of 8 TB/s and the ratio."""
    for case, nbytes in cases_bytes.items():
        for scheme in SCHEMES:
            r = res[case][scheme]
            extra = ""
            if nbytes is not None:
                r["algo_bytes_per_column"] = nbytes
                r["share_of_8TBs"] = nbytes * ncol / (r["ms_median"] * 1e-3) / HBM_PEAK
                extra = "   %6d B/column -> %5.1f %% of 8 TB/s" % (nbytes, 100.0 * r["share_of_8TBs"])
            say("ncol=%-6d %-15s %-8s median %8.4f ms   min %8.4f   max %8.4f%s"
                % (ncol, case, scheme, r["ms_median"], r["ms_min"], r["ms_max"], extra))
        res[case]["ultimate_over_vanleer"] = res[case]["ultimate"]["ms_median"] / res[case]["vanleer"]["ms_median"]
        say("ncol=%-6d %-15s ULTIMATE / van Leer = %.3f" % (ncol, case, res[case]["ultimate_over_vanleer"]))


def measure_1d(a, ncol, say):
    import numpy as np
    import torch
    from kid_amd import KID_FIELDS, ThompsonMP
    m = ThompsonMP(iiwarm=False, device=0)
    F, exner, rho, dz = kid_state(ncol)
    rng = np.random.Generator(np.random.PCG64(15))                   # the w of tools/bench_kid_advect.py
    f = np.arange(NZ + 1) / float(NZ)
    w = rng.uniform(0.3, 1.0, (ncol, 1)) * 8.0 * np.sin(np.pi * f * rng.integers(1, 3, (ncol, 1)))[:, :]
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")   # noqa: E731
    first = {k: cu(F[k]) for k in KID_FIELDS}
    state = {k: v.clone() for k, v in first.items()}
    dw, drho, ddz, dex = cu(w), cu(rho), cu(dz), cu(exner)

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

    calls = {"advect_sum": (lambda: m.kid_advect(state, dw, drho, ddz, DT, want="sum", courant=True, out=o_sum), False),
             "advect_adv_div": (lambda: m.kid_advect(state, dw, drho, ddz, DT, want=("adv", "div"), out=o_ad), False),
             "run_step": (run_step, True)}
    m.set_advection("ultimate")
    differs = float((m.kid_advect(state, dw, drho, ddz, DT)["sum"]["qv"] != o_sum["sum"]["qv"]).double().mean())
    m.set_advection("vanleer")
    say("ncol=%-6d 1-D: courant max %.3f; the two schemes' sum[qv] differ in %.1f %% of the cells" % (ncol, float(o_sum["courant"].max()), 100.0 * differs))
    t = time_variants(m, {"%s/%s" % (c, s): (s, fn, ch) for c, (fn, ch) in calls.items() for s in SCHEMES}, restore, a.reps, a.warmup)
    res = {c: {s: t["%s/%s" % (c, s)] for s in SCHEMES} for c in calls}
    report(say, res, ncol, {"advect_sum": 18 * NZ * 8, "advect_adv_div": 27 * NZ * 8, "run_step": None})
    m.close()
    return dict(res, ncol=ncol, nz=NZ, reps=a.reps)


def measure_slab(a, ncol, say):
    import numpy as np
    import torch
    from kid_amd import KID_FIELDS, ThompsonMP, streamfunction_flow
    nx = a.nx
    assert ncol % nx == 0, (ncol, nx)
    nslab = ncol // nx
    m = ThompsonMP(iiwarm=False, device=0)
    F, exner, rho, dz = kid_state(ncol)
    dx = 4.0 * float(dz.mean())
    rng = np.random.Generator(np.random.PCG64(16))                   # the flow of tools/bench_kid_slab.py
    x = (np.arange(nx) / float(nx))[None, :, None]
    f = (np.arange(NZ + 1) / float(NZ))[None, None, :]
    waves = rng.integers(1, 4, (nslab, 1, 1))
    psi = rng.uniform(0.3, 1.0, (nslab, 1, 1)) * np.sin(2.0 * np.pi * waves * x + rng.uniform(0.0, 6.0, (nslab, 1, 1))) * np.sin(np.pi * f)
    cu = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")   # noqa: E731
    first = {k: cu(F[k]) for k in KID_FIELDS}
    state = {k: v.clone() for k, v in first.items()}
    drho, ddz, dex = cu(rho), cu(dz), cu(exner)
    du, dw = streamfunction_flow(cu(psi.reshape(ncol, NZ + 1)), drho, ddz, dx, nx=nx)
    one = float(m.kid_advect_slab(state, du, dw, drho, ddz, dx, DT, nx, want=(), courant=True)["courant"].max())
    du, dw = du * (0.5 / one), dw * (0.5 / one)

    def restore():
        for k in KID_FIELDS:
            state[k].copy_(first[k])

    o_sum = m.kid_advect_slab(state, du, dw, drho, ddz, dx, DT, nx, want="sum", courant=True)
    work = m.kid_workspace(ncol, NZ, torch.float64)
    mphys = m.kid_interface(state, DT, P0, R_ON_CP, dex, ddz, adv=o_sum["sum"], work=work)
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")

    def run_step():
        m.kid_advect_slab(state, du, dw, drho, ddz, dx, DT, nx, want="sum", courant=True, out=o_sum)
        m.kid_interface(state, DT, P0, R_ON_CP, dex, ddz, adv=o_sum["sum"], work=work, out=mphys)
        m.kid_update(state, DT, o_sum["sum"], mphys)
        ppt.add_(mphys["ppt"])

    calls = {"advect_slab_sum": (lambda: m.kid_advect_slab(state, du, dw, drho, ddz, dx, DT, nx, want="sum", courant=True, out=o_sum), False),
             "run_slab_step": (run_step, True)}
    say("ncol=%-6d = %d slabs x %d cells; courant max %.3f" % (ncol, nslab, nx, float(o_sum["courant"].max())))
    t = time_variants(m, {"%s/%s" % (c, s): (s, fn, ch) for c, (fn, ch) in calls.items() for s in SCHEMES}, restore, a.reps, a.warmup)
    res = {c: {s: t["%s/%s" % (c, s)] for s in SCHEMES} for c in calls}
    report(say, res, ncol, {"advect_slab_sum": 20 * NZ * 8, "run_slab_step": None})
    m.close()
    return dict(res, ncol=ncol, nslab=nslab, nx=nx, nz=NZ, reps=a.reps)


def parent_ab(a, say):
    """The van Leer path of this tree against the parent commit's library, through the parent's own two tools."""
    out = {}
    for tool, case in (("bench_kid_advect.py", "advect_sum"), ("bench_kid_slab.py", "advect_slab_sum")):
        runs = {"parent": [], "this": []}
        for rnd in range(a.ab_rounds):
            for who, lib in (("parent", a.parent_lib), ("this", None)):
                with tempfile.TemporaryDirectory() as tmp:
                    cmd = [sys.executable, os.path.join(ROOT, "tools", tool), "--reps", str(a.reps), "--warmup", str(a.warmup),
                           "--ncols"] + [str(n) for n in a.ncols] + ["--out", os.path.join(tmp, "out.txt")]
                    if lib:
                        cmd += ["--lib", lib]
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.ab_timeout)
                    if p.returncode != 0:
                        sys.exit("bench_kid_ultimate: %s failed (%d):\n%s" % (" ".join(cmd), p.returncode, p.stderr[-2000:]))
                    results = json.loads(p.stdout.strip().splitlines()[-1])["results"]
                runs[who].append({r["ncol"]: r[case] for r in results})
        for ncol in a.ncols:
            line = "ncol=%-6d %-15s van Leer through tools/%s:" % (ncol, case, tool)
            for who in ("parent", "this"):
                med = [r[ncol]["ms_median"] for r in runs[who]]
                line += "   %s medians %s ms (spread %.4f)" % (who, " ".join("%.4f" % x for x in med), max(med) - min(med))
                out.setdefault(case, {}).setdefault(str(ncol), {})[who] = {"ms_medians": med, "ms_min": [r[ncol]["ms_min"] for r in runs[who]]}
            p_med = statistics.median(out[case][str(ncol)]["parent"]["ms_medians"])
            t_med = statistics.median(out[case][str(ncol)]["this"]["ms_medians"])
            out[case][str(ncol)]["this_over_parent"] = t_med / p_med
            say(line + "   this / parent = %.4f" % (t_med / p_med))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ncols", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--nx", type=int, default=1000, help="cells per slab; every --ncols must be a multiple")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library: adds the A/B of the van Leer path")
    ap.add_argument("--ab-rounds", type=int, default=2)
    ap.add_argument("--ab-timeout", type=float, default=600.0, help="seconds allowed to one child run of the A/B")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_kid_ultimate.txt"))
    a = ap.parse_args()
    import torch
    import kid_amd
    if not torch.cuda.is_available():
        sys.exit("bench_kid_ultimate: no GPU visible (this measurement has no CPU path)")
    m = kid_amd.ThompsonMP(iiwarm=True, device=0)
    lines = ["# tools/bench_kid_ultimate.py  %s  %s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0)),
             "# fingerprint: %s" % m.kernel_fingerprint()]
    m.close()

    def say(s):
        print(s, flush=True)
        lines.append(s)

    res = {"bench": "kid_ultimate", "device": torch.cuda.get_device_name(0),
           "one_d": [measure_1d(a, n, say) for n in a.ncols], "slab": [measure_slab(a, n, say) for n in a.ncols]}
    if a.parent_lib:
        torch.cuda.synchronize()
        res["parent_ab"] = parent_ab(a, say)
    lines.append(json.dumps(res))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
