#!/usr/bin/env python
"""tools/bench_kid_slab.py -- time the slab advection (include/kidmp_slab.h: one launch of kidmp::k_kid_advect_slab) on one
MI355X beside the 1-D advection on the same state, a torch composite of the same bits and the adapter it feeds.

Workloads: 10^5 and 10^4 mixed-phase columns x 120 levels (BASELINE config 3) in KiD's theta form, fp64, state in HBM, as
--nx (1000) cells per slab, i.e. 100 and 10 periodic slabs; a stream-function flow per slab (both signs of u and w) scaled
to an unsplit courant number of 0.5.  All variants run in ONE process, warmed up, taking turns launch by launch; every
launch is timed with device events of its own and the median of --reps (30) launches is reported with the minimum and
maximum beside it.  Variants:
  advect_slab_sum  advect_slab(want="sum") with courant: what a run_slab step calls
  advect_1d_sum    the 1-D advect(want="sum") with courant on the same state and w: a lower bound, the slab entry does
                   strictly more
  composite        the same `sum` of the nine fields from torch operations on the device tensors (checked against
                   advect_slab once: the difference must be zero)
  kid_interface    the adapter alone on the same state (adv = sum)
  run_slab_step    one full step of run_slab(): advect_slab, kid_interface, update, the ppt accumulation
The state is put back before every launch that changes it (outside the timed span).  Algorithmic bytes per column:
advect_slab(sum) reads nine profiles and writes nine, plus one profile of u and one of w; its share of 8 TB/s is printed.
Prints one line per variant and workload and ONE JSON line at the end; the lines also go to --out
(profiles/r16_kid_slab.txt) under a header with the date and the library's fingerprint."""
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
HBM_PEAK = 8.0e12
P0, R_ON_CP, DT = 1.0e5, 287.058 / 1005.0, 10.0


def torch_composite(state, u, w, rho, dz, dx, dt, nx):
    """tests/kid_slab_ref.py in torch, on device tensors: `sum` of every member of `state`, operation for operation."""
    import torch
    nz = rho.shape[0]
    rf = torch.cat([rho[:1], 0.5 * (rho[:-1] + rho[1:]), rho[-1:]])
    M = rf[None, :] * w
    up = w[:, 1:nz] >= 0
    c = (w[:, 1:nz].abs() * dt) / torch.where(up, dz[None, :-1], dz[None, 1:])
    hc = 0.5 * (1.0 - c)
    den = (rho * dz)[None, :]
    dM = (M[:, 1:] - M[:, :-1]) / den
    f = torch.arange(1, nz, device=w.device)[None, :]
    inside = torch.where(up, f >= 2, f + 1 < nz)
    ncol = u.shape[0]
    x3 = lambda a: a.view(ncol // nx, nx, nz)   # noqa: E731
    dx = torch.full((), dx, dtype=u.dtype, device=u.device)      # a tensor: torch divides by a Python number as a product with 1/dx
    Mx = rho * u
    pos = u >= 0
    hx = 0.5 * (1.0 - (u.abs() * dt) / dx)
    denx = (rho * dx)[None, :]
    dMx = (torch.roll(x3(Mx), -1, 1).reshape(ncol, nz) - Mx) / denx
    out = {}
    for k, q in state.items():
        pad = torch.nn.functional.pad(q, (2, 1))                     # pad[:, i + 2] = q[:, i]
        qm1, q0, qm2, qp1 = pad[:, 2:nz + 1], pad[:, 3:nz + 2], pad[:, 1:nz], pad[:, 4:nz + 3]      # of faces 1 .. nz-1
        qu, qd, quu = torch.where(up, qm1, q0), torch.where(up, q0, qm1), torch.where(up, qm2, qp1)
        dq, b = qd - qu, qu - quu
        bd = b * dq
        s = torch.where(inside & (bd > 0), (2.0 * bd) / torch.where(bd > 0, b + dq, torch.ones_like(bd)), torch.zeros_like(bd))
        qf = torch.cat([q[:, :1], qu + hc * s, q[:, -1:]], 1)
        F = M * qf
        advz = -((F[:, 1:] - F[:, :-1]) / den)
        left, left2, right = (torch.roll(x3(q), r, 1).reshape(ncol, nz) for r in (1, 2, -1))
        xu, xd, xuu = torch.where(pos, left, q), torch.where(pos, q, left), torch.where(pos, left2, right)
        dqx, bx = xd - xu, xu - xuu
        bdx = bx * dqx
        sx = torch.where(bdx > 0, (2.0 * bdx) / torch.where(bdx > 0, bx + dqx, torch.ones_like(bdx)), torch.zeros_like(bdx))
        Fx = Mx * (xu + hx * sx)
        advx = -((torch.roll(x3(Fx), -1, 1).reshape(ncol, nz) - Fx) / denx)
        out[k] = (advz + advx) + (q * dM + q * dMx)
    return out


def measure(a, ncol, lines):
    import numpy as np
    import torch
    import cases
    from kid_amd import KID_FIELDS, ThompsonMP, streamfunction_flow

    def say(s):
        print(s)
        lines.append(s)

    nx = a.nx
    assert ncol % nx == 0, (ncol, nx)
    nslab = ncol // nx
    m = ThompsonMP(iiwarm=False, device=0)
    st = cases.config3(ncol)
    exner = (st["p"] / P0) ** R_ON_CP
    F = {k: st[k] for k in KID_FIELDS[1:]}
    F["theta"] = st["t"] / exner
    rho = 0.622 * st["p"][0] / (287.04 * st["t"][0] * (st["qv"][0] + 0.622))
    dz = st["dz"][0]
    dx = 4.0 * float(dz.mean())
    rng = np.random.Generator(np.random.PCG64(16))
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
    o_1d = m.kid_advect(state, dw, drho, ddz, DT, want="sum", courant=True)
    work = m.kid_workspace(ncol, NZ, torch.float64)
    mphys = m.kid_interface(state, DT, P0, R_ON_CP, dex, ddz, adv=o_sum["sum"], work=work)
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")

    def run_step():
        m.kid_advect_slab(state, du, dw, drho, ddz, dx, DT, nx, want="sum", courant=True, out=o_sum)
        m.kid_interface(state, DT, P0, R_ON_CP, dex, ddz, adv=o_sum["sum"], work=work, out=mphys)
        m.kid_update(state, DT, o_sum["sum"], mphys)
        ppt.add_(mphys["ppt"])

    # name -> (call, algorithmic profiles per column or None, changes the state)
    variants = {
        "advect_slab_sum": (lambda: m.kid_advect_slab(state, du, dw, drho, ddz, dx, DT, nx, want="sum", courant=True, out=o_sum), 20, False),
        "advect_1d_sum": (lambda: m.kid_advect(state, dw, drho, ddz, DT, want="sum", courant=True, out=o_1d), 19, False),
        "composite": (lambda: torch_composite(state, du, dw, drho, ddz, dx, DT, nx), None, False),
        "kid_interface": (lambda: m.kid_interface(state, DT, P0, R_ON_CP, dex, ddz, adv=o_sum["sum"], work=work, out=mphys), None, False),
        "run_slab_step": (run_step, None, True),
    }
    comp = torch_composite(state, du, dw, drho, ddz, dx, DT, nx)
    diff = {k: float((o_sum["sum"][k] - comp[k]).abs().max() / o_sum["sum"][k].abs().max().clamp(min=1e-300)) for k in KID_FIELDS}
    say("ncol=%-6d = %d slabs x %d cells; composite - advect_slab_sum, max |difference| / max |profile|: %s   courant max %.3f"
        % (ncol, nslab, nx, "  ".join("%s %.1e" % kv for kv in diff.items()), float(o_sum["courant"].max())))
    for _ in range(a.warmup):
        for fn, _n, _c in variants.values():
            fn()
    restore()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, (fn, _n, changes) in variants.items():
            if changes:
                restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"ncol": ncol, "nslab": nslab, "nx": nx, "nz": NZ, "reps": a.reps, "composite_max_diff_over_max": max(diff.values())}
    for k, t in times.items():
        res[k] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
        nprof = variants[k][1]
        extra = ""
        if nprof is not None:
            res[k]["algo_bytes_per_column"] = nprof * NZ * 8
            res[k]["share_of_8TBs"] = res[k]["algo_bytes_per_column"] * ncol / (res[k]["ms_median"] * 1e-3) / HBM_PEAK
            extra = "   %6d B/column -> %5.1f %% of 8 TB/s" % (res[k]["algo_bytes_per_column"], 100.0 * res[k]["share_of_8TBs"])
        say("ncol=%-6d %-15s median %8.4f ms   min %8.4f   max %8.4f%s" % (ncol, k, res[k]["ms_median"], min(t), max(t), extra))
    ms = {k: res[k]["ms_median"] for k in variants}
    res["advect_slab_over_composite"] = ms["advect_slab_sum"] / ms["composite"]
    res["advect_slab_over_advect_1d"] = ms["advect_slab_sum"] / ms["advect_1d_sum"]
    res["kinematic_share_of_run_slab_step"] = (ms["run_slab_step"] - ms["kid_interface"]) / ms["run_slab_step"]
    say("ncol=%-6d advect_slab_sum %.3fx composite, %.2fx the 1-D advect; a run_slab step is %.4f ms, of which advection + update + "
        "accumulation add %.1f %% over kid_interface alone (%.4f ms)"
        % (ncol, res["advect_slab_over_composite"], res["advect_slab_over_advect_1d"], ms["run_slab_step"],
           100.0 * res["kinematic_share_of_run_slab_step"], ms["kid_interface"]))
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ncols", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--nx", type=int, default=1000, help="cells per slab; every --ncols must be a multiple")
    ap.add_argument("--lib", default=None, help="another build of the library (an A/B of the kernel)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_kid_slab.txt"))
    a = ap.parse_args()
    import torch
    import kid_amd
    if not torch.cuda.is_available():
        sys.exit("bench_kid_slab: no GPU visible (this measurement has no CPU path)")
    if a.lib:
        kid_amd.load_library(a.lib)
    m = kid_amd.ThompsonMP(iiwarm=True, device=0)
    lines = ["# tools/bench_kid_slab.py  %s  %s%s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0),
                                                       "  --lib " + a.lib if a.lib else ""),
             "# fingerprint: %s" % m.kernel_fingerprint()]
    m.close()
    results = [measure(a, n, lines) for n in a.ncols]
    lines.append(json.dumps({"bench": "kid_slab", "device": torch.cuda.get_device_name(0), "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
