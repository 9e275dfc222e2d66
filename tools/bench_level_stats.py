#!/usr/bin/env python
"""tools/bench_level_stats.py -- time the per-level ensemble statistics (kidmp_level_stats_device, include/kidmp_stats.h)
on one MI355X against what a user can do without them: the torch composite on the device and the download of the arrays.

Workload: BASELINE config 3 (10^5 mixed-phase columns x 120 levels, fp64) after one column step, state in HBM.  Cases:
  a_one_field     1 field (t), moments only
  b_state_64bins  the 12 state profiles, moments + 64-bin histograms (edges: 65 equal steps over each field's range)
  c_outputs_8grp  dBZ + the three radii of column_outputs, 8 ensemble groups, moments + 19 bins (dBZ: 5-dB edges from -35)
Per case, in ONE process, warmed up, alternating in blocks of --block calls, --blocks times each, a block timed with
device events around it:
  level_stats     the entry (two launches; workspace and outputs allocated once, outside the timing)
  torch           per field and group: mean / var / amin / amax over dim 0, and bucketize + scatter_add_ per level for the
                  histogram (NaN, the floor and the non-finite values are NOT treated: the composite does less)
  download        the same arrays copied into page-locked host memory (what a host-side reduction would need first)
Prints one JSON line for the run (date, device, the column kernel's fingerprint) and one per case: ms_min / ms_mean of each
variant, the bytes of the fields (what the algorithm must read) and level_stats' bytes / time as a fraction of the 8 TB/s
HBM roofline, and whether count / min / max agree with torch's where the composite computes them.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NZ = 120
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()

    import numpy as np
    import torch
    import cases
    from kid_amd import STATE_NAMES, ThompsonMP
    from kid_amd.stats import NMOM, _StatsRequest, library

    if not torch.cuda.is_available():
        sys.exit("bench_level_stats: no GPU visible (this measurement has no CPU path)")
    L = library()
    m = ThompsonMP(iiwarm=False, device=0)
    ncol = a.ncol
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in cases.config3(ncol).items()}
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                 # config 3 after one step
    dbz, radii = m.column_outputs(dev)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    group8 = (torch.arange(ncol, device="cuda:0") % 8).to(torch.int32)

    def spread(x, nbin):
        lo, hi = float(x.min()), float(x.max())
        return np.linspace(lo, hi if hi > lo else lo + 1.0, nbin + 1)

    outs = {"dbz": dbz, "re_qc": radii[0], "re_qi": radii[1], "re_qs": radii[2]}
    case_list = [
        ("a_one_field", {"t": dev["t"]}, None, 1, None, None),
        ("b_state_64bins", {k: dev[k] for k in STATE_NAMES}, None, 1, {k: spread(dev[k], 64) for k in STATE_NAMES}, None),
        ("c_outputs_8grp", outs, group8, 8, dict({k: spread(outs[k], 19) for k in outs}, dbz=np.arange(-35.0, 65.0, 5.0)),
         {"dbz": -35.0}),
    ]
    print(json.dumps({"metric": "per-level ensemble statistics fp64, config3 after one step", "ncol": ncol, "nz": NZ,
                      "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0),
                      "fingerprint": m.kernel_fingerprint(), "block": a.block, "blocks": a.blocks, "warmup": a.warmup}), flush=True)

    for name, fields, group, ngroup, edges, floor in case_list:
        names, tensors = list(fields), list(fields.values())
        nfield = len(names)
        nbin = 0 if edges is None else len(edges[names[0]]) - 1
        need = int(L.kidmp_stats_workspace_bytes(ncol, NZ, nfield, ngroup, nbin))
        work = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        mom = torch.empty(ngroup, nfield, NMOM, NZ, dtype=torch.float64, device="cuda:0")
        hist = torch.empty(ngroup, nfield, NZ, nbin + 3, dtype=torch.int64, device="cuda:0") if nbin else None
        d_edges = torch.from_numpy(np.stack([np.asarray(edges[k], dtype=np.float64) for k in names])).to("cuda:0") if nbin else None
        req = _StatsRequest()
        ptrs = (C.c_void_p * nfield)(*[x.data_ptr() for x in tensors])
        floors = (C.c_double * nfield)(*[float((floor or {}).get(k, -np.inf)) for k in names])
        req.nfield, req.field, req.floor = nfield, C.cast(ptrs, C.POINTER(C.c_void_p)), C.cast(floors, C.POINTER(C.c_double))
        req.group, req.ngroup, req.nbin = (group.data_ptr() if group is not None else None), ngroup, nbin
        req.edges = d_edges.data_ptr() if nbin else None

        def level_stats():
            rc = L.kidmp_level_stats_device(m._h, ncol, NZ, C.byref(req), mom.data_ptr(), hist.data_ptr() if nbin else None,
                                            work.data_ptr(), need, s)
            if rc != 0:
                sys.exit("bench_level_stats: entry failed (%d): %s" % (rc, L.kidmp_last_error(m._h).decode()))

        members = [torch.nonzero(group == g).squeeze(1) for g in range(ngroup)] if group is not None else [None]
        level_of = torch.arange(NZ, device="cuda:0") * (nbin + 2)
        kept = {}

        def composite():
            for g, idx in enumerate(members):
                for f, x in enumerate(tensors):
                    xs = x if idx is None else x.index_select(0, idx)
                    r = [xs.mean(0), xs.var(0, unbiased=False), xs.amin(0), xs.amax(0)]
                    if nbin:
                        slot = torch.bucketize(xs, d_edges[f], right=True) + level_of
                        h = torch.zeros(NZ * (nbin + 2), dtype=torch.int64, device="cuda:0")
                        h.scatter_add_(0, slot.reshape(-1), torch.ones(slot.numel(), dtype=torch.int64, device="cuda:0"))
                        r.append(h)
                    kept[(g, f)] = r

        pinned = [torch.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in tensors]

        def download():
            for p, x in zip(pinned, tensors):
                p.copy_(x, non_blocking=True)

        variants = {"level_stats": level_stats, "torch": composite, "download": download}
        for _ in range(a.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.blocks):                    # alternating: a block of every variant, then the next round
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.block):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.block)
        torch.cuda.synchronize()
        # agreement where the composite computes the same thing: fields without NaN / inf and without a floor
        agree = True
        for (g, f), r in kept.items():
            if floor and names[f] in floor:
                continue
            agree = agree and bool(torch.equal(r[2], mom[g, f, 3]) and torch.equal(r[3], mom[g, f, 4])
                                   and torch.allclose(r[0], mom[g, f, 1], rtol=1e-12, atol=0.0))
            if nbin:
                agree = agree and bool(torch.equal(r[4].view(NZ, nbin + 2), hist[g, f, :, :nbin + 2]))
        field_bytes = nfield * ncol * NZ * 8
        res = {"case": name, "nfield": nfield, "ngroup": ngroup, "nbin": nbin, "field_bytes": field_bytes, "workspace_bytes": need,
               "agrees_with_torch": agree}
        for k, t in times.items():
            res[k] = {"ms_min": round(min(t), 4), "ms_mean": round(sum(t) / len(t), 4), "ms_max": round(max(t), 4)}
        t_min = res["level_stats"]["ms_min"] * 1e-3
        res["level_stats"]["field_TBps_at_min"] = round(field_bytes / t_min / 1e12, 4)
        res["level_stats"]["fraction_of_8TBps_roofline"] = round(field_bytes / t_min / HBM_PEAK, 4)
        res["torch_over_level_stats"] = round(res["torch"]["ms_min"] / res["level_stats"]["ms_min"], 3)
        res["download_over_level_stats"] = round(res["download"]["ms_min"] / res["level_stats"]["ms_min"], 3)
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()
    m.close()


if __name__ == "__main__":
    main()
