"""Inputs of the rate-buffer tests (test_rates_inputs.py on the CPU, test_gpu_rates_shapes.py on the GPU): the smallest
batches that reach every level-count bucket of the column kernel (<1,64,4>, <2,120,4>, <2,128,1>, <3,192,1>, <4,256,1>)
from both sides of every edge, with all 36 rates non-zero somewhere from nz = 64 on.

Mixed phase and aerosol-aware: the five columns of test_gpu_pass5_handover._columns(nz) -- a melt at the T_0 crossing
with rain to the ground, a dry no_micro column (index DRY), heavy rain with graupel and no snow, snow at 1.5 R1 with
exact zeros, a column 1.3 K warmer; w = 2 m/s for an aerosol-aware context (activation needs an updraft).
Warm rain: the five columns of test_gpu_variants.test_other_level_counts_warm, frozen species present in two of them.
"""
import functools

import numpy as np

import cases
import kat_cases as kc
from test_gpu_pass5_handover import _batch as _handover_batch
from test_gpu_variants import _resample

NZ = (2, 17, 64, 65, 120, 121, 128, 129, 192, 193, 256)          # both sides of every bucket edge, and the smallest
NZ_WARM = (2, 33, 64, 65, 120, 121, 128, 190, 256)               # those of test_other_level_counts_warm
KINDS = ("mixed", "aero", "warm")
DRY = 1                                                           # the no_micro column of the mixed / aero batch
NCOL = 5
W_AERO = 2.0
DT = 10.0


def levels(kind):
    return NZ_WARM if kind == "warm" else NZ


@functools.lru_cache(maxsize=None)
def _warm_columns(nz):
    cols = [_resample(kc.kat_a(False), nz), _resample(kc.kat_a(True), nz), _resample(kc.kat_c(), nz),
            _resample(kc.kat_a(False), nz), _resample(kc.kat_a(False), nz)]
    cols[3]["qr"] = cols[3]["qr"] * 4.0
    return cols


def batch(kind, nz, pick=None):
    """A fresh [ncol, nz] float64 batch of the kind ("mixed", "aero", "warm", "warm_aero"); pick: column indices
    (default: all five, in order)."""
    pick = tuple(range(NCOL)) if pick is None else tuple(pick)
    if kind in ("mixed", "aero"):
        return _handover_batch(nz, len(pick), w=W_AERO if kind == "aero" else None, pick=pick)
    cols = [_warm_columns(nz)[i] for i in pick]
    st = {k: np.ascontiguousarray(np.stack([c[k] for c in cols])) for k in cases.KEYS}
    if kind == "warm_aero":
        st["w"][:] = W_AERO
    return st


def all_dry(kind, nz, ncol=NCOL):
    """ncol copies of the dry column: every column of the batch leaves at the no_micro exit."""
    return batch("aero" if kind == "aero" else "mixed", nz, pick=(DRY,) * ncol)


def to32(st):
    return {k: np.ascontiguousarray(v.astype(np.float32)) for k, v in st.items()}
