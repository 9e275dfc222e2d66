"""The geometry cases of the range-height scan (include/kidmp_scan.h), shared by tests/test_scan_abi.py, which runs them
through kid_amd/csrc/kidmp_scan_geom.h on the host, and tests/test_gpu_scan.py, which runs them through k_scan.

A case is a dict: name, nz, nx, nslab, ngate, periodic, half_inv_ae, r0, dr, dx, zf [nz+1], rays [nrow, 6] (nsub = 1).
"""
import itertools

import numpy as np

import scan_ref as ref

NZS = (2, 63, 64, 65, 256)
NXS = (3, 7, 64)
NGATES = (1, 63, 64, 65, 130, 1024)
ELEVATIONS = (0.5, 30.0, 90.0, 150.0)        # at 150 degrees ce < 0 and x is negative: floor and wrap act on negative numbers
A_E = 8.5e6
NSLAB = 2
DX, R0, DR, TOP = 1000.0, 150.0, 97.3, 12000.0


def sweep_rows(nx, dx=DX):
    """Both slabs' sweep over ELEVATIONS from a radar a little off a cell centre, then the rows no gate of which is inside:
    a slab that is not one, weights that are none, a NaN row, positions beyond every cell index."""
    x0, z0 = 0.37 * nx * dx, 10.0
    rows = [ref.unit_rows(s, x0, z0, ELEVATIONS) for s in range(NSLAB)]
    nan, inf = float("nan"), float("inf")
    ce, se = rows[0][1, 3], rows[0][1, 4]
    bad = [[2.0, x0, z0, ce, se, 1.0], [-1.0, x0, z0, ce, se, 1.0], [0.5, x0, z0, ce, se, 1.0], [nan, x0, z0, ce, se, 1.0],
           [0.0, x0, z0, ce, se, 0.0], [0.0, x0, z0, ce, se, -1.0], [1.0, x0, z0, ce, se, inf], [1.0, x0, z0, ce, se, nan],
           [nan] * 6, [0.0, inf, z0, ce, se, 1.0], [0.0, x0, -inf, ce, se, 1.0], [0.0, 1e300, z0, ce, se, 1.0],
           [1.0, -1e19, z0, ce, se, 1.0], [1.0, x0, z0, nan, se, 1.0], [0.0, 2.0 ** 52 * dx, z0, 0.0, 1.0, 1.0],
           [0.0, -3.0 * dx, z0, 0.0, 1.0, 1.0]]                     # the last: a whole number of cells to the left, vertical
    return np.concatenate(rows + [np.array(bad)])


def case(nz, nx, ngate, periodic, curved):
    return dict(name="nz%d-nx%d-ng%d-p%d-c%d" % (nz, nx, ngate, periodic, curved), nz=nz, nx=nx, nslab=NSLAB, ngate=ngate,
                periodic=periodic, half_inv_ae=1.0 / (2.0 * A_E) if curved else 0.0, r0=R0, dr=DR, dx=DX,
                zf=ref.stretched_faces(nz, TOP), rays=sweep_rows(nx))


def on_the_face():
    """A vertical beam over uniform levels of 125 m with r0 = 0 and dr = 250: every gate centre lies exactly on a face and
    belongs to the level above it; x0 on the edge between cells 1 and 2 belongs to cell 2.  The top gates leave the slab."""
    nz, nx = 40, 7
    zf = 125.0 * np.arange(nz + 1)
    rays = np.array([[0.0, 2.0 * DX, 0.0, 0.0, 1.0, 1.0], [1.0, 0.0, 0.0, 0.0, 1.0, 1.0], [1.0, 7.0 * DX, 0.0, 0.0, 1.0, 1.0]])
    return dict(name="on-the-face", nz=nz, nx=nx, nslab=NSLAB, ngate=24, periodic=0, half_inv_ae=0.0, r0=0.0, dr=250.0, dx=DX, zf=zf,
                rays=rays)


def full(nz):
    """Every combination of the ranges at one nz: 72 cases."""
    return [case(nz, nx, ng, p, c) for nx, ng, p, c in itertools.product(NXS, NGATES, (0, 1), (0, 1))]


def covering():
    """Every nz with every ngate, the other ranges cycling so that each of their values meets each nz and each ngate: the
    30 cases the host program prints, and the face case."""
    out = []
    for a, nz in enumerate(NZS):
        for b, ng in enumerate(NGATES):
            out.append(case(nz, NXS[(a + b) % 3], ng, (a + b // 3) % 2, (a // 2 + b) % 2))
    return out + [on_the_face()]


def reference(c):
    """(valid [nrow], inside, i, k [nrow, ngate], h [nrow, ngate]) of a case by scan_ref."""
    rows = c["rays"]
    valid = np.array([ref.ray_valid(r, c["nslab"]) for r in rows])
    g = [ref.geometry(r, c["zf"], c["dx"], c["nx"], c["r0"], c["dr"], c["ngate"], c["half_inv_ae"], c["periodic"]) for r in rows]
    return valid, np.array([x[0] for x in g]), np.array([x[1] for x in g]), np.array([x[2] for x in g]), np.array([x[3] for x in g])
