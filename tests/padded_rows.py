"""Padded rows for the host entries whose C ABI takes a column stride (dz_col_stride, k_gas_col_stride) that the Python
layer never sets to anything but nz: the wrapper is called as usual and, on the way into the library, the packed [ncol, nz]
array is replaced by a copy with rows of nz + PAD elements and the stride that goes with it."""
import numpy as np

PAD = 5
FILL = -7.0                                                    # what the padding holds: a depth nobody may read


def widen(a):
    """[ncol, nz] -> contiguous [ncol, nz + PAD], the rows' tails filled with FILL"""
    wide = np.full((a.shape[0], a.shape[1] + PAD), FILL, dtype=a.dtype)
    wide[:, :a.shape[1]] = a
    return wide


def with_padded(monkeypatch, L, name, at):
    """Entry `name` of the library L takes, for this test, its argument at[i] (a pointer, followed by its column stride) as
    the widened copy of the array found there; at: {argument index: the packed array the wrapper will pass}.  Returns the
    list of calls made, as (index, stride) pairs, so that the test can see that the substitution took place."""
    fn, seen = getattr(L, name), []
    wide = {i: widen(a) for i, a in at.items()}

    def call(*args):
        args = list(args)
        for i, a in at.items():
            assert args[i] == a.ctypes.data and args[i + 1] == a.shape[1], (name, i)
            args[i], args[i + 1] = wide[i].ctypes.data, a.shape[1] + PAD
            seen.append((i, args[i + 1]))
        return fn(*args)

    monkeypatch.setattr(L, name, call)
    return seen
