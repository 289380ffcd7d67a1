"""Reference for bmnas_grad_combine_multi (csrc/accum.hip): grad = sum_i w_i * part_i in numpy fp32, ONE rounding per
operation (no fused multiply-add), over the non-NULL parts in ascending order; a None part is left out, not added as
zero.  tests/test_accum_ref.py pins it bit for bit to torch.mul / torch.add on the CPU."""
import numpy as np


def combine(parts, weights, shape=None):
    """parts: list of fp32 arrays or None; weights: as many floats (taken as fp32, like the kernel's arguments).
    -> fp32 array; with every part None, +0 of `shape`."""
    if len(parts) != len(weights):
        raise ValueError('one weight per part')
    acc = None
    for g, w in zip(parts, weights):
        if g is None:
            continue
        g = np.asarray(g)
        assert g.dtype == np.float32
        with np.errstate(all='ignore'):
            t = np.multiply(np.float32(w), g, dtype=np.float32)
            acc = t if acc is None else np.add(acc, t, dtype=np.float32)
    if acc is None:
        return np.zeros(shape, dtype=np.float32)
    return acc
