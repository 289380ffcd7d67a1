"""numpy restatement of the architecture relaxation of include/bmnas_hip.h (bmnas_arch_relax_fwd / _bwd), built on the
Philox restatement of oracle/philox.py.  TEST INFRASTRUCTURE ONLY.

The tensors of a call form one flat element sequence (tensor order, row-major) starting at flat index e0; element e draws
  w = philox4x32_10(ctr = (step << 32) + (e >> 2), key = seed ^ SALT)[e & 3]
  u = ((w >> 9) + 0.5) * 2^-23          exact in fp32, in [2^-24, 1 - 2^-24]
  G = -log(-log(u))
  z = (a + G) / tau                     every operation rounded on its own
"""
import numpy as np

from oracle.philox import philox4x32_10

SALT = 0x6A09E667F3BCC908
MASK64 = 0xFFFFFFFFFFFFFFFF


def words(seed, step, e0, count):
    """The uint32 word of each of the flat elements e0 .. e0 + count - 1."""
    e = np.arange(count, dtype=np.uint64) + np.uint64(e0)
    ctr = (np.uint64((int(step) << 32) & MASK64) + (e >> np.uint64(2))) & np.uint64(MASK64)
    four = philox4x32_10(ctr, (int(seed) ^ SALT) & MASK64)
    return four[np.arange(count), (e & np.uint64(3)).astype(np.int64)]


def uniform32(w):
    """u in fp32, every step exact."""
    w = np.asarray(w, dtype=np.uint32)
    return ((w >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def gumbel32(w):
    """G the way the kernel forms it: two fp32 logarithms of the fp32 u."""
    u = uniform32(w)
    return (-np.log(-np.log(u, dtype=np.float32), dtype=np.float32)).astype(np.float32)


def gumbel64(w):
    """G in float64 from the SAME (exact) u."""
    u = uniform32(w).astype(np.float64)
    return -np.log(-np.log(u))


def gumbel_bound(g64):
    """|G_fp32 - G_float64| allowed: 8 * 2^-23 * max(1, |G|) — two logarithms of 3 ulp each (OpenCL's bound, which the
    device library meets): the inner one's relative error is an absolute error of the outer one's result."""
    return 8.0 * 2.0 ** -23 * np.maximum(1.0, np.abs(g64))


def split(flat, shapes):
    out, at = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(flat[at:at + n].reshape(s))
        at += n
    return out


def noise64(shapes, seed, step, e0=0):
    """float64 G of every tensor of `shapes`."""
    total = sum(int(np.prod(s)) for s in shapes)
    return split(gumbel64(words(seed, step, e0, total)), shapes)


def noise32(shapes, seed, step, e0=0):
    total = sum(int(np.prod(s)) for s in shapes)
    return split(gumbel32(words(seed, step, e0, total)), shapes)


def relax(a, noise, tau):
    """fp32 z = (a + G) / tau per tensor (noise None: a / tau), add and division each rounded on their own."""
    tau = np.float32(tau)
    if noise is None:
        return [(np.asarray(x, np.float32) / tau).astype(np.float32) for x in a]
    return [((np.asarray(x, np.float32) + np.asarray(g, np.float32)).astype(np.float32) / tau).astype(np.float32)
            for x, g in zip(a, noise)]


def relax_bwd(dz, tau):
    tau = np.float32(tau)
    return [(np.asarray(g, np.float32) / tau).astype(np.float32) for g in dz]


def schedule(tau_max, tau_min, epochs, epoch):
    """tau_e = tau_max * (tau_min / tau_max) ** (e / (epochs - 1)) in float64; epochs == 1 gives tau_max."""
    if epochs == 1:
        return float(tau_max)
    return float(tau_max) * (float(tau_min) / float(tau_max)) ** (epoch / (epochs - 1))
