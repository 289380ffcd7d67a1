"""Shared by tests/test_fc_edges_gpu.py and tests/test_fc_edges_network_gpu.py; the float64 activations and the
NaN-guarded buffers by tests/test_found_fc_abi_gpu.py, tests/test_fc_edges_kernels_gpu.py and tests/fc_sum_ref.py."""
import contextlib

import numpy as np
import torch


def act64(u, mish):
    return u * torch.tanh(torch.nn.functional.softplus(u)) if mish else torch.relu(u)


def dact64(u, mish):
    if not mish:
        return (u > 0).double()
    sp = torch.nn.functional.softplus(u)
    t = torch.tanh(sp)
    return t + u * torch.sigmoid(u) * (1 - t * t)


def guarded(n_rows, row_shape, guard=2):
    """n_rows tensors of row_shape laid out in one NaN-filled buffer with `guard` NaN rows in front of, between and
    behind them -> (buffer, views, guard views)."""
    from gpu_util import dev
    per = int(np.prod(row_shape))
    buf = torch.full(((guard + 1) * n_rows + guard, per), float('nan'), device=dev(), dtype=torch.float32)
    rows = [buf[guard + (guard + 1) * i].view(*row_shape) for i in range(n_rows)]
    keep = torch.ones(buf.shape[0], dtype=torch.bool)
    for i in range(n_rows):
        keep[guard + (guard + 1) * i] = False
    return buf, rows, keep.to(dev())


def guards_intact(buf, keep):
    return bool(torch.isnan(buf[keep]).all())


@contextlib.contextmanager
def edited_primitives(prims):
    """PRIMITIVES edited in place (every module holds the same list object) and restored."""
    import models.search.darts.genotypes as gt
    saved = list(gt.PRIMITIVES)
    gt.PRIMITIVES[:] = prims
    try:
        yield
    finally:
        gt.PRIMITIVES[:] = saved


@contextlib.contextmanager
def recorded_sites():
    """Collects (descriptor, numel) of every live dropout site the HIP path issues, in issue order."""
    from bmnas import cell as K
    assert K.DROP.record is None
    K.DROP.record = rec = []
    try:
        yield rec
    finally:
        K.DROP.record = None


def device_kernels(fn):
    """Names of the device events (kernels, memcpys, memsets) of one call of fn, under torch.profiler."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
