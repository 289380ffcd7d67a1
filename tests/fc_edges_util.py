"""Shared by tests/test_fc_edges_gpu.py and tests/test_fc_edges_network_gpu.py."""
import contextlib


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
