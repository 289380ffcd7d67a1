"""The rule of the reshape layers' pooling (csrc/pool.hip), stated on the CPU in numpy: AdaptiveMaxPool2d of
(b, C, H, W) to (oh, ow) with torch's adaptive windows, for fp32, bf16 and fp16 inputs.

  window of output row i   [floor(i H / oh), ceil((i + 1) H / oh)), columns alike
  forward                  the first maximum in row-major window order; a NaN is a maximum, and the first NaN of a
                           window is the one kept; the value is the fp32 widening of that element (exact), the index
                           its flat h * W + w (int32)
  backward                 dx[e] = the fp32 sum, in (i, j) order, of g over the windows whose argmax is e, rounded ONCE
                           (to nearest even) to the element type

tests/test_pool_ref.py pins this to F.adaptive_max_pool2d(..., return_indices=True) on the CPU.  One difference is
known and stated there: in a window that holds SEVERAL NaNs the aten CPU loop keeps the last of them (its update is
`val > max || isnan(val)`), the kernels keep the first — the value is a NaN either way, only the index differs.

Also the inputs the GPU tests share: few-level feature maps full of ties, with planted special windows, and upstream
gradients whose window sums are exact in fp32 whatever their order."""
import numpy as np
import torch


def windows(n_in, n_out):
    return [((i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)) for i in range(n_out)]


def pool_fwd(x, oh, ow):
    """x: (b, C, H, W) CPU tensor of any float type -> (out fp32 (b, C, oh * ow), idx int32 alike)"""
    v = x.detach().to(torch.float32).numpy()                     # exact for bf16 / fp16
    b, C, H, W = v.shape
    out = np.empty((b, C, oh * ow), np.float32)
    idx = np.empty((b, C, oh * ow), np.int32)
    for i, (hs, he) in enumerate(windows(H, oh)):
        for j, (ws, we) in enumerate(windows(W, ow)):
            ww = we - ws
            win = v[:, :, hs:he, ws:we].reshape(b, C, -1)
            nan = np.isnan(win)
            first_nan = nan.argmax(-1)
            first_max = np.where(nan, -np.inf, win).argmax(-1)   # np.argmax: the first occurrence
            sel = np.where(nan.any(-1), first_nan, first_max)
            out[:, :, i * ow + j] = np.take_along_axis(win, sel[..., None], -1)[..., 0]
            idx[:, :, i * ow + j] = (hs + sel // ww) * W + ws + sel % ww
    return torch.from_numpy(out), torch.from_numpy(idx)


def pool_bwd(g, idx, H, W, dtype):
    """g fp32 (b, C, n_out), idx int32 alike -> dx (b, C, H, W) of `dtype`: fp32 sums in output order, rounded once"""
    g = g.detach().to(torch.float32).numpy()
    idx = idx.numpy().astype(np.int64)
    b, C, n = g.shape
    dx = np.zeros((b, C, H * W), np.float32)
    for o in range(n):                                           # (i, j) order; one term per (b, C) and step
        cur = np.take_along_axis(dx, idx[:, :, o:o + 1], -1)
        np.put_along_axis(dx, idx[:, :, o:o + 1], (cur + g[:, :, o:o + 1]).astype(np.float32), -1)
    return torch.from_numpy(dx.reshape(b, C, H, W)).to(dtype)    # torch narrows to nearest even; a NaN stays a NaN


def make_input(shape, oh, ow, dtype, seed, several_nans=True):
    """(b, C, H, W) of `dtype`, to be pooled to (oh, ow): round(2 relu(x)) / 2 — zeros and ties in every window —,
    +0 / -0 mixed, one all-equal window, one all -inf window, a NaN in some planes and (several_nans) two adjacent NaNs."""
    b, C, H, W = shape
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.round(np.maximum(rng.standard_normal(shape), 0) * 2) / 2
    x = np.where((x == 0) & (rng.random(shape) < 0.5), -0.0, x).astype(np.float32)
    (hs, he), (ws, we) = windows(H, oh)[0], windows(W, ow)[0]
    x[0, 0, hs:he, ws:we] = 1.5                                   # all equal: the first element wins
    if C > 1:
        (hs, he), (ws, we) = windows(H, oh)[-1], windows(W, ow)[-1]
        x[0, 1, hs:he, ws:we] = -np.inf                           # all -inf: still the first element
    for k in range(b * C):                                        # a NaN in every third plane
        if k % 3 == 2:
            x[k // C, k % C, int(rng.integers(H)), int(rng.integers(W))] = np.nan
    if several_nans and H * W >= 2:
        flat = x[b - 1, C - 1].reshape(-1)                        # (a view: plants into x)
        flat[H * W - 1] = np.nan
        flat[H * W - 2] = np.nan
    return torch.from_numpy(x).to(dtype)


def make_grad(shape, seed):
    """fp32 multiples of 2^-6 in [-4, 4]: every sum of a few of them is exact in fp32, in any order"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((rng.integers(-256, 257, shape) / 64.0).astype(np.float32))
