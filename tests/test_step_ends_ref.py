"""CPU self-check of tests/step_ends_ref.py: the hand-written float64 formulas tests/test_step_ends_kernels_gpu.py holds
the cell prologue, the backward epilogue and their stand-alone pieces to are pinned here against torch (softmax and
F.layer_norm under autograd, slicing, the two-line pair-sum expression).  A GPU mismatch is then the kernel's."""
import pytest
import torch
import torch.nn.functional as F

import step_ends_ref as sr

TOL = 1e-12                                                        # float64 against float64, of the tensor's scale
EPS = 1e-5


def _close(name, got, want, rel=TOL):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got - want).abs().max())
    assert err <= rel * scale, f'{name}: {err:.3e} of scale {scale:.3e}'


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize('rows,cols', [(1, 1), (8, 2), (3, 3), (5, 4), (257, 4), (2, 5)])
def test_row_softmax_matches_torch(rows, cols):
    a = _rand(_gen(10 + rows + cols), rows, cols) * 3.0
    a[0, 0] += 90.0                                                 # the others of this row underflow
    a[-1] += 1e4                                                    # a common offset changes nothing
    _close('softmax', sr.row_softmax(a), torch.softmax(a, dim=1))
    _close('rows sum to one', sr.row_softmax(a).sum(1), torch.ones(rows, dtype=torch.float64))


@pytest.mark.parametrize('n_shards', [1, 2, 17])
@pytest.mark.parametrize('rows,cols', [(1, 1), (8, 2), (3, 3), (5, 4), (2, 5)])
def test_row_softmax_bwd_matches_autograd(rows, cols, n_shards):
    g = _gen(20 + rows + cols + n_shards)
    a = (_rand(g, rows, cols) * 1.5).requires_grad_(True)
    dw = _rand(g, n_shards, rows, cols)
    w = torch.softmax(a, dim=1)
    (w * dw.sum(0)).sum().backward()
    got = sr.row_softmax_bwd(w.detach(), dw)
    _close('dlogits', got, a.grad)
    if cols == 1:
        assert float(got.abs().max()) == 0.0


def _ln_case(g, b, shapes, resid):
    srcs = [_rand(g, b, C, L) * 1.5 + 0.2 for C, L in shapes]
    N = sum(C * L for C, L in shapes)
    r = _rand(g, b, *shapes[0]) if resid else None
    w, bias = _rand(g, N) * 0.3 + 1.0, _rand(g, N) * 0.2
    return srcs, r, w, bias, _rand(g, b, N), N


@pytest.mark.parametrize('gscale', [None, 0.37])
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('b', [1, 5, 37])
@pytest.mark.parametrize('shapes,resid', [([(1, 4)], False), ([(63, 4)] * 3, False), ([(16, 4)] * 4, False),
                                          ([(65, 4)], True), ([(68, 16)], True), ([(192, 16)] * 2, False)])
def test_ln_affine_matches_autograd(shapes, resid, b, relu, gscale):
    g = _gen(30 + b + len(shapes) + shapes[0][0])
    srcs, r, w, bias, gy, N = _ln_case(g, b, shapes, resid)
    w, bias = w.requires_grad_(True), bias.requires_grad_(True)
    x = torch.cat([s.reshape(b, -1) for s in srcs], dim=1)
    if r is not None:
        x = x + r.reshape(b, -1)
    out = F.layer_norm(x, (N,), w, bias, EPS)
    if relu:
        out = F.relu(out)
    (out * gy * (1.0 if gscale is None else gscale)).sum().backward()
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False) + EPS)
    stats = torch.stack([mean, rstd], dim=1)
    gs = None if gscale is None else torch.tensor([gscale], dtype=torch.float64)
    dw, db = sr.ln_affine(gy, gs, srcs, r, w, bias, stats, relu, 0)
    _close('dln_w', dw, w.grad)
    _close('dln_b', db, bias.grad)
    # the prenorm form: srcs[0] is xhat itself, no statistics, no residual
    xhat = ((x - mean[:, None]) * rstd[:, None]).detach()
    dw2, db2 = sr.ln_affine(gy, gs, [xhat], None, w, bias, None, relu, 1)
    _close('dln_w (prenorm)', dw2, w.grad)
    _close('dln_b (prenorm)', db2, bias.grad)


@pytest.mark.parametrize('n_in', [1, 2, 3, 8, 15])
def test_pair_sum_matches_the_torch_expression(n_in):
    g = _gen(40 + n_in)
    xs = [_rand(g, 3, 5, 4) for _ in range(n_in)]
    alpha, beta = _rand(g, n_in, 2) * 2.0, _rand(g, 2, 2) * 2.0
    h, z = sr.pair_sum(xs, alpha, beta)
    want_h = sum(torch.softmax(alpha, dim=-1)[j, 1] * xs[j] for j in range(n_in))
    want_z = torch.softmax(beta, dim=-1)[:, 1].sum() * want_h
    _close('h', h, want_h)
    _close('z', z, want_z)


@pytest.mark.parametrize('M,C', [(16, 4), (48, 16), (5, 3)])
def test_fold_matches_slicing(M, C):
    W = _rand(_gen(50 + M), M, 2 * C)
    got = sr.fold(W)
    assert got.shape == (M, C)
    assert torch.equal(got, W[:, :C] + W[:, C:])
    assert torch.equal(sr.fold(W.float()), W.float().double()[:, :C] + W.float().double()[:, C:])


@pytest.mark.parametrize('n_chunk,n', [(1, 4), (3, 1020), (16, 36)])
def test_chunk_sum_matches_a_reshape(n_chunk, n):
    part = _rand(_gen(60 + n), n_chunk * n)
    _close('chunk sum', sr.chunk_sum(part, n_chunk), part.reshape(n_chunk, n).sum(0))
    assert torch.equal(sr.chunk_sum(part[:n], 1), part[:n])
