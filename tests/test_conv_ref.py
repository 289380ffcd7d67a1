"""CPU self-check of tests/conv_ref.py: the float64 statement tests/test_conv_kernels_gpu.py holds the 1x1-conv GEMM
kernels to is pinned here against torch in float64 — F.conv1d of torch.cat of the sources, the conv of cat[z, z] for
the weight fold and the duplicated weight-gradient columns, F.batch_norm (training and eval) under autograd for the
folded BatchNorm gradient, plain slicing for the per-n-group partials and the sharded sums.  A GPU mismatch is then
the kernel's."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as cr

TOL = 1e-12                                                        # float64 against float64, of the tensor's scale


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


SHAPES = [(5, 8, 1, 16, 48), (7, 4, 3, 16, 16), (3, 16, 2, 48, 32), (1, 4, 4, 16, 80)]     # b, L, n_src, C_src, M


@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('pad', [0, 12])
@pytest.mark.parametrize('b,L,n_src,C_src,M', SHAPES)
def test_forward_matches_conv1d_of_cat(b, L, n_src, C_src, M, pad, bias):
    g = _gen(100 + b + L + n_src + M + pad)
    K = n_src * C_src
    srcs = [_rand(g, b, C_src, L) for _ in range(n_src)]
    W, bv = _rand(g, M, K + pad), (_rand(g, M) * 3 if bias else None)
    got = cr.conv_fwd(srcs, W, bv)
    want = F.conv1d(torch.cat(srcs, 1), W[:, :K, None], bv)
    _close('U', got['U'], want)
    assert got['stat'] is None


@pytest.mark.parametrize('b,L,C,M', [(5, 8, 16, 48), (3, 4, 48, 16)])
def test_fold_is_the_conv_of_cat_z_z(b, L, C, M):
    g = _gen(200 + b + C)
    z, W, bv = _rand(g, b, C, L), _rand(g, M, 2 * C + 4), _rand(g, M)
    got = cr.conv_fwd([z], W, bv, fold_cols=C)
    _close('U', got['U'], F.conv1d(torch.cat([z, z], 1), W[:, :2 * C, None], bv))
    dU = _rand(g, b, M, L)
    zr = z.clone().requires_grad_(True)
    (F.conv1d(torch.cat([zr, zr], 1), W[:, :2 * C, None], bv) * dU).sum().backward()
    _close('dz', cr.conv_bwd_data(dU, W, C, C, [torch.zeros_like(z)], 0)[0], zr.grad)


@pytest.mark.parametrize('b,L,M', [(5, 8, 16), (7, 4, 32), (3, 16, 16), (1, 4, 16), (4, 4, 16), (9, 4, 16)])
def test_group_partials_match_slicing_and_add_up_to_the_batch_statistics(b, L, M):
    U = _rand(_gen(300 + b + L), b, M, L) * 2 + 5
    part = cr.group_partials(U)
    ng = cr.n_groups(b, L)
    assert part.shape == (M, ng, 2)
    cols = U.permute(1, 0, 2).reshape(M, b * L)
    counts = [min(16, b * L - 16 * g) for g in range(ng)]
    for g_, cnt in enumerate(counts):
        blk = cols[:, 16 * g_:16 * g_ + cnt]
        _close(f'sum {g_}', part[:, g_, 0], blk.sum(1))
        _close(f'm2 {g_}', part[:, g_, 1], blk.var(1, unbiased=False) * cnt)
    mean, var = cr.chan_combine(part, counts)
    _close('mean', mean, U.mean(dim=(0, 2)))
    _close('var', var, U.var(dim=(0, 2), unbiased=False), rel=1e-11)


@pytest.mark.parametrize('per_block', [1, 2, 4])
@pytest.mark.parametrize('shards', [1, 2, 3, 5])
@pytest.mark.parametrize('b,L', [(5, 8), (7, 4), (3, 16), (21, 4)])
def test_shard_sums_match_slicing(b, L, shards, per_block):
    g = _gen(400 + b + L + shards)
    M = 16
    z, W, bv = _rand(g, b, 16, L), _rand(g, M, 16), _rand(g, M) * 10
    got = cr.conv_fwd([z], W, bv, stat_shards=shards, groups_per_block=per_block)['stat']
    d = F.conv1d(z, W[:, :, None])
    cols = d.permute(1, 0, 2).reshape(M, b * L)
    want = torch.zeros(shards, M, 2, dtype=torch.float64)
    for blk in range((cr.n_groups(b, L) + per_block - 1) // per_block):
        c = cols[:, 16 * per_block * blk:16 * per_block * (blk + 1)]
        want[blk % shards, :, 0] += c.sum(1)
        want[blk % shards, :, 1] += (c * c).sum(1)
    _close('stat', got, want)
    _close('all shards: sum d', got[:, :, 0].sum(0), d.sum(dim=(0, 2)))
    _close('all shards: sum d^2', got[:, :, 1].sum(0), (d * d).sum(dim=(0, 2)))


@pytest.mark.parametrize('bn', ['none', 'train', 'eval'])
@pytest.mark.parametrize('b,L,n_src,C_src,M', SHAPES)
def test_backward_matches_autograd(b, L, n_src, C_src, M, bn):
    """conv (+ BatchNorm) under autograd: the data gradients with a NULL destination and an accumulate mask, the
    weight and bias gradients accumulated into previous values, the BatchNorm input gradient of both modes."""
    g = _gen(500 + b + L + n_src + M)
    K = n_src * C_src
    srcs = [_rand(g, b, C_src, L).requires_grad_(True) for _ in range(n_src)]
    W, bv = (_rand(g, M, K + 6)).requires_grad_(True), _rand(g, M).requires_grad_(True)
    bn_w, bn_b = _rand(g, M) * 0.3 + 1, _rand(g, M)
    rm, rv = _rand(g, M), _rand(g, M).abs() + 0.5
    dV = _rand(g, b, M, L)
    U = F.conv1d(torch.cat(srcs, 1), W[:, :K, None], bv)
    if bn == 'none':
        V = U
    else:
        V = F.batch_norm(U, rm.clone(), rv.clone(), bn_w, bn_b, training=bn == 'train', eps=cr.EPS)
    (V * dV).sum().backward()
    Ud = U.detach()
    if bn == 'train':
        dU, chan, bn_grad = cr.bn_input_grad(dV, Ud, bn_w)
        _close('chan mean', chan[:M], Ud.mean(dim=(0, 2)))
    elif bn == 'eval':
        chan = cr.bn_eval_chan(bn_w, bn_b, rm, rv)
        _close('eval forward', Ud * chan[2 * M:3 * M, None] + chan[3 * M:, None], V.detach())
        dU = cr.bn_eval_input_grad(dV, chan[2 * M:3 * M])
    else:
        dU = dV
    prevs = [_rand(g, b, C_src, L) for _ in range(n_src)]
    mask = 0b0101
    null = 1 if n_src > 2 else None
    got = cr.conv_bwd_data(dU, W.detach(), 0, C_src, [None if q == null else p for q, p in enumerate(prevs)], mask)
    for q in range(n_src):
        if q == null:
            assert got[q] is None
        else:
            _close(f'dsrc {q}', got[q], srcs[q].grad + (prevs[q] if (mask >> q) & 1 else 0))
    pW, pb = _rand(g, M, K + 6), _rand(g, M)
    dW, db = cr.conv_bwd_weight(dU, [s.detach() for s in srcs], pW, pb)
    _close('dW', dW, pW + W.grad)
    assert torch.equal(dW[:, K:], pW[:, K:])
    _close('dbias', db, pb + bv.grad)
    assert cr.conv_bwd_weight(dU, [s.detach() for s in srcs], pW, None)[1] is None


@pytest.mark.parametrize('pad', [0, 4])
def test_dup_cols_is_the_weight_gradient_of_cat_z_z(pad):
    g = _gen(600 + pad)
    b, L, C, M = 5, 8, 16, 48
    z, dU = _rand(g, b, C, L), _rand(g, b, M, L)
    W = _rand(g, M, 2 * C + pad).requires_grad_(True)
    (F.conv1d(torch.cat([z, z], 1), W[:, :2 * C, None]) * dU).sum().backward()
    pW = _rand(g, M, 2 * C + pad)
    dW, _ = cr.conv_bwd_weight(dU, [z], pW, None, dup_cols=C)
    _close('dW', dW, pW + W.grad)
    assert torch.equal(dW[:, 2 * C:], pW[:, 2 * C:])
