"""BatchNorm momentum in the native finalisers (csrc/bn_fin.hpp: bn_fin_fill; csrc/bnmix.hip: bn_finalize_k), kernel by
kernel through the C ABI against the float64 statement in tests/bn_momentum_ref.py (pinned to torch on the CPU by
tests/test_bn_momentum_ref.py).  It follows tests/test_bn_kernels_gpu.py: outputs and buffers are views into guarded NaN
buffers (gpu_util.Pool), the inputs are rounded to float32 once and the expectation is formed in float64 from the ROUNDED
values, the running statistics are compared with gpu_util.assert_close_scaled at that file's bound 2e-5, counters exactly.

Entries: bmnas_bn_relu_fwd (bn_fin_fill), bmnas_bn_relu_fwd_group (three problems, three modes, one launch),
bmnas_node_mix_fwd at C 4 (M 12: one stacked descriptor, two counters) and bmnas_bn_finalize_ex.  Shapes: the smallest at
which the fill can go wrong (that file established them): M 4, 8, 12 (one thread, two, three) and 1028 (thread 0's second
trip), (b, L) = (1, 4) and (3, 8), 1 and 4 shards; M 64 at (8, 8) for more than one workgroup; bmnas_bn_finalize_ex at
M 1, 5, 64 with 1 and 65 partials.

Properties: value mode at 0.05, 0.5, 1.0 (= the batch's statistics) and 0.0 (buffers bit-unchanged, counter + 1);
cumulative mode over three consecutive launches on different data from counters 0 (= the plain mean of the three batch
statistics, whatever the buffers held), 5 and 2^33 + 5 (factors 1/6, 1/7, 1/8 and about 1e-10); value mode at 0.1f is
bit-identical to the default mode; and in EVERY case `out` and `chan` are bit-identical to the default-mode launch on the
same inputs: momentum reaches nothing but the running buffers.  The second counter of a stacked launch starts elsewhere
than the first: the factor must come from the first, and both move by one per launch."""
import math

import pytest
import torch

import bn_momentum_ref as mr
import bn_ref as br
from gpu_util import Pool, assert_close_scaled, dev

pytestmark = pytest.mark.gpu

R_RUN = 2e-5
F64 = torch.float64
DEFAULT, VALUE, CUMULATIVE = 0, 1, 2


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.int64 else torch.int32)


def _same(name, a, b):
    assert torch.equal(_bits(a), _bits(b)), f'{name} differs bit-wise'


class _Data:
    """One batch for an M-channel BatchNorm behind a conv: U float32, the sharded sums of d = U - bias and d^2 as float32,
    and the batch statistics in float64 FROM those rounded sums (what bn_fin_fill is given)."""

    def __init__(self, M, b, L, shards, seed):
        g = _gen(100 * seed + 7 * b + 3 * M + L + shards)
        self.M, self.b, self.L, self.shards, self.N = M, b, L, shards, b * L
        std = 0.5 + torch.randn(M, generator=g, dtype=F64).abs()
        mu = 2.0 * torch.randn(M, generator=g, dtype=F64)
        self.cb = (torch.randn(M, generator=g, dtype=F64) + 0.5).float()
        self.U = (torch.randn(b, M, L, generator=g, dtype=F64) * std[None, :, None] + mu[None, :, None]).float()
        S = br.sums_of(self.U, self.cb, 1)[0]
        w = 0.1 + 0.5 * torch.rand(max(shards - 1, 0), M, 2, generator=g, dtype=F64)
        parts = w * S[None]
        self.stat = torch.cat([parts, (S - parts.sum(0))[None]], 0).float()
        s = self.stat.double().sum(0)
        dm = s[:, 0] / self.N
        var = torch.clamp(s[:, 1] / self.N - dm * dm, min=0.0)
        self.mean, self.unbiased = dm + self.cb.double(), var * self.N / (self.N - 1)
        self.Ud, self.statd, self.cbd = self.U.to(dev()), self.stat.to(dev()), self.cb.to(dev())


class _Bn:
    """The affine parameters (device) and the guarded running buffers of one BatchNorm (or one stacked launch)."""

    def __init__(self, pool, M, seed, counters):
        g = _gen(seed)
        self.bn_w = (1.0 + 0.3 * torch.randn(M, generator=g, dtype=F64)).float().to(dev())
        self.bn_b = (0.5 * torch.randn(M, generator=g, dtype=F64)).float().to(dev())
        self.rm0 = torch.randn(M, generator=g, dtype=F64).float()
        self.rv0 = (0.5 + torch.randn(M, generator=g, dtype=F64).abs()).float()
        self.n0 = torch.tensor(counters, dtype=torch.int64)
        self.rm, self.rv = pool.new(M, base=self.rm0), pool.new(M, base=self.rv0)
        self.nbt = pool.new_i64(self.n0) if len(counters) else None

    def fin(self, data, momentum=0.0, mode=DEFAULT):
        from bmnas import lib
        return lib.BnFin(data.statd.data_ptr(), data.cbd.data_ptr(), self.bn_w.data_ptr(), self.bn_b.data_ptr(),
                         self.rm.data_ptr(), self.rv.data_ptr(), None if self.nbt is None else self.nbt.data_ptr(),
                         data.shards, 0 if self.nbt is None else self.nbt.numel(), 1, 1, momentum, mode)


def _relu(pool, data, fin):
    from bmnas import lib
    chan, out = pool.new(4 * data.M), pool.new(data.b, data.M, data.L)
    lib.bn_relu_fwd(data.Ud, chan, out, data.b, data.M, data.L, lib.NO_DROP, fin)
    return chan, out


def _baseline(data, bn_seed, counters):
    """the default-mode launch on the same inputs: (chan, out, running_mean, running_var) as CPU tensors"""
    pool = Pool()
    bn = _Bn(pool, data.M, bn_seed, counters)
    chan, out = _relu(pool, data, bn.fin(data))
    pool.check()
    return chan.cpu(), out.cpu(), bn.rm.cpu(), bn.rv.cpu()


def _expect(bn, datas, momentum):
    """float64 running statistics and the first counter after the launches over `datas` in turn"""
    rm, rv, n = bn.rm0.double(), bn.rv0.double(), int(bn.n0[0])
    for d in datas:
        rm, rv, n = mr.update(rm, rv, n, d.mean, d.unbiased, momentum)
    return rm, rv


#         M, b, L, shards
SHAPES = [(4, 1, 4, 1), (4, 3, 8, 4), (8, 1, 4, 4), (8, 3, 8, 1), (12, 3, 8, 4), (12, 1, 4, 1), (1028, 1, 4, 4),
          (1028, 3, 8, 1)]


@pytest.mark.parametrize('momentum', [0.05, 0.5, 1.0])
@pytest.mark.parametrize('M,b,L,shards', SHAPES)
def test_value_mode_through_bn_relu_fwd(M, b, L, shards, momentum):
    data = _Data(M, b, L, shards, 1)
    counters = [7, 2 ** 33 + 5][:1 + (M > 4)]
    base = _baseline(data, 5, counters)
    pool = Pool()
    bn = _Bn(pool, M, 5, counters)
    chan, out = _relu(pool, data, bn.fin(data, momentum, VALUE))
    pool.check()
    _same('chan', chan, base[0])
    _same('out', out, base[1])
    rm, rv = _expect(bn, [data], momentum)
    assert_close_scaled('running_mean', bn.rm, rm, rel=R_RUN)
    assert_close_scaled('running_var', bn.rv, rv, rel=R_RUN)
    if momentum == 1.0:                                       # the batch's own statistics, whatever the buffers held
        assert_close_scaled('running_mean = batch mean', bn.rm, data.mean, rel=R_RUN)
        assert_close_scaled('running_var = unbiased batch variance', bn.rv, data.unbiased, rel=R_RUN)
    assert torch.equal(bn.nbt.cpu(), bn.n0 + 1)


@pytest.mark.parametrize('M,b,L,shards', SHAPES)
def test_value_mode_zero_leaves_the_buffers_and_counts(M, b, L, shards):
    data = _Data(M, b, L, shards, 2)
    base = _baseline(data, 6, [7])
    pool = Pool()
    bn = _Bn(pool, M, 6, [7])
    chan, out = _relu(pool, data, bn.fin(data, 0.0, VALUE))
    pool.check()
    _same('chan', chan, base[0])
    _same('out', out, base[1])
    _same('running_mean', bn.rm, bn.rm0)
    _same('running_var', bn.rv, bn.rv0)
    assert torch.equal(bn.nbt.cpu(), bn.n0 + 1)


@pytest.mark.parametrize('M,b,L,shards', SHAPES)
def test_value_mode_at_a_tenth_is_the_default_mode_bit_for_bit(M, b, L, shards):
    import ctypes
    data = _Data(M, b, L, shards, 3)
    base = _baseline(data, 7, [3, 3])
    pool = Pool()
    bn = _Bn(pool, M, 7, [3, 3])
    chan, out = _relu(pool, data, bn.fin(data, ctypes.c_float(0.1).value, VALUE))
    pool.check()
    for name, got, want in zip(('chan', 'out', 'running_mean', 'running_var'), (chan, out, bn.rm, bn.rv), base):
        _same(name, got, want)
    assert torch.equal(bn.nbt.cpu(), bn.n0 + 1)


@pytest.mark.parametrize('start', [0, 5, 2 ** 33 + 5])
@pytest.mark.parametrize('M,b,L,shards', SHAPES)
def test_cumulative_mode_over_three_launches(M, b, L, shards, start):
    datas = [_Data(M, b, L, shards, 10 + i) for i in range(3)]
    counters = [start, start + 100][:1 + (M > 4)]             # the factor comes from the FIRST counter
    pool = Pool()
    bn = _Bn(pool, M, 8, counters)
    for d in datas:
        base = _baseline(d, 8, counters)
        chan, out = _relu(pool, d, bn.fin(d, 0.0, CUMULATIVE))
        _same('chan', chan, base[0])
        _same('out', out, base[1])
    pool.check()
    rm, rv = _expect(bn, datas, None)
    assert_close_scaled('running_mean', bn.rm, rm, rel=R_RUN)
    assert_close_scaled('running_var', bn.rv, rv, rel=R_RUN)
    assert torch.equal(bn.nbt.cpu(), bn.n0 + 3)
    if start == 0:                                            # the plain mean, independent of the initial buffers
        assert_close_scaled('mean of the batch means', bn.rm, sum(d.mean for d in datas) / 3, rel=R_RUN)
        assert_close_scaled('mean of the batch variances', bn.rv, sum(d.unbiased for d in datas) / 3, rel=R_RUN)
    if start == 5:
        assert [mr.factor(None, start + i) for i in range(3)] == [1 / 6, 1 / 7, 1 / 8]
    if start > 2 ** 33:
        assert 1e-10 < mr.factor(None, start) < 1.2e-10


@pytest.mark.parametrize('momentum,mode', [(0.5, VALUE), (0.0, CUMULATIVE)])
def test_more_than_one_workgroup_moves_the_buffers_once(momentum, mode):
    """b 8, L 8, M 64: four workgroups finalise, workgroup 0 alone writes"""
    data = _Data(64, 8, 8, 4, 4)
    counters = [5, 9, 5, 9]
    base = _baseline(data, 9, counters)
    pool = Pool()
    bn = _Bn(pool, 64, 9, counters)
    chan, out = _relu(pool, data, bn.fin(data, momentum, mode))
    pool.check()
    _same('chan', chan, base[0])
    _same('out', out, base[1])
    rm, rv = _expect(bn, [data], None if mode == CUMULATIVE else momentum)
    assert_close_scaled('running_mean', bn.rm, rm, rel=R_RUN)
    assert_close_scaled('running_var', bn.rv, rv, rel=R_RUN)
    assert torch.equal(bn.nbt.cpu(), bn.n0 + 1)


@pytest.mark.parametrize('M,b,L', [(4, 1, 4), (12, 3, 8), (1028, 3, 8)])
def test_three_modes_in_one_grouped_launch(M, b, L):
    from bmnas import lib
    datas = [_Data(M, b, L, 1 + i, 20 + i) for i in range(3)]
    modes = [(0.0, DEFAULT, 0.1), (0.3, VALUE, 0.3), (0.0, CUMULATIVE, None)]
    bases = [_baseline(d, 30 + i, [5]) for i, d in enumerate(datas)]
    pool = Pool()
    bns = [_Bn(pool, M, 30 + i, [5]) for i in range(3)]
    chans, outs = [pool.new(4 * M) for _ in range(3)], [pool.new(b, M, L) for _ in range(3)]
    fins = [bn.fin(d, m, mode) for bn, d, (m, mode, _) in zip(bns, datas, modes)]
    lib.bn_relu_fwd_group([d.Ud for d in datas], chans, outs, fins, [lib.NO_DROP] * 3, b, M, L)
    pool.check()
    for i, (bn, d, (_, _, momentum)) in enumerate(zip(bns, datas, modes)):
        _same(f'chan {i}', chans[i], bases[i][0])
        _same(f'out {i}', outs[i], bases[i][1])
        rm, rv = _expect(bn, [d], momentum)
        assert_close_scaled(f'running_mean {i}', bn.rm, rm, rel=R_RUN)
        assert_close_scaled(f'running_var {i}', bn.rv, rv, rel=R_RUN)
        assert torch.equal(bn.nbt.cpu(), bn.n0 + 1)
    _same('the default problem of the group', bns[0].rm, bases[0][2])


@pytest.mark.parametrize('momentum,mode', [(0.05, VALUE), (1.0, VALUE), (0.0, VALUE), (0.0, CUMULATIVE)])
@pytest.mark.parametrize('b,L', [(1, 4), (3, 8)])
def test_node_mix_fwd_stacked_descriptor(b, L, momentum, mode):
    """bmnas_node_mix_fwd at C 4: M = 3 C = 12 channels of [LinearGLU | ConcatFC] under ONE descriptor with the two
    BatchNorms' counters; the mixed output and chan do not depend on the mode"""
    from bmnas import lib
    C, M = 4, 12
    data = _Data(M, b, L, 4, 40)
    g = _gen(41)
    x, y, p1 = (torch.randn(b, C, L, generator=g).to(dev()) for _ in range(3))
    gamma = torch.softmax(torch.randn(4, generator=g), 0).to(dev())
    counters = [5, 12]

    def launch(m, md):
        pool = Pool()
        bn = _Bn(pool, M, 42, counters)
        chan, out = pool.new(4 * M), pool.new(b, C, L)
        lib.node_mix_fwd(x, y, p1, data.Ud, chan, gamma, out, b, C, L, lib.NO_DROP, lib.NO_DROP, bn.fin(data, m, md))
        pool.check()
        return bn, chan.cpu(), out.cpu()

    _, chan0, out0 = launch(0.0, DEFAULT)
    bn, chan, out = launch(momentum, mode)
    _same('chan', chan, chan0)
    _same('out', out, out0)
    assert bool(torch.isfinite(out).all())
    rm, rv = _expect(bn, [data], None if mode == CUMULATIVE else momentum)
    if mode == VALUE and momentum == 0.0:
        _same('running_mean', bn.rm, bn.rm0)
        _same('running_var', bn.rv, bn.rv0)
    assert_close_scaled('running_mean', bn.rm, rm, rel=R_RUN)
    assert_close_scaled('running_var', bn.rv, rv, rel=R_RUN)
    assert torch.equal(bn.nbt.cpu(), bn.n0 + 1)


# ------------------------------------------------------------------------------------------------ bmnas_bn_finalize_ex
@pytest.mark.parametrize('momentum', [0.05, 0.5, 1.0, 0.0, 0.1, None])
@pytest.mark.parametrize('M,b,L', [(1, 1, 4), (5, 1, 16), (64, 1, 8), (1, 65, 16), (5, 65, 16), (64, 65, 16)])
def test_bn_finalize_ex(M, b, L, momentum):
    """n_part 1 (N <= 16) and 65 (N 1040); three consecutive launches on different data over the same buffers; chan is
    the default launch's bit for bit; momentum 0.1 goes through the default mode (bmnas.lib.bn_momentum)"""
    from bmnas import lib
    N = b * L
    n_part = (N + 15) // 16
    assert n_part in (1, 65)
    g = _gen(50 + M + b)
    bn_w, bn_b = (1.0 + 0.3 * torch.randn(M, generator=g)).to(dev()), (0.5 * torch.randn(M, generator=g)).to(dev())
    rm0, rv0 = torch.randn(M, generator=g), 0.5 + torch.randn(M, generator=g).abs()
    n0 = torch.tensor([5, 11][:min(M, 2)], dtype=torch.int64)
    pool = Pool()
    rm, rv, nbt = pool.new(M, base=rm0), pool.new(M, base=rv0), pool.new_i64(n0)
    want_rm, want_rv, n = rm0.double(), rv0.double(), 5
    for i in range(3):
        U = (torch.randn(b, M, L, generator=g, dtype=F64) * 1.5 + 0.7 * (i + 1)).float()
        part = br.group_partials(U).float()
        ref = br.fin_from_partials(part.double(), bn_w.cpu(), bn_b.cpu(), torch.zeros(M), torch.zeros(M), None, N)
        mean, unbiased = ref['rm'] / br.MOMENTUM, ref['rv'] / br.MOMENTUM      # (from zero buffers: 0.1 x the batch's)
        pd = part.to(dev())
        chan, chan0 = pool.new(4 * M), pool.new(4 * M)
        lib.bn_finalize(pd, n_part, b, L, M, bn_w, bn_b, None, None, None, True, chan0)
        lib.bn_finalize(pd, n_part, b, L, M, bn_w, bn_b, rm, rv, nbt, True, chan, momentum=momentum)
        _same('chan', chan, chan0)
        assert_close_scaled('chan: mean', chan[:M], ref['chan'][:M], rel=R_RUN)
        want_rm, want_rv, n = mr.update(want_rm, want_rv, n, mean, unbiased, momentum)
    pool.check()
    if momentum == 0.0:
        _same('running_mean', rm, rm0)
        _same('running_var', rv, rv0)
    assert_close_scaled('running_mean', rm, want_rm, rel=R_RUN)
    assert_close_scaled('running_var', rv, want_rv, rel=R_RUN)
    assert torch.equal(nbt.cpu(), n0 + 3)


def test_bn_finalize_ex_cumulative_from_zero_is_the_plain_mean():
    from bmnas import lib
    M, b, L = 5, 3, 8
    g = _gen(60)
    bn_w, bn_b = torch.ones(M, device=dev()), torch.zeros(M, device=dev())
    pool = Pool()
    rm, rv = pool.new(M, base=torch.randn(M, generator=g)), pool.new(M, base=torch.rand(M, generator=g) + 0.5)
    nbt = pool.new_i64(torch.zeros(1, dtype=torch.int64))
    means, variances = [], []
    for i in range(3):
        U = (torch.randn(b, M, L, generator=g, dtype=F64) + i).float()
        part = br.group_partials(U).float()
        mean, _, unbiased = mr.batch_stats(U)
        means.append(mean)
        variances.append(unbiased)
        lib.bn_finalize(part.to(dev()), 2, b, L, M, bn_w, bn_b, rm, rv, nbt, True, pool.new(4 * M), momentum=None)
    pool.check()
    assert_close_scaled('running_mean', rm, sum(means) / 3, rel=R_RUN)
    assert_close_scaled('running_var', rv, sum(variances) / 3, rel=R_RUN)
    assert int(nbt[0]) == 3


# ------------------------------------------------------------------------------------------------------ host contract
def test_bad_momentum_descriptors_are_refused_before_any_launch():
    """an unknown mode, a NaN momentum, cumulative mode in training with running statistics and no counter: BMNAS_E_ARG
    (the launchers return before launching: chan and the buffers keep their NaN / initial bits)"""
    from bmnas import lib
    data = _Data(8, 3, 8, 2, 70)
    pool = Pool()
    bn = _Bn(pool, 8, 71, [5])
    chan, out = pool.new(32), pool.new(3, 8, 8)
    before = chan.clone()
    bad = [bn.fin(data, 0.0, 3), bn.fin(data, 0.0, -1), bn.fin(data, math.nan, VALUE)]
    no_counter = bn.fin(data, 0.0, CUMULATIVE)
    no_counter.num_batches_tracked, no_counter.n_nbt = None, 0
    for fin in bad + [no_counter]:
        with pytest.raises(lib.BmnasError, match='bad argument'):
            lib.bn_relu_fwd(data.Ud, chan, out, 3, 8, 8, lib.NO_DROP, fin)
        with pytest.raises(lib.BmnasError, match='bad argument'):
            lib.bn_relu_fwd_group([data.Ud], [chan], [out], [fin], [lib.NO_DROP], 3, 8, 8)
    part = torch.zeros(8 * 2 * 2, device=dev())
    ex = lib.load().bmnas_bn_finalize_ex
    args = (part.data_ptr(), 2, 3, 8, 8, bn.bn_w.data_ptr(), bn.bn_b.data_ptr(), bn.rm.data_ptr(), bn.rv.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    assert ex(*args, bn.nbt.data_ptr(), 1, 1, 0.0, 3, chan.data_ptr(), stream) == -1
    assert ex(*args, bn.nbt.data_ptr(), 1, 1, math.nan, VALUE, chan.data_ptr(), stream) == -1
    assert ex(*args, None, 0, 1, 0.0, CUMULATIVE, chan.data_ptr(), stream) == -1
    # a NaN momentum outside value mode is not read; cumulative mode without running statistics needs no counter
    ok = bn.fin(data, math.nan, DEFAULT)
    lib.bn_relu_fwd(data.Ud, pool.new(32), pool.new(3, 8, 8), 3, 8, 8, lib.NO_DROP, ok)
    pool.check()
    _same('chan', chan, before)
    assert torch.equal(bn.nbt.cpu(), bn.n0 + 1)
