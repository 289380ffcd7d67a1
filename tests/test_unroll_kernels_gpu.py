"""-m gpu: the four kernels of the unrolled architecture step (csrc/unroll.hip) through the C ABI, on hand-built
bmnas_adam_tensor_t tables, against tests/unroll_ref.py.

One table of six tensors of 1 ... 4099 elements (one lane, a ragged float4, one element short of a chunk, a whole chunk, one
past it, several chunks with a ragged end), alternating between TWO scalar rows with different wd and mu; every column in
turn one float off the 16-byte alignment (the pointers select the float4 branch: off alignment the scalar path runs);
NaN guards on both sides of every buffer.

The kernels contract nothing into a fused multiply-add, so unroll_ref's fp32 mode — numpy, one rounding per operation — is
their bit-for-bit reference.  The one quantity that is not a fixed sequence is the norm (a tree sum whose order differs
from numpy's): R_out is compared with r / ||v|| in float64 at 1e-6 relative (256 partials of <= 24 chunks each and a
256-leaf tree in fp32: the relative error of the sum of squares is far below 100 eps = 6e-6, halved by the square root), and
the perturbed weights are then bit-equal to the reference evaluated with the R the launch itself reported."""
import numpy as np
import pytest
import torch

import unroll_ref as ur
from gpu_util import dev

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 1023, 1024, 1025, 4099]
PAD = 4                                   # guard floats on each side of a buffer (keeps 16-byte alignment)
ETA, R0 = 1e-2, 1e-2
ROWS = [(0.9, 3e-4), (0.5, 0.1)]          # (mu, wd) of the two scalar rows
W_COLS = {'p': 'param', 'g': 'grad', 'b': 'exp_avg', 'k': 'exp_avg_sq'}
A_COLS = {'p': 'param', 'g': 'grad', 'b': 'exp_avg'}         # combine: dalpha, g+, g-


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _np_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).view(torch.int32)


def _rand(seed, n, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * scale


class _Table:
    """Device tensors + bmnas_adam_tensor_t[] + chunk list for direct calls.  cols: key -> descriptor field; off: the keys
    whose buffers sit one float off the 16-byte alignment; null: keys staged as NULL pointers (for every tensor, or for
    the tensor indices given)."""

    def __init__(self, seed, cols=W_COLS, off=(), null=(), null_at=None, sizes=SIZES):
        from bmnas import lib
        from bmnas.optim import _DESC
        self.sizes, self.cols = sizes, cols
        scale = {'p': 1.0, 'g': 0.3, 'b': 0.1, 'k': 7.0}
        self.host = {k: [_rand(seed + 10 * j + i, n, scale[k]) for i, n in enumerate(sizes)]
                     for j, k in enumerate(cols)}
        self.dev, self.stores = {}, {}
        for k, ts in self.host.items():
            self.dev[k], self.stores[k] = [], []
            for t in ts:
                store = torch.full((t.numel() + 2 * PAD + 1,), float('nan'), device=dev())
                o = PAD + (1 if k in off else 0)
                view = store[o:o + t.numel()]
                view.copy_(t)
                assert view.data_ptr() % 16 == (4 if k in off else 0)
                self.dev[k].append(view)
                self.stores[k].append(store)
        E = lib.adam_chunk_elems()
        tab = np.zeros(len(sizes), dtype=_DESC)
        for k, field in cols.items():
            ptrs = [t.data_ptr() for t in self.dev[k]]
            if k in null:
                ptrs = [0 if (null_at is None or i in null_at) else q for i, q in enumerate(ptrs)]
            tab[field] = ptrs
        tab['numel'] = sizes
        tab['hyp_row'] = [i % 2 for i in range(len(sizes))]
        chunks = [(i, c) for i, n in enumerate(sizes) for c in range((n + E - 1) // E)]
        self.tab = torch.from_numpy(tab.view(np.uint8)).to(dev())
        self.chunks = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(dev())
        self.n = len(chunks)
        self.partials = torch.zeros(lib.grad_norm_parts(), device=dev())
        self.n_parts = min(self.n, lib.grad_norm_parts())
        self.r = torch.tensor([R0], device=dev())
        self.R = torch.zeros(1, device=dev())
        torch.cuda.synchronize()
        self.start = {k: [_bits(s).clone() for s in ss] for k, ss in self.stores.items()}

    def get(self, k):
        torch.cuda.synchronize()
        return [t.clone().cpu() for t in self.dev[k]]

    def check(self, untouched=()):
        """The floats around every view are bit-unchanged (`untouched`: these columns' views as well)."""
        torch.cuda.synchronize()
        for k, ss in self.stores.items():
            for i, (s, was) in enumerate(zip(ss, self.start[k])):
                n, o = self.sizes[i], PAD + (1 if self.dev[k][i].data_ptr() % 16 else 0)
                now = _bits(s)
                assert torch.equal(now[:o], was[:o]) and torch.equal(now[o + n:], was[o + n:]), (k, i)
                if k in untouched:
                    assert torch.equal(now, was), (k, i)


def _hyp(rows=ROWS, eta=ETA):
    return torch.tensor([[-eta, mu, wd, 0, 0, 0, 0, 0] for mu, wd in rows], dtype=torch.float32, device=dev())


OFFS = [(), ('p',), ('g',), ('b',), ('k',)]
OFF_IDS = ['aligned', 'param_off1', 'vector_off1', 'buffer_off1', 'backup_off1']


@pytest.mark.parametrize('off', OFFS, ids=OFF_IDS)
@pytest.mark.parametrize('momentum', [False, True], ids=['plain', 'momentum'])
def test_virtual_step_bits(momentum, off):
    from bmnas import lib
    d = _Table(100, off=off, null=() if momentum else ('b',))
    lib.unroll_virtual_step(d.tab, d.chunks, d.n, _hyp(), lib.UNROLL_MOMENTUM if momentum else 0)
    p, k = d.get('p'), d.get('k')
    d.check(untouched=('g', 'b'))                                     # buf and g: read, never written
    for i in range(len(SIZES)):
        mu, wd = ROWS[i % 2]
        want, bak = ur.virtual_step(d.host['p'][i], d.host['g'][i], d.host['b'][i] if momentum else None, ETA, mu, wd,
                                    dtype=np.float32)
        assert torch.equal(_bits(p[i]), _np_bits(want)), (i, 'param')
        assert torch.equal(_bits(k[i]), _np_bits(bak)) and torch.equal(_bits(k[i]), _bits(d.host['p'][i])), (i, 'backup')
        assert not torch.equal(p[i], d.host['p'][i])


def test_virtual_step_null_buffers():
    """Without the flag a NULL exp_avg is never dereferenced; with it, the tensors whose exp_avg is NULL take no momentum
    term beside tensors that do."""
    from bmnas import lib
    a = _Table(110, null=('b',))
    lib.unroll_virtual_step(a.tab, a.chunks, a.n, _hyp(), 0)
    b = _Table(110, null=('b',), null_at={0, 3, 5})
    lib.unroll_virtual_step(b.tab, b.chunks, b.n, _hyp(), lib.UNROLL_MOMENTUM)
    pa, pb = a.get('p'), b.get('p')
    a.check(untouched=('g', 'b'))
    b.check(untouched=('g', 'b'))
    for i in range(len(SIZES)):
        mu, wd = ROWS[i % 2]
        plain, _ = ur.virtual_step(a.host['p'][i], a.host['g'][i], None, ETA, mu, wd, dtype=np.float32)
        assert torch.equal(_bits(pa[i]), _np_bits(plain)), i
        buf = None if i in (0, 3, 5) else b.host['b'][i]
        want, _ = ur.virtual_step(b.host['p'][i], b.host['g'][i], buf, ETA, mu, wd, dtype=np.float32)
        assert torch.equal(_bits(pb[i]), _np_bits(want)), i
        assert (buf is None) == torch.equal(pa[i], pb[i])


def test_zero_decay_and_zero_momentum_leave_the_bits_of_the_sequence_without_them():
    from bmnas import lib
    for off in ((), ('p',)):
        d = _Table(120, off=off)
        lib.unroll_virtual_step(d.tab, d.chunks, d.n, _hyp([(0.0, 0.0), (0.0, 0.0)]), lib.UNROLL_MOMENTUM)
        p = d.get('p')
        for i in range(len(SIZES)):
            want = d.host['p'][i].numpy() + np.float32(-ETA) * d.host['g'][i].numpy()         # no decay, no momentum term
            assert torch.equal(_bits(p[i]), _np_bits(want)), (off, i)
        # ... and each alone: wd == 0 with momentum, mu == 0 with decay
        d = _Table(121, off=off)
        lib.unroll_virtual_step(d.tab, d.chunks, d.n, _hyp([(0.9, 0.0), (0.0, 0.1)]), lib.UNROLL_MOMENTUM)
        p = d.get('p')
        for i in range(len(SIZES)):
            mu, wd = [(0.9, 0.0), (0.0, 0.1)][i % 2]
            want, _ = ur.virtual_step(d.host['p'][i], d.host['g'][i], d.host['b'][i], ETA, mu, wd, dtype=np.float32,
                                      plain_terms=True)
            assert torch.equal(_bits(p[i]), _np_bits(want)), (off, i)


def _perturb(d, sign):
    from bmnas import lib
    lib.unroll_perturb(d.tab, d.chunks, d.n, d.partials, d.n_parts, d.r, sign, d.R)


@pytest.mark.parametrize('off', [(), ('p',), ('g',), ('k',)], ids=['aligned', 'param_off1', 'vector_off1', 'backup_off1'])
def test_perturb_and_restore(off):
    from bmnas import lib
    d = _Table(200, off=off, null=('b',))
    w0 = [t.clone() for t in d.host['p']]
    lib.unroll_virtual_step(d.tab, d.chunks, d.n, _hyp(), 0)                      # fills the backups with w
    lib.grad_sqnorm_multi(d.tab, d.chunks, d.n, d.partials)                       # `grad` doubles as v here
    want_R = ur.R_of(d.host['g'], R0)
    runs = {}
    for sign in (1, -1, 1):
        _perturb(d, sign)
        p = d.get('p')
        R = d.R.cpu().numpy()[0]
        assert R.dtype == np.float32
        print(f'R_out {float(R)!r} against r / ||v|| in float64 {want_R!r}: {abs(float(R) - want_R) / want_R:.2e} relative')
        assert abs(float(R) - want_R) <= 1e-6 * want_R
        for i in range(len(SIZES)):
            want = ur.perturb(w0[i], d.host['g'][i], R, sign, dtype=np.float32)  # from the BACKUP, whatever p held
            assert torch.equal(_bits(p[i]), _np_bits(want)), (sign, i)
        if sign in runs:                                                          # two runs: identical bits
            assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(runs[sign], p))
        runs[sign] = p
    assert not torch.equal(runs[1][5], runs[-1][5])
    d.check(untouched=('g',))
    # restore: the original w bit for bit, v not read — a NaN there cannot leak
    for v in d.dev['g']:
        v.fill_(float('nan'))
    lib.unroll_restore(d.tab, d.chunks, d.n)
    p = d.get('p')
    for i in range(len(SIZES)):
        assert torch.equal(_bits(p[i]), _bits(w0[i])), i
    d.check()


@pytest.mark.parametrize('off', [(), ('p',), ('g',), ('b',)], ids=['aligned', 'dalpha_off1', 'gplus_off1', 'gminus_off1'])
def test_combine_bits(off):
    from bmnas import lib
    d = _Table(300, cols=A_COLS, off=off)
    for gp, gn in zip(d.dev['g'], d.dev['b']):                                    # g- close to g+, as in the step
        gn.copy_(gp + 1e-3 * gn)
    torch.cuda.synchronize()
    gn_host = [t.clone().cpu() for t in d.dev['b']]
    d.start = {k: [_bits(s).clone() for s in ss] for k, ss in d.stores.items()}
    d.R.fill_(3.7e-3)
    eta = torch.tensor([ETA], device=dev())
    lib.unroll_combine(d.tab, d.chunks, d.n, eta, d.R)
    out = d.get('p')
    d.check(untouched=('g', 'b'))
    R = d.R.cpu().numpy()[0]
    for i in range(len(SIZES)):
        want = ur.combine(d.host['p'][i], d.host['g'][i], gn_host[i], R, ETA, dtype=np.float32)
        assert torch.equal(_bits(out[i]), _np_bits(want)), i
        assert not torch.equal(out[i], d.host['p'][i])


def test_rejected_arguments_launch_nothing():
    from bmnas import lib
    d = _Table(400, sizes=[1025, 7])
    hyp = _hyp()
    lib.grad_sqnorm_multi(d.tab, d.chunks, d.n, d.partials)
    torch.cuda.synchronize()
    so = lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    t, c, h = d.tab.data_ptr(), d.chunks.data_ptr(), hyp.data_ptr()
    pa, r, R = d.partials.data_ptr(), d.r.data_ptr(), d.R.data_ptr()
    M = lib.UNROLL_MOMENTUM
    virt, pert, rest, comb = (so.bmnas_unroll_virtual_step, so.bmnas_unroll_perturb, so.bmnas_unroll_restore,
                              so.bmnas_unroll_combine)
    bad = [
        (virt, (None, c, d.n, h, M)), (virt, (t, None, d.n, h, M)), (virt, (t, c, d.n, None, M)),      # NULL pointers
        (virt, (t, c, -1, h, M)),                                                                      # n_chunks < 0
        (virt, (t, c, d.n, h, 2)), (virt, (t, c, d.n, h, M | 4)), (virt, (t, c, d.n, h, -1)),          # unknown flag bits
        (pert, (None, c, d.n, pa, d.n_parts, r, 1.0, R)), (pert, (t, None, d.n, pa, d.n_parts, r, 1.0, R)),
        (pert, (t, c, d.n, None, d.n_parts, r, 1.0, R)), (pert, (t, c, d.n, pa, d.n_parts, None, 1.0, R)),
        (pert, (t, c, d.n, pa, d.n_parts, r, 1.0, None)),
        (pert, (t, c, -1, pa, d.n_parts, r, 1.0, R)), (pert, (t, c, 0, pa, 0, r, 1.0, R)),             # a norm is needed
        (pert, (t, c, d.n, pa, d.n_parts, r, 0.0, R)), (pert, (t, c, d.n, pa, d.n_parts, r, 2.0, R)),  # sign not +-1
        (pert, (t, c, d.n, pa, d.n_parts, r, -0.5, R)), (pert, (t, c, d.n, pa, d.n_parts, r, float('nan'), R)),
        (pert, (t, c, d.n, pa, d.n_parts + 1, r, 1.0, R)), (pert, (t, c, d.n, pa, 0, r, 1.0, R)),      # not the norm
        (pert, (t, c, d.n, pa, 256, r, -1.0, R)),                                                      # launch's G
        (rest, (None, c, d.n)), (rest, (t, None, d.n)), (rest, (t, c, -1)),
        (comb, (None, c, d.n, h, R)), (comb, (t, None, d.n, h, R)), (comb, (t, c, d.n, None, R)),
        (comb, (t, c, d.n, h, None)), (comb, (t, c, -1, h, R)),
    ]
    for fn, args in bad:
        assert fn(*args, stream) == -1, (fn.__name__, args)
    # nothing to do: no error, nothing launched
    assert virt(t, c, 0, h, M, stream) == 0 and rest(t, c, 0, stream) == 0 and comb(t, c, 0, h, R, stream) == 0
    with pytest.raises(lib.BmnasError, match='bad argument'):
        lib.unroll_perturb(d.tab, d.chunks, d.n, d.partials, d.n_parts, d.r, 3, d.R)
    d.check(untouched=('p', 'g', 'b', 'k'))
    assert float(d.R) == 0.0
    lib.unroll_virtual_step(d.tab, d.chunks, d.n, hyp, M)                          # the accepted forms do launch
    _perturb(d, -1)
    torch.cuda.synchronize()
    assert float(d.R) > 0 and not torch.equal(_bits(d.get('p')[0]), _bits(d.host['p'][0]))
