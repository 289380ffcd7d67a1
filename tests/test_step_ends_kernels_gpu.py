"""The launches that open and close a search step — bmnas_cell_prologue / bmnas_cell_prologue_pair (csrc/bnmix.hip) and
bmnas_backward_epilogue (csrc/layernorm.hip, csrc/arch_body.hpp) — and the entry points made of the same pieces
(bmnas_arch_softmax_fwd / _bwd / _multi, bmnas_ln_affine_bwd / _multi, bmnas_fold_weight, bmnas_sum_chunks), job by job,
against the float64 statement in tests/step_ends_ref.py (pinned by tests/test_step_ends_ref.py on the CPU) and against
one another.  What these kernels can get wrong is how a workgroup finds its job, so the job counts, row totals, shard
counts and sizes here sit on both sides of every boundary the job-finding code has.

Bounds: 1e-4 of the expected tensor's scale against float64 (assert_close_scaled at its default), rel = 2e-5 kernel
against kernel on identical inputs, bit equality (torch.equal) where the code promises it: the forward softmax forms
(the comment above softmax2_col1), the folds (one fp32 add), the zero-fill, the counter, the arch and chunk-sum slices
of the epilogue (no atomics, one summation order).
Every output starts as NaN — or, where the ABI adds into it (dln_w / dln_b), as a random base that the expectation
includes — inside a larger NaN buffer with GUARD floats on each side that must still be NaN afterwards (_Pool).
The K7-like ReLU is the only discontinuity a float64 comparison crosses: the bias is redrawn on the CPU until no ReLU
argument lies within 1e-3 of zero (lazy_ln_ref.clear_relu_bias), and no element is left out anywhere.

Architecture-tensor columns: the packed forms (multi, prologue, epilogue) take 1 to 4 and refuse 5 (ARG); the
single-tensor forms loop over any number of columns — bmnas.functions.ArchSoftmaxFn hands them whatever width an edited
primitive list gives the tensor — so they stay ungated and are tested at 5 and 7 columns.

Evidence that the tests bite — six value-only mutations (none moves an address), each built into a scratch copy of
the library and this file run once against it on an MI355X (150 cases; with the committed kernels all pass):
  1. arch_body.hpp, shard walk `sh += 16` -> `sh += 32`: 13 fail — test_row_softmax_bwd_three_forms at 17 and 40
     shards for each of the six tensor sets (1, 2 and 16 shards pass) and the full epilogue (G, 17 shards).
  2. ln_affine_body, sample walk `s += 4` -> `s += 8`: 41 fail — all 36 of test_ln_affine_three_forms, both
     test_ln_affine_multi_of_eight_widths, the deterministic mode, the chunk sums on a wide LayerNorm grid, G.
  3. ln_affine_body ignores gscale: 22 fail — the 18 gscale cases of test_ln_affine_three_forms (the 18 without
     gscale pass), both multis of eight widths, the deterministic mode, G.
  4. cell_prologue_body, `ld4(r + F.C)` -> `ld4(r)`: 29 fail — all 12 of test_prologue_fold, all jobs in one launch,
     all 16 of test_cell_prologue_pair (their folds).
  5. backward_epilogue_k, chunk loop from c = 2: 7 fail — test_epilogue_chunk_sums except n_chunk = 1, the wide
     LayerNorm grid, the accepted call of test_epilogue_sum_refusals (n_chunk = 2), G.
  6. softmax2_col1 returns e0 / (e0 + e1): 17 fail — all 16 of test_cell_prologue_pair and the pair launch without
     prologue jobs."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import step_ends_ref as sr
from gpu_util import assert_close_scaled, dev

pytestmark = pytest.mark.gpu

KK = 2e-5                                          # kernel against kernel, same math, same inputs
GUARD = 8                                          # NaN floats on each side of every output (a multiple of 4: float4 stores)
E_ARG, E_SHAPE, E_LIMIT = r'rc=-1\)', r'rc=-2\)', r'rc=-3\)'
NAN = float('nan')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


class _Pool:
    """Outputs of a test: each a view into its own NaN buffer with GUARD floats before and after it."""

    def __init__(self):
        self.bufs = []

    def new(self, *shape, base=None, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= int(s)
        buf = torch.full((n + 2 * GUARD,), NAN, device=dev(), dtype=dtype)
        view = buf[GUARD:GUARD + n].view(*shape)
        if base is not None:
            view.copy_(base)
        self.bufs.append((buf, n))
        return view

    def check(self):
        torch.cuda.synchronize()
        for buf, n in self.bufs:
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), \
                f'a guard of a {n}-float output was written'


def _same(name, a, b):
    assert a.shape == b.shape and torch.equal(a, b), f'{name}: not bit-equal'


def _is_plus_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


# ------------------------------------------------------------------------------------------------ architecture tensors
ARCH_SETS = {
    'net': [(8, 2), (2, 2), (3, 4)],                              # a search net's: alphas, betas, gammas
    'max16': [(t + 1, t % 4 + 1) for t in range(16)],             # BMNAS_MAX_PTRS tensors, columns 1, 2, 3, 4, 1, ...
    'rows64': [(63, 2), (1, 4)],                                  # the multi kernel's 64-thread workgroups: full | + 1
    'rows65': [(63, 2), (2, 4)],                                  # (the second tensor straddles the edge)
    'rows256': [(200, 4), (56, 2)],                               # the prologue's 256-thread workgroups: full | + 1
    'rows257': [(200, 4), (57, 2)],
}
LOGIT_KINDS = ['normal', 'equal', 'winner', 'offset']


def _logits(g, rows, cols, kind):
    if kind == 'normal':
        return _rand(g, rows, cols) * 3.0
    if kind == 'equal':
        return (_rand(g, rows, 1) * 3.0).expand(rows, cols).contiguous()
    if kind == 'winner':                                           # one entry 90 above the rest
        a = _rand(g, rows, cols)
        k = torch.randint(0, cols, (rows,), generator=g)
        a[torch.arange(rows), k] += 90.0
        return a
    return _rand(g, rows, cols) * 3.0 + 1e4                        # a common offset of 1e4


def _tiny_ln(g, pool):
    """The smallest LayerNorm problem an epilogue launch can carry (it needs one): C L = 4 at b = 1, prenorm.
    -> (problem dict, check())"""
    p = _ln_problem(g, 'attn', 1, 4, 1, 1, False)
    dw, db = pool.new(p.N, base=p.base_w), pool.new(p.N, base=p.base_b)

    def check():
        assert_close_scaled('tiny LN dln_w', dw, p.want_w)
        assert_close_scaled('tiny LN dln_b', db, p.want_b)
    return p.prob(dw, db), check


# ---------------------------------------------------------------------------------- A. forward row softmax, three forms
@pytest.mark.parametrize('kind', LOGIT_KINDS)
@pytest.mark.parametrize('name', sorted(ARCH_SETS))
def test_row_softmax_fwd_three_forms(name, kind):
    from bmnas import lib
    shapes = ARCH_SETS[name]
    g = _gen(1000 + len(name) + 7 * LOGIT_KINDS.index(kind) + shapes[0][0])
    logits = [_logits(g, r, c, kind) for r, c in shapes]
    ld = [a.to(dev()) for a in logits]
    pool = _Pool()
    single = [pool.new(r, c) for r, c in shapes]
    multi = [pool.new(r, c) for r, c in shapes]
    pro = [pool.new(r, c) for r, c in shapes]
    for a, o, (r, c) in zip(ld, single, shapes):
        lib.arch_softmax_fwd(a, o, r, c)
    lib.arch_softmax_multi(ld, None, multi, 0)
    lib.cell_prologue(ld, pro, [], [], 0, 0)
    pool.check()
    for t, a in enumerate(logits):
        want = sr.row_softmax(a)
        for form, outs in (('arch_softmax_fwd', single), ('arch_softmax_multi', multi), ('cell_prologue', pro)):
            assert_close_scaled(f'{form} tensor {t}', outs[t], want)
        _same(f'tensor {t}: arch_softmax_fwd | arch_softmax_multi', single[t], multi[t])
        _same(f'tensor {t}: arch_softmax_multi | cell_prologue', multi[t], pro[t])
        if kind == 'winner':
            assert bool((pro[t].max(dim=1).values == 1.0).all()), f'tensor {t}: the winner is not exactly 1.0'
        if kind == 'equal':
            assert bool((pro[t] == pro[t][:, :1]).all())


@pytest.mark.parametrize('rows,cols', [(3, 5), (65, 5), (2, 7)])
def test_single_tensor_forms_take_more_than_four_columns(rows, cols):
    """bmnas_arch_softmax_fwd / _bwd are not gated at 4 columns (ArchSoftmaxFn passes any width on); the packed forms
    are, and say so."""
    from bmnas import lib
    g = _gen(1100 + rows + cols)
    a, dw = _rand(g, rows, cols) * 3.0, _rand(g, rows, cols)
    pool = _Pool()
    w, da = pool.new(rows, cols), pool.new(rows, cols)
    lib.arch_softmax_fwd(a.to(dev()), w, rows, cols)
    lib.arch_softmax_bwd(w, dw.to(dev()), da, rows, cols)
    pool.check()
    assert_close_scaled('softmax', w, sr.row_softmax(a))
    assert_close_scaled('softmax backward', da, sr.row_softmax_bwd(w, dw[None]))
    ad, o = a.to(dev()), pool.new(rows, cols)
    with pytest.raises(lib.BmnasError, match=E_ARG):
        lib.arch_softmax_multi([ad], None, [o], 0)
    with pytest.raises(lib.BmnasError, match=E_ARG):
        lib.arch_softmax_multi([w], [dw.to(dev())], [o], 1)
    with pytest.raises(lib.BmnasError, match=E_ARG):
        lib.cell_prologue([ad], [o], [], [], 0, 0)
    pool.check()
    assert bool(torch.isnan(o).all())


# ------------------------------------------------------------------------------------------ B. the prologue's other jobs
FOLD_SHAPES = [(16, 4), (48, 16), (576, 192), (576, 256)]          # (576, 256): 36864 float4 > 128 x 256, the stride loop
SCRUB_WIDE = 512 * 256 * 4 + 4                                     # one float4 more than 512 workgroups take in one pass


def _fold_inputs(g, n_fold, M, Cc):
    return [_rand(g, M, 2 * Cc) for _ in range(n_fold)]


@pytest.mark.parametrize('n_fold', [1, 2, 8])
@pytest.mark.parametrize('M,Cc', FOLD_SHAPES)
def test_prologue_fold(M, Cc, n_fold):
    from bmnas import lib
    Ws = _fold_inputs(_gen(1200 + M + Cc + n_fold), n_fold, M, Cc)
    Wd = [w.to(dev()) for w in Ws]
    pool = _Pool()
    Weffs = [pool.new(M, Cc) for _ in Ws]
    alone = [pool.new(M, Cc) for _ in Ws]
    lib.cell_prologue([], [], Wd, Weffs, M, Cc)
    for w, o in zip(Wd, alone):
        lib.fold_weight(w, o, M, Cc)
    pool.check()
    for q, w in enumerate(Ws):
        _same(f'fold {q}: fp32 W[:, :C] + W[:, C:]', Weffs[q].cpu(), w[:, :Cc] + w[:, Cc:])
        _same(f'fold {q}: cell_prologue | fold_weight', Weffs[q], alone[q])
        assert_close_scaled(f'fold {q}', Weffs[q], sr.fold(w))


def _counter():
    d = dev()
    return (torch.tensor([2 ** 40 + 5], dtype=torch.int64, device=d), torch.tensor([7], dtype=torch.int64, device=d))


def _pair_inputs(g, n_in, n_elem):
    """xs, alpha (n_in + 3, 2) whose rows 2 .. 2 + n_in are the step's, beta (3, 2) whose third row is NaN"""
    xs = [_rand(g, n_elem) for _ in range(n_in)]
    alpha = _rand(g, n_in + 3, 2) * 2.0
    beta = _rand(g, 3, 2) * 2.0
    beta[2] = NAN
    return xs, alpha, beta


@pytest.mark.parametrize('launch', ['alone', 'scrub', 'jobs', 'pair'])
def test_prologue_step_counter(launch):
    """counter += span exactly once per launch, whatever else the grid does (one thread of the LAST workgroup adds)"""
    from bmnas import lib
    g, d = _gen(1300), dev()
    counter, span = _counter()
    pool = _Pool()
    a = [_logits(g, r, c, 'normal').to(d) for r, c in ARCH_SETS['rows257']]
    outs = [pool.new(r, c) for r, c in ARCH_SETS['rows257']]
    Ws = [w.to(d) for w in _fold_inputs(g, 2, 48, 16)]
    Weffs = [pool.new(48, 16) for _ in Ws]
    scrub = pool.new(SCRUB_WIDE)
    xs, alpha, beta = _pair_inputs(g, 2, 1024)
    xs, alpha, beta = [x.to(d) for x in xs], alpha.to(d), beta.to(d)
    h, z = pool.new(1024), pool.new(1024)
    for k in (1, 2):
        if launch == 'alone':
            lib.cell_prologue([], [], [], [], 0, 0, step=(counter, span))
        elif launch == 'scrub':                                    # widens the grid to 512 workgroups
            lib.cell_prologue([], [], [], [], 0, 0, step=(counter, span), scrub=scrub)
        elif launch == 'jobs':
            lib.cell_prologue(a, outs, Ws, Weffs, 48, 16, step=(counter, span))
        else:
            lib.cell_prologue_pair(a, outs, Ws, Weffs, 48, 16, (counter, span), scrub, xs, alpha[2:], beta, h, z)
        pool.check()
        assert int(counter.item()) == 2 ** 40 + 5 + 7 * k, (launch, k, int(counter.item()))
        assert int(span.item()) == 7
    if launch in ('scrub', 'pair'):
        assert _is_plus_zero(scrub)
    else:
        assert bool(torch.isnan(scrub).all())                      # scrub=None: nothing of it is touched


@pytest.mark.parametrize('with_jobs', [False, True])
@pytest.mark.parametrize('scrub_n', [4, 1020, 4100, SCRUB_WIDE])
def test_prologue_scrub(scrub_n, with_jobs):
    from bmnas import lib
    g, d = _gen(1400 + scrub_n % 997), dev()
    pool = _Pool()
    scrub = pool.new(scrub_n)
    untouched = pool.new(scrub_n)
    if with_jobs:
        a = [_logits(g, r, c, 'normal').to(d) for r, c in ARCH_SETS['net']]
        outs = [pool.new(r, c) for r, c in ARCH_SETS['net']]
        Ws = [w.to(d) for w in _fold_inputs(g, 1, 16, 4)]
        lib.cell_prologue(a, outs, Ws, [pool.new(16, 4)], 16, 4, scrub=scrub)
    else:
        lib.cell_prologue([], [], [], [], 0, 0, scrub=scrub)
    pool.check()
    assert _is_plus_zero(scrub), 'the range is not all +0.0'
    assert bool(torch.isnan(untouched).all())


def test_prologue_all_jobs_equal_each_job_alone():
    from bmnas import lib
    g, d = _gen(1500), dev()
    shapes = ARCH_SETS['max16']
    M, Cc = 576, 256
    logits = [_logits(g, r, c, 'normal').to(d) for r, c in shapes]
    Ws = [w.to(d) for w in _fold_inputs(g, 8, M, Cc)]
    pool = _Pool()
    outs, outs1 = [pool.new(r, c) for r, c in shapes], [pool.new(r, c) for r, c in shapes]
    Weffs, Weffs1 = [pool.new(M, Cc) for _ in Ws], [pool.new(M, Cc) for _ in Ws]
    scrub = pool.new(4100)
    counter, span = _counter()
    lib.cell_prologue(logits, outs, Ws, Weffs, M, Cc, step=(counter, span), scrub=scrub)
    lib.cell_prologue(logits, outs1, [], [], 0, 0)
    lib.cell_prologue([], [], Ws, Weffs1, M, Cc)
    pool.check()
    for t in range(len(shapes)):
        _same(f'softmax {t}', outs[t], outs1[t])
        assert_close_scaled(f'softmax {t}', outs[t], sr.row_softmax(logits[t]))
    for q in range(len(Ws)):
        _same(f'fold {q}', Weffs[q], Weffs1[q])
        _same(f'fold {q} against fp32', Weffs[q], Ws[q][:, :Cc] + Ws[q][:, Cc:])
    assert _is_plus_zero(scrub)
    assert int(counter.item()) == 2 ** 40 + 12


def test_prologue_refusals():
    from bmnas import lib
    g, d = _gen(1600), dev()
    pool = _Pool()
    nine = [_rand(g, 16, 8).to(d) for _ in range(9)]
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.cell_prologue([], [], nine, [pool.new(16, 4) for _ in nine], 16, 4)
    a17 = [_rand(g, 2, 2).to(d) for _ in range(17)]
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.cell_prologue(a17, [pool.new(2, 2) for _ in a17], [], [], 0, 0)
    with pytest.raises(lib.BmnasError, match=E_SHAPE):
        lib.cell_prologue([], [], [_rand(g, 16, 12).to(d)], [pool.new(16, 6)], 16, 6)
    with pytest.raises(lib.BmnasError, match=E_ARG):
        lib.cell_prologue([_rand(g, 3, 5).to(d)], [pool.new(3, 5)], [], [], 0, 0)
    with pytest.raises(lib.BmnasError, match=E_ARG):
        lib.cell_prologue([], [], [], [], 0, 0, scrub=pool.new(6))
    # a counter without a span: the wrapper always passes both, so straight through the C ABI
    counter, _ = _counter()
    none_p, none_i = (C.c_void_p * 1)(), (C.c_int * 1)()
    rc = lib.load().bmnas_cell_prologue(none_p, none_p, none_i, none_i, 0, none_p, none_p, 0, 0, 0, counter.data_ptr(),
                                        None, None, 0, None)
    assert rc == -1, rc
    pool.check()
    for buf, _ in pool.bufs:
        assert bool(torch.isnan(buf).all())                         # a refused call writes nothing
    assert int(counter.item()) == 2 ** 40 + 5


# ------------------------------------------------------------------------------------------------ C. cell_prologue_pair
PAIR_BIG = 4 * (2048 * 256 + 300)                                  # above the 2048-workgroup cap: the stride loop


@pytest.mark.parametrize('n_in,n_elem', [(n, e) for n in (1, 2, 3, 8, 15) for e in (4, 1020, 1024)] + [(2, PAIR_BIG)])
def test_cell_prologue_pair(n_in, n_elem):
    from bmnas import lib
    g, d = _gen(1700 + n_in + n_elem % 1009), dev()
    xs, alpha, beta = _pair_inputs(g, n_in, n_elem)
    xd, ad, bd = [x.to(d) for x in xs], alpha.to(d), beta.to(d)
    M, Cc = 48, 16
    Ws = [w.to(d) for w in _fold_inputs(g, 2, M, Cc)]
    a_list = [ad, bd[:2]]
    pool = _Pool()
    outs = [pool.new(n_in + 3, 2), pool.new(2, 2)]
    outs1 = [pool.new(n_in + 3, 2), pool.new(2, 2)]
    Weffs, Weffs1 = [pool.new(M, Cc) for _ in Ws], [pool.new(M, Cc) for _ in Ws]
    scrub, scrub1 = pool.new(1020), pool.new(1020)
    h, z, h1, z1 = pool.new(n_elem), pool.new(n_elem), pool.new(n_elem), pool.new(n_elem)
    lib.cell_prologue_pair(a_list, outs, Ws, Weffs, M, Cc, None, scrub, xd, ad[2:], bd, h, z)
    lib.cell_prologue(a_list, outs1, Ws, Weffs1, M, Cc, scrub=scrub1)
    # the stand-alone pair sum, fed the weights the pair launch itself stored (column 1 of the softmaxed rows)
    lib.mixsum_pair_fwd(xd, outs[0].reshape(-1)[2 * 2 + 1:], 2, outs[1].reshape(-1)[1:], 2, h1, z1)
    pool.check()
    want_h, want_z = sr.pair_sum(xs, alpha[2:2 + n_in], beta[:2])
    assert_close_scaled('h', h, want_h)
    assert_close_scaled('z', z, want_z)
    assert_close_scaled('h against mixsum_pair_fwd', h, h1.cpu(), rel=KK)
    assert_close_scaled('z against mixsum_pair_fwd', z, z1.cpu(), rel=KK)
    for t in range(2):
        _same(f'softmax {t}: pair launch | cell_prologue', outs[t], outs1[t])
        assert_close_scaled(f'softmax {t}', outs[t], sr.row_softmax(a_list[t]))
    for q in range(len(Ws)):
        _same(f'fold {q}: pair launch | cell_prologue', Weffs[q], Weffs1[q])
        _same(f'fold {q} against fp32', Weffs[q], Ws[q][:, :Cc] + Ws[q][:, Cc:])
    assert _is_plus_zero(scrub) and _is_plus_zero(scrub1)


def test_cell_prologue_pair_without_prologue_jobs():
    """no arch tensor, fold, counter or scrub: zero prologue workgroups in front of the pair sum"""
    from bmnas import lib
    g, d = _gen(1800), dev()
    xs, alpha, beta = _pair_inputs(g, 3, 1020)
    pool = _Pool()
    h, z = pool.new(1020), pool.new(1020)
    lib.cell_prologue_pair([], [], [], [], 0, 0, None, None, [x.to(d) for x in xs], alpha.to(d)[2:], beta.to(d), h, z)
    pool.check()
    want_h, want_z = sr.pair_sum(xs, alpha[2:5], beta[:2])
    assert_close_scaled('h', h, want_h)
    assert_close_scaled('z', z, want_z)


def test_cell_prologue_pair_refusals():
    from bmnas import lib
    g, d = _gen(1900), dev()
    pool = _Pool()
    xs, alpha, beta = _pair_inputs(g, 16, 8)
    xd, ad, bd = [x.to(d) for x in xs], alpha.to(d), beta.to(d)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.cell_prologue_pair([], [], [], [], 0, 0, None, None, xd, ad[2:], bd, pool.new(8), pool.new(8))
    x6 = [_rand(g, 6).to(d)]
    with pytest.raises(lib.BmnasError, match=E_SHAPE):
        lib.cell_prologue_pair([], [], [], [], 0, 0, None, None, x6, ad[2:], bd, pool.new(6), pool.new(6))
    pool.check()
    for buf, _ in pool.bufs:
        assert bool(torch.isnan(buf).all())


# ------------------------------------------------------------------------------------- D. softmax backward, three forms
def _arch_bwd_inputs(g, shapes, n_shards, pad):
    """w: softmaxed rows; shards (n_shards, total + pad): the gradient copies, the pad floats NaN; dws: views of shard 0"""
    total = sum(r * c for r, c in shapes)
    stride = total + pad
    ws = [sr.row_softmax(_rand(g, r, c)).float() for r, c in shapes]
    shards = torch.full((n_shards, stride), NAN)
    shards[:, :total] = _rand(g, n_shards, total)
    return ws, shards, stride


def _shard_views(shards, shapes):
    """per tensor: (n_shards, rows, cols) of the CPU copy, for the reference"""
    out, at = [], 0
    for r, c in shapes:
        out.append(shards[:, at:at + r * c].reshape(shards.shape[0], r, c))
        at += r * c
    return out


def _shard0_views(shards_dev, shapes):
    """per tensor: the (rows, cols) view of shard 0 in place — the kernels find shard s at + s * shard_stride floats"""
    out, at = [], 0
    for r, c in shapes:
        out.append(shards_dev[0, at:at + r * c].view(r, c))
        at += r * c
    return out


@pytest.mark.parametrize('n_shards', [1, 2, 16, 17, 40])
@pytest.mark.parametrize('name', sorted(ARCH_SETS))
def test_row_softmax_bwd_three_forms(name, n_shards):
    from bmnas import lib
    shapes = ARCH_SETS[name]
    d = dev()
    for pad in (0, 12):
        g = _gen(2000 + len(name) + shapes[0][0] + 3 * n_shards + pad)
        ws, shards, stride = _arch_bwd_inputs(g, shapes, n_shards, pad)
        wd, sd = [w.to(d) for w in ws], shards.to(d)
        dws = _shard0_views(sd, shapes)
        cpu_views = _shard_views(shards, shapes)
        pool = _Pool()
        multi = [pool.new(r, c) for r, c in shapes]
        epi = [pool.new(r, c) for r, c in shapes]
        lib.arch_softmax_multi(wd, dws, multi, 1, n_shards, stride)
        # with the 257-row sets this is the widened grid: the LayerNorm problem alone would make it 1 x 1
        prob, check_ln = _tiny_ln(g, pool)
        lib.backward_epilogue([prob], 1, 4, wd, dws, epi, n_shards, stride)
        single = None
        if n_shards == 1:
            single = [pool.new(r, c) for r, c in shapes]
            for t, (r, c) in enumerate(shapes):
                lib.arch_softmax_bwd(wd[t], dws[t].contiguous(), single[t], r, c)
        pool.check()
        check_ln()
        for t, (r, c) in enumerate(shapes):
            want = sr.row_softmax_bwd(ws[t], cpu_views[t])
            assert_close_scaled(f'{name} pad {pad} tensor {t}: arch_softmax_multi', multi[t], want)
            assert_close_scaled(f'{name} pad {pad} tensor {t}: backward_epilogue', epi[t], want)
            _same(f'{name} pad {pad} tensor {t}: arch_softmax_multi | backward_epilogue', multi[t], epi[t])
            if single is not None:
                assert_close_scaled(f'{name} pad {pad} tensor {t}: arch_softmax_bwd', single[t], want)
                assert_close_scaled(f'{name} tensor {t}: arch_softmax_bwd against multi', single[t], multi[t].cpu(),
                                    rel=KK)
            if c == 1:                                             # softmax of one column is the constant 1
                for o in (multi[t], epi[t]) + ((single[t],) if single is not None else ()):
                    assert float(o.abs().max()) == 0.0, f'tensor {t}: a one-column tensor has a gradient'


def test_arch_bwd_refusals():
    from bmnas import lib
    g, d = _gen(2100), dev()
    pool = _Pool()
    w17 = [sr.row_softmax(_rand(g, 2, 2)).float().to(d) for _ in range(17)]
    dw17 = [_rand(g, 2, 2).to(d) for _ in range(17)]
    o17 = [pool.new(2, 2) for _ in range(17)]
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.arch_softmax_multi(w17, dw17, o17, 1, 1, 0)
    prob, _ = _tiny_ln(g, _Pool())
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.backward_epilogue([prob], 1, 4, w17, dw17, o17, 1, 0)
    w5 = [sr.row_softmax(_rand(g, 3, 5)).float().to(d)]
    with pytest.raises(lib.BmnasError, match=E_ARG):
        lib.backward_epilogue([prob], 1, 4, w5, [_rand(g, 3, 5).to(d)], [pool.new(3, 5)], 1, 0)
    pool.check()
    for buf, _ in pool.bufs:
        assert bool(torch.isnan(buf).all())


# ------------------------------------------------------------------------------ E. LayerNorm-affine reductions, three forms
# per-source (C, L) and, for the K7-like kind, the number of sources (the other kinds take one source)
LN_SHAPES = [(1, 4, 1), (63, 4, 3), (16, 4, 4), (65, 4, 1), (68, 16, 1), (192, 16, 2)]   # (16, 4) x 4: one 64-column block
LN_BATCHES = [1, 3, 16, 17, 37, 257]                   # 257 (L = 4 only): 16 chunks of 17 samples, the last holding 2
LN_KINDS = ['k7', 'k6', 'attn']


def _ln_problem(g, kind, Cc, L, n_src, b, gscale):
    """One reduction with its float64 expectation.  k7: relu over cat(srcs), the bias cleared of near-zero ReLU
    arguments; k6: one source + resid, no relu; attn: prenorm, srcs[0] = xhat, no statistics."""
    d = dev()
    if kind != 'k7':
        n_src = 1
    N = n_src * Cc * L
    srcs = [_rand(g, b, Cc, L) * 1.5 + 0.2 for _ in range(n_src)]
    resid = _rand(g, b, Cc, L) if kind == 'k6' else None
    ln_w, ln_b = _rand(g, N) * 0.3 + 1.0, _rand(g, N) * 0.2
    gy = _rand(g, b, N)
    x = torch.cat([s.double().reshape(b, -1) for s in srcs], dim=1)
    if resid is not None:
        x = x + resid.double().reshape(b, -1)
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + 1e-5)
    stats = torch.stack([mean, rstd], dim=1).float().contiguous()
    relu = prenorm = 0
    if kind == 'k7':
        relu = 1
        ln_b = sr.clear_relu_bias(g, srcs, ln_w, ln_b)             # raises if the margin cannot be reached
        xhat = (x - stats[:, 0:1].double()) * stats[:, 1:2].double()
        margin = float((xhat * ln_w.double() + ln_b.double()).abs().min())
        assert margin >= sr.RELU_MARGIN, f'a ReLU argument lies {margin:.2e} from zero'
    if kind == 'attn':
        prenorm = 1
        srcs = [((x - mean[:, None]) * rstd[:, None]).float().reshape(b, Cc, L)]
        stats, ln_w, ln_b = None, None, None
    gs = torch.tensor([0.37]) if gscale else None
    dw, db = sr.ln_affine(gy, gs, srcs, resid, ln_w, ln_b, stats, relu, prenorm)
    base_w, base_b = _rand(g, N), _rand(g, N)
    dv = lambda t: None if t is None else t.to(d)
    dev_in = dict(g=dv(gy), gscale=dv(gs), srcs=[dv(s) for s in srcs], resid=dv(resid), ln_w=dv(ln_w), ln_b=dv(ln_b),
                  stats=dv(stats), C=Cc, relu=relu, prenorm=prenorm)

    def prob(dln_w, dln_b):
        return dict(dev_in, dln_w=dln_w, dln_b=dln_b)
    return SimpleNamespace(N=N, Cc=Cc, L=L, b=b, base_w=base_w, base_b=base_b, want_w=base_w.double() + dw,
                           want_b=base_b.double() + db, prob=prob)


def _ln_single(lib, p, pr):
    lib.ln_affine_bwd(pr['g'], pr['gscale'], pr['srcs'], pr['resid'], pr['ln_w'], pr['ln_b'], pr['stats'], pr['dln_w'],
                      pr['dln_b'], p.b, p.Cc, p.L, pr['relu'], pr['prenorm'])


def _ln_outs(pool, p):
    return pool.new(p.N, base=p.base_w), pool.new(p.N, base=p.base_b)


def _ln_check(name, p, outs, pinned=None):
    assert_close_scaled(name + ' dln_w', outs[0], p.want_w)
    assert_close_scaled(name + ' dln_b', outs[1], p.want_b)
    if pinned is not None:
        assert_close_scaled(name + ' dln_w (kernel vs kernel)', outs[0], pinned[0].cpu(), rel=KK)
        assert_close_scaled(name + ' dln_b (kernel vs kernel)', outs[1], pinned[1].cpu(), rel=KK)


@pytest.mark.parametrize('gscale', [False, True])
@pytest.mark.parametrize('kind', LN_KINDS)
@pytest.mark.parametrize('Cc,L,n_src', LN_SHAPES)
def test_ln_affine_three_forms(Cc, L, n_src, kind, gscale):
    from bmnas import lib
    for b in LN_BATCHES:
        if b == 257 and L != 4:
            continue
        g = _gen(3000 + 13 * Cc + L + 101 * b + LN_KINDS.index(kind) + 7 * int(gscale))
        p = _ln_problem(g, kind, Cc, L, n_src, b, gscale)
        pool = _Pool()
        single, multi, epi = _ln_outs(pool, p), _ln_outs(pool, p), _ln_outs(pool, p)
        _ln_single(lib, p, p.prob(*single))
        lib.ln_affine_bwd_multi([p.prob(*multi)], b, L)
        lib.backward_epilogue([p.prob(*epi)], b, L, [], [], [], 1, 0)      # n_arch = 0, n_sums = 0: the per-op path's form
        pool.check()
        tag = f'{kind} C {Cc} L {L} b {b}'
        _ln_check(tag + ' ln_affine_bwd', p, single)
        _ln_check(tag + ' ln_affine_bwd_multi', p, multi, single)
        _ln_check(tag + ' backward_epilogue', p, epi, single)


def _eight_problems(g, b):
    """widths d4 = 1 .. 130 (L = 4, one source: d4 = C) of mixed kinds: the narrow problems' workgroups return early"""
    spec = [(1, 'attn', False), (2, 'k7', True), (16, 'k6', False), (63, 'k7', False), (64, 'attn', True),
            (65, 'k6', True), (129, 'k7', True), (130, 'k6', False)]
    return [_ln_problem(g, kind, Cc, 4, 1, b, gs) for Cc, kind, gs in spec]


@pytest.mark.parametrize('b', [17, 257])
def test_ln_affine_multi_of_eight_widths(b):
    from bmnas import lib
    g = _gen(3100 + b)
    ps = _eight_problems(g, b)
    pool = _Pool()
    multi, epi, single = ([_ln_outs(pool, p) for p in ps] for _ in range(3))
    lib.ln_affine_bwd_multi([p.prob(*o) for p, o in zip(ps, multi)], b, 4)
    lib.backward_epilogue([p.prob(*o) for p, o in zip(ps, epi)], b, 4, [], [], [], 1, 0)
    for p, o in zip(ps, single):
        _ln_single(lib, p, p.prob(*o))
    pool.check()
    for i, p in enumerate(ps):
        _ln_check(f'problem {i} single', p, single[i])
        _ln_check(f'problem {i} multi', p, multi[i], single[i])
        _ln_check(f'problem {i} epilogue', p, epi[i], single[i])
    nine = ps + [ps[0]]
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.ln_affine_bwd_multi([p.prob(*_ln_outs(pool, p)) for p in nine], b, 4)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.backward_epilogue([p.prob(*_ln_outs(pool, p)) for p in nine], b, 4, [], [], [], 1, 0)


def test_ln_affine_deterministic_mode():
    """one chunk for the whole batch: a single add per element, so two runs give the same bits"""
    from bmnas import cell as K
    from bmnas import lib
    cases = [('k7', 63, 4, 3, 37), ('k6', 65, 4, 1, 257), ('attn', 68, 16, 1, 17), ('k7', 16, 4, 4, 3)]
    lib.set_deterministic(True)
    try:
        for kind, Cc, L, n_src, b in cases:
            g = _gen(3200 + Cc + b)
            p = _ln_problem(g, kind, Cc, L, n_src, b, True)
            pool = _Pool()
            r1, r2, multi, epi = (_ln_outs(pool, p) for _ in range(4))
            _ln_single(lib, p, p.prob(*r1))
            _ln_single(lib, p, p.prob(*r2))
            lib.ln_affine_bwd_multi([p.prob(*multi)], b, L)
            lib.backward_epilogue([p.prob(*epi)], b, L, [], [], [], 1, 0)
            pool.check()
            tag = f'deterministic {kind} C {Cc} b {b}'
            _ln_check(tag, p, r1)
            for other, nm in ((r2, 'second run'), (multi, 'multi'), (epi, 'epilogue')):
                _same(f'{tag} dln_w: first run | {nm}', r1[0], other[0])
                _same(f'{tag} dln_b: first run | {nm}', r1[1], other[1])
    finally:
        lib.set_deterministic(K.DETERMINISTIC)


def test_ln_affine_refusals():
    from bmnas import lib
    g, d = _gen(3300), dev()
    b, Cc, L = 3, 4, 4
    pool = _Pool()
    src = lambda: _rand(g, b, Cc, L).to(d)
    vec = lambda n: _rand(g, n).to(d)
    stats = torch.stack([torch.zeros(b), torch.ones(b)], 1).to(d)
    dw, db = pool.new(5 * Cc * L), pool.new(5 * Cc * L)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):               # five sources
        lib.ln_affine_bwd(vec(b * 5 * Cc * L), None, [src() for _ in range(5)], None, vec(5 * Cc * L), vec(5 * Cc * L),
                          stats, dw, db, b, Cc, L, 1, 0)
    with pytest.raises(lib.BmnasError, match=E_ARG):                 # a residual with two sources
        lib.ln_affine_bwd(vec(b * 2 * Cc * L), None, [src(), src()], src(), vec(2 * Cc * L), vec(2 * Cc * L), stats, dw,
                          db, b, Cc, L, 0, 0)
    with pytest.raises(lib.BmnasError, match=E_SHAPE):               # C L = 6
        lib.ln_affine_bwd(vec(b * 6), None, [_rand(g, b, 3, 2).to(d)], None, vec(6), vec(6), stats, dw, db, b, 3, 2, 0, 0)
    with pytest.raises(lib.BmnasError, match=E_ARG):                 # relu without the affine
        lib.ln_affine_bwd(vec(b * Cc * L), None, [src()], None, None, None, stats, dw, db, b, Cc, L, 1, 0)
    with pytest.raises(lib.BmnasError, match=E_ARG):                 # no statistics, not prenorm
        lib.ln_affine_bwd(vec(b * Cc * L), None, [src()], None, vec(Cc * L), vec(Cc * L), None, dw, db, b, Cc, L, 0, 0)
    pool.check()
    assert bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all())


# ------------------------------------------------------------------------------------------ F. chunk sums in the epilogue
SUM_BIG = 4 * (256 * 256 + 5)                                      # above the 256-workgroup wish: S.reps > 1
SUM_CASES = [(1, 4), (3, 1020), (16, SUM_BIG)]


def _epilogue_rc(lib, prob, b, L, sums):
    """bmnas_backward_epilogue with one LayerNorm problem, no arch tensors and (part, out, n_chunk, n) sums, straight
    through the C ABI -> rc (lib.backward_epilogue asserts n % 4 == 0 itself)"""
    P, PP = C.c_void_p, C.POINTER(C.c_void_p)
    one = lambda key: (P * 1)(None if prob[key] is None else prob[key].data_ptr())
    src_arr = (P * len(prob['srcs']))(*[s.data_ptr() for s in prob['srcs']])
    srcs = (PP * 1)(C.cast(src_arr, PP))
    i1 = lambda v: (C.c_int * 1)(int(v))
    ns = len(sums)
    none_p, none_i = (P * 1)(), (C.c_int * 1)()
    sp = (P * ns)(*[s[0].data_ptr() for s in sums])
    so = (P * ns)(*[s[1].data_ptr() for s in sums])
    sc = (C.c_int * ns)(*[int(s[2]) for s in sums])
    sn = (C.c_int64 * ns)(*[int(s[3]) for s in sums])
    return lib.load().bmnas_backward_epilogue(1, one('g'), one('gscale'), srcs, i1(len(prob['srcs'])), one('resid'),
                                              one('ln_w'), one('ln_b'), one('stats'), one('dln_w'), one('dln_b'), b,
                                              i1(prob['C']), L, i1(prob['relu']), i1(prob['prenorm']), none_p, none_p,
                                              none_p, none_i, none_i, 0, 1, 0, ns, sp, so, sc, sn,
                                              torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize('case', ['one_chunk', 'three', 'big', 'two_unequal', 'two_unequal_swapped'])
def test_epilogue_chunk_sums(case):
    from bmnas import lib
    which = {'one_chunk': [0], 'three': [1], 'big': [2], 'two_unequal': [1, 2], 'two_unequal_swapped': [2, 0]}[case]
    g, d = _gen(4000 + len(case)), dev()
    parts = [_rand(g, SUM_CASES[i][0] * SUM_CASES[i][1]) for i in which]
    pd = [p.to(d) for p in parts]
    pool = _Pool()
    outs = [pool.new(SUM_CASES[i][1]) for i in which]
    alone = [pool.new(SUM_CASES[i][1]) for i in which]
    prob, check_ln = _tiny_ln(g, pool)                              # a 1 x 1 LayerNorm grid: reps carries the width
    lib.backward_epilogue([prob], 1, 4, [], [], [], 1, 0,
                          sums=[(p, o, SUM_CASES[i][0]) for p, o, i in zip(pd, outs, which)])
    for p, o, i in zip(pd, alone, which):
        lib.sum_chunks(p, o, SUM_CASES[i][0])
    pool.check()
    check_ln()
    for k, i in enumerate(which):
        assert_close_scaled(f'sum {k}', outs[k], sr.chunk_sum(parts[k], SUM_CASES[i][0]))
        assert_close_scaled(f'sum_chunks {k}', alone[k], sr.chunk_sum(parts[k], SUM_CASES[i][0]))
        assert_close_scaled(f'sum {k} against sum_chunks', outs[k], alone[k].cpu(), rel=KK)


def test_epilogue_chunk_sums_on_a_wide_ln_grid():
    """the same sums next to a LayerNorm problem whose own grid is 3 x 3: reps = ceil(256 / 9), slices of 9 workgroups"""
    from bmnas import lib
    g, d = _gen(4100), dev()
    p = _ln_problem(g, 'k6', 129, 4, 1, 37, False)
    n_chunk, n = SUM_CASES[2]
    part = _rand(g, n_chunk * n)
    pool = _Pool()
    out, lnw, lnb = pool.new(n), *_ln_outs(pool, p)
    lib.backward_epilogue([p.prob(lnw, lnb)], 37, 4, [], [], [], 1, 0, sums=[(part.to(d), out, n_chunk)])
    pool.check()
    _ln_check('LN', p, (lnw, lnb))
    assert_close_scaled('sum', out, sr.chunk_sum(part, n_chunk))


def test_epilogue_sum_refusals():
    from bmnas import lib
    g, d = _gen(4200), dev()
    pool = _Pool()
    prob, _ = _tiny_ln(g, _Pool())
    three = [(_rand(g, 8).to(d), pool.new(4), 2) for _ in range(3)]
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.backward_epilogue([prob], 1, 4, [], [], [], 1, 0, sums=three)
    out6 = pool.new(6)
    rc = _epilogue_rc(lib, prob, 1, 4, [(_rand(g, 12).to(d), out6, 2, 6)])
    assert rc == -1, rc
    pool.check()
    for buf, _ in pool.bufs:
        assert bool(torch.isnan(buf).all())
    # ... and the same call with n % 4 == 0 goes through (the refusal above was the size's, not the call's)
    out8 = pool.new(8)
    part = _rand(g, 16)
    prob2, _ = _tiny_ln(g, _Pool())
    assert _epilogue_rc(lib, prob2, 1, 4, [(part.to(d), out8, 2, 8)]) == 0
    pool.check()
    assert_close_scaled('sum', out8, sr.chunk_sum(part, 2))


# --------------------------------------------------------------------------------------------------- G. one full epilogue
def test_full_epilogue_equals_its_jobs_launched_separately():
    from bmnas import lib
    g, d = _gen(5000), dev()
    b, L, n_shards, pad = 17, 4, 17, 12
    ps = _eight_problems(g, b)
    shapes = ARCH_SETS['max16']
    ws, shards, stride = _arch_bwd_inputs(g, shapes, n_shards, pad)
    wd, sd = [w.to(d) for w in ws], shards.to(d)
    dws = _shard0_views(sd, shapes)
    sum_cases = [SUM_CASES[1], SUM_CASES[2]]
    parts = [_rand(g, c * n) for c, n in sum_cases]
    pd = [p.to(d) for p in parts]
    pool = _Pool()
    ln_e, ln_s = [_ln_outs(pool, p) for p in ps], [_ln_outs(pool, p) for p in ps]
    arch_e, arch_s = [pool.new(r, c) for r, c in shapes], [pool.new(r, c) for r, c in shapes]
    sum_e, sum_s = [pool.new(n) for _, n in sum_cases], [pool.new(n) for _, n in sum_cases]
    lib.backward_epilogue([p.prob(*o) for p, o in zip(ps, ln_e)], b, L, wd, dws, arch_e, n_shards, stride,
                          sums=[(p, o, c) for p, o, (c, _) in zip(pd, sum_e, sum_cases)])
    lib.ln_affine_bwd_multi([p.prob(*o) for p, o in zip(ps, ln_s)], b, L)
    lib.arch_softmax_multi(wd, dws, arch_s, 1, n_shards, stride)
    for p, o, (c, _) in zip(pd, sum_s, sum_cases):
        lib.sum_chunks(p, o, c)
    pool.check()
    cpu_views = _shard_views(shards, shapes)
    for i, p in enumerate(ps):
        _ln_check(f'LN problem {i}', p, ln_e[i], ln_s[i])          # 2e-5: the atomics' order differs
    for t in range(len(shapes)):
        _same(f'arch tensor {t}', arch_e[t], arch_s[t])
        assert_close_scaled(f'arch tensor {t}', arch_e[t], sr.row_softmax_bwd(ws[t], cpu_views[t]))
    for k, (c, _) in enumerate(sum_cases):
        _same(f'sum {k}', sum_e[k], sum_s[k])
        assert_close_scaled(f'sum {k}', sum_e[k], sr.chunk_sum(parts[k], c))
