"""The 1x1-conv GEMM kernels of csrc/conv1x1.hip, instantiation by instantiation, through the C ABI (bmnas.lib) against
the float64 statement in tests/conv_ref.py (pinned by tests/test_conv_ref.py on the CPU).  tests/test_dispatch_gpu.py
runs the reference's production shapes; here are the smallest shapes at which each template instantiation and each
edge path of the four stand-alone entry points (bmnas_conv1x1_fwd, _bwd_data, _bwd_weight, _bwd_all) exists.

How every case is checked
  * every output starts as NaN, every accumulated output (destinations with their accumulate bit, dW, dbias, the
    sharded sums) as a random previous value that the expectation includes;
  * every output is a view into a larger NaN buffer, GUARD floats on each side, that must be bit-unchanged afterwards
    (_Pool.check): an edge tile that stores past its tensor fails here instead of faulting;
  * outputs are compared in full (every n-group's partial, every shard) with gpu_util.assert_close_scaled at the
    bounds of the existing conv kernel tests: U 2e-5, data gradients 3e-5, dW / dbias / anything behind the BatchNorm
    fold 5e-5, partial sums 5e-5, second moments 2e-4.  dbias behind a training-mode BatchNorm is mathematically zero
    and is also bounded in absolute terms (2e-6 b L + 1e-4, as tests/test_reshape_group_gpu.py does);
  * each case names the families (bmnas_conv_family_calls) that must have served it — exactly those, so every other
    family is asserted absent; `forbid` repeats the near miss of a threshold case for the reader.  Only this
    assertion is dropped when BMNAS_CONV_PIPE / BMNAS_FUSE_ATTN_GEMM / BMNAS_FUSE_BWD_PAIR force a family; the values
    are always compared.  Which shard a column block's sums go to depends on the family (conv_ref.shard_sums): the
    expectation takes the block size from the family that actually ran.

ng = ceil(b L / 16) n-groups; b is ragged (the last n-group partly empty) wherever L < 16.  By the dispatch rules of
csrc/conv1x1.hip as written (launch_gemm, launch_ksplit, launch_pipe_fwd, pipe_bwd_serves, bwd_pair_serves):

  A  split-K 1x1, forward + data gradient: b 5, L 8 (ng 3), 48 channels on the other side; K = 16 .. 768 gives
     kpw = ceil(K / 64) = 1, 2, 3, 4, 5, 7, 10, 12 -> conv_ksplit_k<., 1, 1, KPW>, KPW 1, 2, 3, 4, 6, 9, 12, 12: every
     KS_CASE, and all but K = 768 with blocks past the end of K (16: 1 of the four waves' 4, 80: 5 of 8, 144: 9 of 12,
     208: 13 of 16, 272: 17 of 24, 400: 25 of 36, 592: 37 of 48).  Sources / destinations 3 x 48 and 4 x 16; L 4 / b 7
     and L 16 / b 3 at K 144 and 272.  Forward options (bias NULL, part NULL, ldw = K + 12, the fold, stat_shards
     1 / 2 / 5 at ng 3) and data-gradient options
     (ldw = J + 2, the fold, masks 0 / 0b101 / all ones over 3 and 4 destinations, a NULL destination in the middle).
  B  split-K 2x2 (conv_ksplit_k<., 2, 2, KPW>: ceil(ng / 2) ceil(J / 32) >= 1024 on a shape the pipelined kernels
     refuse): forward with two sources, L 4, b 8187 (ng 2047, odd: the last tile's second n-group is clamped), M 16
     (the second column tile lies outside: jcl clamped, `continue` in the store loop), K 2 x 16; forward M 512,
     b 127, L 16 (64 x 16 = 1024 workgroups) with K 2 x 48, 2 x 80, 3 x 112, 2 x 384: kpw 2, 3, 6, 12; data gradient
     J 48 (three 16-wide tiles: odd) at ng 1023 with M 16 (no multiple of 48) and with M 48, ldw = J + 2.  One
     workgroup fewer (ng 2045; ng 126; ng 1021) stays ksplit and runs the 1x1 tiles — the family counter cannot tell
     the two tile shapes apart, the values are what both sides assert.
  C  multi-round split-K (conv_ksplit_multi_k: kpw > 12, one source, no fold, <= 512 workgroups): K 784 (49 blocks:
     the second round holds ONE block, three waves own none) and 1552 (97: the third round holds one), b 3, L 8,
     32 output channels; the data gradient with M 784 into two and three destinations, one accumulating.  K 800 as
     2 x 400 must go to lds.
  D  whole-K LDS tiles (conv_lds_k, the generic fallback): forward K 800 as 2 x 400 — 32x32 at b 5, L 8, M 48 (the
     second n-tile and the second j-tile half outside); the issue's 64x64 shape (ng 400, M 256) would need a 5 M-float
     input, so the thresholds are crossed along M instead, with b ragged at L 4: 32x64 at ng 200, M 256
     (100 x 4 = 400 workgroups; ng 198: 396 -> 32x32), 64x64 at ng 200, M 512 (50 x 8 = 400; ng 196: 392 -> 32x64).
     Data gradient M 800: at a small grid the multi-round kernel takes it, so the fold (which that kernel refuses)
     or more than 512 workgroups (ng 200, J 48) send it to lds; with accumulate masks.  K 80 at ng 191, M 16 (no
     multiple of 32 on a pipelined-size grid) is not pipe_fwd — and, K being short, ksplit rather than lds.
  E  pipelined forward tiles.  conv_pipe_fwd_k<32, 2>: 96 tiles of two n-groups — (ng 191 | 192, M 16: an output
     count below one 96-wide tile) and (ng 95 | 96, M 112: the second tile 16 wide; the issue's ng 191 at M 112
     already gives 96 four-group tiles); the odd ng leave the last tile 1 of 2 n-groups.  K 32, 96, 160 (1, 3, 5
     chunks) and 128, 256 (4, 8: the two-chunks-in-flight loop).  conv_pipe_fwd_k<32, 4>: ng 190, M 112 (48 x 2 tiles,
     the last with 2 of 4 n-groups), K 64, 96, 160, 128.  conv_pipe_fwd_k<48, 4> is UNREACHABLE: with the L + 4 row
     padding conv_pipe_lds<48, 4> is 89088 / 76800 / 70656 bytes at L = 4 / 8 / 16, never <= 65536, so K 96 (a
     multiple of both 48 and 32) runs as <32, 4> at every L, and K 48 and 144 (multiples of 48 only) are refused by
     the pipelined launcher and fall to ksplit — asserted as such.  95 tiles (ng 189, M 16) fall to ksplit.
  F  pipelined data gradient (conv_pipe_bwd_k<48, 2>, >= 96 tiles of 32 columns x 64 channels): M 48 and 144; J 16
     (narrower than the tile, ng 191 / 192); J 80 in one destination (ng 95: the second tile 16 wide, the last
     n-tile half empty); a tile that spans destinations: J 96 as 2 x 48 and J 64 as 4 x 16 (five destinations exceed
     the four pointers of the ABI); accumulate bits, a NULL destination; through bmnas_conv1x1_bwd_all the
     BatchNorm fold in training and in eval.
  G  weight gradient (conv_w_k): (M, K) = (16, 16) (a 32x32 tile half outside both ways), (48, 48), (48, 3 x 16)
     (lanes of one wave read different sources), (80, 2 x 48); ng 1, 7 (fewer groups than the eight waves), 9 (2
     splits of 5 + 4), 17 (3 splits: 6, 6, 5), 191 (24 splits: 8 ... 7); dup_cols = K at ldw 2K and 2K + 4; dbias
     NULL; deterministic mode (one split, plain stores: two calls bit-equal); the BatchNorm fold through
     bmnas_conv1x1_bwd_all with every destination NULL.
  H  one-launch backward (conv_bwd_pair_k<1..4>): M 16, 80, 144, 208, 256 (kpw 1, 2, 3, 4, 4; 80 / 144 / 208 with
     blocks past the end) merge; M 272 (kpw 5) must not — ksplit + conv_w after an in-place bmnas_bn_bwd_apply.  Two
     and three sources, the BatchNorm fold in training, in eval and absent, an accumulate mask; dV bit-unchanged
     wherever the launch folds (merged, pipelined, no data gradient) or there is no BatchNorm.

A finding of these cases: bmnas_conv1x1_bwd_all in eval mode with bn_grad NULL (which its argument check accepts,
tests/test_conv_host_contract.py) returned BMNAS_E_ARG at every shape that neither folding family serves (here
M 272: test_bwd_pair_refuses_kpw_5[eval]), because the in-place bmnas_bn_bwd_apply launch it falls back to refuses a
NULL bn_grad although its eval branch never reads it; the launcher now hands it bn_chan in that place.

Evidence that the tests bite — value-only mutations of csrc/conv1x1.hip (none moves an address or changes a launch
shape), each built into a scratch copy of the library and this file run once against it on an MI355X (264 cases; with
the committed kernels all pass, also under BMNAS_CONV_PIPE=0 and under BMNAS_FUSE_BWD_PAIR=0):
   1. conv_ksplit_body, `av = vb ? t : 0.f` -> `av = t` (a block past the end is no longer zeroed): 115 fail — every
      split-K case in which a wave owns a block past K (A, B, C, the H merges, the cases that fall to ksplit); K 768
      and the 2 x 384 2x2 case (48 blocks fill 4 x 12) and the four-destination M 64 case (4 fill 4 x 1) pass.
   2. the forward fold's second load dropped — conv_ksplit_body: 6 fail (the three fold options of
      test_ksplit_1x1_fwd_options at both K); conv_lds_k: 1 fails (test_lds_fwd_tiles[32x32 fold]).
   3. the multi-round loop skips its last round: 6 fail — all of test_ksplit_multi_round_fwd / _bwd_data.
   4. bn_tile_stats, cnt always 16: 73 fail — every forward case with partials and L < 16 (the ragged last group);
      the L 16 cases pass.
   5. shard index always 0 — bn_tile_stats: 9 fail (shards 2 and 5 of test_ksplit_1x1_fwd_options, the 2x2 case with
      3 shards, the two sharded test_lds_fwd_tiles; shards 1 passes); the pipelined epilogue: 8 fail (the sharded
      cases of test_pipe_fwd_options, both tile forms).
   6. conv_pipe_fwd_body adds the bias of channel lo ^ 1: 59 fail — every pipelined forward case with a bias.
   7. conv_pipe_bwd_body builds the training coefficients in eval: 3 fail — test_bwd_all_pipe_with_bn_fold[eval].
   8. conv_lds_k ignores the accumulate mask: 4 fail — the test_lds_bwd_data cases with a mask.
   9. conv_w_body drops the dup_cols add (atomic and plain): 13 fail — the 12 dup cases of test_conv_w_options and
      the dup case of the deterministic mode.
  10. conv_w_body skips the last group of a split: 72 fail — every weight gradient (G, H, the fold cases of F).
  11. conv_bwd_pair_k ignores bn_train (always eval): 5 fail — test_bwd_pair_merges[train] at every M.
   0. the library of the parent commit: 1 fails — test_bwd_pair_refuses_kpw_5[eval], the finding above.
"""
import functools
import os

import pytest
import torch

import conv_ref as cr
from gpu_util import GUARD, Pool as _Pool, assert_close_scaled, dev

pytestmark = pytest.mark.gpu

# the family expectations describe the DEFAULT dispatch (tests/test_dispatch_gpu.py does the same)
_FORCED = [k for k in ('BMNAS_CONV_PIPE', 'BMNAS_FUSE_ATTN_GEMM', 'BMNAS_FUSE_BWD_PAIR')
           if os.environ.get(k) is not None]
NAN = float('nan')
R_U, R_DATA, R_W, R_SUM, R_M2 = 2e-5, 3e-5, 5e-5, 5e-5, 2e-4


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


def _b(ng, L):
    """the ragged batch of ng n-groups: one sample in the last group (L 16: one sample is a whole group)"""
    return (ng - 1) * (16 // L) + 1


def _served(expect, forbid=()):
    """the families that ran since the last reset; under the default switches: exactly `expect`"""
    from bmnas import lib
    got = {k for k, v in lib.conv_family_calls(reset=True).items() if v > 0}
    if not _FORCED:
        assert got == set(expect), (got, expect)
        assert not (got & set(forbid)), (got, forbid)
    return got


def _pipe_fwd_groups(ng, M):
    """n-groups per pipelined forward tile (pipe_fwd_ngv): the column block of the sharded sums when pipe_fwd serves"""
    gy = (M + 95) // 96
    return 4 if (ng + 3) // 4 * gy >= 96 else 2


# ------------------------------------------------------------------------------------------------------------ forward
@functools.lru_cache(maxsize=4)
def _fwd_problem(b, L, n_src, C_src, M, ldw, fold, seed):
    """CPU inputs and the float64 expectation of one forward problem, shared by the option variants of a shape (and,
    sliced along b and M, by the LDS threshold cases).  Read-only."""
    g = _gen(seed + 7 * b + L + 31 * n_src + C_src + 3 * M + ldw)
    K = n_src * C_src
    srcs = [_rand(g, b, C_src, L) + 0.25 for _ in range(n_src)]
    W = _rand(g, M, ldw) / float(K) ** 0.5
    bias = _rand(g, M) * 2.0 + 1.0
    d = cr.conv_fwd(srcs, W, None, fold)['U']                   # d = U - bias
    return srcs, W, bias, d


def _run_fwd(b, L, n_src, C_src, M, expect, *, forbid=(), bias=True, part=True, ldw_pad=0, fold=False, shards=0,
             of=None):
    """of = (b, M) of a larger cached problem this one is a slice of (first b samples, first M weight rows)."""
    from bmnas import lib
    K = n_src * C_src
    ldw = (2 * K if fold else K) + ldw_pad
    bb, MM = of or (b, M)
    srcs, W, bv, d = _fwd_problem(bb, L, n_src, C_src, MM, ldw, K if fold else 0, 11)
    srcs, W, bv, d = [s[:b].contiguous() for s in srcs], W[:M].contiguous(), bv[:M].contiguous(), d[:b, :M]
    want_U = d + bv.double()[None, :, None] if bias else d
    ng = cr.n_groups(b, L)
    assert lib.conv1x1_num_partials(b, L) == ng
    pool = _Pool()
    U = pool.new(b, M, L)
    g = _gen(5 + b + M)
    prev = _rand(g, max(shards, 1), M, 2)
    out = None
    if shards > 0:
        out = pool.new(shards, M, 2, base=prev[:shards])
    elif part:
        out = pool.new(M, ng, 2)
    lib.conv_family_calls(reset=True)
    lib.conv1x1_fwd([s.to(dev()) for s in srcs], C_src, W.to(dev()), ldw, bv.to(dev()) if bias else None, U, out, b,
                    L, M, K if fold else 0, shards)
    pool.check()
    got = _served(expect, forbid)
    assert_close_scaled('U', U, want_U, rel=R_U)
    if shards > 0:
        per_block = _pipe_fwd_groups(ng, M) if 'pipe_fwd' in got else 1
        want = cr.shard_sums(d, shards, per_block) + prev[:shards].double()
        assert_close_scaled('stat: sum d', out[:, :, 0], want[:, :, 0], rel=R_SUM)
        assert_close_scaled('stat: sum d^2', out[:, :, 1], want[:, :, 1], rel=R_M2)
        assert_close_scaled('stat: all shards', out.double().sum(0).cpu(), want.sum(0), rel=R_M2)
    elif part:
        want = cr.group_partials(want_U)
        assert_close_scaled('part: sum', out[:, :, 0], want[:, :, 0], rel=R_SUM)
        assert_close_scaled('part: m2', out[:, :, 1], want[:, :, 1], rel=R_M2)


KS_K = [16, 80, 144, 208, 272, 400, 592, 768]


@pytest.mark.parametrize('K', KS_K)
def test_ksplit_1x1_fwd_every_register_variant(K):
    """A: conv_ksplit_k<true, 1, 1, 1 | 2 | 3 | 4 | 6 | 9 | 12 | 12>, a half-full last n-group"""
    _run_fwd(5, 8, 1, K, 48, {'ksplit'})


@pytest.mark.parametrize('b,L,n_src,C_src', [(5, 8, 3, 48), (5, 8, 4, 16), (7, 4, 1, 144), (7, 4, 1, 272),
                                             (3, 16, 1, 144), (3, 16, 1, 272)])
def test_ksplit_1x1_fwd_sources_and_lengths(b, L, n_src, C_src):
    """A: blocks of one wave in different sources (3 x 48: a wave's 3 blocks = one source each; 4 x 16: one block
    per wave); L 4 (12 of 16 columns in the last group) and L 16 (no padding) at KPW 3 and 6"""
    _run_fwd(b, L, n_src, C_src, 48, {'ksplit'})


FWD_OPTS = {
    'bias NULL': dict(bias=False), 'part NULL': dict(part=False), 'ldw K+12': dict(ldw_pad=12), 'fold': dict(fold=True),
    'shards 1': dict(shards=1), 'shards 2': dict(shards=2), 'shards 5': dict(shards=5),
    'fold, ldw 2K+12, bias NULL, shards 2': dict(fold=True, ldw_pad=12, bias=False, shards=2),
    'fold, ldw 2K+12, bias NULL, part': dict(fold=True, ldw_pad=12, bias=False),
}


@pytest.mark.parametrize('K', [144, 272])
@pytest.mark.parametrize('opt', list(FWD_OPTS))
def test_ksplit_1x1_fwd_options(opt, K):
    """A: the forward options at KPW 3 and 6 (blocks past the end), each alone and together; 5 shards at ng 3 leaves
    two shards with their previous value, 2 shards puts groups 0 and 2 into shard 0"""
    _run_fwd(5, 8, 1, K, 48, {'ksplit'}, **FWD_OPTS[opt])


@pytest.mark.parametrize('b,L,n_src,C_src,M,shards', [
    (8187, 4, 2, 16, 16, 0), (8179, 4, 2, 16, 16, 0),                   # 1024 | 1023 workgroups of 2x2
    (127, 16, 2, 48, 512, 0), (127, 16, 2, 80, 512, 3), (127, 16, 3, 112, 512, 0), (127, 16, 2, 384, 512, 0),
    (126, 16, 2, 80, 512, 0)])                                          # 63 x 16 = 1008: the 1x1 tiles
def test_ksplit_2x2_fwd(b, L, n_src, C_src, M, shards):
    """B: conv_ksplit_k<true, 2, 2, 1 | 2 | 3 | 6 | 12> and the 1x1 tiles one workgroup below the threshold"""
    _run_fwd(b, L, n_src, C_src, M, {'ksplit'}, forbid={'pipe_fwd', 'lds'}, shards=shards)


@pytest.mark.parametrize('K,M', [(784, 32), (1552, 32)])
def test_ksplit_multi_round_fwd(K, M):
    """C: conv_ksplit_multi_k<true>, a last round with a single valid block"""
    _run_fwd(3, 8, 1, K, M, {'ksplit'}, forbid={'lds'})


LDS_BIG = (798, 512)                                                 # the cached problem the threshold cases slice


@pytest.mark.parametrize('b,L,M,of,opts', [
    (5, 8, 48, None, {}),                                              # 32x32, half outside; K 800 must not be multi
    (5, 8, 48, None, dict(shards=2, bias=False)),
    (5, 8, 48, None, dict(fold=True)),                                 # (fold_cols = 800, ldw = 1600)
    (798, 4, 256, LDS_BIG, dict(shards=3)),                            # 100 x 4 = 400 of 32x64
    (790, 4, 256, LDS_BIG, {}),                                        # 99 x 4 = 396 -> 32x32
    (798, 4, 512, LDS_BIG, {}),                                        # 50 x 8 = 400 of 64x64
    (782, 4, 512, LDS_BIG, {})],                                       # 49 x 8 = 392 -> 32x64
    ids=['32x32', '32x32 shards', '32x32 fold', '32x64 at 400', '32x32 at 396', '64x64 at 400', '32x64 at 392'])
def test_lds_fwd_tiles(b, L, M, of, opts):
    """D: conv_lds_k<true, 32, 32 | 32, 64 | 64, 64>, K = 2 x 400 (two sources: neither pipelined nor multi-round;
    kpw 13: no register variant)"""
    _run_fwd(b, L, 2, 400, M, {'lds'}, forbid={'ksplit', 'pipe_fwd'}, of=of, **opts)


def test_short_k_no_multiple_of_32_on_a_pipelined_grid():
    """D: K 80 at ng 191, M 16: the pipelined two-group tiles need K % 32 == 0"""
    _run_fwd(_b(191, 4), 4, 1, 80, 16, {'ksplit'}, forbid={'pipe_fwd'})


PIPE2 = [(191, 16), (192, 16), (95, 112), (96, 112)]
PIPE2_CASES = [(ng, M, K, L) for ng, M in PIPE2 for K in (32, 96, 160) for L in (4, 8, 16)]
PIPE2_CASES += [(191, 16, 128, 8), (95, 112, 256, 4), (96, 112, 128, 16)]       # even chunk counts >= 4


@pytest.mark.parametrize('ng,M,K,L', PIPE2_CASES)
def test_pipe_fwd_two_group_tiles(ng, M, K, L):
    """E: conv_pipe_fwd_k<32, 2> at exactly 96 tiles"""
    _run_fwd(_b(ng, L), L, 1, K, M, {'pipe_fwd'}, forbid={'ksplit'})


@pytest.mark.parametrize('L', [4, 8, 16])
@pytest.mark.parametrize('K', [64, 96, 160, 128])
def test_pipe_fwd_four_group_tiles(K, L):
    """E: conv_pipe_fwd_k<32, 4> (ng 190, M 112: 48 x 2 tiles); K 96 would fit <48, 4> by its channel count, but that
    form's LDS size exceeds 64 KB at every L, so the rule gives <32, 4>"""
    _run_fwd(_b(190, L), L, 1, K, 112, {'pipe_fwd'}, forbid={'ksplit'})


@pytest.mark.parametrize('L', [4, 8, 16])
@pytest.mark.parametrize('K', [48, 144])
def test_pipe_fwd_48_channel_chunks_are_refused(K, L):
    """E: K % 48 == 0 but K % 32 != 0 on the four-group grid: <48, 4> never fits its LDS, <32, 4> does not divide K —
    the launcher refuses and the split-K 1x1 tiles serve (95 x 4 = 380 < 1024 workgroups of 2x2)"""
    _run_fwd(_b(190, L), L, 1, K, 112, {'ksplit'}, forbid={'pipe_fwd', 'lds'})


PIPE_OPTS = {'bias NULL': dict(bias=False), 'part NULL': dict(part=False), 'shards 3': dict(shards=3),
             'shards 3, bias NULL': dict(shards=3, bias=False)}


@pytest.mark.parametrize('ng,M,K,L', [(191, 16, 96, 4), (95, 112, 128, 8), (190, 112, 64, 4), (190, 112, 128, 16)])
@pytest.mark.parametrize('opt', list(PIPE_OPTS))
def test_pipe_fwd_options(opt, ng, M, K, L):
    """E: bias, partials and sharded sums (one atomic pair per channel per TILE: shard = tile % 3) on both tile forms"""
    _run_fwd(_b(ng, L), L, 1, K, M, {'pipe_fwd'}, **PIPE_OPTS[opt])


@pytest.mark.parametrize('ng', [189, 190])
def test_pipe_fwd_95_tiles_fall_to_ksplit(ng):
    _run_fwd(_b(ng, 4), 4, 1, 32, 16, {'ksplit'}, forbid={'pipe_fwd'})


# ------------------------------------------------------------------------------------------------------ data gradient
def _run_bwd_data(b, L, M, n_dst, C_src, expect, *, forbid=(), ldw_pad=0, fold=False, mask=0, null=None):
    from bmnas import lib
    J = n_dst * C_src
    ldw = (2 * J if fold else J) + ldw_pad
    g = _gen(23 + 7 * b + L + 3 * M + 31 * n_dst + C_src + ldw)
    dU = _rand(g, b, M, L)
    W = _rand(g, M, ldw) / float(M) ** 0.5
    prevs = [None if q == null else _rand(g, b, C_src, L) for q in range(n_dst)]
    want = cr.conv_bwd_data(dU, W, J if fold else 0, C_src, prevs, mask)
    pool = _Pool()
    dsts = [None if p is None else pool.new(b, C_src, L, base=p if (mask >> q) & 1 else None)
            for q, p in enumerate(prevs)]
    lib.conv_family_calls(reset=True)
    lib.conv1x1_bwd_data(dU.to(dev()), W.to(dev()), ldw, dsts, C_src, mask, b, L, M, J if fold else 0)
    pool.check()
    _served(expect, forbid)
    for q in range(n_dst):
        if dsts[q] is not None:
            assert_close_scaled(f'dsrc{q}', dsts[q], want[q], rel=R_DATA)


@pytest.mark.parametrize('M', KS_K)
def test_ksplit_1x1_bwd_data_every_register_variant(M):
    """A: conv_ksplit_k<false, 1, 1, KPW>, one destination of 48 channels"""
    _run_bwd_data(5, 8, M, 1, 48, {'ksplit'})


@pytest.mark.parametrize('b,L,M,n_dst,C_src', [(7, 4, 144, 1, 48), (7, 4, 272, 1, 48), (3, 16, 144, 1, 48),
                                               (3, 16, 272, 1, 48), (5, 8, 144, 3, 48), (5, 8, 64, 4, 16)])
def test_ksplit_1x1_bwd_data_destinations_and_lengths(b, L, M, n_dst, C_src):
    """A: L 4 and L 16 at KPW 3 and 6; three destinations of 48 and four of 16 channels (a tile per destination)"""
    _run_bwd_data(b, L, M, n_dst, C_src, {'ksplit'})


BWD_OPTS = {
    'ldw J+2': dict(n_dst=1, C_src=48, ldw_pad=2), 'fold': dict(n_dst=1, C_src=48, fold=True),
    'fold, ldw 2J+2': dict(n_dst=1, C_src=48, fold=True, ldw_pad=2, mask=1),
    '3 dst, mask 0': dict(n_dst=3, C_src=16, mask=0), '3 dst, mask 101': dict(n_dst=3, C_src=16, mask=0b101),
    '3 dst, mask 111': dict(n_dst=3, C_src=16, mask=0b111), '4 dst, mask 0': dict(n_dst=4, C_src=16, mask=0),
    '4 dst, mask 0101': dict(n_dst=4, C_src=16, mask=0b0101), '4 dst, mask 1111': dict(n_dst=4, C_src=16, mask=0b1111),
    '3 dst, middle NULL': dict(n_dst=3, C_src=16, mask=0b100, null=1),
    '4 dst, NULL, ldw J+2': dict(n_dst=4, C_src=16, mask=0b1010, null=2, ldw_pad=2),
}


@pytest.mark.parametrize('b,L,M', [(5, 8, 144), (7, 4, 272), (3, 16, 144)])
@pytest.mark.parametrize('opt', list(BWD_OPTS))
def test_ksplit_1x1_bwd_data_options(opt, b, L, M):
    """A: the data-gradient options at KPW 3 and 6, the three row lengths"""
    _run_bwd_data(b, L, M, expect={'ksplit'}, **BWD_OPTS[opt])


@pytest.mark.parametrize('ng,M,ldw_pad,mask', [(1023, 16, 0, 0), (1023, 48, 2, 0b010), (1021, 16, 0, 0b001)])
def test_ksplit_2x2_bwd_data(ng, M, ldw_pad, mask):
    """B: conv_ksplit_k<false, 2, 2, 1>, J = 3 x 16 (the second column tile half outside), ng odd; ng 1021: 1022
    workgroups, the 1x1 tiles"""
    _run_bwd_data(_b(ng, 4), 4, M, 3, 16, {'ksplit'}, forbid={'pipe_bwd'}, ldw_pad=ldw_pad, mask=mask)


@pytest.mark.parametrize('M,n_dst,mask,null', [(784, 2, 0b10, None), (784, 3, 0b001, None), (784, 3, 0b100, 1),
                                               (1552, 2, 0b01, None)])
def test_ksplit_multi_round_bwd_data(M, n_dst, mask, null):
    """C: conv_ksplit_multi_k<false>: the source index is fixed to 0, the destination still picked per tile"""
    _run_bwd_data(3, 8, M, n_dst, 16, {'ksplit'}, forbid={'lds'}, mask=mask, null=null)


@pytest.mark.parametrize('b,L,n_dst,C_src,opts', [
    (5, 8, 1, 48, dict(fold=True)), (5, 8, 1, 48, dict(fold=True, mask=1)),
    (5, 8, 3, 16, dict(fold=True, mask=0b101)), (5, 8, 3, 16, dict(fold=True, mask=0b010, null=0)),
    (798, 4, 3, 16, dict(mask=0b110))], ids=['fold', 'fold acc', 'fold 3 dst', 'fold NULL', 'ng 200'])
def test_lds_bwd_data(b, L, n_dst, C_src, opts):
    """D: conv_lds_k<false, 32, 32>, M 800: the fold at a small grid, 600 workgroups without it"""
    _run_bwd_data(b, L, 800, n_dst, C_src, {'lds'}, forbid={'ksplit'}, **opts)


@pytest.mark.parametrize('ng,L,M,n_dst,C_src,mask,null', [
    (191, 4, 48, 1, 16, 0, None), (192, 8, 144, 1, 16, 1, None), (95, 4, 144, 1, 80, 0, None),
    (96, 16, 48, 1, 80, 1, None), (95, 8, 48, 2, 48, 0b10, None), (96, 4, 144, 2, 48, 0b01, 1),
    (191, 4, 144, 4, 16, 0b0110, None), (192, 16, 48, 4, 16, 0b1001, 2)])
def test_pipe_bwd_data(ng, L, M, n_dst, C_src, mask, null):
    """F: conv_pipe_bwd_k<48, 2> at exactly 96 tiles"""
    _run_bwd_data(_b(ng, L), L, M, n_dst, C_src, {'pipe_bwd'}, forbid={'ksplit'}, mask=mask, null=null)


def test_pipe_bwd_data_95_tiles_fall_to_ksplit():
    _run_bwd_data(_b(190, 4), 4, 48, 1, 16, {'ksplit'}, forbid={'pipe_bwd'})


# ---------------------------------------------------------------------------------------------------- weight gradient
def _w_problem(b, L, M, n_src, C_src, ldw, seed):
    g = _gen(seed + 7 * b + L + 3 * M + 31 * n_src + C_src + ldw)
    dU = _rand(g, b, M, L)
    srcs = [_rand(g, b, C_src, L) + 0.25 for _ in range(n_src)]
    return dU, srcs, _rand(g, M, ldw), _rand(g, M)


def _run_bwd_weight(b, L, M, n_src, C_src, *, dup=False, ldw_pad=0, dbias=True, twice=False):
    from bmnas import lib
    K = n_src * C_src
    ldw = (2 * K if dup else K) + ldw_pad
    dU, srcs, pW, pb = _w_problem(b, L, M, n_src, C_src, ldw, 41)
    want_W, want_b = cr.conv_bwd_weight(dU, srcs, pW, pb if dbias else None, K if dup else 0)
    dUd, sd = dU.to(dev()), [s.to(dev()) for s in srcs]
    runs = []
    for _ in range(2 if twice else 1):
        pool = _Pool()
        dW, db = pool.new(M, ldw, base=pW), (pool.new(M, base=pb) if dbias else None)
        lib.conv_family_calls(reset=True)
        lib.conv1x1_bwd_weight(dUd, sd, C_src, dW, ldw, db, K if dup else 0, b, L, M)
        pool.check()
        _served({'conv_w'})
        assert_close_scaled('dW', dW, want_W, rel=R_W)
        named = 2 * K if dup else K
        assert torch.equal(dW[:, named:].cpu(), pW[:, named:]), 'columns the call does not name were written'
        if dbias:
            assert_close_scaled('dbias', db, want_b, rel=R_W)
        runs.append((dW.cpu(), None if db is None else db.cpu()))
    return runs


W_SHAPES = [(16, 1, 16), (48, 1, 48), (48, 3, 16), (80, 2, 48)]


@pytest.mark.parametrize('ng', [1, 7, 9, 17, 191])
@pytest.mark.parametrize('i', range(len(W_SHAPES)))
def test_conv_w_tiles_and_splits(i, ng):
    """G: conv_w_k, dW and dbias accumulated into random values"""
    M, n_src, C_src = W_SHAPES[i]
    L = (4, 8, 16)[(i + ng) % 3]
    _run_bwd_weight(_b(ng, L), L, M, n_src, C_src)


@pytest.mark.parametrize('ng,L', [(7, 8), (17, 4)])
@pytest.mark.parametrize('opts', [dict(dup=True), dict(dup=True, ldw_pad=4), dict(dbias=False),
                                  dict(dup=True, ldw_pad=4, dbias=False)],
                         ids=['dup', 'dup ldw 2K+4', 'dbias NULL', 'dup ldw 2K+4 dbias NULL'])
@pytest.mark.parametrize('M,n_src,C_src', [(48, 1, 48), (16, 1, 16)])
def test_conv_w_options(M, n_src, C_src, opts, ng, L):
    """G: dup_cols = K (plain stores at ng 7, atomics over 3 splits at ng 17), dbias NULL"""
    _run_bwd_weight(_b(ng, L), L, M, n_src, C_src, **opts)


@pytest.mark.parametrize('ng,L,M,n_src,C_src,dup', [(17, 4, 48, 3, 16, False), (191, 8, 80, 2, 48, False),
                                                   (17, 8, 16, 1, 16, True)])
def test_conv_w_deterministic_mode(ng, L, M, n_src, C_src, dup):
    """G: one split, plain stores: two calls give the same bits, within the same bound of the reference"""
    from bmnas import lib
    lib.set_deterministic(True)
    try:
        (W1, b1), (W2, b2) = _run_bwd_weight(_b(ng, L), L, M, n_src, C_src, dup=dup, twice=True)
    finally:
        lib.set_deterministic(False)
    assert torch.equal(W1, W2) and torch.equal(b1, b2)


# ------------------------------------------------------------------------------------------- bmnas_conv1x1_bwd_all
def _run_bwd_all(b, L, M, n_src, C_src, bn, expect, *, forbid=(), mask=0, null=(), untouched=True):
    """bn: None (no BatchNorm in the call), 'train', 'eval'.  null: the NULL destinations."""
    from bmnas import lib
    K = n_src * C_src
    g = _gen(61 + 7 * b + L + 3 * M + 31 * n_src + C_src)
    dV, U = _rand(g, b, M, L), _rand(g, b, M, L) * 1.5 + 0.3
    W = _rand(g, M, K) / float(M) ** 0.5
    bn_w = _rand(g, M) * 0.3 + 1.0
    srcs = [_rand(g, b, C_src, L) + 0.25 for _ in range(n_src)]
    prevs = [None if q in null else _rand(g, b, C_src, L) for q in range(n_src)]
    pW, pb = _rand(g, M, K), _rand(g, M)
    fold = None
    if bn == 'train':
        dU, chan, bn_grad = cr.bn_input_grad(dV, U, bn_w)
        fold = (U.to(dev()), chan.float().to(dev()), bn_grad.float().to(dev()), 1)
    elif bn == 'eval':
        chan = cr.bn_eval_chan(bn_w, _rand(g, M), _rand(g, M) * 0.2, _rand(g, M).abs() + 0.5).float()
        dU = cr.bn_eval_input_grad(dV, chan[2 * M:3 * M])           # (the fp32 scale the kernel reads)
        fold = (U.to(dev()), chan.to(dev()), None, 0)
    else:
        dU = dV.double()
    want_d = cr.conv_bwd_data(dU, W, 0, C_src, prevs, mask)
    want_W, want_b = cr.conv_bwd_weight(dU, srcs, pW, pb)
    pool = _Pool()
    dsts = [None if p is None else pool.new(b, C_src, L, base=p if (mask >> q) & 1 else None)
            for q, p in enumerate(prevs)]
    dW, db = pool.new(M, K, base=pW), pool.new(M, base=pb)
    dVd = pool.new(b, M, L, base=dV)
    lib.conv_family_calls(reset=True)
    lib.conv1x1_bwd_all(dVd, W.to(dev()), K, dsts, C_src, mask, b, L, M, 0, [s.to(dev()) for s in srcs], dW, K, db, 0,
                        fold)
    pool.check()
    _served(expect, forbid)
    for q in range(n_src):
        if dsts[q] is not None:
            assert_close_scaled(f'dsrc{q}', dsts[q], want_d[q], rel=R_W if bn else R_DATA)
    assert_close_scaled('dW', dW, want_W, rel=R_W)
    assert_close_scaled('dbias', db, want_b, rel=R_W)
    if bn == 'train':                                               # mathematically zero: absolute
        assert float((db.cpu().double() - pb.double()).abs().max()) < 2e-6 * b * L + 1e-4
    if untouched:
        assert torch.equal(dVd.cpu(), dV), 'dV was written'
    else:
        assert_close_scaled('dU in place', dVd, dU, rel=R_W)


@pytest.mark.parametrize('bn', [None, 'train', 'eval'])
@pytest.mark.parametrize('M,n_src,C_src,mask', [(16, 2, 16, 0), (80, 3, 16, 0b101), (144, 2, 48, 0b10),
                                                (208, 3, 16, 0), (256, 2, 16, 0b01)])
def test_bwd_pair_merges(M, n_src, C_src, mask, bn):
    """H: conv_bwd_pair_k<1 | 2 | 3 | 4 | 4>: one launch, dV left alone"""
    _run_bwd_all(5, 8, M, n_src, C_src, bn, {'bwd_pair'}, forbid={'ksplit', 'conv_w'}, mask=mask)


@pytest.mark.parametrize('bn', [None, 'train', 'eval'])
def test_bwd_pair_refuses_kpw_5(bn):
    """H: M 272: bmnas_bn_bwd_apply in place, then conv_ksplit_k<false, 1, 1, 6> and conv_w_k"""
    _run_bwd_all(5, 8, 272, 2, 16, bn, {'ksplit', 'conv_w'}, forbid={'bwd_pair'}, mask=0b10, untouched=bn is None)


@pytest.mark.parametrize('bn', ['train', 'eval'])
@pytest.mark.parametrize('ng,L,M,n_src,C_src,mask,null', [(191, 4, 48, 1, 16, 1, ()), (95, 8, 144, 2, 48, 0b01, (1,)),
                                                         (96, 16, 144, 1, 80, 0, ())])
def test_bwd_all_pipe_with_bn_fold(ng, L, M, n_src, C_src, mask, null, bn):
    """F: conv_pipe_bwd_k<48, 2> with FOLD and conv_w_k with FOLD, two launches, dV left alone"""
    _run_bwd_all(_b(ng, L), L, M, n_src, C_src, bn, {'pipe_bwd', 'conv_w'}, forbid={'bwd_pair', 'ksplit'}, mask=mask,
                 null=null)


@pytest.mark.parametrize('bn', [None, 'train', 'eval'])
@pytest.mark.parametrize('ng,L,M,n_src,C_src', [(7, 8, 48, 3, 16), (17, 4, 80, 2, 48), (9, 16, 16, 1, 16)])
def test_bwd_all_without_data_gradient(ng, L, M, n_src, C_src, bn):
    """G: every destination NULL: conv_w_k alone, with the BatchNorm fold, dV left alone"""
    _run_bwd_all(_b(ng, L), L, M, n_src, C_src, bn, {'conv_w'}, forbid={'bwd_pair', 'ksplit'},
                 null=tuple(range(n_src)))
