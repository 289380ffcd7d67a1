"""Same bits from two builds of the library: every kernel that holds the per-sample LayerNorm arithmetic, on cuda:0.

    python tools/ln_ab.py LIB_A LIB_B            (e.g. a tools/build_variant.sh build of the parent commit and
                                                  bm-nas_amd/bmnas/libbmnas_hip.so)

Each library is loaded through BMNAS_LIB in a fresh child process of its own, which runs on the same seeded inputs
  cat_ln_fwd / _bwd                     relu 0 / 1, with / without resid, out_sums, n_src 1 / 3 / 2 / 4
  node_mix_ln_fwd / _bwd                with / without out_sums
  bn_relu_ln_fwd / _bwd                 plain, and with the pair rider at n_prev 1 / 3
  node_mix_pre_fwd + node_mix_lnp_bwd
  sdpa_ln_fwd / _bwd
  head_fwd / head_bwd                   mode 0
once with dropout off and, where the wrapper takes a dropout site, once with dropout on, and saves every output.  The
shapes are the smallest that reach each instantiation the launchers pick (wide = b <= 256 and d4 >= 512, VPT =
ceil(d4 / BS), d4 = n_src C L / 4), always with a ragged last trip; a kernel takes the rows its launcher accepts.

The parent process (which never touches the GPU) compares byte for byte
  * every output that no atomic writes, at every shape;
  * outputs accumulated with atomics (bn_grad, dgamma, the rider's dw / dw2, dln_w / dln_b of cat_ln_bwd, the head's
    hb) only where each address receives a single add onto zero: batch 1 (dgamma over one shard per workgroup; hb where
    the head runs a single k-slice).  At larger batches the order of the adds is not fixed: the float64 suites check those.
Exit status 1 if a tensor differs (its largest difference is printed), 0 otherwise.  No GPU: the children fail.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'bm-nas_amd'))
import torch

SENTINEL = -7777.0
DROP_SEED = 0x5EED0123456789
ATOMIC = ('bn_grad', 'dgamma', 'dw', 'dw2', 'dln_w', 'dln_b', 'hb')

# (b, C, L, n_src): the rows of the shape table; cat_ln takes all of them
CAT_ROWS = [(3, 12, 4, 1), (5, 85, 4, 3), (5, 80, 16, 1), (3, 128, 16, 1), (5, 192, 16, 1), (3, 272, 16, 1),
            (5, 510, 16, 1), (3, 510, 16, 2), (3, 510, 16, 4), (257, 144, 16, 1)]
# single-source kernels with C % 4 == 0 (bn_fin_fill): 508 / 1020 stand in for 510 / 2 x 510 (VPT 4 and 8 at 512 threads)
ONE_ROWS = [(3, 12, 4), (5, 80, 16), (3, 128, 16), (5, 192, 16), (3, 272, 16), (5, 508, 16), (3, 1020, 16),
            (257, 144, 16)]
PAIR_ROWS = [(3, 12, 4, 1), (5, 60, 16, 3), (3, 60, 16, 1), (5, 12, 4, 3)]         # C L / 4 <= 256, b <= 128
LAZY_ROWS = [(3, 12, 4), (5, 80, 16), (3, 192, 16), (5, 252, 16)]                  # C L / 4 <= 1024
SDPA_ROWS = [(3, 16, 4), (5, 80, 8), (2, 272, 16), (3, 192, 16)]
HEAD_ROWS = [(1, 4, 16, 1, 3), (5, 8, 16, 3, 17), (3, 192, 16, 2, 23), (17, 20, 8, 4, 33)]   # (b, C, L, n_src, O)


def with_b1(rows):
    """every row also at batch 1 (where the atomic outputs are comparable), except the b > 256 rows"""
    out = []
    for r in rows:
        out.append(r)
        if 1 < r[0] <= 256:
            out.append((1,) + tuple(r[1:]))
    return list(dict.fromkeys(out))


def child(path):
    from bmnas import lib
    assert torch.cuda.is_available(), 'tools/ln_ab.py compares runs on the GPU: no device, no result'
    dev = torch.device('cuda:0')
    res = {}

    def gen(*key):
        return torch.Generator().manual_seed(hash(key) & 0x7FFFFFFF)

    def R(g, *shape, scale=1.0, shift=0.0):
        return torch.rand(*shape, generator=g).mul(2).sub(1).mul(scale).add(shift).to(dev)

    def out(*shape):
        return torch.full(shape, SENTINEL, device=dev)

    def zeros(*shape):
        return torch.zeros(*shape, device=dev)

    def chan_of(g, M):
        return torch.cat([R(g, M, scale=0.2), R(g, M, scale=0.3, shift=1.0), R(g, M, scale=0.3, shift=1.0),
                          R(g, M, scale=0.2)]).contiguous()

    def stats_of(g, b):
        return torch.stack([R(g, b, scale=0.1), R(g, b, scale=0.3, shift=1.0)], dim=1).contiguous()

    def drops(on, n):
        if not on:
            return lib.NO_DROP, lib.NO_DROP
        return lib.make_dropout(0.1, DROP_SEED, 3 << 33), lib.make_dropout(0.2, DROP_SEED, (3 << 33) + n // 4)

    # ---- cat_ln (no dropout site)
    for b, C, L, n_src in with_b1(CAT_ROWS):
        for relu in (0, 1):
            for has_r in ((False, True) if n_src == 1 else (False,)):
                g = gen(1, b, C, L, n_src, relu, has_r)
                srcs = [R(g, b, C, L) for _ in range(n_src)]
                resid = R(g, b, C, L) if has_r else None
                ln_w, ln_b = R(g, n_src * C, L, scale=0.3, shift=1.0), R(g, n_src * C, L, scale=0.2)
                o, st, osum = out(b, n_src * C, L), out(b, 2), out(b, 2)
                lib.cat_ln_fwd(srcs, resid, ln_w, ln_b, o, st, b, C, L, relu, out_sums=osum)
                gy = R(g, b, n_src * C, L)
                dsrcs = [out(b, C, L) for _ in range(n_src)]
                dres = out(b, C, L) if has_r else None
                dln_w, dln_b = zeros(n_src * C, L), zeros(n_src * C, L)
                scrub = torch.ones(64, device=dev)
                lib.cat_ln_bwd(gy, srcs, resid, ln_w, ln_b, st, dsrcs, dres, 0, dln_w, dln_b, b, C, L, relu, scrub)
                r = {'out': o, 'stats': st, 'out_sums': osum, 'scrub': scrub, 'dln_w': dln_w, 'dln_b': dln_b}
                r.update({f'dsrc{q}': t for q, t in enumerate(dsrcs)})
                if has_r:
                    r['dresid'] = dres
                res[f'cat_ln b{b} C{C} L{L} n{n_src} relu{relu} resid{int(has_r)}'] = r

    for drop_on in (False, True):
        tag = f'drop{int(drop_on)}'
        # ---- node_mix_ln
        for b, C, L in with_b1(ONE_ROWS):
            for sums in (False, True):
                g = gen(2, b, C, L, sums)
                x, y, p1, resid = (R(g, b, C, L) for _ in range(4))
                U, chan = R(g, b, 3 * C, L), chan_of(g, 3 * C)
                gamma = torch.softmax(R(g, 4), 0).contiguous()
                ln_w, ln_b = R(g, C, L, scale=0.3, shift=1.0), R(g, C, L, scale=0.2)
                dglu, dfc = drops(drop_on, b * C * L)
                pre, o, st = out(b, C, L), out(b, C, L), out(b, 2)
                osum = out(b, 2) if sums else None
                lib.node_mix_ln_fwd(x, y, p1, U, chan, gamma, resid, ln_w, ln_b, pre, o, st, b, C, L, dglu, dfc,
                                    out_sums=osum)
                r = {'pre': pre, 'out': o, 'stats': st}
                if sums:
                    r['out_sums'] = osum
                if lib.node_mix_ln_bwd_ok(b, C, L):
                    gy = R(g, b, C, L)
                    gin, dres, dx, dy, dV = out(b, C, L), out(b, C, L), out(b, C, L), out(b, C, L), out(b, 3 * C, L)
                    dgam, bn_grad = zeros(2 * 4), zeros(6 * C)
                    lib.node_mix_ln_bwd(gy, pre, ln_w, st, gin, dres, 0, x, y, p1, U, chan, gamma, dgam, dx, dy, 0, dV,
                                        bn_grad, b, C, L, dglu, dfc, 2, 4)
                    r.update(g_in=gin, dresid=dres, dx=dx, dy=dy, dV=dV, dgamma=dgam, bn_grad=bn_grad)
                res[f'node_mix_ln b{b} C{C} L{L} sums{int(sums)} {tag}'] = r
        # ---- bn_relu_ln, plain (n_prev 0) and with the pair rider
        for b, C, L, n_prev in with_b1([r + (0,) for r in ONE_ROWS] + PAIR_ROWS):
            g = gen(3, b, C, L, n_prev)
            U, x, chan = R(g, b, C, L), R(g, b, C, L), chan_of(g, C)
            ln_w, ln_b = R(g, C, L, scale=0.3, shift=1.0), R(g, C, L, scale=0.2)
            drop = drops(drop_on, b * C * L)[0]
            o, y, st, osum = out(b, C, L), out(b, C, L), out(b, 2), out(b, 2)
            gy, dV, bn_grad, dres = R(g, b, C, L), out(b, C, L), zeros(2 * C), out(b, C, L)
            r = {'o': o, 'out': y, 'stats': st, 'out_sums': osum, 'dV': dV, 'bn_grad': bn_grad, 'dresid': dres}
            if n_prev == 0:
                lib.bn_relu_ln_fwd(U, chan, x, ln_w, ln_b, o, y, st, b, C, L, drop, lib.NO_FIN, osum)
                lib.bn_relu_ln_bwd(gy, o, x, ln_w, st, U, chan, dV, bn_grad, dres, 0, b, C, L, drop)
            else:
                assert lib.bn_relu_ln_fwd_pair_ok(b, C, L, n_prev)
                prev = [R(g, b, C, L) for _ in range(n_prev)]
                w = torch.softmax(R(g, n_prev + 1, 2), -1).contiguous()
                w2 = torch.softmax(R(g, 3, 2), -1).contiguous()
                h, z = out(b, C, L), out(b, C, L)
                lib.bn_relu_ln_fwd(U, chan, x, ln_w, ln_b, o, y, st, b, C, L, drop, lib.NO_FIN, osum,
                                   (prev, w[:, 1], 2, w2[:, 1], 2, h, z))
                gh, gz, gz2 = R(g, b, C, L), R(g, b, C, L), R(g, b, C, L)
                dxs = [out(b, C, L) for _ in range(n_prev)]
                dw, dw2, gfull = zeros(64), zeros(64), out(b, C, L)
                lib.bn_relu_ln_bwd(gy, o, x, ln_w, st, U, chan, dV, bn_grad, dres, 0, b, C, L, drop,
                                   (prev, dxs, 0, y, w[:, 1], 2, w2[:, 1], 2, h, gh, gz, gz2, dw, dw2, 1, 64, gfull))
                r.update(h=h, z=z, dw=dw, dw2=dw2, g_full=gfull)
                r.update({f'dxs{j}': t for j, t in enumerate(dxs)})
            res[f'bn_relu_ln b{b} C{C} L{L} prev{n_prev} {tag}'] = r
        # ---- node_mix_pre_fwd + node_mix_lnp_bwd
        for b, C, L in with_b1(LAZY_ROWS):
            g = gen(4, b, C, L)
            assert lib.lazy_ln_ok(C, L)
            P = lib.lazy_ln_parts(C, L)
            x, y, p1, resid = (R(g, b, C, L) for _ in range(4))
            U, chan = R(g, b, 3 * C, L), chan_of(g, 3 * C)
            gamma = torch.softmax(R(g, 4), 0).contiguous()
            ln_w, ln_b = R(g, C, L, scale=0.3, shift=1.0), R(g, C, L, scale=0.2)
            dglu, dfc = drops(drop_on, b * C * L)
            pre, rec, prm = out(b, C, L), out(b, P, 8), out(P, 8)
            lib.node_mix_pre_fwd(x, y, p1, U, chan, gamma, resid, ln_w, ln_b, pre, rec, prm, b, C, L, dglu, dfc)
            gy, st = R(g, b, C, L), stats_of(g, b)
            lnp0 = R(g, b, max(1, C * L // 64), 2)
            gin, dres, dx, dy, dV = out(b, C, L), out(b, C, L), out(b, C, L), out(b, C, L), out(b, 3 * C, L)
            shards = (C * L // 4 + 63) // 64 * ((b + 3) // 4)        # one dgamma shard per workgroup
            dgam, bn_grad = zeros(shards * 4), zeros(6 * C)
            lib.node_mix_lnp_bwd(gy, pre, ln_w, st, lnp0, None, gin, dres, 0, x, y, p1, U, chan, gamma, dgam, dx, dy, 0,
                                 dV, bn_grad, b, C, L, dglu, dfc, shards, 4)
            res[f'lazy b{b} C{C} L{L} {tag}'] = dict(pre=pre, rec=rec, prm=prm, g_in=gin, dresid=dres, dx=dx, dy=dy,
                                                      dV=dV, dgamma=dgam, bn_grad=bn_grad)
        # ---- sdpa_ln
        for b, C, L in SDPA_ROWS:
            g = gen(5, b, C, L)
            x, y, go = (R(g, b, C, L) for _ in range(3))
            ln_w, ln_b = R(g, C, L, scale=0.5, shift=1.0), R(g, C, L, scale=0.5)
            drop = lib.make_dropout(0.25, DROP_SEED, 3 << 33) if drop_on else lib.NO_DROP
            o, xhat, dx, dy, st = out(b, C, L), out(b, C, L), out(b, C, L), out(b, C, L), out(b, 2)
            lib.sdpa_ln_fwd(x, y, ln_w, ln_b, o, xhat, st, b, C, L, drop)
            lib.sdpa_ln_bwd(go, None, x, y, ln_w, xhat, st, dx, dy, 0, b, C, L, drop)
            res[f'sdpa_ln b{b} C{C} L{L} {tag}'] = dict(out=o, xhat=xhat, stats=st, dx=dx, dy=dy)

    # ---- head, mode 0 (no dropout site).  The backward reads a seeded hb, not the forward's: at more than one k-slice
    # the forward's is a sum of atomics
    for b, C, L, n_src, O in HEAD_ROWS:
        g = gen(6, b, C, L, n_src, O)
        D = n_src * C * L
        srcs = [R(g, b, C, L) for _ in range(n_src)]
        sums = [torch.stack([s.double().sum(dim=(1, 2)), (s.double() ** 2).sum(dim=(1, 2))], dim=1).float().contiguous()
                for s in srcs]
        ln_w, ln_b = R(g, n_src * C, L, scale=0.3, shift=1.0), R(g, n_src * C, L, scale=0.2)
        W, bias = R(g, O, D, scale=0.05), R(g, O, scale=0.1)
        hb, st = zeros(3, b, O), out(b, 2)
        lib.head_fwd(srcs, sums, ln_w, ln_b, W, bias, hb, st, b, C, L, O)
        r = {'stats': st}
        if b == 1 and D <= 64:                    # a single k-slice: one add per address
            r['hb'] = hb
        hb_in, gl = R(g, 3, b, O), R(g, b, O)
        dsrcs = [out(b, C, L) for _ in range(n_src)]
        part = out(lib.head_chunks(b), O + 3, D)
        loss = zeros(1)
        lib.head_bwd(srcs, sums, dsrcs, 0, ln_w, ln_b, W, hb_in, st, 0, gl, None, None, loss, part, b, C, L, O)
        r.update(part=part, loss=loss)
        r.update({f'dsrc{q}': t for q, t in enumerate(dsrcs)})
        res[f'head b{b} C{C} L{L} n{n_src} O{O}'] = r

    torch.cuda.synchronize()
    torch.save({k: {n: v.cpu() for n, v in d.items()} for k, d in res.items()}, path)


def batch_of(key):
    return int(key.split(' b')[1].split()[0])


def main():
    if len(sys.argv) == 3 and sys.argv[1] == '--child':
        return child(sys.argv[2])
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    libs = [os.path.abspath(p) for p in sys.argv[1:]]
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib_path in enumerate(libs):
            assert os.path.exists(lib_path), lib_path
            out = os.path.join(tmp, f'run{i}.pt')
            subprocess.run([sys.executable, os.path.abspath(__file__), '--child', out],
                           env={**os.environ, 'BMNAS_LIB': lib_path}, check=True)
            runs.append(torch.load(out))
    a, b = runs
    assert a.keys() == b.keys()
    print(f'A = {sys.argv[1]}\nB = {sys.argv[2]}')
    bad = tensors = skipped = 0
    for key in a:
        notes, names = [], []
        for name, ta in a[key].items():
            tb = b[key][name]
            if name in ATOMIC and batch_of(key) != 1:
                skipped += 1
                continue
            tensors += 1
            names.append(name)
            assert not (ta == SENTINEL).all() and not (tb == SENTINEL).all(), (key, name, 'not written')
            if not torch.equal(ta.view(torch.int32), tb.view(torch.int32)):
                bad += 1
                notes.append(f'{name} DIFFERS (max |A - B| = {float((ta.double() - tb.double()).abs().max()):.3e})')
        print(f'{key:48s} ' + (', '.join(notes) if notes else 'byte-equal: ' + ' '.join(names)))
    print(f'{tensors} tensors of {len(a)} cases compared, {bad} differ; {skipped} atomic outputs at b > 1 left to the '
          'float64 suites')
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
