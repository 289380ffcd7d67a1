"""Same bits from two builds of the library: every multi-tensor launch of csrc/adam.hip and csrc/unroll.hip on cuda:0.

    python tools/optim_ab.py LIB_A LIB_B         (e.g. a tools/build_variant.sh build of the parent commit and
                                                  bm-nas_amd/bmnas/libbmnas_hip.so)

Each library is loaded through BMNAS_LIB in a fresh child process of its own, which runs, through the C ABI and on the
same seeded inputs, over ONE table of tensors of 1, 3, 1023, 1024, 1025, 4099 and 300 * 1024 + 5 elements (a lone
element, a scalar tail only, a tail after full lanes, exactly one chunk, one chunk and one element, several chunks and a
tail of three, and more chunks than the norm launch has workgroups) — once 16-byte aligned, once offset by one float —
  bmnas_grad_sqnorm_multi, bmnas_grad_scale_multi,
  bmnas_adam_multi_ex with flags 0 .. 3, unclipped and clipped (flags 0: bmnas_adam_multi / bmnas_adam_multi_clip),
  bmnas_sgd_multi with flags 0, 1, 3, unclipped and clipped,
  bmnas_unroll_virtual_step (flags 0, 1; one tensor without a momentum buffer), _perturb (+1, -1), _restore, _combine
and saves everything a launch wrote.  The parent process (which never touches the GPU) compares byte for byte: these
kernels use no atomics, so two builds that do the same arithmetic in the same order agree in every bit.  Exit status 1
if a tensor differs (its largest difference is printed), 0 otherwise.  No GPU: the children fail, nothing falls back.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'bm-nas_amd'))
import numpy as np
import torch

SIZES = (1, 3, 1023, 1024, 1025, 4099, 300 * 1024 + 5)
COLS = ('param', 'grad', 'exp_avg', 'exp_avg_sq')


def child(path):
    from bmnas import lib, optim
    assert torch.cuda.is_available(), 'tools/optim_ab.py compares runs on the GPU: no device, no result'
    dev = torch.device('cuda:0')
    chunks, n_chunks = optim._chunk_list(SIZES, dev)
    n_parts = min(n_chunks, lib.grad_norm_parts())
    res = {}

    def scalar(*v):
        return torch.tensor(v, dtype=torch.float32, device=dev)

    for off in (0, 1):
        gen = torch.Generator().manual_seed(77 + off)

        def fresh(positive=False):
            """One tensor per size, `off` floats behind a 16-byte boundary."""
            out = []
            for n in SIZES:
                base = torch.randn(n + 1, generator=gen)
                out.append((base.abs() if positive else base).to(dev)[off:off + n])
            return out

        def table(**cols):
            """-> uint8 device tensor holding bmnas_adam_tensor_t[] over the given columns (None: a null pointer)."""
            tab = np.zeros(len(SIZES), dtype=optim._DESC)
            for name, ts in cols.items():
                tab[name] = [0 if t is None else t.data_ptr() for t in ts]
                assert all(t is None or t.data_ptr() % 16 == 4 * off for t in ts)
            tab['numel'] = SIZES
            tab['hyp_row'] = [i % 2 for i in range(len(SIZES))]
            return torch.from_numpy(tab.view(np.uint8).copy()).to(dev)

        src = {c: fresh(positive=c == 'exp_avg_sq') for c in COLS}
        src['max'] = fresh(positive=True)
        clone = lambda ts: [torch.cat([t.new_zeros(4 + off), t])[4 + off:] for t in ts]    # same alignment, own storage
        blank = lambda ts: [t.fill_(float('nan')) for t in clone(ts)]                      # ... for what a launch fills

        def keep(key, **named):
            res[f'off{off} {key}'] = {k: (torch.cat([t.reshape(-1) for t in v]) if isinstance(v, list) else v)
                                      for k, v in named.items()}

        partials = torch.full((lib.grad_norm_parts(),), float('nan'), device=dev)
        lib.grad_sqnorm_multi(table(grad=src['grad']), chunks, n_chunks, partials)
        keep('grad_sqnorm', partials=partials[:n_parts].clone())
        clip = scalar(0.5, 0, 0, 0)

        g, norm = clone(src['grad']), scalar(float('nan'))
        lib.grad_scale_multi(table(grad=g), chunks, n_chunks, partials, n_parts, clip, norm)
        keep('grad_scale', grad=g, norm=norm)

        # rows as Adam.prepare_replay() stages them, steps 3 and 7; slot 5 is weight_decay or the decoupled factor
        def adam_rows(decoupled):
            rows = []
            for t, lr, wd in ((3.0, 1e-3, 1e-4), (7.0, 3e-4, 0.0)):
                b1, b2 = 0.9, 0.999
                w = (1 - lr * wd if wd else 1.0) if decoupled else wd
                rows.append((-(lr / (1 - b1 ** t)), (1 - b2 ** t) ** 0.5, b1, b2, 1e-8, w, 1 - b1, 1 - b2))
            return scalar(*rows)
        for flags in range(4):
            for clipped in (False, True):
                st = {c: clone(src[c]) for c in ('param', 'exp_avg', 'exp_avg_sq', 'max')}
                mx = None
                if flags & lib.ADAM_AMSGRAD:
                    mx = torch.tensor([t.data_ptr() for t in st['max']], dtype=torch.int64, device=dev)
                norm = scalar(float('nan'))
                extra = (partials, n_parts, clip, norm) if clipped else ()
                tab = table(param=st['param'], grad=src['grad'], exp_avg=st['exp_avg'], exp_avg_sq=st['exp_avg_sq'])
                lib.adam_multi_ex(tab, chunks, n_chunks, adam_rows(flags & lib.ADAM_DECOUPLED), mx, flags, *extra)
                keep(f'adam flags{flags} clip{int(clipped)}', norm=norm if clipped else scalar(0.0), **st)

        sgd_rows = scalar((-0.05, 0.9, 0.75, 0.9, 3e-4, 0, 0, 0), (-0.01, 0.0, 1.0, 0.5, 0.0, 0, 0, 0))
        for flags in (0, lib.SGD_MOMENTUM, lib.SGD_MOMENTUM | lib.SGD_NESTEROV):
            for clipped in (False, True):
                st = {c: clone(src[c]) for c in ('param', 'exp_avg')}
                norm = scalar(float('nan'))
                extra = (partials, n_parts, clip, norm) if clipped else ()
                tab = table(param=st['param'], grad=src['grad'], exp_avg=st['exp_avg'] if flags else [None] * len(SIZES))
                lib.sgd_multi(tab, chunks, n_chunks, sgd_rows, flags, *extra)
                keep(f'sgd flags{flags} clip{int(clipped)}', norm=norm if clipped else scalar(0.0), **st)

        virt_rows = scalar((-0.025, 0.9, 3e-4, 0, 0, 0, 0, 0), (-0.025, 0.0, 0.0, 0, 0, 0, 0, 0))
        for flags in (0, lib.UNROLL_MOMENTUM):
            st = {'param': clone(src['param']), 'bak': blank(src['param'])}
            buf = [None if not flags or i == 2 else t for i, t in enumerate(src['exp_avg'])]
            tab = table(param=st['param'], grad=src['grad'], exp_avg=buf, exp_avg_sq=st['bak'])
            lib.unroll_virtual_step(tab, chunks, n_chunks, virt_rows, flags)
            keep(f'unroll virtual flags{flags}', **st)
        for sign in (1, -1):
            p, R = clone(src['param']), scalar(float('nan'))
            tab = table(param=p, grad=src['grad'], exp_avg_sq=src['exp_avg'])
            lib.unroll_perturb(tab, chunks, n_chunks, partials, n_parts, scalar(1e-2), sign, R)
            keep(f'unroll perturb {sign:+d}', param=p, R=R)
        p = blank(src['param'])
        lib.unroll_restore(table(param=p, exp_avg_sq=src['exp_avg']), chunks, n_chunks)
        keep('unroll restore', param=p)
        p = clone(src['param'])
        tab = table(param=p, grad=src['grad'], exp_avg=src['exp_avg'])
        lib.unroll_combine(tab, chunks, n_chunks, scalar(0.025), scalar(3.7e-4))
        keep('unroll combine', param=p)
    torch.cuda.synchronize()
    torch.save({k: {n: v.cpu() for n, v in d.items()} for k, d in res.items()}, path)


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
    bad = tensors = 0
    for key in a:
        notes = []
        for name, ta in a[key].items():
            tb = b[key][name]
            tensors += 1
            assert torch.isfinite(ta).all() and torch.isfinite(tb).all(), (key, name, 'not finite / not written')
            if not torch.equal(ta.view(torch.int32), tb.view(torch.int32)):
                bad += 1
                notes.append(f'{name} DIFFERS (max |A - B| = {float((ta.double() - tb.double()).abs().max()):.3e})')
        print(f'{key:34s} ' + (', '.join(notes) if notes else 'byte-equal: ' + ' '.join(a[key])))
    print(f'{tensors} tensors of {len(a)} cases compared, {bad} differ')
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
