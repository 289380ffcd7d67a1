"""Same bits from two builds of the library: the attention kernels of both families on cuda:0, dropout off and on.

    python tools/attn_ab.py LIB_A LIB_B          (e.g. a tools/build_variant.sh build of the parent commit and
                                                  bm-nas_amd/bmnas/libbmnas_hip.so)

Each library is loaded through BMNAS_LIB in a fresh child process of its own, which runs, on the same seeded inputs,
  bmnas_sdpa_ln_fwd / _bwd   at (b, C, L) = (3, 16, 4) a ragged last tile group, (5, 80, 8) ragged chunks,
                             (2, 272, 16) a rounded-up KCH, (3, 192, 16) a flagship width;
  bmnas_mha_core_fwd / _bwd  over tests/mha_ref.py's KERNEL_TABLE
and saves every output tensor.  The parent process (which never touches the GPU) compares them byte for byte: these
kernels use no atomics, so two builds that do the same arithmetic in the same order agree in every bit.  Exit status 1
if a tensor differs (its largest difference is printed), 0 otherwise.  No GPU: the children fail, nothing falls back.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'bm-nas_amd')):
    sys.path.insert(0, p)
import torch

SDPA_SHAPES = [(3, 16, 4), (5, 80, 8), (2, 272, 16), (3, 192, 16)]
DROP_P, DROP_SEED, DROP_OFFSET = 0.25, 0x5EED0123456789, 3 << 33


def child(path):
    import mha_ref
    from bmnas import lib
    assert torch.cuda.is_available(), 'tools/attn_ab.py compares runs on the GPU: no device, no result'
    dev = torch.device('cuda:0')
    res = {}
    for drop_on in (False, True):
        drop = lib.make_dropout(DROP_P, DROP_SEED, DROP_OFFSET) if drop_on else lib.NO_DROP
        for b, C, L in SDPA_SHAPES:
            g = torch.Generator().manual_seed(1000 * C + 10 * L + b)
            x, y, go = (torch.rand(b, C, L, generator=g).mul(2).sub(1).to(dev) for _ in range(3))
            ln_w = torch.rand(C, L, generator=g).add(0.5).to(dev)
            ln_b = torch.rand(C, L, generator=g).sub(0.5).to(dev)
            out, xhat, dx, dy = (torch.full((b, C, L), float('nan'), device=dev) for _ in range(4))
            stats = torch.full((b, 2), float('nan'), device=dev)
            lib.sdpa_ln_fwd(x, y, ln_w, ln_b, out, xhat, stats, b, C, L, drop)
            lib.sdpa_ln_bwd(go, None, x, y, ln_w, xhat, stats, dx, dy, 0, b, C, L, drop)
            key = f'sdpa b{b} C{C} L{L} drop{int(drop_on)}'
            res[key] = {'out': out, 'xhat': xhat, 'stats': stats, 'dx': dx, 'dy': dy}
        for C, heads, L, b in mha_ref.KERNEL_TABLE:
            t = {k: v.to(dev) for k, v in mha_ref.make_core_inputs(C, heads, L, b).items()}
            O, dq, dk, dv = (torch.full((b, C, L), float('nan'), device=dev) for _ in range(4))
            P = torch.full((b, heads, L, L), float('nan'), device=dev)
            lib.mha_core_fwd(t['Q'], t['K'], t['V'], O, P, b, C, L, heads, drop)
            lib.mha_core_bwd(t['dO'], t['Q'], t['K'], t['V'], P, dq, dk, dv, b, C, L, heads, drop)
            key = f'mha C{C} h{heads} L{L} b{b} drop{int(drop_on)}'
            res[key] = {'O': O, 'P': P, 'dq': dq, 'dk': dk, 'dv': dv}
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
