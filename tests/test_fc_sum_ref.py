"""The float64 reference of tests/fc_sum_ref.py (what tests/test_fc_edges_kernels_gpu.py holds the kernels of
csrc/fcedge.hip against) checked on the CPU: against oracle.fusion_oracle.mixed_edge_general summed over the edges
(evaluated in float64, the exported-mask injection standing in for the dropout draws), against torch.autograd on the
forward expression written out here (dw, dx, every parameter gradient, dU through the retained pre-activations), and
against one central finite difference on a dw entry.  Also the fp32 emulation behind the bias constant of the
shifted-variance case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fc_sum_ref as R
from oracle import fusion_oracle as fo

CHECKED = [R.CASES[2], R.CASES[5], R.CASES[6]]        # permuted columns; shared / own / ungraded sources; n = 15, P = 8
TOL = 1e-10                                           # float64 against float64: relative to the tensor's largest value


def close(name, got, want, tol=TOL):
    got, want = got.detach().double(), want.detach().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err, scale = float((got - want).abs().max()), max(float(want.abs().max()), 1e-30)
    assert err <= tol * scale, f'{name}: max|err| {err:.3e} at scale {scale:.3e}'


def cpu_masks(case, training, seed):
    """Bernoulli(1 - p) / (1 - p) multipliers per (edge, FC primitive) site (training with n > 1), else ones."""
    Cc, L, b, prims, src, _ = case
    rng = np.random.Generator(np.random.PCG64(seed))
    F_ = len(R.columns(prims)[0])
    live = training and len(src) > 1
    return [[torch.from_numpy((rng.random(b * Cc * L) >= R.P_DROP) / (1.0 - R.P_DROP)) if live
             else torch.ones(b * Cc * L, dtype=torch.float64) for _ in range(F_)] for _ in src], live


def forward_expr(case, xs, prm, w, masks, training):
    """The sum as a differentiable float64 expression.  prm[j][f] = (W, bias, bn_w, bn_b, rm, rv) -> (out, U[j][f])."""
    Cc, L, b, prims, src, _ = case
    fcols, kinds, _ = R.columns(prims)
    out, Us = 0, []
    for j, s in enumerate(src):
        x, row = xs[s], []
        for p, name in enumerate(prims):
            if name == 'skip':
                out = out + w[j, p] * x
            elif name != 'none':
                f = fcols.index(p)
                W, bias, bn_w, bn_b, rm, rv = prm[j][f]
                U = (W @ x) + bias[:, None]                                   # (b, C, L): W over the channel dim
                row.append(U)
                a = F.mish(U) if kinds[f] else torch.clamp(U, min=0)
                mean, var = (a.mean(dim=(0, 2)), ((a - a.mean(dim=(0, 2), keepdim=True)) ** 2).mean(dim=(0, 2))) \
                    if training else (rm, rv)
                y = (a - mean[:, None]) / torch.sqrt(var[:, None] + R.EPS) * bn_w[:, None] + bn_b[:, None]
                out = out + w[j, p] * masks[j][f].view(b, Cc, L) * y
        Us.append(row)
    return out, Us


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('case', CHECKED, ids=R.case_id)
def test_reference_against_oracle_autograd_and_difference(case, training):
    Cc, L, b, prims, src, _ = case
    fcols, kinds, skip_cols = R.columns(prims)
    n, P = len(src), len(prims)
    xs, edges, w, g = R.make_case(case, 500 + Cc + L + n)
    masks, live = cpu_masks(case, training, 9)
    ref = R.reference(case, xs, edges, w, g, masks, training)

    # --- the oracle, in float64, masks injected at its dropout sites (edge by edge, primitives in list order)
    p = {}
    for j in range(n):
        for f, c in enumerate(fcols):
            q, k = edges[j][f], f'cell._ops.{j}._ops.{c}'
            p[k + '.linear.weight'], p[k + '.linear.bias'] = q['W'].double(), q['bias'].double()
            p[k + '.bn.weight'], p[k + '.bn.bias'] = q['bn_w'].double(), q['bn_b'].double()
            p[k + '.bn.running_mean'], p[k + '.bn.running_var'] = q['rm'].double(), q['rv'].double()
            p[k + '.bn.num_batches_tracked'] = torch.tensor(7)
    po = {k: (v.clone() if fo.is_buffer(k) else v.clone().requires_grad_(True)) for k, v in p.items()}
    xo = [x.double().requires_grad_(True) for x in xs]
    wo = w.double().requires_grad_(True)
    flat = [m for row in masks for m in row]
    with fo.injected_masks(flat if live else []) as inj:
        o_out = sum(fo.mixed_edge_general(xo[src[j]], wo[j], po, f'cell._ops.{j}', prims, training,
                                          R.P_DROP if live else 0.0) for j in range(n))
    assert inj.used == (len(flat) if live else 0)
    o_out.backward(g.double())
    close('out (oracle)', ref['out'], o_out)
    close('dw (oracle)', ref['dw'], wo.grad)
    for s in range(len(xs)):
        close(f'dx[{s}] (oracle)', ref['dx'][s], xo[s].grad)
    for j in range(n):
        for f, c in enumerate(fcols):
            k, r = f'cell._ops.{j}._ops.{c}', ref['fc'][j][f]
            close(k + ' dW', r['dW'], po[k + '.linear.weight'].grad)
            close(k + ' dbias', r['dbias'], po[k + '.linear.bias'].grad)
            close(k + ' bn_grad', r['bn_grad'], torch.cat([po[k + '.bn.weight'].grad, po[k + '.bn.bias'].grad]))
            close(k + ' running_mean', r['rm'], po[k + '.bn.running_mean'])
            close(k + ' running_var', r['rv'], po[k + '.bn.running_var'])
            assert int(po[k + '.bn.num_batches_tracked']) == 7 + int(training)

    # --- torch.autograd on the forward expression written out above
    xa = [x.double().requires_grad_(True) for x in xs]
    wa = w.double().requires_grad_(True)
    prm = [[tuple(q[k].double().requires_grad_(k not in ('rm', 'rv')) for k in ('W', 'bias', 'bn_w', 'bn_b', 'rm', 'rv'))
            for q in edges[j]] for j in range(n)]
    out, Us = forward_expr(case, xa, prm, wa, masks, training)
    for row in Us:
        for U in row:
            U.retain_grad()
    out.backward(g.double())
    close('out (autograd)', ref['out'], out)
    close('dw (autograd)', ref['dw'], wa.grad)
    for c, name in enumerate(prims):
        if name == 'none':
            assert float(ref['dw'][:, c].abs().max()) == 0.0
    for s in range(len(xs)):
        close(f'dx[{s}] (autograd)', ref['dx'][s], xa[s].grad)
    for j in range(n):
        for f in range(len(fcols)):
            r, (W, bias, bn_w, bn_b, _, _) = ref['fc'][j][f], prm[j][f]
            close(f'U[{j}][{f}]', r['U'], Us[j][f])
            close(f'dU[{j}][{f}]', r['dU'], Us[j][f].grad)
            close(f'dW[{j}][{f}]', r['dW'], W.grad)
            close(f'dbias[{j}][{f}]', r['dbias'], bias.grad)
            close(f'bn_grad[{j}][{f}]', r['bn_grad'], torch.cat([bn_w.grad, bn_b.grad]))
            mean, rstd, scale, shift = r['chan']
            close(f'scale[{j}][{f}]', scale, bn_w.detach() * rstd)
            close(f'shift[{j}][{f}]', shift, bn_b.detach() - mean * scale)

    # --- one central finite difference: dw[j, col] = d <g, out> / d w[j, col]
    jd, cd, h = n - 1, fcols[-1], 1.0 / 64
    with torch.no_grad():
        vals = []
        for sgn in (+1, -1):
            wd = w.double().clone()
            wd[jd, cd] += sgn * h
            vals.append(float((forward_expr(case, [x.double() for x in xs], prm, wd, masks, training)[0]
                               * g.double()).sum()))
    fd = (vals[0] - vals[1]) / (2 * h)
    assert abs(fd - float(ref['dw'][jd, cd])) <= 1e-9 * max(1.0, abs(fd)), (fd, float(ref['dw'][jd, cd]))


def test_inputs_are_exact_in_fp32():
    """Every pre-activation of every case is an odd multiple of 1/512 and identical whether formed in fp32 or
    float64; the same with the shifted-variance constant on the fc_relu bias."""
    for case, shift in [(c, 0.0) for c in R.CASES] + [(R.CASES[1], R.SHIFT_BIAS)]:
        Cc, L, b, prims, src, _ = case
        xs, edges, w, g = R.make_case(case, 1)
        for j, fc in enumerate(edges):
            for q in fc:
                U64 = torch.einsum('mk,bkl->bml', q['W'].double(), xs[src[j]].double()) + q['bias'].double()[None, :, None]
                U32 = torch.einsum('mk,bkl->bml', q['W'], xs[src[j]]) + q['bias'][None, :, None]
                assert torch.equal(U32.double(), U64)
                k = U64 * 512
                assert torch.equal(k, k.round()) and bool((k.abs() % 2 == 1).all())
                assert float(U64.abs().max()) * 512 < 2 ** 24


def shifted_case_errors():
    """Errors (in units of the rel = 1e-4 tolerance of the tensor's scale) of chan.rstd and running_var of the
    shifted-variance case's fc_relu sites under the fp32 emulation of the shifted and the unshifted formula, the worse
    of sequential and pairwise summation for the former, the better for the latter."""
    case = R.CASES[1]
    Cc, L, b, prims, src, _ = case
    xs, edges, w, g = R.make_case(case, R.SHIFT_SEED, R.SHIFT_BIAS)
    ones = [[torch.ones(b * Cc * L)] * 2 for _ in src]
    ref = R.reference(case, xs, edges, w, g, ones, True)
    N = b * L
    worst = {True: 0.0, False: float('inf')}
    for shifted in (True, False):
        for tree in (False, True):
            over = 0.0
            for j in range(len(src)):
                q, r = edges[j][0], ref['fc'][j][0]
                assert q['mish'] == 0
                U = r['U'].float().numpy()                                    # exact
                mv = [R.emulated_batch_stats(U[:, c, :].reshape(-1), q['bias'].numpy()[c], 0, shifted, tree)
                      for c in range(Cc)]
                mean, var = np.float32([m for m, _ in mv]), np.float32([v for _, v in mv])
                rstd = (1.0 / np.sqrt(var + np.float32(R.EPS))).astype(np.float32)
                rv = (np.float32(0.9) * q['rv'].numpy() + np.float32(0.1) * var * np.float32(N / (N - 1.0)))
                for got, want in ((mean, r['chan'][0]), (rstd, r['chan'][1]), (rv, r['rv'])):
                    want = want.numpy()
                    over = max(over, float(np.abs(got - want).max() / (1e-4 * np.abs(want).max())))
            worst[shifted] = max(worst[shifted], over) if shifted else min(worst[shifted], over)
    return worst[True], worst[False]


def test_shifted_variance_constant():
    """R.SHIFT_BIAS on the fc_relu bias: the kernel's shifted sums stay inside rel = 1e-4, sums of act(u) and act(u)^2
    in fp32 miss it by at least 3x — so the GPU case fails a kernel that lost the shift and passes one that has it."""
    ok, lost = shifted_case_errors()
    print(f'SHIFT_BIAS {R.SHIFT_BIAS}: shifted {ok:.3g} x tol, unshifted {lost:.3g} x tol')
    assert ok <= 0.5, ok
    assert lost >= 3.0, lost
