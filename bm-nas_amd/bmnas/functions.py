"""torch.autograd.Function wrappers over bmnas.cell / bmnas.lib.

Every Function requires CUDA(HIP) fp32 tensors and the built shared library; there is no
CPU or eager-PyTorch fallback on the product path (bmnas.lib raises if the .so is absent).
"""
from __future__ import annotations

import torch
from torch.autograd import Function

from . import cell as K
from . import lib


def _require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f'bmnas: {what} needs tensors on a HIP device (got {t.device}); the fusion-cell '
                           'hot path runs only on the gfx950 kernels — there is no CPU fallback')


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _f32(t):
    if t.dtype != torch.float32:
        raise TypeError(f'bmnas kernels are fp32 only (got {t.dtype})')
    return t


def _round4(n):
    """n floats rounded up to a multiple of four: slices carved at such offsets stay 16-byte aligned."""
    return (n + 3) // 4 * 4


# ---- the gradients a conv + BatchNorm of M rows and weight row stride ldw accumulates with atomics: ONE zero-filled chunk
# bn_grad [2M: the BatchNorm's dweight | dbias] | dW (M, ldw) | dbias [M] — the layout of every conv + BatchNorm Function
def conv_grad_floats(M, ldw):
    return 2 * M + M * ldw + M


def conv_grad_split(buf, M, ldw, off=0):
    """-> (bn_grad, dW, dbias) of the chunk that starts at float `off` of buf."""
    w, e = off + 2 * M, off + 2 * M + M * ldw
    return buf[off:w], buf[w:e].view(M, ldw), buf[e:e + M]


def conv_grad_offsets(M, ldws, base=0):
    """The group form: where the chunks of len(ldws) convs start behind `base` floats, each on a multiple of four floats;
    one entry more than chunks, the last being the floats of the whole buffer."""
    offs = [base]
    for ldw in ldws:
        offs.append(offs[-1] + _round4(conv_grad_floats(M, ldw)))
    return offs


# ------------------------------------------------------------------- arch softmax
class ArchSoftmaxFn(Function):
    """softmax(logits, dim=-1) for the (rows, 2|4) architecture parameters
    (model_search.py:95, node_search.py:102-103)."""

    @staticmethod
    def forward(ctx, logits):
        _require_gpu(logits, 'arch softmax')
        a = _c(_f32(logits))
        w = torch.empty_like(a)
        lib.arch_softmax_fwd(a, w, a.shape[0], a.shape[1])
        ctx.save_for_backward(w)
        return w

    @staticmethod
    def backward(ctx, dw):
        (w,) = ctx.saved_tensors
        da = torch.empty_like(w)
        lib.arch_softmax_bwd(w, _c(dw), da, w.shape[0], w.shape[1])
        return da


def arch_softmax(logits, device):
    if logits.device != device:
        logits = logits.to(device)        # reference keeps alphas on the CPU; tracked copy
    return ArchSoftmaxFn.apply(logits)


class ArchRelaxFn(Function):
    """z_t = (a_t + G_t) / tau for EVERY architecture tensor as one autograd node and one launch (csrc/relax.hip;
    bmnas.nn.ArchRelaxation owns `state`, the device block with tau, the seed and the noise counter).
    ArchRelaxFn.apply(state, gumbel, advance, *logits) -> *z.  The backward, da_t = dz_t / tau, is one launch over the
    inputs that need a gradient and received one — none under bmnas.cell.weight_grads_only."""

    @staticmethod
    def forward(ctx, state, gumbel, advance, *logits):
        dev = state.device
        # (the reference keeps the arch tensors wherever the model was built: copy over first, as arch_softmax does)
        a = [_c(_f32(t if t.device == dev else t.to(dev))) for t in logits]
        z = [torch.empty_like(t) for t in a]
        lib.arch_relax_fwd(a, z, None, state, gumbel, advance)
        ctx.state = state
        ctx.devices = [t.device for t in logits]
        ctx.set_materialize_grads(False)
        return tuple(z)

    @staticmethod
    def backward(ctx, *dz):
        n = len(dz)
        out = [None] * n
        if not K._NO_ARCH[0]:
            sel = [i for i in range(n) if dz[i] is not None and ctx.needs_input_grad[3 + i]]
            if sel:
                g = [_c(dz[i]) for i in sel]
                da = [torch.empty_like(t) for t in g]
                lib.arch_relax_bwd(g, da, ctx.state)
                for i, d in zip(sel, da):
                    out[i] = d if d.device == ctx.devices[i] else d.to(ctx.devices[i])
        return (None, None, None, *out)


# --------------------------------------------------------------------------- K1
class MixSumFn(Function):
    """out = sum_j w[j] * xs[j]  (w: (n_in,) device tensor)."""

    @staticmethod
    def forward(ctx, w, *xs):
        _require_gpu(xs[0], 'mixed-edge sum')
        xs = [_c(_f32(x)) for x in xs]
        w = _c(_f32(w))
        out = torch.empty_like(xs[0])
        lib.mixsum_fwd(xs, w, 1, out)
        ctx.xs, ctx.w = xs, w
        return out

    @staticmethod
    def backward(ctx, g):
        xs, w = ctx.xs, ctx.w
        g = _c(g)
        need_w = ctx.needs_input_grad[0]
        dw = torch.zeros_like(w) if need_w else None
        dxs = [torch.empty_like(x) if ctx.needs_input_grad[1 + j] else None for j, x in enumerate(xs)]
        lib.mixsum_bwd(xs, dxs, w, 1, g, dw, 0)
        return (dw, *dxs)


# ---- LayerNorm-affine reductions of the per-op path: ONE launch per backward pass ----------------------------------
# The fused search cell ends its backward with one batched launch for every LayerNorm's (dweight, dbias) (reductions
# over the batch: bmnas_ln_affine_bwd_multi); the per-op Functions below (Found_* nets, standalone modules) paid one
# launch per LayerNorm — 4 of the 22 launches of an MM-IMDB found-stage step.  Inside `deferred_affine()` (entered by
# bmnas.graph.GraphedTrainStep around its torch.autograd.grad call, whose results nobody reads before the context
# ends) they only note the job; the context's exit launches them together.  Plain `loss.backward()` keeps the
# immediate launches: an AccumulateGrad node may ADD a parameter's incoming gradient to an existing .grad right away.
# Constraint: a deferred job's (dweight, dbias) are handed to autograd BEFORE the launch that fills them has run,
# so nothing may read them inside the torch.autograd.grad call.  That holds when the LayerNorm's weight / bias are leaf
# tensors used by ONE Function of the pass (the engine passes a single incoming gradient through untouched).  A parameter
# that reaches the Function through an op (a cast, a view, a parametrization: not a leaf) or that is used twice (the engine
# adds the two gradients out of place as soon as the second arrives) gets its launches immediately instead — `_ln_affine`
# checks both.
AFFINE_DEFER = None
_DEFER_KEYS = {}          # id(ln_w storage) -> its pending job, for the pass in progress


class deferred_affine:
    def __enter__(self):
        global AFFINE_DEFER, _DEFER_KEYS
        self.prev, AFFINE_DEFER = AFFINE_DEFER, []
        self.prev_keys, _DEFER_KEYS = _DEFER_KEYS, {}
        return self

    def __exit__(self, *exc):
        global AFFINE_DEFER, _DEFER_KEYS
        jobs, AFFINE_DEFER = AFFINE_DEFER, self.prev
        _DEFER_KEYS = self.prev_keys
        groups, sums = {}, []
        for b, L, prob in jobs:
            if prob is None:
                continue                          # launched early (its parameter came up a second time)
            if b is None:
                sums.append(prob)                 # (part, out, n_chunk): the fused found head's per-chunk partials
            else:
                groups.setdefault((b, L), []).append(prob)
        for (b, L), probs in groups.items():
            for i in range(0, len(probs), 8):
                if sums:                          # ride in the same launch (bmnas_backward_epilogue: affine + sums)
                    lib.backward_epilogue(probs[i:i + 8], b, L, [], [], [], 1, 0, sums=tuple(sums[:2]))
                    sums = sums[2:]
                else:
                    lib.ln_affine_bwd_multi(probs[i:i + 8], b, L)
        for part, out, n_chunk in sums:
            lib.sum_chunks(part, out, n_chunk)
        return False


def _ln_affine(g, srcs, resid, ln_w, ln_b, stats, dw, db, b, C, L, relu, prenorm, key=None, leaf=True):
    """key: identifies the LayerNorm's weight (its data pointer) — a second job for the same key inside one deferral, or a
    weight that is not a leaf (`leaf=False`), is launched at once, and so is the earlier job of that key."""
    if AFFINE_DEFER is not None and leaf and (key is None or key not in _DEFER_KEYS):
        AFFINE_DEFER.append((b, L, dict(g=g, gscale=None, srcs=list(srcs), resid=resid, ln_w=ln_w, ln_b=ln_b, stats=stats,
                                        dln_w=dw, dln_b=db, C=C, relu=relu, prenorm=prenorm)))
        if key is not None:
            _DEFER_KEYS[key] = len(AFFINE_DEFER) - 1
        return
    if AFFINE_DEFER is not None and key is not None and _DEFER_KEYS.get(key) is not None:
        i = _DEFER_KEYS[key]                      # the first use's job: its gradient is about to be added to this one
        b0, L0, p0 = AFFINE_DEFER[i]
        AFFINE_DEFER[i] = (b0, L0, None)
        _DEFER_KEYS[key] = None
        lib.ln_affine_bwd(p0['g'], None, p0['srcs'], p0['resid'], p0['ln_w'], p0['ln_b'], p0['stats'], p0['dln_w'],
                          p0['dln_b'], b0, p0['C'], L0, p0['relu'], p0['prenorm'])
    lib.ln_affine_bwd(g, None, srcs, resid, ln_w, ln_b, stats, dw, db, b, C, L, relu, prenorm)


# ---- the zero-filled accumulators of a CAPTURED per-op step: one persistent arena, cleared in front of the replay --------
# The per-op Functions (Found_* nets, standalone modules, the torch-side classifier) add into zero-filled buffers with
# atomics: BatchNorm batch sums (_FwdStatPool), bn_grad | dW | dbias and the LayerNorm affine gradients (_ZeroPool), the
# classifier's split-K output.  Each pool cost a torch.zeros fill launch inside the step (and LinearFn a zero_fill of its
# own).  A captured step (bmnas.graph) now measures what a pass needs during its dress rehearsal (`arena_measure()`), owns
# ONE persistent fp32 arena of that size, and the launch that copies the batch in front of every replay also clears it
# (bmnas_copy_batch's zero-fill jobs): inside the capture (`arena_use(arena)`) the pools carve from it without any fill.
# Anything beyond the measured size falls back to a fill of its own, as before.
class _StepArena:
    def __init__(self, buf):
        self.buf, self.off = buf, 0

    def take(self, n):
        """n floats (exactly n: callers view the slice by shape); the cursor advances by n rounded up to a multiple of
        four so that every slice stays 16-byte aligned."""
        step = _round4(n)
        if self.off + step > self.buf.numel():
            return None
        v = self.buf[self.off:self.off + n]
        self.off += step
        return v


_ARENA = None            # the arena of the capture in progress
_ARENA_NEED = None       # [floats] while a rehearsal pass is being measured


class arena_measure:
    """with arena_measure() as m: one pass of the step -> m.need = floats of zero-filled scratch it took."""

    def __enter__(self):
        global _ARENA_NEED
        self.prev, _ARENA_NEED = _ARENA_NEED, [0]
        self.cell = _ARENA_NEED
        return self

    def __exit__(self, *exc):
        global _ARENA_NEED
        self.need, _ARENA_NEED = self.cell[0], self.prev
        return False


class arena_use:
    def __init__(self, buf):
        self.arena = _StepArena(buf) if buf is not None and buf.numel() else None

    def __enter__(self):
        global _ARENA
        self.prev, _ARENA = _ARENA, self.arena
        reset_pools()                     # nothing of an earlier (eager) pass may be handed out inside the capture
        return self

    def __exit__(self, *exc):
        global _ARENA
        _ARENA = self.prev
        reset_pools()                     # ... nor arena slices to the eager passes that follow
        return False


def zeros_for_step(n, device):
    """n zero-filled floats: a slice of the captured step's arena (cleared in front of every replay by the batch-copy
    launch), else torch.zeros — one fill launch."""
    if _ARENA_NEED is not None:
        _ARENA_NEED[0] += _round4(n)
    if _ARENA is not None and _ARENA.buf.device == device:
        v = _ARENA.take(n)
        if v is not None:
            return v
    return torch.zeros(n, device=device, dtype=torch.float32)


def _zero_pair(like):
    """Two zero-filled tensors shaped like `like` (a LayerNorm's dln_w, dln_b), slices of the backward pass's one
    zero-filled chunk (ZERO_POOL; the forward announced them)."""
    n = like.numel()
    buf = ZERO_POOL.take(2 * n, like.device)
    return buf[:n].view_as(like), buf[n:2 * n].view_as(like)


# ------------------------------------------------------------------------ K6 / K7
class CatLnFn(Function):
    """LayerNorm([n_src*C, L]) of cat(srcs, 1) (+ resid), optional ReLU; output (b, n_src*C, L)."""

    @staticmethod
    def forward(ctx, relu, ln_w, ln_b, resid, *srcs):
        _require_gpu(srcs[0], 'concat + LayerNorm')
        srcs = [_c(_f32(s)) for s in srcs]
        resid = None if resid is None else _c(resid)
        b, C, L = srcs[0].shape
        n = len(srcs)
        out = torch.empty((b, n * C, L), device=srcs[0].device, dtype=torch.float32)
        stats = torch.empty(b * 2, device=srcs[0].device, dtype=torch.float32)
        lw, lb = _c(ln_w), _c(ln_b)
        lib.cat_ln_fwd(srcs, resid, lw, lb, out, stats, b, C, L, relu)
        ctx.relu, ctx.srcs, ctx.resid, ctx.lw, ctx.lb, ctx.stats = relu, srcs, resid, lw, lb, stats
        ctx.leaf = ln_w.is_leaf and ln_b.is_leaf
        if any(ctx.needs_input_grad):
            ZERO_POOL.announce(2 * lw.numel())      # dln_w | dln_b of the backward: one fill per pass for all modules
        return out

    @staticmethod
    def backward(ctx, g):
        srcs, resid = ctx.srcs, ctx.resid
        b, C, L = srcs[0].shape
        g = _c(g)
        dsrcs = [torch.empty_like(s) if ctx.needs_input_grad[4 + q] else None for q, s in enumerate(srcs)]
        dres = torch.empty_like(resid) if (resid is not None and ctx.needs_input_grad[3]) else None
        dw, db = _zero_pair(ctx.lw)
        lib.cat_ln_bwd(g, srcs, resid, ctx.lw, ctx.lb, ctx.stats, dsrcs, dres, 0, None, None, b, C, L,
                       ctx.relu)
        _ln_affine(g, srcs, resid, ctx.lw, ctx.lb, ctx.stats, dw, db, b, C, L, ctx.relu, False,
                   key=ctx.lw.data_ptr(), leaf=ctx.leaf)
        return (None, dw, db, dres, *dsrcs)


class CatLnSumsFn(Function):
    """CatLnFn (no ReLU) that also hands out each sample's (sum, sum of squares) of its output — what the fused head
    (FoundHeadFn, csrc/head.hip) takes the K7 LayerNorm statistics from.  -> (out, sums (b, 2))."""

    @staticmethod
    def forward(ctx, ln_w, ln_b, resid, *srcs):
        _require_gpu(srcs[0], 'concat + LayerNorm')
        srcs = [_c(_f32(s)) for s in srcs]
        resid = None if resid is None else _c(resid)
        b, C, L = srcs[0].shape
        n = len(srcs)
        out = torch.empty((b, n * C, L), device=srcs[0].device, dtype=torch.float32)
        stats = torch.empty(b * 2, device=srcs[0].device, dtype=torch.float32)
        sums = torch.empty((b, 2), device=srcs[0].device, dtype=torch.float32)
        lw, lb = _c(ln_w), _c(ln_b)
        lib.cat_ln_fwd(srcs, resid, lw, lb, out, stats, b, C, L, False, sums)
        ctx.relu, ctx.srcs, ctx.resid, ctx.lw, ctx.lb, ctx.stats = False, srcs, resid, lw, lb, stats
        ctx.leaf = ln_w.is_leaf and ln_b.is_leaf
        if any(ctx.needs_input_grad):
            ZERO_POOL.announce(2 * lw.numel())
        ctx.mark_non_differentiable(sums)
        ctx.set_materialize_grads(False)          # (else autograd fills a zero tensor for `sums`' absent gradient: a launch)
        return out, sums

    @staticmethod
    def backward(ctx, g, _g_sums):
        srcs, resid = ctx.srcs, ctx.resid
        b, C, L = srcs[0].shape
        if g is None:                             # nobody differentiated the output (materialisation is off)
            return (None,) * (3 + len(srcs))
        g = _c(g)
        dsrcs = [torch.empty_like(s) if ctx.needs_input_grad[3 + q] else None for q, s in enumerate(srcs)]
        dres = torch.empty_like(resid) if (resid is not None and ctx.needs_input_grad[2]) else None
        dw, db = _zero_pair(ctx.lw)
        lib.cat_ln_bwd(g, srcs, resid, ctx.lw, ctx.lb, ctx.stats, dsrcs, dres, 0, None, None, b, C, L, False)
        _ln_affine(g, srcs, resid, ctx.lw, ctx.lb, ctx.stats, dw, db, b, C, L, False, False,
                   key=ctx.lw.data_ptr(), leaf=ctx.leaf)
        return (dw, db, dres, *dsrcs)


class FoundHeadFn(Function):
    """The found cell's tail + central classifier (+ criterion) as the two launches of csrc/head.hip — K7
    `relu(LayerNorm(cat(states[-M:])))` (model.py:157-160), `central_classifier` (mmimdb_darts_searchable.py:185-188) and,
    inside bmnas.nn.fused_criterion(), the criterion evaluated by the backward launch — instead of cat_ln + linear +
    criterion and their three backward launches.  states: the M concatenated step-node outputs with their per-sample
    sums (CatLnSumsFn).  Returns the logits; the caller attaches K.LAST_HEAD.pop() to them as `_bmnas_head`."""

    @staticmethod
    def forward(ctx, ln_w, ln_b, W, bias, M, *tensors):
        states = [_c(_f32(t)) for t in tensors[:M]]
        sums = [_c(t) for t in tensors[M:2 * M]]
        _require_gpu(states[0], 'found cell head')
        dev = states[0].device
        b, C, L = states[0].shape
        Wc, bc = _c(_f32(W)), _c(_f32(bias))
        O = Wc.shape[0]
        hb_n = _round4(3 * b * O)
        buf = zeros_for_step(hb_n + 4, dev)                   # logits | A | B accumulate with atomics; + the loss scalar
        head = K.HeadState(W=Wc, bias=bc, hb=buf[:3 * b * O].view(3, b, O), loss=buf[hb_n:hb_n + 1],
                           marker=torch.empty((b, O), device=dev, dtype=torch.float32))
        stats = torch.empty(b * 2, device=dev, dtype=torch.float32)
        lw, lb = _c(ln_w), _c(ln_b)
        lib.head_fwd(states, sums, lw, lb, Wc, bc, head.hb, stats, b, C, L, O)
        ctx.states, ctx.sums, ctx.lw, ctx.lb, ctx.stats, ctx.head, ctx.M = states, sums, lw, lb, stats, head, M
        ctx.leaf = all(t.is_leaf for t in (ln_w, ln_b, W, bias))      # (see deferred_affine: only leaves may be deferred)
        K.LAST_HEAD.append(head)
        return head.hb[0]

    @staticmethod
    def backward(ctx, g):
        states, sums, head, M = ctx.states, ctx.sums, ctx.head, ctx.M
        b, C, L = states[0].shape
        O, D = head.W.shape[0], M * C * L
        mode, gten, gscale, labels = head.resolve(g)
        want = any(ctx.needs_input_grad[:4])
        n_chunk = lib.head_chunks(b)
        part = torch.empty(n_chunk * (O + 3) * D, device=states[0].device, dtype=torch.float32) if want else None
        dstates = [torch.empty_like(s) if ctx.needs_input_grad[5 + i] else None for i, s in enumerate(states)]
        lib.head_bwd(states, sums, dstates, 0, ctx.lw, ctx.lb, head.W, head.hb, ctx.stats, mode, gten, gscale, labels,
                     head.loss, part, b, C, L, O, None, crit=head.crit if mode else None)
        dlw = dlb = dW = dbias = None
        if want:
            hsum = torch.empty((O + 3) * D, device=states[0].device, dtype=torch.float32)
            if AFFINE_DEFER is not None and ctx.leaf:
                AFFINE_DEFER.append((None, None, (part, hsum, n_chunk)))      # summed with the pass's affine reductions
            else:
                lib.sum_chunks(part, hsum, n_chunk)
            dW = hsum[:O * D].view(O, D)
            dlw = hsum[O * D:(O + 1) * D].view_as(ctx.lw)
            dlb = hsum[(O + 1) * D:(O + 2) * D].view_as(ctx.lb)
            dbias = hsum[(O + 2) * D:(O + 2) * D + O]
        return (dlw, dlb, dW, dbias, None, *dstates, *([None] * M))


# ----------------------------------------------------------------------------- K3
class SdpaLnFn(Function):
    """ScaledDotAttn.forward (node_operations.py:92-108)."""

    @staticmethod
    def forward(ctx, x, y, ln_w, ln_b, p, training):
        _require_gpu(x, 'scaled-dot attention')
        x, y = _c(_f32(x)), _c(_f32(y))
        b, C, L = x.shape
        out = torch.empty_like(x)
        stats = torch.empty(b * 2, device=x.device, dtype=torch.float32)
        drop = K.DROP.make(p, x.numel(), training)
        lw, lb = _c(ln_w), _c(ln_b)
        xhat = torch.empty_like(x)
        lib.sdpa_ln_fwd(x, y, lw, lb, out, xhat, stats, b, C, L, drop)
        ctx.x, ctx.y, ctx.lw, ctx.stats, ctx.drop, ctx.xhat = x, y, lw, stats, drop, xhat
        ctx.leaf = ln_w.is_leaf and ln_b.is_leaf
        if any(ctx.needs_input_grad):
            ZERO_POOL.announce(2 * lw.numel())
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.x, ctx.y
        b, C, L = x.shape
        dx, dy = torch.empty_like(x), torch.empty_like(y)
        dw, db = _zero_pair(ctx.lw)
        g = _c(g)
        lib.sdpa_ln_bwd(g, None, x, y, ctx.lw, ctx.xhat, ctx.stats, dx, dy, 0, b, C, L, ctx.drop)
        _ln_affine(g, [ctx.xhat], None, None, None, None, dw, db, b, C, L, False, True,
                   key=ctx.lw.data_ptr(), leaf=ctx.leaf)
        return dx, dy, dw, db, None, None


class SdpaLnThruFn(Function):
    """SdpaLnFn whose two inputs are ALSO handed back as outputs: -> (out, x', y'), for a discrete step node that reads
    an inner state again after this op (Found_NodeCell.forward: a later inner step, the out_conv tail, the residual).
    The later readers take the alias, their gradient arrives here as the grad_output of it, and the backward launch
    ACCUMULATES onto that tensor in place (the kernel's accumulate mask) instead of leaving an `at::add` launch to the
    engine — ConvBnActThruFn's arrangement, under the same condition (the arriving gradient is the fresh result of the
    later reader's backward; no retain_grad / hooks on these inner tensors)."""

    @staticmethod
    def forward(ctx, x, y, ln_w, ln_b, p, training):
        out = SdpaLnFn.forward(ctx, x, y, ln_w, ln_b, p, training)
        ctx.set_materialize_grads(False)
        return out, x.view_as(x), y.view_as(y)

    @staticmethod
    def backward(ctx, g, gx, gy):
        if g is None:                       # only the handed-back inputs were differentiated: identity
            return gx, gy, None, None, None, None
        x, y = ctx.x, ctx.y
        b, C, L = x.shape
        onto = lambda t: (t is not None and t.shape == x.shape and t.is_contiguous() and t.dtype == torch.float32
                          and t.device == x.device and t.data_ptr() % 16 == 0)
        dx = gx if onto(gx) else torch.empty_like(x)
        dy = gy if onto(gy) and gy is not gx else torch.empty_like(y)
        acc = (1 if dx is gx else 0) | (2 if dy is gy else 0)
        dw, db = _zero_pair(ctx.lw)
        g = _c(g)
        lib.sdpa_ln_bwd(g, None, x, y, ctx.lw, ctx.xhat, ctx.stats, dx, dy, acc, b, C, L, ctx.drop)
        _ln_affine(g, [ctx.xhat], None, None, None, None, dw, db, b, C, L, False, True,
                   key=ctx.lw.data_ptr(), leaf=ctx.leaf)
        if gx is not None and dx is not gx:
            dx = dx + gx                    # (an arrival that cannot be accumulated onto: the engine's way)
        if gy is not None and dy is not gy:
            dy = dy + gy
        return dx, dy, dw, db, None, None


# ------------------------------------------------------------------ multi-head attention
def mha_runs(roles):
    """The projection GEMMs of a multi-head attention whose q / k / v roles read the unique sources roles[0..2]:
    one per maximal run of CONSECUTIVE roles with the same source -> [(first role, end role, source index)].
    (0, 0, 0): one GEMM with M = 3C; (0, 1, 1): M = C and M = 2C; (0, 1, 2) and (0, 1, 0): three."""
    runs, r0 = [], 0
    for r in range(1, 4):
        if r == 3 or roles[r] != roles[r0]:
            runs.append((r0, r, roles[r0]))
            r0 = r
    return runs


class MhaFn(Function):
    """Attention.forward (reference operations.py:67-86): nn.MultiheadAttention over (b, C, L) tensors, tokens = the L
    positions.  in_proj as bmnas_conv1x1_fwd launches (mha_runs), the per-head core (csrc/mha.hip), out_proj as one
    more; the backward mirrors it launch for launch.  `roles`: for q, k, v the index of its tensor among the unique
    `srcs` — a tensor that plays two roles is passed once and receives ONE gradient, summed by the data-gradient
    launches' accumulate bit instead of by the engine."""

    @staticmethod
    def forward(ctx, heads, p, training, roles, W, bi, Wo, bo, *srcs):
        _require_gpu(srcs[0], 'multi-head attention')
        srcs = [_c(_f32(s)) for s in srcs]
        b, C, L = srcs[0].shape
        dev = srcs[0].device
        W, bi, Wo, bo = _c(W).view(3 * C, C), _c(bi), _c(Wo).view(C, C), _c(bo)
        runs = mha_runs(roles)
        proj, views = [], [None] * 3
        for r0, r1, _ in runs:
            U = torch.empty((b, (r1 - r0) * C, L), device=dev, dtype=torch.float32)
            proj.append(U)
            for r in range(r0, r1):
                views[r] = U[:, (r - r0) * C:(r - r0 + 1) * C]
        O = torch.empty((b, C, L), device=dev, dtype=torch.float32)
        P = torch.empty((b, heads, L, L), device=dev, dtype=torch.float32)
        out = torch.empty((b, C, L), device=dev, dtype=torch.float32)
        drop = K.DROP.make(p, P.numel(), training)
        for (r0, r1, si), U in zip(runs, proj):
            lib.conv1x1_fwd([srcs[si]], C, W[r0 * C:r1 * C], C, bi[r0 * C:r1 * C], U, None, b, L, (r1 - r0) * C)
        lib.mha_core_fwd(views[0], views[1], views[2], O, P, b, C, L, heads, drop)
        lib.conv1x1_fwd([O], C, Wo, C, bo, out, None, b, L, C)
        ctx.heads, ctx.runs, ctx.drop = heads, runs, drop
        ctx.srcs, ctx.W, ctx.Wo, ctx.proj, ctx.views, ctx.O, ctx.P = srcs, W, Wo, proj, views, O, P
        if any(ctx.needs_input_grad):
            ZERO_POOL.announce(4 * C * C + 4 * C)
        return out

    @staticmethod
    def backward(ctx, g):
        srcs, W, Wo, O, P, runs = ctx.srcs, ctx.W, ctx.Wo, ctx.O, ctx.P, ctx.runs
        b, C, L = O.shape
        dev = O.device
        g = _c(g)
        want_w = any(ctx.needs_input_grad[4:8])
        if want_w:
            # the weight gradients are accumulated with atomics: one zero-filled slab, taken before the first launch
            zero = ZERO_POOL.take(4 * C * C + 4 * C, dev)
            dWin, dWo = zero[:3 * C * C].view(3 * C, C), zero[3 * C * C:4 * C * C].view(C, C)
            dbin, dbo = zero[4 * C * C:4 * C * C + 3 * C], zero[4 * C * C + 3 * C:]
        else:
            dWin = dWo = dbin = dbo = None
        dO = torch.empty_like(O)
        dproj, dviews = [], [None] * 3
        for (r0, r1, _), U in zip(runs, ctx.proj):
            dU = torch.empty_like(U)
            dproj.append(dU)
            for r in range(r0, r1):
                dviews[r] = dU[:, (r - r0) * C:(r - r0 + 1) * C]
        dsrcs = [torch.empty_like(s) if ctx.needs_input_grad[8 + i] else None for i, s in enumerate(srcs)]
        lib.conv1x1_bwd_data(g, Wo, C, [dO], C, 0, b, L, C)
        if want_w:
            lib.conv1x1_bwd_weight(g, [O], C, dWo, C, dbo, 0, b, L, C)
        v = ctx.views
        lib.mha_core_bwd(dO, v[0], v[1], v[2], P, dviews[0], dviews[1], dviews[2], b, C, L, ctx.heads, ctx.drop)
        written = set()
        for (r0, r1, si), dU in zip(runs, dproj):
            M = (r1 - r0) * C
            if dsrcs[si] is not None:
                lib.conv1x1_bwd_data(dU, W[r0 * C:r1 * C], C, [dsrcs[si]], C, 1 if si in written else 0, b, L, M)
                written.add(si)
            if want_w:
                lib.conv1x1_bwd_weight(dU, [srcs[si]], C, dWin[r0 * C:r1 * C], C, dbin[r0 * C:r1 * C], 0, b, L, M)
        return (None, None, None, None, dWin, dbin, dWo, dbo, *dsrcs)


# ------------------------------------------------- conv1x1 + BN + {GLU | ReLU} + dropout
class _ZeroPool:
    """Zero-filled scratch for the gradients that the standalone conv + BatchNorm modules accumulate with
    atomics (bn_grad | dW | dbias per module): ONE torch.zeros per backward pass instead of one per module
    (the six reshape layers of a step paid six ~5 us fills).  Forward calls announce their need; the first
    backward call of a pass allocates for all of them — also inside a hipGraph capture, where the fill
    becomes one memset node.  Anything unexpected (a second backward over the same graph, a module that
    never announced) gets its own torch.zeros, as before."""

    def __init__(self):
        self.pending = 0          # floats announced by forwards since the last backward pass began
        self.chunk = None
        self.off = 0
        self.in_backward = False

    def announce(self, n):
        if self.in_backward:      # a new step's forward: the previous pass is over
            self.in_backward, self.pending, self.chunk = False, 0, None
        self.pending += _round4(n)

    def take(self, n, device):
        n = _round4(n)
        cap = device.type == 'cuda' and torch.cuda.is_current_stream_capturing()
        if self.chunk is not None and getattr(self, 'captured', cap) != cap:
            self.chunk, self.in_backward = None, False      # allocated inside / outside a capture that is over
        self.captured = cap
        if not self.in_backward:
            self.in_backward = True
            FWD_STAT_POOL.close()
            # (capped: forwards that were never followed by a backward must not inflate the fill)
            self.chunk = zeros_for_step(max(min(self.pending, 1 << 24), n), device)
            self.off = 0
        if self.chunk is None or self.chunk.device != device or self.off + n > self.chunk.numel():
            return zeros_for_step(n, device)
        v = self.chunk[self.off:self.off + n]
        self.off += n
        return v


ZERO_POOL = _ZeroPool()


class _FwdStatPool:
    """Zero-filled BatchNorm batch-sum buffers (StatArena layout) for the standalone conv + BatchNorm + ReLU
    modules, so that their statistics are finalised inside bn_relu_fwd like on the search path instead of by
    a bn_finalize launch per module.  A forward pass cannot announce its needs, so the chunk is sized by the
    previous pass (a pass ends when a backward pass begins); the first pass, and anything beyond the chunk,
    gets a fill of its own."""
    CAP = 1 << 24                 # floats: never carry more than 64 MB from a run of forwards without backward

    def __init__(self):
        self.open = False
        self.chunk = None
        self.off = 0
        self.total = 0
        self.last_total = 0

    def close(self):              # a backward pass began (called by the first ZERO_POOL.take of the pass)
        if self.open:
            self.open = False
            self.last_total = min(self.total, self.CAP)

    def take(self, M):
        """-> zero-filled view of STAT_SHARDS * M * 2 floats (the interface conv_bn_fwd expects of `stats`)."""
        n = _round4(K.STAT_SHARDS * M * 2)
        dev = self.device
        cap = dev.type == 'cuda' and torch.cuda.is_current_stream_capturing()
        if self.open and getattr(self, 'captured', cap) != cap:
            self.open, self.chunk = False, None             # the pass that opened the chunk belonged to a capture
        self.captured = cap
        if not self.open:
            self.open, self.off, self.total = True, 0, 0
            self.chunk = zeros_for_step(self.last_total, dev) if self.last_total else None
        self.total += n
        if self.chunk is None or self.chunk.device != dev or self.off + n > self.chunk.numel():
            return zeros_for_step(n, dev)
        v = self.chunk[self.off:self.off + n]
        self.off += n
        return v


FWD_STAT_POOL = _FwdStatPool()


def reset_pools():
    """Forget every buffer the two pools hold.  Called when a hipGraph capture aborts: slices handed out inside
    the dead capture point at memory of a released capture pool whose zero-fill node never ran — the next
    eager forward must not be given the rest of that chunk as 'zero-filled' BatchNorm sums."""
    ZERO_POOL.pending, ZERO_POOL.chunk, ZERO_POOL.off, ZERO_POOL.in_backward = 0, None, 0, False
    FWD_STAT_POOL.open, FWD_STAT_POOL.chunk, FWD_STAT_POOL.off, FWD_STAT_POOL.total = False, None, 0, 0
# BMNAS_FUSE_BN_FINALIZE=0: bn_finalize launches, as in round 1
FUSE_STANDALONE_BN = K.FUSE_BN_FINALIZE


# activation -> (forward wrapper, backward wrapper, divisor of the output channels: GLU halves them).  NAMES, looked up in
# bmnas.lib when the launch is issued: lib.profile_begin swaps those module attributes for timed wrappers, which function
# objects bound here at import would bypass
_ACTS = {'glu': ('bn_glu_fwd', 'bn_glu_bwd', 2), 'relu': ('bn_relu_fwd', 'bn_relu_bwd', 1),
         'mish': ('bn_mish_fwd', 'bn_mish_bwd', 1)}


def _conv_bn_front(srcs, conv_w, conv_b, bn_w, bn_b, rm, rv, nbt, training, momentum):
    """The front end of every conv + BatchNorm forward: contiguous fp32 sources, W viewed as (M, K_in), the conv GEMM with
    its batch statistics -> (srcs, U, chan, sv)."""
    srcs = [_c(_f32(s)) for s in srcs]
    C_src = srcs[0].shape[1]
    M = conv_w.shape[0]
    K_in = len(srcs) * C_src
    pool = None
    if training and FUSE_STANDALONE_BN:
        pool = FWD_STAT_POOL             # statistics finalised inside the consumer launch (no bn_finalize launch)
        pool.device = srcs[0].device
    U, chan, sv = K.conv_bn_fwd(srcs, C_src, _c(conv_w).view(M, K_in), K_in, _c(conv_b), _c(bn_w), _c(bn_b), rm, rv, nbt,
                                training, stats=pool, momentum=momentum)
    return srcs, U, chan, sv


def _take_conv_grads(sv):
    """(bn_grad, dW, dbias) of the conv saved in sv: ONE zero-filled buffer for the three gradients that are accumulated
    with atomics, carved out of one fill per backward pass (_ZeroPool)."""
    return conv_grad_split(ZERO_POOL.take(conv_grad_floats(sv.M, sv.ldw), sv.U.device), sv.M, sv.ldw)


def _conv_bn_act_bwd(ctx, g, g_thru=()):
    """The backward of ConvBnActFn and — g_thru: the gradients that arrived for the handed-back sources — of
    ConvBnActThruFn."""
    sv = ctx.sv
    U = sv.U
    b, M, L = U.shape
    _, bwd, div = _ACTS[ctx.act]
    g = _c(g)
    dV = torch.empty_like(U)
    bn_grad, dW, dbias = _take_conv_grads(sv)
    getattr(lib, bwd)(g, U, sv.chan, dV, bn_grad, b, M // div, L, ctx.drop)
    arrived = [g_thru[q] if q < len(g_thru) else None for q in range(len(sv.srcs))]
    slots = []
    for q, (s, gt) in enumerate(zip(sv.srcs, arrived)):
        if not ctx.needs_input_grad[11 + q]:
            slots.append(None)
            continue
        slot = K.GradSlot(s)
        if gt is not None and gt.is_contiguous() and gt.dtype == torch.float32:
            slot.t, slot.written = gt, True          # the later readers' gradient: accumulated onto, in place
        slots.append(slot)
    K.conv_bn_bwd(sv, dV, bn_grad, slots, dW, dbias)
    dsrcs = []
    for slot, gt in zip(slots, arrived):
        d = slot.get() if slot is not None else None
        if slot is not None and gt is not None and d is not gt:
            d = gt if d is None else d + gt          # (a non-contiguous arrival: the engine's way)
        dsrcs.append(d)
    return (None, None, None, None, None, None, None, dW.view(ctx.wshape), dbias, bn_grad[:M], bn_grad[M:], *dsrcs)


class ConvBnActFn(Function):
    """cat(srcs) -> Conv1d(k=1) -> BatchNorm1d -> glu(dim=1) | relu | mish -> Dropout(p).
    LinearGLU (node_operations.py:30-39), ConcatFC (:49-56), CatConvMish (:74-82), NodeCell out_conv
    (node_search.py:59-64).  bn buffers are updated in place in training mode."""

    @staticmethod
    def forward(ctx, act, p, training, rm, rv, nbt, momentum, conv_w, conv_b, bn_w, bn_b, *srcs):
        _require_gpu(srcs[0], 'conv1x1 + BatchNorm')
        if act not in _ACTS:                                 # before anything is launched or a buffer is updated
            raise ValueError(f'conv1x1 + BatchNorm: no kernel for the activation {act!r}')
        fwd, _, div = _ACTS[act]
        srcs, U, chan, sv = _conv_bn_front(srcs, conv_w, conv_b, bn_w, bn_b, rm, rv, nbt, training, momentum)
        b, M, L = U.shape
        out = torch.empty((b, M // div, L), device=U.device, dtype=torch.float32)
        drop = K.DROP.make(p, out.numel(), training)
        getattr(lib, fwd)(U, chan, out, b, M // div, L, drop, sv.fin)
        ctx.act, ctx.sv, ctx.drop, ctx.wshape = act, sv, drop, tuple(conv_w.shape)
        if any(ctx.needs_input_grad):
            ZERO_POOL.announce(conv_grad_floats(M, sv.ldw))
        return out

    @staticmethod
    def backward(ctx, g):
        return _conv_bn_act_bwd(ctx, g)


class ConvBnActThruFn(Function):
    """ConvBnActFn whose sources are ALSO handed back as outputs: -> (out, *srcs).  A discrete step node reads an inner
    state more than once (Found_NodeCell.forward, node.py:45-76: a later inner step, the out_conv tail, the residual); as
    separate autograd nodes every extra reader costs an `at::add` launch when the engine sums the gradients.  Here the
    later readers take the handed-back alias instead, so their gradient arrives as this node's grad_output for it — and
    the data-gradient launch ACCUMULATES onto that tensor in place (the kernels' accumulate mask) instead of writing a
    fresh one for the engine to add.  (The arriving gradient is written in place: it is the fresh result of the later
    reader's backward, which nothing else holds — no retain_grad / hooks on these inner tensors.)"""

    @staticmethod
    def forward(ctx, act, p, training, rm, rv, nbt, momentum, conv_w, conv_b, bn_w, bn_b, *srcs):
        out = ConvBnActFn.forward(ctx, act, p, training, rm, rv, nbt, momentum, conv_w, conv_b, bn_w, bn_b, *srcs)
        ctx.set_materialize_grads(False)
        return (out, *[s.view_as(s) for s in srcs])

    @staticmethod
    def backward(ctx, g, *g_thru):
        if g is None:                       # only the handed-back sources were differentiated: identity
            return (None,) * 11 + tuple(g_thru)
        return _conv_bn_act_bwd(ctx, g, g_thru)


class ConvBnReluLnFn(Function):
    """The tail of a discrete step node with node_multiplier != 1 (Found_NodeCell.forward, node.py:62-76):
        out = LayerNorm_[C, L]( dropout(relu(bn(out_conv(cat(tail))))) + x )
    as the conv GEMM + ONE tail launch per direction (bmnas_bn_relu_ln_fwd / _bwd: the kernels the search path's
    NodeCell ends in) instead of ConvBnActFn + CatLnFn (conv, BatchNorm tail, LayerNorm: one launch more each way).
    -> (out, sums): sums (b, 2) = each sample's (sum, sum of squares) of `out` when want_sums (the fused head's K7
    statistics), else an empty tensor.  Callers check `usable(b, C)` first."""

    @staticmethod
    def usable(b, C):
        return K.FUSE_BN_TAIL and b <= K.BN_TAIL_MAX_B and C <= 1024

    @staticmethod
    def forward(ctx, p, training, want_sums, rm, rv, nbt, momentum, conv_w, conv_b, bn_w, bn_b, ln_w, ln_b, x, *srcs):
        _require_gpu(srcs[0], 'conv1x1 + BatchNorm + LayerNorm tail')
        x = _c(_f32(x))
        srcs, U, chan, sv = _conv_bn_front(srcs, conv_w, conv_b, bn_w, bn_b, rm, rv, nbt, training, momentum)
        b, M, L = U.shape
        o = torch.empty_like(x)                  # dropout(relu(bn(U))), saved for the backward
        out = torch.empty_like(x)
        stats = torch.empty(b * 2, device=x.device, dtype=torch.float32)
        sums = torch.empty((b, 2) if want_sums else (0,), device=x.device, dtype=torch.float32)
        drop = K.DROP.make(p, out.numel(), training)
        lw, lb = _c(ln_w), _c(ln_b)
        lib.bn_relu_ln_fwd(U, chan, x, lw, lb, o, out, stats, b, M, L, drop, sv.fin, sums if want_sums else None)
        ctx.sv, ctx.drop, ctx.wshape, ctx.x, ctx.o, ctx.stats, ctx.lw, ctx.lb = sv, drop, tuple(conv_w.shape), x, o, stats, lw, lb
        ctx.leaf = ln_w.is_leaf and ln_b.is_leaf
        if any(ctx.needs_input_grad):
            ZERO_POOL.announce(conv_grad_floats(M, sv.ldw))
            ZERO_POOL.announce(2 * lw.numel())
        ctx.mark_non_differentiable(sums)
        ctx.set_materialize_grads(False)
        return out, sums

    @staticmethod
    def backward(ctx, g, _g_sums):
        sv = ctx.sv
        n_in = 14 + len(sv.srcs)
        if g is None:
            return (None,) * n_in
        U, x = sv.U, ctx.x
        b, M, L = U.shape
        g = _c(g)
        dV = torch.empty_like(U)
        bn_grad, dW, dbias = _take_conv_grads(sv)
        dx = torch.empty_like(x) if ctx.needs_input_grad[13] else None
        dlw, dlb = _zero_pair(ctx.lw)
        # LayerNorm input gradient, ReLU / dropout mask, BatchNorm reductions and the residual's gradient: one launch
        lib.bn_relu_ln_bwd(g, ctx.o, x, ctx.lw, ctx.stats, U, sv.chan, dV, bn_grad, dx, 0, b, M, L, ctx.drop)
        slots = [K.GradSlot(s) if ctx.needs_input_grad[14 + q] else None for q, s in enumerate(sv.srcs)]
        K.conv_bn_bwd(sv, dV, bn_grad, slots, dW, dbias)
        _ln_affine(g, [ctx.o], x, ctx.lw, ctx.lb, ctx.stats, dlw, dlb, b, M, L, False, False,
                   key=ctx.lw.data_ptr(), leaf=ctx.leaf)
        dsrcs = [s.get() if s is not None else None for s in slots]
        return (None, None, None, None, None, None, None, dW.view(ctx.wshape), dbias, bn_grad[:M], bn_grad[M:], dlw, dlb,
                dx,
                *dsrcs)


POOL_DTYPES = tuple(lib.POOL_DTYPES)      # element types of the pooling launches' inputs: fp32, bf16, fp16


class PoolGroupFn(Function):
    """The AdaptiveMaxPool2d in front of every reshape conv (aux_models.py:62-70, 101-108), all modalities in ONE
    launch per direction (csrc/pool.hip), output in the (b, C_in, L) layout the grouped GEMM reads.
    dims[i] = (C, H, W, oh, ow) of input i viewed as (b, C, H, W).  Inputs are fp32, bf16 or fp16, each its own (the
    feature maps of a backbone under torch.autocast are pooled as they are); the outputs are fp32 — the exact widening
    of the winning elements — and every input's gradient has the input's dtype."""

    @staticmethod
    def forward(ctx, dims, *xs):
        xs = [_c(x if x.dtype in POOL_DTYPES else _f32(x)) for x in xs]
        _require_gpu(xs[0], 'reshape-layer pooling')
        b, dev = xs[0].shape[0], xs[0].device
        outs = [torch.empty((b, d[0], d[3] * d[4]), device=dev, dtype=torch.float32) for d in dims]
        need = any(ctx.needs_input_grad)
        idxs = [torch.empty((b, d[0], d[3] * d[4]), device=dev, dtype=torch.int32) if need else None for d in dims]
        lib.adaptive_maxpool_group(xs, dims, outs, idxs, b)
        ctx.dims, ctx.idxs, ctx.shapes, ctx.b = dims, idxs, [tuple(x.shape) for x in xs], b
        ctx.dtypes = [x.dtype for x in xs]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        sel = [i for i in range(len(gs)) if ctx.needs_input_grad[1 + i]]
        dxs = [None] * len(gs)
        if sel:
            dev = ctx.idxs[sel[0]].device
            g = [torch.zeros_like(ctx.idxs[i], dtype=torch.float32) if gs[i] is None else _c(gs[i]) for i in sel]
            dx = [torch.empty(ctx.shapes[i], device=dev, dtype=ctx.dtypes[i]) for i in sel]
            lib.adaptive_maxpool_group_bwd(g, [ctx.idxs[i] for i in sel], dx, [ctx.dims[i] for i in sel], ctx.b)
            for i, t in zip(sel, dx):
                dxs[i] = t
        return (None, *dxs)


class ReshapeGroupFn(Function):
    """The N reshape layers in front of the fusion cell (ReshapeInputLayer{,_MMIMDB}.forward after the pooling,
    aux_models.py:71-74 / 111-114: Conv1d(C_in_i, C, 1) -> BatchNorm1d(C) -> ReLU -> Dropout(drpt) on each of the
    N pooled modality features) as FOUR launches for the whole group instead of five per layer: grouped GEMM
    (+ BatchNorm batch sums), grouped BN-finalise + ReLU + dropout; grouped activation / BatchNorm-reduction
    backward, grouped weight- and data-gradient GEMMs with the BatchNorm input gradient folded in.
    Same kernels bodies, same arithmetic and same dropout sites (layer 0 first) as N ConvBnActFn calls."""

    @staticmethod
    def forward(ctx, n, p, training, buffers, *tensors):
        xs = [_c(_f32(t)) for t in tensors[:n]]
        _require_gpu(xs[0], 'reshape layers')
        prm = [tensors[n + 4 * i:n + 4 * i + 4] for i in range(n)]          # conv.weight, conv.bias, bn.weight, bn.bias
        b, L = xs[0].shape[0], xs[0].shape[2]
        M = prm[0][0].shape[0]
        dev = xs[0].device
        Ws = [_c(w).view(M, -1) for w, _, _, _ in prm]
        cbs = [_c(cb) for _, cb, _, _ in prm]
        Us = [torch.empty((b, M, L), device=dev, dtype=torch.float32) for _ in range(n)]
        chans = [torch.empty(4 * M, device=dev, dtype=torch.float32) for _ in range(n)]
        stats, shards = None, 0
        if training and b * L < 2:
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {[b, M, L]}')
        # ONE zero-filled buffer for everything the group accumulates with atomics — the forward's BatchNorm
        # batch sums and (when a backward will follow) bn_grad | dW | dbias of every layer — cleared by ONE
        # launch, which under hipGraph capture also advances the dropout step counter: it is the first launch
        # of the step, in front of every dropout site (bmnas.cell._DropState.take_advance)
        per = K.STAT_SHARDS * M * 2 if training else 0
        want_bwd = any(ctx.needs_input_grad)              # (all False when autograd is not recording)
        offs = conv_grad_offsets(M, [W.shape[1] for W in Ws] if want_bwd else [], base=n * per)
        adv = K.DROP.take_advance() if (training and p > 0.0) else None
        pool = torch.empty(offs[-1], device=dev, dtype=torch.float32) if offs[-1] else None
        if pool is not None or adv is not None:
            lib.cell_prologue([], [], [], [], 4, 4, adv, pool)
        if training:
            shards = K.STAT_SHARDS
            stats = [pool[i * per:(i + 1) * per] for i in range(n)]
        ctx.zero = (pool, offs) if want_bwd else None
        lib.conv1x1_fwd_group(xs, Ws, cbs, Us, stats, shards, b, L, M)
        outs = [torch.empty((b, M, L), device=dev, dtype=torch.float32) for _ in range(n)]
        drops = [K.DROP.make(p, outs[i].numel(), training) for i in range(n)]
        fins = [lib.make_bn_fin(None if stats is None else stats[i], shards, cbs[i], _c(prm[i][2]), _c(prm[i][3]),
                                buffers[i][0], buffers[i][1], buffers[i][2], training,
                                momentum=buffers[i][3] if len(buffers[i]) > 3 else 0.1) for i in range(n)]
        lib.bn_relu_fwd_group(Us, chans, outs, fins, drops, b, M, L)
        ctx.n, ctx.xs, ctx.Ws, ctx.Us, ctx.chans, ctx.drops, ctx.training = n, xs, Ws, Us, chans, drops, training
        for i in range(n):
            K.bn_ratio_note(chans[i], cbs[i], M, f'reshape layer {i} ({Ws[i].shape[1]}->{M})', training)
        ctx.wshapes = [tuple(w.shape) for w, _, _, _ in prm]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        n, xs, Ws, Us = ctx.n, ctx.xs, ctx.Ws, ctx.Us
        b, M, L = Us[0].shape
        dev = Us[0].device
        gs = [torch.zeros_like(Us[i]) if g is None else _c(g) for i, g in enumerate(gs)]
        # bn_grad | dW | dbias of every layer: the buffer the forward's first launch cleared (a second backward
        # over the same graph gets a fresh one)
        ldws = [W.shape[1] for W in Ws]
        if ctx.zero is not None:
            zero, offs = ctx.zero
            ctx.zero = None
        else:
            offs = conv_grad_offsets(M, ldws)
            zero = torch.zeros(offs[-1], device=dev, dtype=torch.float32)
        bn_grads, dWs, dbs = map(list, zip(*[conv_grad_split(zero, M, ldw, off) for ldw, off in zip(ldws, offs)]))
        dVs = [torch.empty_like(U) for U in Us]
        lib.bn_relu_bwd_group(gs, Us, ctx.chans, dVs, bn_grads, ctx.drops, b, M, L)
        dxs = [torch.empty_like(x) if ctx.needs_input_grad[4 + i] else None for i, x in enumerate(xs)]
        lib.conv1x1_bwd_group(dVs, Ws, xs, dxs, dWs, dbs, Us, ctx.chans, bn_grads, ctx.training, b, L, M)
        grads = []
        for i in range(n):
            grads += [dWs[i].view(ctx.wshapes[i]), dbs[i], bn_grads[i][:M], bn_grads[i][M:]]
        return (None, None, None, None, *dxs, *grads)


# ---------------------------------------------------------------- mixed-edge sum with FC primitives
FC_KINDS = {'fc_relu': 0, 'fc_mish': 1}


class FcEdgeSumFn(Function):
    """out = sum_j sum_p w[j, p] OPS[prims[p]](x_j) over n states (FusionCell.forward model_search.py:58 /
    NodeCell.forward node_search.py:54 with FusionMixedOp.forward operations.py:104-105) when `prims` — the
    participating primitives, one per column of the weight rows `w` (n, P) — holds one or two of fc_relu / fc_mish
    (operations.py:22-38, 48-65) next to none / skip: three launches forward (zero-fill of the BatchNorm batch sums —
    training only —, grouped GEMM, finalise + weighted sum), four backward (zero-fill, reductions, dU, grouped
    GEMMs), whatever n is.  tensors: the n states, then per edge and FC primitive (list order) linear.weight,
    linear.bias, bn.weight, bn.bias; buffers[j][f] = (running_mean, running_var, num_batches_tracked), updated in
    place in training mode.  One dropout site per (edge, FC primitive), edge by edge, primitives in list order.
    States that are the same tensor object share one gradient (returned for the first of them).
    The pre-activations stay reachable as `out.grad_fn.fc_U` (n, b, F*C, L)."""

    @staticmethod
    def forward(ctx, n, prims, training, p, buffers, w, *tensors):
        xs_in = tensors[:n]
        _require_gpu(xs_in[0], 'mixed-edge sum with FC primitives')
        xs = [_c(_f32(t)) for t in xs_in]
        fcols = [c for c, name in enumerate(prims) if name in FC_KINDS]
        F, P = len(fcols), len(prims)
        skip_cols = sum(1 << c for c, name in enumerate(prims) if name == 'skip')
        if any(name not in FC_KINDS and name not in ('none', 'skip') for name in prims):
            raise ValueError(f'FcEdgeSumFn: unknown primitive in {prims}')
        b, Cc, L = xs[0].shape
        w = _c(_f32(w))
        if tuple(w.shape) != (n, P) or not lib.fc_edges_ok(n, F, P, b, Cc, L):
            raise lib.BmnasError(f'FcEdgeSumFn: unsupported sum (n={n}, prims={prims}, w {tuple(w.shape)}, '
                                 f'x {tuple(xs[0].shape)})')
        if training and b * L < 2:
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {[b, Cc, L]}')
        dev = xs[0].device
        prm = [[[_c(_f32(t)) for t in tensors[n + 4 * (j * F + f):n + 4 * (j * F + f) + 4]] for f in range(F)]
               for j in range(n)]
        U = torch.empty((n, b, F * Cc, L), device=dev, dtype=torch.float32)
        chan = torch.empty((n, F, 4 * Cc), device=dev, dtype=torch.float32)
        stat = None
        if training:
            adv = K.DROP.take_advance() if p > 0.0 else None
            stat = torch.empty((n, F, 2 * Cc), device=dev, dtype=torch.float32)
            lib.fc_edges_zero(stat.view(-1), 'fwd', adv)
        drops = [[K.DROP.make(p, b * Cc * L, training) for _ in range(F)] for _ in range(n)]
        edges = [dict(x=xs[j], U=U[j],
                      fc=[dict(W=prm[j][f][0], bias=prm[j][f][1], bn_w=prm[j][f][2], bn_b=prm[j][f][3],
                               running_mean=buffers[j][f][0], running_var=buffers[j][f][1],
                               num_batches_tracked=buffers[j][f][2], stat=None if stat is None else stat[j, f],
                               chan=chan[j, f], drop=drops[j][f], col=fcols[f], mish=FC_KINDS[prims[fcols[f]]])
                          for f in range(F)]) for j in range(n)]
        arr = lib.make_fc_edges(edges)
        lib.fc_edges_gemm_fwd(arr, F, training, b, Cc, L)
        out = torch.empty_like(xs[0])
        lib.fc_edges_mix_fwd(arr, F, w, P, skip_cols, training, out, b, Cc, L)
        # which states are one tensor object: they share a gradient buffer (NodeCell's states = [sif, sif])
        first = [next(i for i in range(j + 1) if xs_in[i] is xs_in[j]) for j in range(n)]
        ctx.n, ctx.F, ctx.P, ctx.skip_cols, ctx.training = n, F, P, skip_cols, training
        ctx.edges, ctx.w, ctx.first, ctx.fc_U, ctx.fc_chan, ctx.fc_drops = edges, w, first, U, chan, drops
        ctx.wshapes = [[tuple(t.shape) for t in tensors[n + 4 * (j * F + f):n + 4 * (j * F + f) + 2]]
                       for j in range(n) for f in range(F)]
        return out

    @staticmethod
    def backward(ctx, g):
        n, F, P, edges, w = ctx.n, ctx.F, ctx.P, ctx.edges, ctx.w
        g = _c(g)
        b, Cc, L = g.shape
        dev = g.device
        per = 2 * Cc + Cc * Cc + Cc                    # bn_grad | dW | dbias of one (edge, FC primitive)
        head = _round4(n * P)
        pool = torch.empty(head + n * F * per, device=dev, dtype=torch.float32)
        lib.fc_edges_zero(pool, 'bwd')
        dw = pool[:n * P].view(n, P)
        dU = torch.empty_like(ctx.fc_U)
        grads = []
        for j in range(n):
            edges[j]['dU'] = dU[j]
            for f in range(F):
                o = head + (j * F + f) * per
                q = edges[j]['fc'][f]
                q['bn_grad'], q['dW'], q['dbias'] = pool[o:o + 2 * Cc], pool[o + 2 * Cc:o + 2 * Cc + Cc * Cc], \
                    pool[o + 2 * Cc + Cc * Cc:o + per]
                ws, bs = ctx.wshapes[j * F + f]
                grads += [q['dW'].view(ws), q['dbias'].view(bs), q['bn_grad'][:Cc], q['bn_grad'][Cc:]]
        arr = lib.make_fc_edges(edges)
        lib.fc_edges_bwd_reduce(arr, F, w, P, ctx.skip_cols, g, dw, b, Cc, L)
        lib.fc_edges_bwd_du(arr, F, w, P, g, ctx.training, b, Cc, L)
        dxs, targets, masks = [None] * n, [], []
        for j in range(n):
            if ctx.first[j] == j and ctx.needs_input_grad[6 + j]:
                dxs[j] = torch.empty_like(g)
                targets.append(dxs[j])
                masks.append(sum(1 << i for i in range(n) if ctx.first[i] == j))
        lib.fc_edges_bwd_gemm(arr, F, w, P, ctx.skip_cols, g, targets, masks, b, Cc, L)
        return (None, None, None, None, None, dw, *dxs, *grads)


class FoundFcEdgesFn(Function):
    """The E fc_relu / fc_mish edges of a found cell (Found_FusionCell.forward model.py:140-148 calling FC_Relu /
    FC_Mish.forward operations.py:22-65), every edge with an output of its own:
        h_e = Dropout(BatchNorm1d(act_e(Linear_e(x_e)))),   act_e ReLU (kinds[e] = 0) | Mish (1).
    Forward: zero-fill of the BatchNorm batch sums (training only), the grouped GEMM once per kind present (one or
    two launches), finalise + activation + dropout of all edges in one launch.  Backward — called once by autograd,
    when all E output gradients exist —: zero-fill, reductions, dU, grouped GEMMs: four launches whatever E is.
    tensors: the E sources, then per edge linear.weight, linear.bias, bn.weight, bn.bias; buffers[e] =
    (running_mean, running_var, num_batches_tracked), updated in place in training mode.  Sources that are the same
    tensor object share one gradient (returned for the first of them); sources that need no gradient get no
    data-gradient tiles.  The pre-activations stay reachable as `out.grad_fn.fc_U` (E, b, C, L).

    Dropout sites: one per edge, made edge by edge in the order of `tensors` (genotype order).  Found_FusionCell
    evaluates every FC edge that reads a cell input in ONE call in front of its step loop, so the sites of those
    edges all precede the step nodes' sites; the reference runs step i's two edge sites, then step i's node sites.
    The masks are as good as any — nothing depends on the order — but a comparison that injects exported masks into a
    restatement of the reference's execution order has to permute them accordingly."""

    @staticmethod
    def forward(ctx, E, kinds, training, p, buffers, *tensors):
        xs_in = tensors[:E]
        _require_gpu(xs_in[0], 'FC edges of a found network')
        xs = [_c(_f32(t)) for t in xs_in]
        b, Cc, L = xs[0].shape
        if len(kinds) != E or any(k not in (0, 1) for k in kinds) or any(x.shape != xs[0].shape for x in xs) \
                or not lib.fc_edges_ok(E, 1, 1, b, Cc, L):
            raise lib.BmnasError(f'FoundFcEdgesFn: unsupported group (E={E}, kinds={kinds}, '
                                 f'x {[tuple(x.shape) for x in xs]})')
        if training and b * L < 2:
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {[b, Cc, L]}')
        dev = xs[0].device
        prm = [[_c(_f32(t)) for t in tensors[E + 4 * e:E + 4 * e + 4]] for e in range(E)]
        U = torch.empty((E, b, Cc, L), device=dev, dtype=torch.float32)
        chan = torch.empty((E, 4 * Cc), device=dev, dtype=torch.float32)
        stat = None
        if training:
            adv = K.DROP.take_advance() if p > 0.0 else None
            stat = torch.empty((E, 2 * Cc), device=dev, dtype=torch.float32)
            lib.fc_edges_zero(stat.view(-1), 'fwd', adv)
        drops = [K.DROP.make(p, b * Cc * L, training) for _ in range(E)]
        edges = [dict(x=xs[e], U=U[e],
                      fc=[dict(W=prm[e][0], bias=prm[e][1], bn_w=prm[e][2], bn_b=prm[e][3],
                               running_mean=buffers[e][0], running_var=buffers[e][1],
                               num_batches_tracked=buffers[e][2], stat=None if stat is None else stat[e],
                               chan=chan[e], drop=drops[e], col=0, mish=kinds[e])]) for e in range(E)]
        # the GEMM's batch-sum epilogue takes one activation per launch: one launch per kind present
        for kind in (0, 1):
            sub = [edges[e] for e in range(E) if kinds[e] == kind]
            if sub:
                lib.fc_edges_gemm_fwd(lib.make_fc_edges(sub), 1, training, b, Cc, L)
        outs = [torch.empty_like(xs[0]) for _ in range(E)]
        lib.fc_found_fwd(lib.make_fc_edges(edges), training, outs, b, Cc, L)
        first = [next(i for i in range(e + 1) if xs_in[i] is xs_in[e]) for e in range(E)]
        ctx.E, ctx.training, ctx.edges, ctx.first = E, training, edges, first
        ctx.fc_U, ctx.fc_chan, ctx.fc_drops = U, chan, drops
        ctx.wshapes = [[tuple(t.shape) for t in tensors[E + 4 * e:E + 4 * e + 2]] for e in range(E)]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        E, edges, U = ctx.E, ctx.edges, ctx.fc_U
        _, b, Cc, L = U.shape
        dev = U.device
        gs = [torch.zeros_like(U[e]) if g is None else _c(g) for e, g in enumerate(gs)]
        per = 2 * Cc + Cc * Cc + Cc                    # bn_grad | dW | dbias of one edge
        pool = torch.empty(E * per, device=dev, dtype=torch.float32)
        lib.fc_edges_zero(pool, 'bwd')
        dU = torch.empty_like(U)
        grads = []
        for e in range(E):
            o = e * per
            q = edges[e]['fc'][0]
            edges[e]['dU'] = dU[e]
            q['bn_grad'], q['dW'], q['dbias'] = pool[o:o + 2 * Cc], pool[o + 2 * Cc:o + 2 * Cc + Cc * Cc], \
                pool[o + 2 * Cc + Cc * Cc:o + per]
            ws, bs = ctx.wshapes[e]
            grads += [q['dW'].view(ws), q['dbias'].view(bs), q['bn_grad'][:Cc], q['bn_grad'][Cc:]]
        arr = lib.make_fc_edges(edges)
        lib.fc_found_bwd_reduce(arr, gs, b, Cc, L)
        lib.fc_found_bwd_du(arr, gs, ctx.training, b, Cc, L)
        dxs, targets, masks = [None] * E, [], []
        for e in range(E):
            if ctx.first[e] == e and ctx.needs_input_grad[5 + e]:
                dxs[e] = torch.empty_like(gs[0])
                targets.append(dxs[e])
                masks.append(sum(1 << i for i in range(E) if ctx.first[i] == e))
        lib.fc_found_bwd_gemm(arr, targets, masks, b, Cc, L)
        return (None, None, None, None, None, *dxs, *grads)


# ---------------------------------------------------------------- search NodeMixedOp
def _node_mixed_fwd(ctx, fwd, op, training, x, y, gamma_row):
    """The shared forward of NodeMixedFn / NodeMixedSelFn: x and y contiguous fp32 (ONE object when x is y), the op's
    parameter pack, the launch sequence `fwd`."""
    _require_gpu(x, 'NodeMixedOp')
    same = x is y
    x = _c(_f32(x))
    y = x if same else _c(_f32(y))
    out, sv = fwd(x, y, _c(gamma_row), op.pack(), training)
    ctx.op, ctx.sv = op, sv
    return out


def _node_mixed_bwd(ctx, bwd, g, dgamma, G):
    """The shared backward: the input-gradient slots, the launch sequence `bwd`, the attention addend
    -> (dx, dy — None when x is y —, parameter gradients)."""
    sv = ctx.sv
    xs = K.GradSlot(sv.x)
    ys = None if sv.same else K.GradSlot(sv.y)
    bwd(sv, _c(g), dgamma, xs, ys, G)
    dx = xs.get()
    if xs.extra is not None:                 # attention part produced next to the GEMM
        dx = dx.add_(xs.extra) if dx is not None else xs.extra
    return dx, (None if sv.same else ys.get()), ctx.op.grads_in_param_order(G)


class NodeMixedFn(Function):
    """NodeMixedOp.forward(x, y, weights) (node_operations.py:118-120) as one fused
    sequence (attention+LN, stacked conv GEMM + BN statistics, gamma-mix)."""

    @staticmethod
    def forward(ctx, op, training, x, y, gamma_row, *params):
        return _node_mixed_fwd(ctx, K.node_mixed_fwd, op, training, x, y, gamma_row)

    @staticmethod
    def backward(ctx, g):
        dev = ctx.sv.x.device
        G = ctx.op.grad_pack(dev)
        dgamma = torch.zeros(4, device=dev, dtype=torch.float32)
        dx, dy, pgrads = _node_mixed_bwd(ctx, K.node_mixed_bwd, g, dgamma, G)
        if ctx.sv.same:
            dy = torch.zeros_like(dx)            # x and y are the same tensor object: autograd adds both returned halves
        return (None, None, dx, dy, dgamma, *pgrads)


class NodeMixedSelFn(Function):
    """NodeMixedOp.forward(x, y, weights) (node_operations.py:118-120) over an edited STEP_STEP_PRIMITIVES list — a
    subset / permutation of Sum, ScaleDotAttn, LinearGLU, ConcatFC | CatConvMish (op._prims) — as the fused sequence of NodeMixedFn
    restricted to the present terms (bmnas.cell.node_mixed_sel_fwd).  gamma_row / its gradient: len(op._prims)."""

    @staticmethod
    def forward(ctx, op, training, x, y, gamma_row, *params):
        return _node_mixed_fwd(ctx, K.node_mixed_sel_fwd, op, training, x, y, _f32(gamma_row))

    @staticmethod
    def backward(ctx, g):
        op = ctx.op
        # ONE zero fill for everything the launches accumulate into with atomics, dgamma included
        arena = K.Arena()
        h = op.plan_grads(arena)
        hg = arena.ask(len(op._prims))
        arena.alloc(ctx.sv.x.device)
        dgamma = arena.view(hg)
        # x is y: the one tensor's whole gradient is returned for x (autograd skips the None)
        dx, dy, pgrads = _node_mixed_bwd(ctx, K.node_mixed_sel_bwd, g, dgamma, op.bind_grads(arena, h))
        return (None, None, dx, dy, dgamma, *pgrads)


# -------------------------------------------------------------------- fused FusionCell
class FusedCellFn(Function):
    """FusionCell.forward in search mode (model_search.py:50-68 with FusionNode(x, x)):
    the whole cell — mixed edges, step nodes, LayerNorm tail — as one autograd node."""

    @staticmethod
    def forward(ctx, cell, training, alpha_is_logits, alpha, n_head, *tensors):
        """tensors = N inputs, 2*S arch tensors, the cell's parameters and — n_head = 2 — the central
        classifier's weight and bias: the cell then ends in the classifier (bmnas_head_fwd) and the
        function returns the logits."""
        N, S = cell.num_input_nodes, cell._steps
        xs = [_c(_f32(t)) for t in tensors[:N]]
        _require_gpu(xs[0], 'FusionCell')
        dev = xs[0].device
        logits = [_c(t) for t in tensors[N:N + 2 * S]]
        if alpha_is_logits:
            logits = [_c(alpha)] + logits
        ws = [torch.empty_like(t) for t in logits]
        CP = cell.pack()
        # every arch softmax and (search mode: conv applied to cat[z, z]) every NodeMixedOp's folded
        # conv weight in ONE launch
        mixed = [m for n in CP.nodes for m in n.mixed]
        b, C_ = xs[0].shape[0], xs[0].shape[1]
        # forward accumulation arena, zero-filled by the prologue launch: the BatchNorm batch sums that
        # the GEMM epilogues add into (finalised by the mix / out_conv kernels: no bn_finalize
        # launches) and the head's logits | A | B | loss
        counts = []
        K.apply_deterministic()
        # (deterministic mode: the BatchNorm statistics go through per-n-group partials + bn_finalize launches — plain
        # stores combined in a fixed order — instead of atomically accumulated sums)
        if K.FUSE_BN_FINALIZE and not K.DETERMINISTIC:
            for n in CP.nodes:
                counts += [3 * C_] * len(n.mixed) + ([C_] if cell.args.node_multiplier != 1 else [])
        stat_n = K.StatArena.numel_for(counts)
        head, head_n = None, 0
        if n_head:
            Wc, bc = _c(_f32(tensors[-2])), _c(_f32(tensors[-1]))
            O = Wc.shape[0]
            hb_n = _round4(3 * b * O)
            head_n = hb_n + 4
        arena = torch.empty(stat_n + head_n, device=dev, dtype=torch.float32) if stat_n + head_n else None
        stats = K.StatArena(xs[0], counts, arena[:stat_n]) if stat_n else None
        if n_head:
            head = K.HeadState(W=Wc, bias=bc, hb=arena[stat_n:stat_n + 3 * b * O].view(3, b, O),
                               loss=arena[stat_n + hb_n:stat_n + hb_n + 1],
                               marker=torch.empty((b, O), device=dev, dtype=torch.float32))
        weffs, prologue = None, None
        if K.FUSE_PROLOGUE and 0 < len(mixed) <= 8:
            weffs = [torch.empty((3 * C_, C_), device=dev, dtype=torch.float32) for _ in mixed]
            # under capture the first prologue of the step also advances the dropout step counter
            # (bmnas.graph.GraphedStep), saving the separate add launch at the end of every replay
            adv = K.DROP.take_advance()
            stackW = [m.stack_W for m in mixed]
            if (K.FUSE_PROLOGUE_PAIR and K.FUSE_PAIR and alpha_is_logits and N <= 15
                    and logits[0].shape[1] == 2 and logits[1].shape[1] == 2 and logits[1].shape[0] >= 2):
                # the prologue's jobs ride in the launch of the first step's pair sum, which takes
                # its edge weights straight from the alpha / beta logits
                ws_all = ws                          # (`ws` is re-bound below: do not capture the name)

                def prologue(states, sif, z0):
                    lib.cell_prologue_pair(logits, ws_all, stackW, weffs, 3 * C_, C_, adv, arena, states,
                                           logits[0], logits[1], sif, z0)
            else:
                lib.cell_prologue(logits, ws, stackW, weffs, 3 * C_, C_, adv, arena)
        else:
            stats = None                                     # bn_finalize launches (no zero-filled sums)
            if head is not None:
                arena[stat_n:].zero_()
            lib.arch_softmax_multi(logits, None, ws, False)      # every arch tensor, one launch
        if alpha_is_logits:
            alpha_w, ws = ws[0], ws[1:]
        else:
            alpha_w = _c(alpha)
        beta_ws, gamma_ws = ws[0::2], ws[1::2]
        ctx.alpha_is_logits = alpha_is_logits
        out, sv = K.fusion_cell_fwd(xs, alpha_w, beta_ws, gamma_ws, CP, training, S,
                                    cell._multiplier, cell.args.node_steps, cell.args.node_multiplier, weffs,
                                    stats, head, prologue)
        ctx.cell, ctx.sv, ctx.beta_ws, ctx.gamma_ws, ctx.N, ctx.S = cell, sv, beta_ws, gamma_ws, N, S
        ctx.dev, ctx.n_head = dev, n_head
        if head is not None:
            K.LAST_HEAD.append(head)
        return out

    @staticmethod
    def backward(ctx, g):
        cell, sv, N, S = ctx.cell, ctx.sv, ctx.N, ctx.S
        dev = ctx.dev
        need_in = [ctx.needs_input_grad[5 + j] and not K._ARCH_ONLY[0] for j in range(N)]
        # one zero-filled arena for every gradient that is accumulated with atomics
        x0 = sv.states[0]
        CG, dalpha_w, dbeta_ws, dgamma_ws = cell.grad_pack(dev, sv.alpha_w, ctx.beta_ws, ctx.gamma_ws,
                                                           K.arch_shards(x0.shape[0], x0.shape[1], x0.shape[2]))
        ws, dws = [], []
        for i in range(S):
            ws += [ctx.beta_ws[i], ctx.gamma_ws[i]]
            dws += [dbeta_ws[i], dgamma_ws[i]]
        if ctx.alpha_is_logits:
            ws, dws = [sv.alpha_w] + ws, [dalpha_w] + dws
        # does anybody differentiate alpha / beta / gamma?  (a captured weight step does not — its optimizer holds the
        # network weights only, K.weight_grads_only — and the pass then ends without the arch-softmax backward)
        need_arch = ((bool(ctx.needs_input_grad[3]) or any(ctx.needs_input_grad[5 + N:5 + N + 2 * S]))
                     and not K._NO_ARCH[0])
        if not need_arch:
            ws, dws = [], []
        darch = [torch.empty_like(w) for w in ws]
        # does ANY parameter of the cell / the fused classifier need its gradient?  (a captured architecture step
        # says no: K.arch_grads_only)
        first_param = 5 + N + 2 * S
        want = any(ctx.needs_input_grad[first_param:]) and not K._ARCH_ONLY[0]
        saved, K.WANT_PARAM_GRADS = K.WANT_PARAM_GRADS, want
        saved_arch, K.WANT_ARCH_GRADS = K.WANT_ARCH_GRADS, need_arch
        try:
            dxs = K.fusion_cell_bwd(sv, g if sv.head is not None else _c(g), need_in, dalpha_w, dbeta_ws, dgamma_ws,
                                    CG, (ws, dws, darch))
        finally:
            K.WANT_PARAM_GRADS = saved
            K.WANT_ARCH_GRADS = saved_arch
        if not sv.epilogue_done and need_arch:
            lib.arch_softmax_multi(ws, dws, darch, True, CG.shards, CG.shard_stride)
        if not need_arch:
            dalpha, darch = None, [None] * (2 * S)
        elif ctx.alpha_is_logits:
            dalpha, darch = darch[0], darch[1:]
        else:
            # the caller owns the alpha softmax: hand back the sum of the atomic shards
            dalpha = torch.as_strided(dalpha_w, (CG.shards, *dalpha_w.shape),
                                      (CG.shard_stride, *dalpha_w.stride()),
                                      dalpha_w.storage_offset()).sum(0)
        head_grads = (sv.head.dW, sv.head.dbias) if ctx.n_head else ()
        pgrads = cell.grads_in_param_order(CG) if want else [None] * len(cell.param_list())
        return (None, None, None, dalpha, None, *dxs, *darch, *pgrads, *head_grads)


# ------------------------------------------------------- classifier + criterion epilogue
class LinearFn(Function):
    """F.linear(feat, W, bias) for the skinny central classifier (classes <= 128)."""

    @staticmethod
    def forward(ctx, feat, W, bias):
        _require_gpu(feat, 'central classifier')
        feat, W, bias = _c(_f32(feat)), _c(_f32(W)), _c(bias)
        b, Kd = feat.shape
        O = W.shape[0]
        # the k-slices add into `out`: zero-filled by the captured step's arena where there is one (no fill launch)
        if _ARENA_NEED is not None:
            _ARENA_NEED[0] += _round4(b * O)
        pre = _ARENA.take(b * O) if (_ARENA is not None and _ARENA.buf.device == feat.device) else None
        out = pre.view(b, O) if pre is not None else torch.empty((b, O), device=feat.device, dtype=torch.float32)
        lib.linear_fwd(feat, W, bias, out, b, O, Kd, out_is_zero=pre is not None)
        ctx.save_for_backward(feat, W)
        return out

    @staticmethod
    def backward(ctx, g):
        feat, W = ctx.saved_tensors
        b, Kd = feat.shape
        O = W.shape[0]
        need = ctx.needs_input_grad
        dfeat = torch.empty_like(feat) if need[0] else None
        dW = torch.empty_like(W) if need[1] else None
        db = torch.empty(O, device=feat.device, dtype=torch.float32) if need[2] else None
        lib.linear_bwd(_c(g), None, feat, W, dfeat, dW, db, b, O, Kd)
        return dfeat, dW, db


_UNIT = {}


def unit_grad(device):
    """A cached 0-dim tensor holding 1.0 to pass as `grad_outputs` / `loss.backward(gradient=...)`.
    autograd otherwise launches a fill kernel for ones_like(loss) and our loss functions a multiply
    by it; when the incoming gradient IS this constant the criterion hands its stored dloss/dlogits
    back untouched (two ~4 us launches less per step; same numbers)."""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    t = _UNIT.get(key)
    if t is None:
        t = _UNIT[key] = torch.ones((), device=f'{key[0]}:{key[1]}', dtype=torch.float32)
    return t


class _LossFn(Function):
    """mean loss with dloss/dlogits produced in the forward pass."""

    @staticmethod
    def _finish(ctx, loss, dz):
        ctx.save_for_backward(dz)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        (dz,) = ctx.saved_tensors
        u = _UNIT.get((gl.device.type, gl.device.index))
        if u is not None and gl.data_ptr() == u.data_ptr():
            return dz, None                      # gradient of the loss is the constant 1
        return dz * gl, None


class DeferredLossFn(Function):
    """The criterion of a fused head, evaluated by the head's BACKWARD launch (bmnas_head_bwd modes
    1 / 2): forward only records kind and labels and hands out the loss scalar that the backward
    will fill — valid once backward has run, which is all a captured step needs (nothing can read a
    value between two nodes of a hipGraph).  Enabled by bmnas.nn.fused_criterion().  crit: the lib.Criterion of a
    weighted / smoothed criterion (bmnas_head_bwd_crit; its weight tensors are read, by address, when the backward
    launch runs), None for the bare mean form."""

    @staticmethod
    def forward(ctx, z, target, head, kind, crit=None):
        if head.deferred is not None:
            raise lib.BmnasError('fused criterion: a second criterion on the same logits (the head evaluates ONE '
                                 'criterion in its backward launch); call it outside bmnas.nn.fused_criterion()')
        head.deferred = (kind, target if target.is_contiguous() else target.contiguous())
        head.crit = crit
        head.gscale = None
        ctx.head = head
        return head.loss.view(())

    @staticmethod
    def backward(ctx, gl):
        head = ctx.head
        u = _UNIT.get((gl.device.type, gl.device.index))
        if not (u is not None and gl.data_ptr() == u.data_ptr()):
            head.gscale = gl.contiguous().float()          # d(loss)/d(loss) other than the constant 1
        return head.marker, None, None, None, None


class BCEWithLogitsFn(_LossFn):
    @staticmethod
    def forward(ctx, z, y):
        _require_gpu(z, 'BCEWithLogits loss')
        z, y = _c(_f32(z)), _c(_f32(y))
        loss = torch.empty(1, device=z.device, dtype=torch.float32)
        dz = torch.empty_like(z)
        lib.bce_logits(z, y, loss, dz)
        return _LossFn._finish(ctx, loss, dz)


class CrossEntropyFn(_LossFn):
    @staticmethod
    def forward(ctx, z, label):
        _require_gpu(z, 'CrossEntropy loss')
        z = _c(_f32(z))
        b, O = z.shape
        loss = torch.empty(1, device=z.device, dtype=torch.float32)
        dz = torch.empty_like(z)
        rows = torch.empty(b, device=z.device, dtype=torch.float32)
        lib.cross_entropy(z, label.contiguous(), loss, dz, rows, b, O)
        return _LossFn._finish(ctx, loss, dz)


class BCEWithLogitsCritFn(_LossFn):
    """BCEWithLogits with per-class weight / pos_weight and reduction mean | sum (bmnas_bce_logits_crit)."""

    @staticmethod
    def forward(ctx, z, y, crit):
        _require_gpu(z, 'BCEWithLogits loss')
        z, y = _c(_f32(z)), _c(_f32(y))
        loss = torch.empty(1, device=z.device, dtype=torch.float32)
        dz = torch.empty_like(z)
        O = z.shape[-1]
        lib.bce_logits_crit(z, y, crit, loss, dz, z.numel() // O, O)
        ctx.save_for_backward(dz)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        return (*_LossFn.backward(ctx, gl), None)


class CrossEntropyCritFn(_LossFn):
    """CrossEntropy with class weights, label smoothing, ignore_index and reduction mean | sum
    (bmnas_cross_entropy_crit)."""

    @staticmethod
    def forward(ctx, z, label, crit):
        _require_gpu(z, 'CrossEntropy loss')
        z = _c(_f32(z))
        b, O = z.shape
        loss = torch.empty(1, device=z.device, dtype=torch.float32)
        dz = torch.empty_like(z)
        rows = torch.empty(b, device=z.device, dtype=torch.float32)
        lib.cross_entropy_crit(z, label.contiguous(), crit, loss, dz, rows, b, O)
        ctx.save_for_backward(dz)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        return (*_LossFn.backward(ctx, gl), None)
