"""torch.optim.Adam with the update of every tensor in one HIP launch.

Drop-in for the two optimizers of the search loop (reference mmimdb_darts_searchable.py:28-33:
`Adam(central_params, lr=eta_max, weight_decay=wd)` and `Adam(arch_parameters, betas=(0.5, 0.999),
weight_decay=arch_wd)`): same constructor, same `param_groups`, same `state` layout (`step`,
`exp_avg`, `exp_avg_sq` per parameter, so `state_dict()` / `load_state_dict()` interoperate with
torch.optim.Adam checkpoints), same arithmetic operation by operation.  What changes is the
execution: the step-dependent scalars are computed on the host in double (as torch does), written
with the tensor descriptors into ONE pinned staging buffer, copied to the device with one async
H2D copy, and one `bmnas_adam_multi` launch updates every tensor (torch's foreach path: ~10
launches per parameter group).  Because all per-step values travel through the staging buffer,
a step captured in a hipGraph replays correctly: `prepare_replay()` before each replay.

`Adam(..., max_grad_norm=c)` clips the global L2 norm of the gradients inside the step — what
`torch.nn.utils.clip_grad_norm_(all parameters, c)` between backward() and step() computes (DARTS'
`--grad_clip`), captured steps included: one norm launch (`bmnas_grad_sqnorm_multi`) in front of the
clipped update (`bmnas_adam_multi_clip`).  The update scales each gradient in registers: `.grad` is
NOT written and keeps the unclipped values.  `clip_grad_norm_` below is the stand-alone, in-place form.

`Adam(..., amsgrad=True)` and `Adam(..., decoupled_weight_decay=True)` / `AdamW` are torch's two switches, kept in
torch's own `param_groups` keys (so a torch.optim.AdamW or amsgrad checkpoint loads and is honoured) and run by the same
single launch (`bmnas_adam_multi_ex`; with both off the launches are `bmnas_adam_multi` / `bmnas_adam_multi_clip` as
before).  AMSGrad keeps torch's per-parameter `max_exp_avg_sq`; its pointers ride behind the descriptor table in the
staging buffer.  Decoupled decay stages float(1 - lr * weight_decay) where the L2 mode stages weight_decay.  One launch
is one kernel instantiation: all groups of an optimizer must agree on each switch.

`SGD` is torch.optim.SGD (momentum, dampening, nesterov, L2 weight decay; DARTS' weight optimizer, reference
models/search/darts/train_search.py:84-88) on the same machinery: the descriptor table, chunk list, staging buffer,
by-value scalar rows and norm launch are Adam's, the update is one `bmnas_sgd_multi` launch, and `max_grad_norm` means
what it means for Adam.  `_OneLaunch` holds what the two classes share — the plan builder over `staging_layout` (the one
place that knows the staging buffer's byte offsets), the switch between plans, the copy and norm launch that open a step,
the refusals that open `prepare_replay` —; each class says which state tensors a descriptor points at (`_state_ptrs`),
what keys a scalar row (`_row_count`) and what it holds (`prepare_replay`), which entries of the plan are its own
(`_plan_fields`) and which launch updates (`_update`).

Every plan of this file — the optimizers', `UnrolledStep`'s, `GradAccumulator`'s, `AveragedModel`'s — keeps what it stages
in one `_Staging`: the pinned buffer, its device copy, the one async copy between them and the event that keeps the host
from rewriting the pinned bytes before that copy has read them (explained there, once).  The bytes are laid out by
`staging_layout`, the (tensor, chunk) list every launch walks comes from `_chunk_pairs`.

`UnrolledStep` (beside `clip_grad_norm_`, at the end) is no optimizer: it holds the weight-side arithmetic of DARTS'
unrolled architecture step — virtual weight step, +-R perturbation, restore, and the combine over alpha — on the kernels
of csrc/unroll.hip, over the same descriptor table, chunk list and norm launch, reading a weight optimizer's groups and
momentum buffers without writing them.

`AveragedModel` (last) is torch.optim.swa_utils.AveragedModel — EMA / SWA of a model's tensors — with the update as one
`bmnas_avg_multi` launch (csrc/average.hip) over the same descriptor table and chunk list, `param` the averaged tensor and
`grad` the live one, and no host synchronisation; inside a captured step its scalar rows ride behind the optimizer's
(`staging_layout(extra_bytes=...)`, `capture_safe(extra=...)`, `rider_rows()`).

`GradAccumulator` (in front of `AveragedModel`) sums up to `lib.accum_max()` micro-batch gradients per tensor into a
persistent `.grad` with ONE `bmnas_grad_combine_multi` launch (csrc/accum.hip) per optimizer step, eager and captured;
`accum_weights` gives the n_i / N weights that make m micro-batches the gradient of their union.

`update_bn` (after it) is torch.optim.swa_utils.update_bn for the native BatchNorm kernels: one cumulative-statistics pass
over a loader (BatchNorm momentum None), optionally as replays of one captured forward.  BatchNorm momentum is read when
a launch is issued: like Adam's switches it may change between eager steps, but a captured plan (GraphedTrainStep,
GraphedForward) keeps the momentum it was captured under — a float is baked into the graph, None replays correctly
because the factor comes from the device counter.
"""
import collections
import math
import weakref

import numpy as np
import torch

from . import lib

# bmnas_adam_tensor_t (include/bmnas_hip.h)
_DESC = np.dtype([('param', '<u8'), ('grad', '<u8'), ('exp_avg', '<u8'), ('exp_avg_sq', '<u8'),
                  ('numel', '<i8'), ('hyp_row', '<i4'), ('reserved', '<i4')])
assert _DESC.itemsize == 48


StagingLayout = collections.namedtuple(
    'StagingLayout', 'row_bytes hyp_slot hyp_bytes tab_bytes tab_slot nbytes rows_at clip_at tab_at tail_at extra_at')


def staging_layout(n_rows, n_tensors, slots=1, clip=False, tail_ptrs_per_tensor=0, extra_bytes=0):
    """The byte offsets of a plan's ONE staging buffer (pinned, and its device copy) — the one place that knows them; they
    are baked into captured graphs, into the poke-mode blob and into what the kernels read behind a descriptor table.

        scalar region   per slot: n_rows rows of 8 floats (32 bytes each), then — when clipping — max_grad_norm in 16
                        bytes of its own (the next slot's rows stay 16-byte aligned).  The slots are packed back to back:
                        the whole region travels by value in poke mode.  Behind the last slot, `extra_bytes` (a multiple
                        of 32; 0: nothing, every offset is what it is without) for a rider's rows — the scalar rows of
                        a bmnas.optim.AveragedModel updated in the same captured step —, which so travel with the
                        optimizer's.  Rounded up to 64 bytes (`hyp_bytes`).
        table region    per slot: n_tensors descriptors of 48 bytes (bmnas_adam_tensor_t) — the table is shared with the
                        norm launch and stays 48 bytes per tensor —, then 8 * tail_ptrs_per_tensor bytes per tensor
                        (AMSGrad: one `float*` per descriptor, max_exp_avg_sq), which so travel with the table's upload.

    slots > 1: a captured graph that holds `slots` consecutive optimizer steps (bmnas.graph.GraphedTrainStep(k=...)): every
    step has its own scalar rows and its own descriptor table (each step's backward leaves its gradients in tensors of
    its own).  -> sizes (`hyp_slot`, `tab_slot`: a slot's stride in its region) and, per slot, where its rows, its clip
    scalar (None without clipping), its table and its tail pointers start.

    The other plans are cases of it: UnrolledStep's is a clipped one-slot plan with (r, eta) where max_grad_norm goes and
    the alpha table behind `nbytes`; GradAccumulator's has no rows and its part pointers as the tail; AveragedModel's has
    no rows but a rider's — its own, or none when they ride in an optimizer's buffer.  The last two keep their chunk list
    in the same buffer, at `_chunks_at`."""
    row_bytes = n_rows * 32
    hyp_slot = row_bytes + (16 if clip else 0)
    if extra_bytes < 0 or extra_bytes % 32:
        raise ValueError('staging_layout: extra_bytes must be a non-negative multiple of 32')
    hyp_bytes = (slots * hyp_slot + extra_bytes + 63) // 64 * 64
    tab_bytes = n_tensors * _DESC.itemsize
    tab_slot = tab_bytes + n_tensors * 8 * tail_ptrs_per_tensor
    rows_at = [i * hyp_slot for i in range(slots)]
    tab_at = [hyp_bytes + i * tab_slot for i in range(slots)]
    return StagingLayout(row_bytes, hyp_slot, hyp_bytes, tab_bytes, tab_slot, hyp_bytes + slots * tab_slot, rows_at,
                         [o + row_bytes for o in rows_at] if clip else None, tab_at, [o + tab_bytes for o in tab_at],
                         slots * hyp_slot)


def _chunks_at(lay):
    """Where the chunk list of a plan that keeps it INSIDE its staging buffer starts: behind the layout, 16-byte aligned."""
    return (lay.nbytes + 15) // 16 * 16


def _chunk_pairs(numels):
    """-> int32 array (n, 2): one (tensor index, chunk index) per workgroup of a multi-tensor launch over tensors of
    `numels` elements (an empty tensor takes none)."""
    E = lib.adam_chunk_elems()
    return np.array([(i, c) for i, n in enumerate(numels) for c in range((n + E - 1) // E)],
                    dtype=np.int32).reshape(-1, 2)


def _chunk_list(numels, device):
    """-> (int32 tensor (n, 2) on `device`, n): `_chunk_pairs` as a device tensor of its own."""
    pairs = _chunk_pairs(numels)
    return torch.from_numpy(pairs).to(device), len(pairs)


class _Staging:
    """A plan's pinned staging buffer (`pin`, `host` its numpy view) and its device copy (`dev`).  Whatever a plan stages
    — descriptor tables, scalar rows, pointers, a chunk list — goes up in ONE async H2D copy.  The copy reads the pinned
    bytes when the stream gets there, not when it is issued, and the host may run ahead of the GPU: `mark()` records an
    event behind the copy, `wait()` blocks on it, and nobody rewrites `host` without `wait()` first — rewriting earlier
    would silently change a step still in flight.  `upload()` is the whole sequence for plans whose bytes often repeat:
    it is skipped when `host` equals `sent`, the bytes the device already holds."""

    def __init__(self, nbytes, device):
        self.pin = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
        self.host = self.pin.numpy()
        self.dev = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.event = None
        self.sent = None

    def wait(self):
        """Block until the last marked copy has read the pinned buffer (at once when there was none)."""
        if self.event is not None:
            self.event.synchronize()

    def copy(self):
        """The bare copy: stream work only, so it can be captured in a graph."""
        self.dev.copy_(self.pin, non_blocking=True)

    def mark(self):
        """Record, on the current stream, that everything queued so far has read the pinned buffer."""
        if self.event is None:
            self.event = torch.cuda.Event()
        self.event.record()

    def upload(self):
        """copy() + mark(), unless the device already holds exactly these bytes; -> whether a copy was issued."""
        if self.sent is not None and np.array_equal(self.sent, self.host):
            return False
        self.copy()
        self.mark()
        self.sent = self.host.copy()
        return True


def _param_device(params, name):
    """-> the one GPU `params` live on; refuses, in `name`'s name, what the kernels cannot take."""
    dev = params[0].device
    for p in params:
        if not p.is_cuda:
            raise lib.BmnasError(f'{name} needs parameters on the GPU (HIP kernel, no CPU path)')
        if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
            raise lib.BmnasError(f'{name}: parameter must be contiguous fp32 on {dev}')
    return dev


def _check_like(t, p, name, what):
    """Refuse, in `name`'s name, a tensor (`what` in the message) that a launch could not read or write beside p."""
    if (not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != p.device
            or t.numel() != p.numel()):
        raise lib.BmnasError(f"{name}: {what} must be contiguous fp32 on the parameter device, of the parameter's size")


class _OneLaunch:
    """What bmnas.optim.Adam and bmnas.optim.SGD share: the plan and its builder (`_build`, over `staging_layout`), the
    eager step over a plan, the captured plan and its replay protocol (capture_safe / captured_plan / activate /
    prepare_replay / replay_blob / wait_staging / mark_launched), switching between plans, and max_grad_norm.  A plan's
    scalars change with every step, so it never takes `_Staging.upload()`'s short-cut: a step is wait_staging(), the bare
    `copy()` in `_launch` (which a capture turns into the graph's copy node) and mark_launched().  Mixed in
    FRONT of the torch optimizer class.  The class supplies `_NAME`, `_SHARED` (what the tensors of a row share, for
    `_switch`'s refusal), `_variant()` (the key of a plan: clipping first, then `_switches()`), `_row_count(p, switches)`
    (a tensor's row count as the state has it now), `_plan_fields(switches)`, `_state_ptrs(plan)`, `_update(...)` (the
    launch of the update) and `prepare_replay(slot)`."""

    def _init_one_launch(self, max_grad_norm):
        self.max_grad_norm = max_grad_norm
        self._clip_value()
        self._plan = None
        self._eager_plan = None
        self._gen = 0            # bumped whenever the state tensors are replaced (load_state_dict)
        self._touch = 0          # bumped by everything that may re-point .grad or move the step counts outside a replay

    def _state_replaced(self):
        """After load_state_dict(): the state tensors are new objects (or gone) — eager steps rebuild their plan, a captured
        plan (held by its GraphedTrainStep) re-reads pointers and counts in activate()."""
        self._plan = None
        self._eager_plan = None
        self._gen += 1

    def _clip_value(self):
        """max_grad_norm as a float (validated), or None."""
        c = self.max_grad_norm
        if c is None:
            return None
        if isinstance(c, bool) or not isinstance(c, (int, float)) or not c > 0:
            raise lib.BmnasError(f'{self._NAME}: max_grad_norm must be None or a positive float, got {c!r}')
        return float(c)

    @property
    def grad_norms(self):
        """The pre-clip gradient norm of every step of the current plan's most recent launch / replay: fp32 device tensor
        of `slots` entries (1 for an eager step, k for a k-step captured plan); None without clipping.  Reading it
        queues no synchronisation of its own."""
        pl = self._plan
        return pl['norms'] if pl is not None and pl.get('clip') else None

    @property
    def last_grad_norm(self):
        """0-dim fp32 device tensor: the pre-clip norm of the most recent step (a view of grad_norms' last entry)."""
        n = self.grad_norms
        return None if n is None else n[-1]

    # ------------------------------------------------------------------ plan
    def _active(self):
        return [(p, gi) for gi, g in enumerate(self.param_groups) for p in g['params'] if p.grad is not None]

    def _flush_counts(self):
        """Write the plan's row counts back into the optimizer's state, where the state keeps them (Adam's `step`)."""

    def _build(self, active, slots=1, extra=0):
        """The plan of `slots` consecutive steps over `active`, in ONE staging buffer (staging_layout).  Tensors of one group
        with the same `_row_count` share a row of scalars; `count` of a row is that count, advanced by prepare_replay().
        extra: bytes behind the scalar rows for a rider (capture_safe)."""
        key = self._variant()
        clip, sw = key[0], key[1:]
        self._flush_counts()
        dev = _param_device([p for p, _ in active], self._NAME)
        rows, row_idx, row_of = [], {}, []
        for p, gi in active:
            rk = (gi, self._row_count(p, sw))
            if rk not in row_idx:
                row_idx[rk] = len(rows)
                rows.append(rk)
            row_of.append(row_idx[rk])
        fields, tail = self._plan_fields(sw)
        lay = staging_layout(len(rows), len(active), slots, clip, tail, extra)
        stage = _Staging(lay.nbytes, dev)
        host, devbuf = stage.host, stage.dev
        tabs = [host[o:o + lay.tab_bytes].view(_DESC) for o in lay.tab_at]
        for tab in tabs:
            tab['numel'] = [p.numel() for p, _ in active]
            tab['hyp_row'] = row_of
        hyps = [host[o:o + lay.row_bytes].view(np.float32).reshape(len(rows), 8) for o in lay.rows_at]
        chunks, n_chunks = _chunk_list([p.numel() for p, _ in active], dev)
        self._plan = dict(ids=tuple(id(p) for p, _ in active), active=active, row_of=row_of, gen=self._gen,
                          groups=[gi for gi, _ in rows], count=[c for _, c in rows],
                          # hyp_all: what a replay carries by value — every slot's scalar rows and, behind them, a rider's
                          # `extra` bytes (an AveragedModel's rows; none: the optimizer's rows alone, as ever)
                          stage=stage, hyp=hyps[0], hyps=hyps, hyp_all=host[:lay.extra_at + extra], tabs=tabs,
                          extra=host[lay.extra_at:lay.extra_at + extra],
                          dev_extra=devbuf[lay.extra_at:lay.extra_at + extra], dev_hyp=devbuf[:lay.hyp_bytes],
                          dev_hyps=[devbuf[o:o + lay.hyp_slot] for o in lay.rows_at],
                          dev_tabs=[devbuf[o:o + lay.tab_bytes] for o in lay.tab_at],
                          chunks=chunks, n_chunks=n_chunks, slots=slots, cap_slot=0, clip=clip, key=key, **fields)
        if tail:                 # (Adam's running maxima)
            size = lay.tab_slot - lay.tab_bytes
            self._plan.update(maxes=[host[o:o + size].view('<u8') for o in lay.tail_at],
                              dev_maxes=[devbuf[o:o + size] for o in lay.tail_at])
        self._state_ptrs(self._plan)
        if clip:
            # the norm launch's partials, the max_grad_norm scalars (host + device view) and the norm outputs belong to the
            # plan: a captured plan's graph reads and writes these addresses for good
            parts = lib.grad_norm_parts()
            self._plan.update(
                n_parts=min(n_chunks, parts),
                partials=[torch.empty(parts, dtype=torch.float32, device=dev) for _ in range(slots)],
                clips=[host[o:o + 4].view(np.float32) for o in lay.clip_at],
                dev_clips=[devbuf[o:o + 4] for o in lay.clip_at],
                norms=torch.zeros(slots, dtype=torch.float32, device=dev))

    def _switch(self, plan):
        """Make `plan` current: the row counts are re-read from the state (`_row_count`), the state pointers when
        load_state_dict() replaced the state tensors."""
        if self._plan is not plan:
            self._flush_counts()
            counts = {}
            for (p, _), r in zip(plan['active'], plan['row_of']):
                c = self._row_count(p, plan['key'][1:])
                if counts.setdefault(r, c) != c:
                    raise lib.BmnasError(f'{self._NAME}: parameters that shared {self._SHARED} when this plan was built '
                                         'have diverged (an eager step on a subset?); re-capture the graph')
            for r, c in counts.items():
                plan['count'][r] = c
            self._plan = plan
        if not plan.get('poke'):
            self.wait_staging()              # the plan's last launch has consumed its pinned buffer
        if plan['gen'] != self._gen:
            self._state_ptrs(plan)
            plan['gen'] = self._gen

    def _begin_replay(self, slot, switched):
        """What opens prepare_replay(): refuse a plan built for other launches than the optimizer now asks for, and stage
        max_grad_norm.  switched: the class' words for its switches having changed."""
        pl = self._plan
        c = self._clip_value()
        if (c is not None) != pl['clip']:
            raise lib.BmnasError(f'{self._NAME}: max_grad_norm was switched between None and a value under a plan built '
                                 'for the other (a captured step holds the launches of one of them); re-capture the graph')
        if self._switches() != pl['key'][1:]:
            raise lib.BmnasError(f'{self._NAME}: {switched} under a plan built for the other value (a captured step holds '
                                 'the launches of one of them); re-capture the graph')
        if c is not None:
            pl['clips'][slot][0] = c

    def _launch(self, slot=0):
        pl = self._plan
        if not pl.get('poke') and slot == 0:
            pl['stage'].copy()               # (captured: one copy node serves every slot of the graph)
        args, clip_args = (pl['dev_tabs'][slot], pl['chunks'], pl['n_chunks'], pl['dev_hyps'][slot]), ()
        if pl['clip']:
            lib.grad_sqnorm_multi(pl['dev_tabs'][slot], pl['chunks'], pl['n_chunks'], pl['partials'][slot])
            clip_args = (pl['partials'][slot], pl['n_parts'], pl['dev_clips'][slot], pl['norms'][slot:slot + 1])
        self._update(pl, slot, args, clip_args)

    def _stage(self, active):
        """Advance the step counts; write this step's scalars and pointers into the staging buffer."""
        self.prepare_replay()
        self._write_ptrs(active)

    def _write_ptrs(self, active, slot=0):
        grads = [p.grad for p, _ in active]
        for gr, (p, _) in zip(grads, active):
            if gr.dtype != torch.float32 or not gr.is_contiguous() or gr.device != p.device:
                raise lib.BmnasError(f'{self._NAME}: gradients must be contiguous fp32 on the parameter device')
        tab = self._plan['tabs'][slot]
        tab['param'] = [p.data_ptr() for p, _ in active]
        tab['grad'] = [gr.data_ptr() for gr in grads]

    def wait_staging(self):
        """Block until the last launch has consumed the current plan's pinned staging buffer (`_Staging.wait`)."""
        stage = None if self._plan is None else self._plan.get('stage')
        if stage is not None:
            stage.wait()

    def mark_launched(self, force=False):
        """Record, on the current stream, that everything queued so far (a step() or a graph
        replay that contains one) has read the staging buffer.  (Poke-mode plans: their replays do not read it —
        nothing to record, and nothing for the next call to wait for: the host may run ahead of the GPU.)"""
        pl = self._plan
        if pl.get('poke') and not force:
            return
        pl['stage'].mark()

    # ------------------------------------------------------------------ torch.optim API
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        active = self._active()
        if not active:
            return loss
        key = self._variant()                   # (first: groups that disagree on a switch are refused before anything moves)
        self._touch += 1
        if torch.cuda.is_current_stream_capturing():
            if self._plan is None or self._plan['ids'] != tuple(id(p) for p, _ in active) or self._plan['key'] != key:
                raise lib.BmnasError(f'{self._NAME}: call capture_safe() before capturing step() in a graph')
            slot = self._plan['cap_slot']
            if slot >= self._plan['slots']:
                raise lib.BmnasError(f'{self._NAME}: more captured steps than capture_safe(slots=...) planned')
            self._write_ptrs(active, slot)      # the capture's static gradient tensors (of THIS step of the graph)
            self._plan['active'] = active
            self._plan.setdefault('slot_grads', {})[slot] = [p.grad for p, _ in active]
            self._launch(slot)                  # scalars are refreshed by prepare_replay()
            self._plan['cap_slot'] = slot + 1
            return loss
        ids = tuple(id(p) for p, _ in active)
        if self._plan is None or self._plan.get('captured') or self._plan['ids'] != ids or self._plan['key'] != key:
            # never stage an eager step through a captured plan: its graph re-reads those buffers
            eager = self._eager_plan
            if eager is not None and eager['ids'] == ids and eager['key'] == key:
                self._switch(eager)
            else:
                self._build(active)
                self._eager_plan = self._plan
        if self._plan['gen'] != self._gen:
            self._switch(self._plan)
        self.wait_staging()
        self._stage(active)
        self._launch()
        self.mark_launched()
        return loss

    def zero_grad(self, set_to_none=True):
        self._touch += 1         # .grad re-pointed / dropped: a captured plan re-attaches its static tensors next time
        return super().zero_grad(set_to_none)

    # ------------------------------------------------------------------ hipGraph support
    def capture_safe(self, poke=False, slots=1, extra=0):
        """Build a plan OF ITS OWN from the gradients that exist NOW (static tensors of the step
        being captured) so that step() inside `torch.cuda.graph` issues only stream work: one
        pinned H2D copy and one launch.  The captured graph keeps reading this plan's staging
        buffers, so the plan is never reused for eager steps: take it with `captured_plan()` after
        the capture and call `activate(plan)` + `prepare_replay()` before every replay.
        extra: bytes (a multiple of 32) kept behind the scalar rows for a rider of the same captured step — the rows of a
        bmnas.optim.AveragedModel (plan['extra'] on the host, plan['dev_extra'] on the device) —: they travel with the
        optimizer's rows, by value in poke mode, else through the plan's copy node."""
        active = self._active()
        self.wait_staging()
        self._build(active, slots, extra)
        self._write_ptrs(active)
        self._plan['captured'] = True
        # "poke" mode (round 5): the captured step holds NO H2D copy node.  The descriptor table is uploaded once after the
        # capture (and again whenever activate() / load_state_dict changed it); the per-step scalars — 32 bytes per row —
        # travel by value in the launch that copies the batch into the step's static tensors (bmnas_copy_batch's blob,
        # replay_blob()).  A captured copy node cost 4.7 us per optimizer step.
        self._plan['poke'] = bool(poke) and self._plan['hyp_all'].nbytes <= lib.copy_blob_max()
        if slots > 1 and not self._plan['poke']:
            rider = f' and {extra} bytes of averaging rows' if extra else ''
            raise lib.BmnasError(f'{self._NAME}: {slots} captured steps x {len(self._plan["groups"])} scalar rows{rider} '
                                 'do not fit the by-value blob of the batch-copy launch')

    def rider_rows(self):
        """-> (host bytes, device bytes) of the current plan's `extra` region (capture_safe(extra=...))."""
        return self._plan['extra'], self._plan['dev_extra']

    def captured_plan(self):
        """The plan a capture has just baked into a graph, with the pointer table as captured
        (parameters, static gradient tensors) snapshotted."""
        pl = self._plan
        if pl is None or not pl.get('captured'):
            raise lib.BmnasError(f'{self._NAME}: no captured plan (capture_safe() + a captured step() first)')
        if pl['cap_slot'] != pl['slots']:
            raise lib.BmnasError(f'{self._NAME}: the capture holds {pl["cap_slot"]} step(s), the plan was built for '
                                 f'{pl["slots"]}')
        pl['snap_param'] = [t['param'].copy() for t in pl['tabs']]
        pl['snap_grad'] = [t['grad'].copy() for t in pl['tabs']]
        # keeps every slot's static gradient tensors alive; .grad is re-attached to the LAST step's (what a sequence of
        # eager steps leaves behind)
        pl['static_grads'] = pl['slot_grads'][pl['slots'] - 1]
        pl['tab_dirty'] = True                                       # poke mode: upload before the first replay
        return pl

    def replay_blob(self):
        """Poke mode, after prepare_replay(): -> (device tensor, host bytes) of this replay's scalar rows for
        bmnas_copy_batch's blob; uploads the descriptor table first when it changed (eagerly, on the current stream, i.e.
        in front of the replay).  None: the captured step carries its own H2D copy node."""
        pl = self._plan
        if not pl.get('poke'):
            return None
        if pl.get('tab_dirty'):
            self.wait_staging()
            pl['stage'].copy()
            self.mark_launched(force=True)       # the pinned buffer must not be rewritten before this copy has read it
            self.wait_staging()                  # (rare: once after a capture / load_state_dict)
            pl['tab_dirty'] = False
        h = pl['hyp_all']
        return pl['dev_hyp'][:h.nbytes], h.tobytes()

    def activate(self, plan):
        """Make `plan` (from captured_plan()) the current one before its graph is replayed.  Eager
        steps in between — a ragged last batch, the Architect's eager path — run on a plan of their
        own, so the staging buffers the graph reads are intact; but they advanced the step counts
        and re-pointed `.grad`.  The counts are carried over, the capture-time parameter / gradient
        pointers are restored and `.grad` is re-attached to the static tensors the graph writes."""
        # fast path (every replay of a training loop): this plan is current, no eager step / zero_grad / load_state_dict
        # happened since its last activation — nothing to restore
        if self._plan is plan and plan['gen'] == self._gen and plan.get('stamp') == self._touch:
            if not plan.get('poke'):
                # the captured step carries an H2D copy node that reads this plan's pinned staging buffer (capture_safe()
                # without poke, or more scalar rows than the blob holds): prepare_replay() is about to rewrite that
                # buffer, so the previous replay's copy must have read it first
                self.wait_staging()
            return
        gen = plan['gen']
        self._switch(plan)
        if plan['gen'] != gen:
            plan['tab_dirty'] = True             # load_state_dict replaced the moment tensors: new pointers in the table
        for tab, sp, sg in zip(plan['tabs'], plan['snap_param'], plan['snap_grad']):
            if plan.get('poke') and ((tab['param'] != sp).any() or (tab['grad'] != sg).any()):
                plan['tab_dirty'] = True
            tab['param'] = sp
            tab['grad'] = sg
        for (p, _), gr in zip(plan['active'], plan['static_grads']):
            p.grad = gr
        plan['stamp'] = self._touch


class Adam(_OneLaunch, torch.optim.Adam):
    _NAME = 'bmnas.optim.Adam'
    _SHARED = 'a step count'

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False,
                 max_grad_norm=None, *, decoupled_weight_decay=False):
        """amsgrad / decoupled_weight_decay: torch.optim.Adam's, stored in `param_groups` under torch's keys and read from
        there when a plan is built (a loaded checkpoint's values count); every group must hold the same value of each.
        They may be edited between eager steps (the plan is rebuilt) but not under a captured plan.
        max_grad_norm (None or a positive float): clip the global L2 norm over every parameter of the optimizer that has
        a gradient, all groups together, before the update.  An attribute, not a `param_groups` entry (state_dict() stays
        that of torch.optim.Adam); it may be edited between steps and replays — it travels with the per-step scalars —
        but not switched between None and a value under a captured plan.  `.grad` is left UNCLIPPED: the scaling happens
        in the update's registers.  `last_grad_norm` / `grad_norms` hold the pre-clip norm(s) on the device."""
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad),
                         decoupled_weight_decay=bool(decoupled_weight_decay))
        self._init_one_launch(max_grad_norm)

    def _variant(self):
        """-> (clip, amsgrad, decoupled): what selects the launches of a step, the key of a plan.  The two switches are
        read from `param_groups` (torch's keys; a checkpoint written before torch had one lacks it: off)."""
        return (self._clip_value() is not None,) + self._switches()

    def _switches(self):
        """-> (amsgrad, decoupled_weight_decay) of the param_groups, which must agree on each."""
        first = None
        for g in self.param_groups:
            sw = (bool(g.get('amsgrad', False)), bool(g.get('decoupled_weight_decay', False)))
            if first is None:
                first = sw
            elif sw != first:
                name = 'amsgrad' if sw[0] != first[0] else 'decoupled_weight_decay'
                raise lib.BmnasError(f"bmnas.optim.Adam: param_groups disagree on '{name}' (one launch updates every "
                                     'group with one kernel: per-group mixing is not supported)')
        return first or (False, False)

    def _init_state(self, p, amsgrad=False):
        """amsgrad: `max_exp_avg_sq` is created with the moments — and, as zeros, for a state that has the moments but
        not it (an amsgrad=False checkpoint continued with amsgrad on: the first maximum then equals exp_avg_sq; torch
        raises KeyError there)."""
        st = self.state[p]
        if len(st) == 0:
            st['step'] = torch.tensor(0.0, dtype=torch.float32)
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        if amsgrad and 'max_exp_avg_sq' not in st:
            st['max_exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    def _state_ptrs(self, plan):
        """(Re)write the state pointers of every descriptor table of `plan` — and the running-maximum pointers behind
        them — from the CURRENT state tensors, validated."""
        names = ('exp_avg', 'exp_avg_sq') + (('max_exp_avg_sq',) if plan['amsgrad'] else ())
        ptrs = {n: [] for n in names}
        for p, _ in plan['active']:
            st = self._init_state(p, plan['amsgrad'])
            for n in names:
                t = st[n]
                if t.device != p.device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                    raise lib.BmnasError(f'bmnas.optim.Adam: {n} must be contiguous fp32 on {p.device}, of the '
                                         "parameter's size")
                ptrs[n].append(t.data_ptr())
        for i, tab in enumerate(plan['tabs']):
            tab['exp_avg'] = ptrs['exp_avg']
            tab['exp_avg_sq'] = ptrs['exp_avg_sq']
            if plan['amsgrad']:
                plan['maxes'][i][:] = ptrs['max_exp_avg_sq']

    def _flush_counts(self):
        """Write the plan's step counts back into the per-parameter `step` tensors."""
        pl = self._plan
        if pl is not None:
            for (p, _), r in zip(pl['active'], pl['row_of']):
                self.state[p]['step'].fill_(pl['count'][r])

    def _row_count(self, p, switches):
        """p's step count (parameters of one group with the same step count share a row of scalars)."""
        return float(self._init_state(p, switches[0])['step'])

    def _plan_fields(self, switches):
        """-> (the plan's own entries, tail pointers per tensor): amsgrad's max_exp_avg_sq pointers ride behind each table."""
        amsgrad, decoupled = switches
        return dict(amsgrad=amsgrad, decoupled=decoupled, flags=(lib.ADAM_AMSGRAD if amsgrad else 0) |
                    (lib.ADAM_DECOUPLED if decoupled else 0)), int(amsgrad)

    def _update(self, pl, slot, args, clip_args):
        if pl['flags']:
            lib.adam_multi_ex(*args, pl['dev_maxes'][slot] if pl['amsgrad'] else None, pl['flags'], *clip_args)
        elif clip_args:
            lib.adam_multi_clip(*args, *clip_args)
        else:
            lib.adam_multi(*args)

    def state_dict(self):
        self._flush_counts()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if torch.is_tensor(st.get('step')) and st['step'].is_cuda:
                st['step'] = st['step'].cpu()
        self._state_replaced()

    def prepare_replay(self, slot=0):
        """Advance the step count and publish the current learning rates for the next replay
        (call wait_staging() first and mark_launched() after the replay; GraphedTrainStep does).
        slot: which of the graph's consecutive steps these scalars are for — a graph of k steps takes k calls, slot 0
        first, each with the learning rates its step runs with (the scheduler moves them between two calls)."""
        self._begin_replay(slot, "'amsgrad' / 'decoupled_weight_decay' was switched")
        pl = self._plan
        h = pl['hyps'][slot]
        for r, gi in enumerate(pl['groups']):
            g = self.param_groups[gi]
            pl['count'][r] += 1.0
            t = pl['count'][r]
            b1, b2 = g['betas']
            # slot 5: weight_decay (L2, added to the gradient), or the decoupled decay's factor on the parameter, formed in
            # double as torch's `param.mul_(1 - lr * weight_decay)` does (exactly 1 without decay)
            wd = g['weight_decay']
            if pl['decoupled']:
                wd = 1 - g['lr'] * wd if wd != 0 else 1.0
            h[r] = (-(g['lr'] / (1 - b1 ** t)), math.sqrt(1 - b2 ** t), b1, b2, g['eps'], wd, 1 - b1, 1 - b2)

    def staged_lrs(self, slot=0):
        """The learning rate of every scalar row of `slot`, decoded from what prepare_replay() STAGED there (the fp32 value
        the Adam launch of that step reads) — for loops that report the rate a batch's step ran with."""
        pl = self._plan
        return [float(-pl['hyps'][slot][r][0]) * (1 - self.param_groups[gi]['betas'][0] ** pl['count'][r])
                for r, gi in enumerate(pl['groups'])]


class AdamW(Adam):
    """torch.optim.AdamW on the same one launch: Adam with decoupled weight decay (p *= 1 - lr * weight_decay in front of
    the update, the gradient untouched), default weight_decay 1e-2.  Like torch's class it stays decoupled whatever state
    it loads; `amsgrad` and `max_grad_norm` as for Adam."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False,
                 max_grad_norm=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                         max_grad_norm=max_grad_norm, decoupled_weight_decay=True)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group['decoupled_weight_decay'] = True


class SGD(_OneLaunch, torch.optim.SGD):
    """torch.optim.SGD with the update of every tensor in one `bmnas_sgd_multi` launch: the weight optimizer DARTS-style
    searches run with (reference models/search/darts/train_search.py:84-88: SGD(lr, momentum, weight_decay), clipped at
    :158).  Same constructor, `param_groups` and per-parameter state (`momentum_buffer` only) as torch's class, so
    checkpoints travel both ways; `max_grad_norm` and the capture protocol are bmnas.optim.Adam's.

    A scalar row is { -lr, mu, 1 - dampening, mu_n, weight_decay }: lr, momentum, dampening and weight_decay are per
    group and may change between steps and replays.  torch's first step of a tensor (`buf = clone(g)`, no dampening) is a
    ROW, not a kernel branch: mu = 0 and damp1 = 1 over a zero-filled buffer.  Rows are keyed by (group, first step or
    not).  A tensor's next step is its first iff its state holds no `momentum_buffer`: the zero buffer a plan allocates
    ahead of the step (capture_safe() must, the graph bakes its address) waits in `_pending` and enters `state` only
    when a step that writes it is staged — state_dict() never shows an unstepped buffer as a stepped one.
    One launch is one kernel: all groups agree on `momentum != 0` and on `nesterov`; `maximize` is refused."""
    _NAME = 'bmnas.optim.SGD'
    _SHARED = 'their first-step status'

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, max_grad_norm=None, *,
                 maximize=False):
        if maximize:
            raise lib.BmnasError('bmnas.optim.SGD: maximize=True is not supported (the kernel descends)')
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                         nesterov=bool(nesterov))
        self._init_one_launch(max_grad_norm)
        self._pending = {}       # parameter -> zero momentum buffer that no staged step has written yet

    def _variant(self):
        """-> (clip, momentum != 0, nesterov): what selects the launches of a step, the key of a plan."""
        return (self._clip_value() is not None,) + self._switches()

    def _switches(self):
        """-> (momentum != 0, nesterov) of the param_groups, which must agree on each; refuses `maximize`."""
        first = None
        for g in self.param_groups:
            if g.get('maximize', False):
                raise lib.BmnasError('bmnas.optim.SGD: maximize=True is not supported (the kernel descends)')
            sw = (g['momentum'] != 0, bool(g.get('nesterov', False)))
            if first is None:
                first = sw
            elif sw != first:
                name = 'momentum' if sw[0] != first[0] else 'nesterov'
                raise lib.BmnasError(f"bmnas.optim.SGD: param_groups disagree on '{name}'"
                                     f"{' being zero' if name == 'momentum' else ''} (one launch updates every "
                                     'group with one kernel: per-group mixing is not supported)')
        return first or (False, False)

    def _stepped(self, p):
        """Whether a step has written p's momentum buffer (or a checkpoint restored one): its next step is no first one."""
        st = self.state.get(p)
        return st is not None and st.get('momentum_buffer') is not None

    def _buffer(self, p):
        """p's momentum buffer: the stepped one of `state`, else a zero buffer kept OUT of `state` until a step is staged."""
        if self._stepped(p):
            return self.state[p]['momentum_buffer']
        if p not in self._pending:
            self._pending[p] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return self._pending[p]

    def _state_ptrs(self, plan):
        """(Re)write the momentum-buffer pointers of every descriptor table of `plan` from the CURRENT tensors, validated
        (without momentum: null, never dereferenced)."""
        ptrs = []
        for p, _ in plan['active']:
            if not plan['momentum']:
                ptrs.append(0)
                continue
            t = self._buffer(p)
            if t.device != p.device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                raise lib.BmnasError(f'bmnas.optim.SGD: momentum_buffer must be contiguous fp32 on {p.device}, of the '
                                     "parameter's size")
            ptrs.append(t.data_ptr())
        for tab in plan['tabs']:
            tab['exp_avg'] = ptrs
            tab['exp_avg_sq'] = 0

    def _row_count(self, p, switches):
        """How many steps were staged for p, as far as a row cares: 0 (the next one is its first) or 1."""
        return 1.0 if not switches[0] or self._stepped(p) else 0.0

    def _plan_fields(self, switches):
        momentum, nesterov = switches
        return dict(momentum=momentum, nesterov=nesterov, flags=(lib.SGD_MOMENTUM if momentum else 0) |
                    (lib.SGD_NESTEROV if nesterov else 0)), 0

    def _stage(self, active):
        """The gradients are validated (and their pointers written) FIRST: prepare_replay() moves the pending zero
        buffers into `state`, and a step refused after that — a non-contiguous or non-fp32 gradient — would leave an
        unstepped buffer shown as a stepped one."""
        self._write_ptrs(active)
        self.prepare_replay()

    def _update(self, pl, slot, args, clip_args):
        lib.sgd_multi(*args, pl['flags'], *clip_args)

    def load_state_dict(self, state_dict):
        if any(g.get('maximize', False) for g in state_dict['param_groups']):
            raise lib.BmnasError('bmnas.optim.SGD: the checkpoint has maximize=True, which is not supported (the kernel '
                                 'descends)')
        super().load_state_dict(state_dict)
        self._pending = {}           # (a checkpoint from before the first step holds no buffers)
        self._state_replaced()

    def prepare_replay(self, slot=0):
        """Publish the current learning rates, momenta, dampenings and weight decays for the next step or replay, and
        count it: a row whose tensors have not stepped gets torch's first-step rule (mu = 0, damp1 = 1 over the zero
        buffer), and their buffers enter `state` — the step staged here writes them.  slot: as for Adam."""
        self._begin_replay(slot, "'momentum' was switched between zero and non-zero, or 'nesterov' was switched,")
        pl = self._plan
        h = pl['hyps'][slot]
        for r, gi in enumerate(pl['groups']):
            g = self.param_groups[gi]
            mu = float(g['momentum'])
            first = pl['momentum'] and pl['count'][r] == 0
            pl['count'][r] += 1.0
            h[r] = (-float(g['lr']), 0.0 if first else mu, 1.0 if first else 1 - g['dampening'], mu,
                    float(g['weight_decay']), 0.0, 0.0, 0.0)
        if pl['momentum'] and self._pending:
            for p, _ in pl['active']:
                if p in self._pending:
                    self.state[p]['momentum_buffer'] = self._pending.pop(p)

    def staged_lrs(self, slot=0):
        """The learning rate of every scalar row of `slot`, as prepare_replay() STAGED it (the fp32 value the launch of
        that step reads)."""
        pl = self._plan
        return [float(-pl['hyps'][slot][r][0]) for r in range(len(pl['groups']))]


_CLIP_CACHE = {}


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ in two launches for fp32 gradients on one GPU: the multi-tensor norm
    (`bmnas_grad_sqnorm_multi`) and an in-place `grad *= min(1, max_norm / (norm + 1e-6))` (`bmnas_grad_scale_multi`).
    -> the pre-clip norm as a 0-dim device tensor (no synchronisation).  Eager only: inside a stream capture it raises —
    `Adam(max_grad_norm=...)` is how a captured step clips.  CPU tensors, other dtypes, `norm_type != 2` and
    `error_if_nonfinite=True` go to torch's function (its behaviour is the contract there)."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    ours = (len(grads) > 0 and float(norm_type) == 2.0 and not error_if_nonfinite and
            all(g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.device == grads[0].device
                for g in grads))
    if not ours:
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=norm_type,
                                              error_if_nonfinite=error_if_nonfinite, foreach=foreach)
    if torch.cuda.is_current_stream_capturing():
        raise lib.BmnasError('bmnas.optim.clip_grad_norm_ is eager only (it stages a descriptor table per call); inside a '
                             'captured step clip with bmnas.optim.Adam(max_grad_norm=...)')
    dev = grads[0].device
    key = (dev, float(max_norm), tuple((g.data_ptr(), g.numel()) for g in grads))
    ent = _CLIP_CACHE.get('last')
    if ent is None or ent['key'] != key:
        tab = np.zeros(len(grads), dtype=_DESC)
        tab['grad'] = [g.data_ptr() for g in grads]
        tab['numel'] = [g.numel() for g in grads]
        chunks, n_chunks = _chunk_list(tab['numel'].tolist(), dev)
        host = np.concatenate([np.array([max_norm, 0, 0, 0], dtype=np.float32).view(np.uint8), tab.view(np.uint8)])
        buf = torch.from_numpy(host).to(dev)
        ent = dict(key=key, buf=buf, clip=buf[:4], tab=buf[16:], chunks=chunks, n_chunks=n_chunks,
                   partials=torch.empty(lib.grad_norm_parts(), dtype=torch.float32, device=dev))
        _CLIP_CACHE['last'] = ent
    norm = torch.empty(1, dtype=torch.float32, device=dev)
    n_parts = min(ent['n_chunks'], lib.grad_norm_parts())
    if ent['n_chunks'] == 0:             # every gradient is empty
        return norm.zero_()[0]
    lib.grad_sqnorm_multi(ent['tab'], ent['chunks'], ent['n_chunks'], ent['partials'])
    lib.grad_scale_multi(ent['tab'], ent['chunks'], ent['n_chunks'], ent['partials'], n_parts, ent['clip'], norm)
    return norm[0]


class UnrolledStep:
    """The weight-side arithmetic of DARTS' unrolled (second-order) architecture step (Liu et al. 2019, eq. 7-8; the
    reference still passes `unrolled=args.unrolled` at models/search/darts/train_search.py:151) on the kernels of
    csrc/unroll.hip.  `models.search.darts.architect.Architect` drives it:

        virtual_step(g)       bak = w;  w = w - eta (moment + g + wd w)          g = grad_w L_train(w, alpha)
        perturb(v, +1 / -1)   w = bak + (+-R) v,  R = r / ||v||                   v = grad_w' L_val(w', alpha)
        restore()             w = bak
        combine(da, gp, gn)   da -= eta (gp - gn) / (2 R)                         gp / gn = grad_alpha L_train(w+ / w-)

    It owns the plan: the descriptor tables of the weights and of alpha, the chunk lists, the norm partials, ONE
    persistent backup tensor per weight tensor (+4 B per parameter, where DARTS copies the whole model) and one staging
    buffer.  Pointers and scalars go up with one `_Staging.upload()` per call (`uploads` counts those that copied); R, the
    norm and eta reach the kernels through device memory: no call synchronises with the host.  Eager only.

    The weight tensors are the network optimizer's own (`for g in param_groups for p in g['params']`); `grads`, `v` are
    lists in that order.  A tensor whose gradient is None in the virtual pass is left out of every launch of that step.
    A scalar row is per (group, has momentum_buffer): wd is the group's `weight_decay`, mu the group's `momentum` when
    `state[p]` holds a `momentum_buffer` and 0 otherwise — DARTS' try / except.  A bmnas.optim.Adam weight optimizer (the
    BM-NAS default) therefore gets the plain step w' = w - eta (g + wd w), as DARTS' code gives any optimizer without
    momentum buffers.  One eta, as in DARTS: every group must hold the same `lr` when the step runs.  The weight
    optimizer's max_grad_norm, dampening, nesterov, amsgrad and decoupled weight decay play no part in the virtual step,
    and its state — moments, buffers, step counts — is read, never written."""

    def __init__(self, network_optimizer, arch_parameters, r=1e-2):
        if network_optimizer is None:
            raise lib.BmnasError('bmnas.optim.UnrolledStep needs the network (weight) optimizer')
        self.optimizer = network_optimizer
        self.arch = list(arch_parameters)
        self.r = float(r)
        self._bak, self._zero = {}, {}
        self._plan = None
        self._normed = False             # the norm of v has been taken since the last virtual_step()
        self._stepped = False            # the weights hold w' or w+-, not w: restore() is owed
        self.uploads = 0                # pinned H2D copies issued so far (a skipped one does not count)

    @property
    def weights(self):
        return [p for g in self.optimizer.param_groups for p in g['params']]

    def eta(self):
        """The one learning rate of the virtual step; BmnasError when the weight groups disagree."""
        lrs = [float(g['lr']) for g in self.optimizer.param_groups]
        if any(lr != lrs[0] for lr in lrs):
            raise lib.BmnasError(f'bmnas.optim.UnrolledStep: the weight optimizer\'s groups hold different learning rates '
                                 f'{lrs}; DARTS\' unrolled step has one eta (per-group eta is not supported)')
        return lrs[0]

    def row_of(self, p, group):
        """-> (has momentum_buffer, mu, wd) of one weight tensor."""
        st = self.optimizer.state.get(p)
        has = st is not None and torch.is_tensor(st.get('momentum_buffer'))
        return has, (float(group.get('momentum', 0.0)) if has else 0.0), float(group['weight_decay'])

    # ------------------------------------------------------------------ plan
    @staticmethod
    def _eager(what):
        if torch.cuda.is_current_stream_capturing():
            raise lib.BmnasError(f'bmnas.optim.UnrolledStep.{what} is eager only (it stages descriptor tables per call); '
                                 'the unrolled architecture step cannot be captured in a graph')

    def _aligned(self, vals, what):
        ws = self.weights
        vals = list(vals)
        if len(vals) != len(ws):
            raise lib.BmnasError(f'bmnas.optim.UnrolledStep: {len(vals)} {what} for {len(ws)} weight tensors')
        return vals

    @staticmethod
    def _check_like(t, p, what):
        _check_like(t, p, 'bmnas.optim.UnrolledStep', what)

    def _zeros(self, p):
        if p not in self._zero:
            self._zero[p] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return self._zero[p]

    def _build(self, active, key, dev):
        """active: [(p, group index, has momentum_buffer)] of this step, all on `dev`.  One staging buffer: a clipped
        one-slot `staging_layout` — scalar rows | r, eta (where max_grad_norm goes) | weight table — and the alpha table
        behind it."""
        rows, row_idx, row_of = [], {}, []
        for p, gi, has in active:
            if p not in self._bak:
                self._bak[p] = torch.empty_like(p, memory_format=torch.contiguous_format)
            if (gi, has) not in row_idx:
                row_idx[(gi, has)] = len(rows)
                rows.append((gi, has))
            row_of.append(row_idx[(gi, has)])
        for a in self.arch:
            if a.device != dev or a.dtype != torch.float32:
                raise lib.BmnasError(f'bmnas.optim.UnrolledStep: architecture tensors must be fp32 on {dev}')
        lay = staging_layout(len(rows), len(active), clip=True)
        stage = _Staging(lay.nbytes + len(self.arch) * _DESC.itemsize, dev)
        host, devbuf = stage.host, stage.dev
        (rows_at,), (scal_at,), (wtab_at,) = lay.rows_at, lay.clip_at, lay.tab_at
        wtab = host[wtab_at:lay.nbytes].view(_DESC)
        wtab['param'] = [p.data_ptr() for p, _, _ in active]
        wtab['exp_avg_sq'] = [self._bak[p].data_ptr() for p, _, _ in active]
        wtab['numel'] = [p.numel() for p, _, _ in active]
        wtab['hyp_row'] = row_of
        parts = lib.grad_norm_parts()
        chunks, n_chunks = _chunk_list([p.numel() for p, _, _ in active], dev)
        self._plan = dict(
            key=key, active=active, rows=rows, stage=stage,
            hyp=host[rows_at:rows_at + lay.row_bytes].view(np.float32).reshape(len(rows), 8),
            scal=host[scal_at:scal_at + 16].view(np.float32),
            wtab=wtab, atab=host[lay.nbytes:].view(_DESC),
            dev_hyp=devbuf[:lay.hyp_bytes], dev_r=devbuf[scal_at:scal_at + 4], dev_eta=devbuf[scal_at + 4:scal_at + 8],
            dev_wtab=devbuf[wtab_at:lay.nbytes], dev_atab=devbuf[lay.nbytes:],
            chunks=chunks, n_chunks=n_chunks, n_parts=min(n_chunks, parts),
            partials=torch.empty(parts, dtype=torch.float32, device=dev), R=torch.zeros(1, dtype=torch.float32, device=dev),
            flags=lib.UNROLL_MOMENTUM if any(has for _, _, has in active) else 0, achunks={})

    # ------------------------------------------------------------------ the four calls
    @torch.no_grad()
    def virtual_step(self, grads):
        """bak = w; w = w - eta (moment + g + wd w) for every weight tensor whose entry of `grads` is not None."""
        eta = self.eta()                                   # (first: refused before anything moves)
        grads = self._aligned(grads, 'gradients')
        active, gs, i = [], [], 0
        for gi, g in enumerate(self.optimizer.param_groups):
            for p in g['params']:
                gr = grads[i]
                i += 1
                if gr is None:
                    continue
                self._check_like(gr, p, 'gradients')
                active.append((p, gi, self.row_of(p, g)[0]))
                gs.append(gr)
        if not active:
            raise lib.BmnasError('bmnas.optim.UnrolledStep: no weight tensor has a gradient')
        dev = _param_device([p for p, _, _ in active], 'bmnas.optim.UnrolledStep')   # (in front of _eager: it needs a GPU)
        self._eager('virtual_step')
        key = tuple((id(p), gi, has) for p, gi, has in active)
        if self._plan is None or self._plan['key'] != key:
            self._build(active, key, dev)
        pl = self._plan
        pl['stage'].wait()
        bufs = []
        for p, gi, has in active:
            buf = self.optimizer.state[p]['momentum_buffer'] if has else None
            if buf is not None:
                self._check_like(buf, p, 'momentum_buffer')
            bufs.append(0 if buf is None else buf.data_ptr())
        for r, (gi, has) in enumerate(pl['rows']):
            g = self.optimizer.param_groups[gi]
            pl['hyp'][r] = (-eta, float(g.get('momentum', 0.0)) if has else 0.0, float(g['weight_decay']), 0, 0, 0, 0, 0)
        pl['scal'][:] = (self.r, eta, 0.0, 0.0)
        pl['wtab']['param'] = [p.data_ptr() for p, _, _ in active]
        pl['wtab']['grad'] = [gr.data_ptr() for gr in gs]
        pl['wtab']['exp_avg'] = bufs
        self.uploads += pl['stage'].upload()
        lib.unroll_virtual_step(pl['dev_wtab'], pl['chunks'], pl['n_chunks'], pl['dev_hyp'], pl['flags'])
        self._normed = False
        self._stepped = True

    def _need_step(self, what):
        if self._plan is None or not self._stepped:
            raise lib.BmnasError(f'bmnas.optim.UnrolledStep.{what}: call virtual_step() first')

    @torch.no_grad()
    def perturb(self, v, sign):
        """w = bak + (sign R) v with R = r / ||v||; the norm is taken once, on the first call after virtual_step()."""
        self._need_step('perturb')
        self._eager('perturb')
        if sign not in (1, -1):
            raise lib.BmnasError(f'bmnas.optim.UnrolledStep.perturb: sign must be +1 or -1, got {sign!r}')
        pl = self._plan
        by_param = dict(zip(self.weights, self._aligned(v, 'vectors')))
        vs = []
        for p, _, _ in pl['active']:
            t = by_param[p]
            if t is None:
                t = self._zeros(p)               # no validation gradient: the tensor is not perturbed
            self._check_like(t, p, 'vectors')
            vs.append(t)
        pl['stage'].wait()
        pl['wtab']['grad'] = [t.data_ptr() for t in vs]
        self.uploads += pl['stage'].upload()
        if not self._normed:
            lib.grad_sqnorm_multi(pl['dev_wtab'], pl['chunks'], pl['n_chunks'], pl['partials'])
            self._normed = True
        lib.unroll_perturb(pl['dev_wtab'], pl['chunks'], pl['n_chunks'], pl['partials'], pl['n_parts'], pl['dev_r'],
                           sign, pl['R'])

    @torch.no_grad()
    def restore(self):
        """w = bak."""
        self._need_step('restore')
        self._eager('restore')
        pl = self._plan
        lib.unroll_restore(pl['dev_wtab'], pl['chunks'], pl['n_chunks'])
        self._stepped = False

    @property
    def R(self):
        """1-element fp32 device tensor: R of the most recent perturb()."""
        return None if self._plan is None else self._plan['R']

    @torch.no_grad()
    def combine(self, dalpha, gp, gn):
        """dalpha[i] -= eta (gp[i] - gn[i]) / (2 R), in place; -> the list.  Lists follow `arch_parameters`; an entry
        that is None in all three stays None, one that is None in some counts as zeros."""
        pl = self._plan
        if pl is None or not self._normed:
            raise lib.BmnasError('bmnas.optim.UnrolledStep.combine: no perturb() has set R')
        self._eager('combine')
        lists = [list(dalpha), list(gp), list(gn)]
        if any(len(x) != len(self.arch) for x in lists):
            raise lib.BmnasError(f'bmnas.optim.UnrolledStep.combine: lists of {len(self.arch)} entries expected')
        out, idx, cols = list(lists[0]), [], []
        for i, a in enumerate(self.arch):
            trio = [x[i] for x in lists]
            if all(t is None for t in trio):
                continue
            trio = [torch.zeros_like(a, memory_format=torch.contiguous_format) if t is None else t for t in trio]
            for t in trio:
                self._check_like(t, a, 'architecture gradients')
            out[i] = trio[0]
            idx.append(i)
            cols.append(trio)
        if not idx:
            return out
        ck = tuple(idx)
        if ck not in pl['achunks']:
            pl['achunks'][ck] = _chunk_list([self.arch[i].numel() for i in idx], pl['stage'].dev.device)
        chunks, n = pl['achunks'][ck]
        pl['stage'].wait()
        tab = pl['atab']
        tab[:] = np.zeros((), dtype=_DESC)
        m = len(idx)
        tab['param'][:m] = [c[0].data_ptr() for c in cols]
        tab['grad'][:m] = [c[1].data_ptr() for c in cols]
        tab['exp_avg'][:m] = [c[2].data_ptr() for c in cols]
        tab['numel'][:m] = [c[0].numel() for c in cols]
        self.uploads += pl['stage'].upload()
        lib.unroll_combine(pl['dev_atab'], chunks, n, pl['dev_eta'], pl['R'])
        return out


def accum_weights(sizes, reduction='mean'):
    """The weights of m micro-batch gradients in the gradient of their union: n_i / N for a criterion that averages
    (`reduction='mean'`: each micro-batch's loss is a mean over its own n_i samples), 1 for one that sums.  Formed in
    double; the combine launch takes them as fp32.  With these weights the combined gradient is what m data-parallel
    ranks holding the same shards would all-reduce.  A class-weighted CrossEntropyLoss mean is
    normalised per micro-batch by its own weight sum — the caveat README states for data parallelism holds here too."""
    sizes = [int(n) for n in sizes]
    if not sizes or any(n <= 0 for n in sizes):
        raise lib.BmnasError(f'accum_weights: micro-batch sizes must be positive, got {sizes}')
    if reduction == 'sum':
        return [1.0] * len(sizes)
    if reduction != 'mean':
        raise lib.BmnasError(f"accum_weights: reduction must be 'mean' or 'sum', got {reduction!r}")
    total = sum(sizes)
    return [n / total for n in sizes]


class GradAccumulator:
    """Gradient accumulation over up to `lib.accum_max()` micro-batches as ONE launch per optimizer step
    (`bmnas_grad_combine_multi`, csrc/accum.hip): what autograd's AccumulateGrad does with m adds per tensor over m
    `backward()` calls, and — with `accum_weights` — what the gradient reduction of the reference's nn.DataParallel
    (`--parallel`, models/search/ntu_darts_searchable.py) computes over its replicas.

        acc = GradAccumulator(optimizer)
        for (inputs, labels), w in zip(micro_batches, accum_weights(sizes)):
            grads = torch.autograd.grad(criterion(model(inputs), labels), acc.tensors, allow_unused=True)
            acc.add(grads, w)                      # keeps references, launches nothing
        acc.combine()                              # one launch: p.grad = sum_i w_i * part_i
        optimizer.step()

    The tensors are the optimizer's (`for g in param_groups for p in g['params']`); `grads` follows that order, None
    entries allowed (`allow_unused`).  A tensor some part covered gets `p.grad` set to its persistent fp32 accumulation
    tensor (+4 B per parameter, allocated on first use); a NULL part is left out of its sum.  A tensor no part covered
    gets `p.grad = None`.  The optimizer and the clipping norm downstream see an ordinary `.grad`: every Adam and SGD
    variant and `max_grad_norm` (the norm of the COMBINED gradient) work unchanged.

    Eager: descriptors, part pointers and the chunk list go up with one `_Staging.upload()` (`uploads` counts those that
    copied).  The weights travel by value in the launch.  combine() synchronises nothing.
    Captured (bmnas.graph.GraphedTrainStep(accumulate=m)): `capture_safe(m)` before the capture, `captured_plan()` after
    it, `abandon_capture()` when it failed.  Inside the capture combine() issues the launch only; the tables — the
    addresses of the graph's static `autograd.grad` outputs — are uploaded by captured_plan(), eagerly, before the first
    replay: the graph holds no H2D node of the accumulator.  The plan keeps the parts alive; the weights are constants of
    the capture."""

    def __init__(self, optimizer):
        if optimizer is None or not hasattr(optimizer, 'param_groups'):
            raise lib.BmnasError('bmnas.optim.GradAccumulator needs an optimizer')
        self.optimizer = optimizer
        self._acc = {}                   # parameter -> its accumulation tensor
        self._acc_storage = set()        # their storages' addresses (what add() refuses as a part)
        self._parts = []                 # [(grads, weight)] since the last combine()
        self._eager = None
        self._capturing = None           # the plan of an open capture (capture_safe() ... captured_plan())
        self._chunk_cache = {}
        self.launches = 0                # bmnas_grad_combine_multi calls issued from Python (a replayed one is none)
        self.uploads = 0                 # pinned H2D copies issued so far (a skipped one does not count)
        self.captures = 0

    @property
    def tensors(self):
        return [p for g in self.optimizer.param_groups for p in g['params']]

    @property
    def pending(self):
        """How many parts wait for combine()."""
        return len(self._parts)

    def accumulation_tensor(self, p):
        """p's accumulation tensor (None before the first plan was built)."""
        return self._acc.get(p)

    def reset(self):
        """Drop the pending parts."""
        self._parts = []

    def add(self, grads, weight):
        """One micro-batch's gradients (a list aligned with `tensors`, None entries allowed) and its weight.  Validates,
        keeps references, launches nothing."""
        ts = self.tensors
        grads = list(grads)
        if len(grads) != len(ts):
            raise lib.BmnasError(f'bmnas.optim.GradAccumulator.add: {len(grads)} gradients for {len(ts)} tensors')
        if len(self._parts) >= lib.accum_max():
            raise lib.BmnasError(f'bmnas.optim.GradAccumulator.add: at most {lib.accum_max()} parts per step '
                                 '(BMNAS_ACCUM_MAX); call combine() first')
        for g, p in zip(grads, ts):
            if g is None:
                continue
            _check_like(g, p, 'bmnas.optim.GradAccumulator.add', 'a part')
            if g.untyped_storage().data_ptr() in self._acc_storage:
                raise lib.BmnasError('bmnas.optim.GradAccumulator.add: a part aliases an accumulation tensor (a '
                                     '`.grad` that combine() set?); the launch reads every part while it writes there')
        self._parts.append((grads, float(weight)))

    # ------------------------------------------------------------------ plan
    def _build(self, ts, m):
        """A plan with room for every tensor and m parts each: ONE staging buffer — a `staging_layout` without scalar rows,
        descriptor table | part pointers (tensor-major, the table's tail) — and the chunk list behind it.  Allocates the
        accumulation tensors."""
        if not ts:
            raise lib.BmnasError('bmnas.optim.GradAccumulator: the optimizer holds no tensors')
        dev = _param_device(ts, 'bmnas.optim.GradAccumulator')
        for p in ts:
            if p not in self._acc:
                self._acc[p] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                self._acc_storage.add(self._acc[p].untyped_storage().data_ptr())
        lay = staging_layout(0, len(ts), tail_ptrs_per_tensor=m)
        parts_at, chunks_at = lay.tail_at[0], _chunks_at(lay)
        stage = _Staging(chunks_at + max(1, len(_chunk_pairs([p.numel() for p in ts]))) * 8, dev)
        return dict(ids=tuple(id(p) for p in ts), m=m, stage=stage, parts_at=parts_at, chunks_at=chunks_at,
                    dev_tab=stage.dev[:parts_at], dev_parts=stage.dev[parts_at:chunks_at],
                    dev_chunks=stage.dev[chunks_at:], n_chunks=0)

    def _fill(self, pl, ts, active, parts):
        """Write the descriptors, part pointers and chunk list of this step's tensors (`active`: indices into ts)."""
        m, host = len(parts), pl['stage'].host
        host[:] = 0
        tab = host[:len(active) * _DESC.itemsize].view(_DESC)
        tab['grad'] = [self._acc[ts[i]].data_ptr() for i in active]
        tab['numel'] = [ts[i].numel() for i in active]
        ptrs = host[pl['parts_at']:pl['parts_at'] + len(active) * m * 8].view('<u8').reshape(len(active), m)
        for j, (gs, _) in enumerate(parts):
            ptrs[:, j] = [0 if gs[i] is None else gs[i].data_ptr() for i in active]
        key = tuple(active)
        if key not in self._chunk_cache:
            self._chunk_cache[key] = _chunk_pairs([ts[i].numel() for i in active])
        chunks = self._chunk_cache[key]
        host[pl['chunks_at']:pl['chunks_at'] + chunks.nbytes].view(np.int32)[:] = chunks.reshape(-1)
        pl['n_chunks'] = len(chunks)

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def combine(self):
        """One launch: p.grad = sum_i w_i * part_i for every tensor a part covered (None for the others); clears the
        list.  Returns nothing, synchronises nothing."""
        if not self._parts:
            raise lib.BmnasError('bmnas.optim.GradAccumulator.combine: no parts (call add() first)')
        ts = self.tensors
        m = len(self._parts)
        active = [i for i in range(len(ts)) if any(gs[i] is not None for gs, _ in self._parts)]
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        if capturing:
            pl = self._capturing
            if pl is None or pl['m'] != m or pl['ids'] != tuple(id(p) for p in ts) or pl.get('parts') is not None:
                raise lib.BmnasError('bmnas.optim.GradAccumulator: call capture_safe(m) before capturing combine() in a '
                                     'graph (once per captured combine, with the number of parts it sums)')
            if not active:
                raise lib.BmnasError('bmnas.optim.GradAccumulator: a captured combine() needs at least one gradient')
        else:
            pl = self._eager
            if pl is None or pl['ids'] != tuple(id(p) for p in ts):
                pl = self._eager = self._build(ts, lib.accum_max())
            pl['stage'].wait()
        parts, self._parts = self._parts, []
        if active:
            self._fill(pl, ts, active, parts)
            if capturing:
                pl['parts'] = parts              # the graph's static autograd.grad outputs: alive as long as the plan
            else:
                self.uploads += pl['stage'].upload()
            lib.grad_combine_multi(pl['dev_tab'], pl['dev_chunks'], pl['n_chunks'], pl['dev_parts'], m,
                                   [w for _, w in parts])
            self.launches += 1
        hit = set(active)
        for i, p in enumerate(ts):
            p.grad = self._acc[p] if i in hit else None
        if not capturing and hasattr(self.optimizer, '_touch'):
            self.optimizer._touch += 1           # .grad re-pointed outside a replay (as zero_grad does)

    # ------------------------------------------------------------------ hipGraph support
    def capture_safe(self, m):
        """Build the plan of ONE captured combine() over m parts: its buffers (and every accumulation tensor) are
        allocated NOW, outside the capture — the graph bakes their addresses."""
        if self._capturing is not None:
            raise lib.BmnasError('bmnas.optim.GradAccumulator: capture_safe() while another capture is open (take it '
                                 'with captured_plan(), or drop it with abandon_capture(), first)')
        m = int(m)
        if not 1 <= m <= lib.accum_max():
            raise lib.BmnasError(f'bmnas.optim.GradAccumulator: m must be in 1 .. {lib.accum_max()}, got {m}')
        self._parts = []
        self._capturing = self._build(self.tensors, m)

    def abandon_capture(self):
        """Drop the plan of a capture that failed."""
        self._capturing = None
        self._parts = []

    def captured_plan(self):
        """The plan a capture has just baked into a graph; uploads its tables (eagerly, in front of the first replay) and
        closes the capture."""
        pl = self._capturing
        if pl is None:
            raise lib.BmnasError('bmnas.optim.GradAccumulator: no open capture (capture_safe() + a captured combine() '
                                 'first)')
        if pl.get('parts') is None:
            raise lib.BmnasError('bmnas.optim.GradAccumulator: the capture holds no combine()')
        self._capturing = None
        self.uploads += pl['stage'].upload()
        pl['stage'].wait()
        pl['weights'] = [w for _, w in pl['parts']]
        self.captures += 1
        return pl


# bmnas_avg_row_t (include/bmnas_hip.h)
_AVG_ROW = np.dtype([('w', '<f4'), ('omw', '<f4'), ('flags', '<u4'), ('reserved0', '<u4'), ('count', '<i8'),
                     ('reserved1', '<i8')])
assert _AVG_ROW.itemsize == 32


def avg_weight(n, decay=None):
    """The weight of the live tensors, in double, in the update that follows `n` completed ones: 1 for the first (torch's
    copy), 1 - decay for an EMA, and for SWA the fp32 quotient 1 / (n + 1) as torch's get_swa_multi_avg_fn forms it."""
    if n == 0:
        return 1.0
    if decay is None:
        return float(np.float32(1.0) / np.float32(n + 1))
    return 1.0 - float(decay)


def avg_row(n, decay=None, raw=False):
    """-> the bmnas_avg_row_t of that update, as a tuple for a numpy record: w, omw = 1 - w (formed in double, rounded
    once), flags, 0, the new count n + 1, 0.  A RAW row carries the count and no weights."""
    if raw:
        return (0.0, 0.0, lib.AVG_RAW, 0, n + 1, 0)
    w = avg_weight(n, decay)
    return (np.float32(w), np.float32(1.0 - w), 0, 0, n + 1, 0)


class AveragedModel(torch.optim.swa_utils.AveragedModel):
    """torch.optim.swa_utils.AveragedModel with `update_parameters` as ONE `bmnas_avg_multi` launch over every tensor and
    no host synchronisation: EMA of the weights (`decay` in [0, 1]: w = 1 - decay) or SWA (`decay=None`:
    w = fp32(1 / (n + 1))).  Same structure (`self.module = deepcopy(model)`, buffer `n_averaged`) and the same
    `state_dict()` keys as torch's class: checkpoints travel both ways.  `avg_fn` / `multi_avg_fn` are not taken.

    torch's `bool(self.n_averaged == 0)` — a host synchronisation per update — is gone: the count is mirrored on the host
    (re-read from the device ONCE after load_state_dict), the first update is the scalar row w = 1 (a copy for finite
    values), and the launch stores the new count into `n_averaged`.  So the update can be captured in a hipGraph
    (bmnas.graph.GraphedTrainStep(averaged=...)): its row rides with the optimizer's rows.

    use_buffers=True averages floating buffers (BatchNorm running statistics) like parameters; False copies every buffer,
    as torch does.  INTEGER buffers (num_batches_tracked) are always copied — the one difference from torch, whose EMA of
    an int64 counter is a truncated n * decay + m * (1 - decay) that nothing reads.
    skip_frozen=True: a parameter with requires_grad=False is copied by the first update and left out of later launches
    (12 B per frozen parameter per step saved).  Exact as long as such tensors do not change between updates — frozen
    backbones; NOT if they are loaded or edited after the first update.  Which parameters are frozen is read from
    `requires_grad` at each eager update and when an update is captured: a tensor frozen LATER keeps the average it had, one
    unfrozen later joins the launches with whatever its copy holds (a captured update never sees the change) — freeze
    before the first update.  False (default) is torch's behaviour.
    A model with non-fp32 floating tensors, tensors off the GPU or non-contiguous ones runs torch's parent class (after
    lib.note_off_path), where integer buffers follow torch's rule."""

    def __init__(self, model, device=None, decay=None, use_buffers=False, skip_frozen=False):
        if decay is not None:
            decay = float(decay)
            if not 0.0 <= decay <= 1.0:
                raise ValueError(f'bmnas.optim.AveragedModel: decay must be None (SWA) or in [0, 1], got {decay!r}')
        multi = torch.optim.swa_utils.get_ema_multi_avg_fn(decay) if decay is not None else None
        super().__init__(model, device=device, multi_avg_fn=multi, use_buffers=bool(use_buffers))
        self.decay = decay
        self.skip_frozen = bool(skip_frozen)
        # torch leaves `n_averaged` on the CPU unless `device` is given; the launch stores the count, so the buffer lives
        # where the averaged tensors do (same key, same dtype: checkpoints do not notice)
        home = next((t.device for t in list(self.module.parameters()) + list(self.module.buffers()) if t.is_cuda), None)
        if home is not None and self.n_averaged.device != home:
            self.register_buffer('n_averaged', self.n_averaged.to(home))
        # modules that keep tensors in shared storage re-point them lazily (node_operations' stacked convs): do it now —
        # a captured update holds the addresses
        for m in self.module.modules():
            settle = getattr(m, 'settle_storage', None)
            if callable(settle):
                settle()
        self._n = 0                  # host mirror of n_averaged; None: re-read it from the device (load_state_dict)
        self._eager = {}             # (id(model), members) -> eager plan
        self._checked = None         # (weak reference to a model, off_path(model)): decided once per model, not per update
        self._capturing = None       # the plan whose updates are being captured (capture_safe() ... captured_plan())
        self.captures = 0            # captured plans handed out so far
        self.launches = 0            # bmnas_avg_multi calls issued from Python so far (a replayed update is none)

    # ------------------------------------------------------------------ membership
    def pairs(self, model):
        """-> [(averaged tensor, live tensor, 'avg' | 'raw', frozen)] in torch's order (parameters, then buffers)."""
        out = [(a, p, 'avg', not p.requires_grad) for a, p in zip(self.module.parameters(), model.parameters())]
        for a, b in zip(self.module.buffers(), model.buffers()):
            out.append((a, b, 'avg' if self.use_buffers and a.is_floating_point() else 'raw', False))
        return out

    def members(self, model, with_frozen):
        """The (averaged, live, kind) triples of a launch: every tensor (with_frozen), or every tensor but the parameters
        that are frozen NOW (`requires_grad` is read at each eager update and at capture_safe())."""
        return [(a, p, k) for a, p, k, frozen in self.pairs(model) if with_frozen or not frozen]

    def _main(self, model):
        """The tensors of an update's one launch: all of them, or — skip_frozen — all but the frozen parameters."""
        return self.members(model, with_frozen=not self.skip_frozen)

    def off_path(self, model):
        """Why this pair of models runs torch's parent class, or None."""
        dev = None
        if not self.n_averaged.is_cuda:
            return 'tensors off the GPU'
        for a, p, kind, _ in self.pairs(model):
            for t in (a, p):
                if not t.is_cuda:
                    return 'tensors off the GPU'
                dev = dev or t.device
                if t.device != dev:
                    return 'tensors on more than one device'
                if not t.is_contiguous():
                    return 'non-contiguous tensors'
            if a.dtype != p.dtype or a.shape != p.shape:
                return 'the models differ in a dtype or shape'
            if kind == 'avg' and a.dtype != torch.float32:
                return f'{a.dtype} tensors to average'
            if kind == 'raw' and ((a.numel() * a.element_size()) % 4 or a.data_ptr() % 4 or p.data_ptr() % 4):
                return f'a {a.dtype} buffer that is no whole number of aligned 32-bit words'
        return None

    def _count(self):
        if self._n is None:
            self._n = int(self.n_averaged)           # once after load_state_dict
        return self._n

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._n = None
        return out

    # ------------------------------------------------------------------ plans
    def _build(self, trio, slots=1, rows=None, dev_rows=None):
        """The plan of `slots` launches over `trio`: per slot a descriptor table (averaged tensors first, then RAW ones),
        one chunk list, and the rows — slot s's row at index s and, when both kinds are present, ONE shared RAW row
        behind them.  rows / dev_rows: where the rows live when they ride in an optimizer's staging buffer (host bytes
        and their device copy); None: in this plan's own buffer, where `staging_layout` puts a rider's rows (in front of
        the tables).  The chunk list lies behind the tables in the same staging buffer: building a plan and uploading it
        copies nothing from pageable memory, so even the first update synchronises nothing."""
        avg = [(a, p) for a, p, k in trio if k == 'avg' and a.numel()]
        raw = [(a, p) for a, p, k in trio if k == 'raw' and a.numel()]
        order = avg + raw
        n_rows = slots + (1 if avg and raw else 0)
        own = rows is None
        numels = [a.numel() for a, _ in avg] + [a.numel() * a.element_size() // 4 for a, _ in raw]
        lay = staging_layout(0, len(order), slots=slots, extra_bytes=n_rows * 32 if own else 0)
        pairs, chunks_at = _chunk_pairs(numels), _chunks_at(lay)
        stage = _Staging(chunks_at + pairs.nbytes, order[0][0].device)
        host, devbuf = stage.host, stage.dev
        host[chunks_at:].view(np.int32)[:] = pairs.reshape(-1)
        if own:
            rows_at = slice(lay.extra_at, lay.extra_at + n_rows * 32)
            rows, dev_rows = host[rows_at], devbuf[rows_at]
        if rows.nbytes != n_rows * 32:
            raise lib.BmnasError(f'bmnas.optim.AveragedModel: {n_rows} rows need {n_rows * 32} bytes, got {rows.nbytes}')
        rows = rows.view(_AVG_ROW)
        tabs = [host[o:o + lay.tab_bytes].view(_DESC) for o in lay.tab_at]
        for s, tab in enumerate(tabs):
            tab['numel'] = numels
            tab['hyp_row'] = [s] * len(avg) + [slots if avg else s] * len(raw)
        if avg and raw:
            rows[slots] = (0.0, 0.0, lib.AVG_RAW, 0, 0, 0)    # (its count is never read: tensor 0 is an averaged one)
        return dict(order=order, numels=numels, raw_only=not avg, slots=slots, own=own, stage=stage,
                    rows=rows, dev_rows=dev_rows, tabs=tabs, chunks=devbuf[chunks_at:],
                    dev_tabs=[devbuf[o:o + lay.tab_bytes] for o in lay.tab_at], n_chunks=len(pairs), cap_slot=0)

    @staticmethod
    def _write_ptrs(pl):
        for tab in pl['tabs']:
            tab['param'] = [a.data_ptr() for a, _ in pl['order']]
            tab['grad'] = [p.data_ptr() for _, p in pl['order']]

    def _write_row(self, pl, slot, n):
        pl['rows'][slot] = avg_row(n, self.decay, raw=pl['raw_only'])

    def _launch(self, pl, slot=0):
        lib.avg_multi(pl['dev_tabs'][slot], pl['chunks'], pl['n_chunks'], pl['dev_rows'], self.n_averaged)
        self.launches += 1

    def _run_eager(self, key, trio, n):
        """Stage and launch an eager update over `trio` (its plan is kept under `key`)."""
        order = [(a, p) for a, p, k in trio if k == 'avg' and a.numel()] + \
                [(a, p) for a, p, k in trio if k == 'raw' and a.numel()]
        pl = self._eager.get(key)
        if pl is None or len(pl['order']) != len(order) or any(
                m != a.numel() * a.element_size() // 4 for m, (a, _) in zip(pl['numels'], order)):
            pl = self._eager[key] = self._build(trio)
        pl['stage'].wait()
        pl['order'] = order                          # (the tensors may have been re-pointed: addresses are re-read)
        self._write_ptrs(pl)
        self._write_row(pl, 0, n)
        pl['stage'].upload()
        self._launch(pl)

    def _copy_frozen(self, model, n):
        """skip_frozen, first update: the frozen parameters, bitwise, in a launch of their own."""
        trio = [(a, p, 'raw') for a, p, _, frozen in self.pairs(model) if frozen and a.numel()]
        if trio:
            self._run_eager((id(model), 'frozen'), trio, n)

    # ------------------------------------------------------------------ torch's API
    @torch.no_grad()
    def update_parameters(self, model):
        """One launch (the first update of a skip_frozen averager: two), no host synchronisation."""
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        if capturing:
            pl = self._capturing
            if pl is None or pl['model'] is not model or pl['cap_slot'] >= pl['slots']:
                raise lib.BmnasError('bmnas.optim.AveragedModel: call capture_safe() before capturing update_parameters() '
                                     'in a graph (once per captured update)')
            self._launch(pl, pl['cap_slot'])
            pl['cap_slot'] += 1
            return
        if self._checked is None or self._checked[0]() is not model:
            self._checked = (weakref.ref(model), self.off_path(model))
        why = self._checked[1]
        if why is not None:
            lib.note_off_path('bmnas.optim.AveragedModel', why)
            self._n = None
            return super().update_parameters(model)
        n = self._count()
        if self.skip_frozen and n == 0:
            self._copy_frozen(model, n)
        trio = self._main(model)
        if any(a.numel() for a, _, _ in trio):
            self._run_eager((id(model), 'all'), trio, n)
        else:
            self.n_averaged.fill_(n + 1)
        self._n = n + 1

    # ------------------------------------------------------------------ hipGraph support
    def capture_rows(self, model, slots=1):
        """How many bytes of rows `slots` captured updates of `model` need behind an optimizer's (capture_safe(extra=...))."""
        why = self.off_path(model)
        if why is not None:
            raise lib.BmnasError(f'bmnas.optim.AveragedModel: a captured update needs the HIP kernel ({why})')
        trio = self._main(model)
        kinds = {k for a, _, k in trio if a.numel()}
        if not kinds:
            raise lib.BmnasError('bmnas.optim.AveragedModel: nothing to average in a captured update')
        return (slots + (1 if len(kinds) == 2 else 0)) * 32

    def capture_safe(self, model, rows, dev_rows, slots=1):
        """Build the plan of `slots` captured updates: the descriptor tables go up NOW (the graph bakes their addresses and
        those of the tensors), the rows live in `rows` / `dev_rows` — an optimizer plan's `extra` / `dev_extra`, whose
        upload (by value in front of the replay, or the plan's copy node) carries them.  update_parameters(model) inside
        `torch.cuda.graph` then issues one launch per call.  Take the plan with captured_plan() after the capture — its
        holder (bmnas.graph.GraphedTrainStep) passes it to prepare_replay(plan, slot) before every replay: an averager
        may ride in several captured steps (the loop's one-step and k-step graphs), each with a plan of its own."""
        if self._capturing is not None:
            raise lib.BmnasError('bmnas.optim.AveragedModel: capture_safe() while another capture is open (take it with '
                                 'captured_plan(), or drop it with abandon_capture(), first)')
        trio = self._main(model)
        pl = self._build(trio, slots, rows, dev_rows)
        self._write_ptrs(pl)
        pl['stage'].upload()
        pl['stage'].wait()
        pl['model'] = model
        self._capturing = pl

    def abandon_capture(self):
        """Drop the plan of a capture that failed."""
        self._capturing = None

    def captured_plan(self):
        """The plan a capture has just baked into a graph; closes the capture."""
        pl = self._capturing
        if pl is None:
            raise lib.BmnasError('bmnas.optim.AveragedModel: no open capture (capture_safe() + captured updates first)')
        if pl['cap_slot'] != pl['slots']:
            raise lib.BmnasError(f'bmnas.optim.AveragedModel: the capture holds {pl["cap_slot"]} update(s), the plan was '
                                 f'built for {pl["slots"]}')
        self._capturing = None
        self.captures += 1
        return pl

    def prepare_replay(self, plan, slot=0):
        """Write the row of update number `slot` of the replay of `plan` (from captured_plan()) into ITS riding rows and
        count it; the first update of a skip_frozen averager copies the frozen parameters here, eagerly, in front of the
        replay."""
        pl = plan
        if pl is None or pl.get('model') is None or pl['cap_slot'] != pl['slots'] or pl is self._capturing:
            raise lib.BmnasError('bmnas.optim.AveragedModel: prepare_replay() needs a plan from captured_plan()')
        if not 0 <= slot < pl['slots']:
            raise lib.BmnasError(f'bmnas.optim.AveragedModel: slot {slot} of a plan of {pl["slots"]} update(s)')
        n = self._count()
        if self.skip_frozen and n == 0:
            self._copy_frozen(pl['model'], n)
        self._write_row(pl, slot, n)
        self._n = n + 1


def update_bn(loader, model, device=None, *, unpack=None, criterion=None, graph=True):
    """torch.optim.swa_utils.update_bn — the pass that ends the SWA recipe — for a model on the native BatchNorm
    kernels: every BatchNorm's running statistics are reset and recomputed as the CUMULATIVE average over one pass of
    `loader` (momentum None: factor 1 / num_batches_tracked, which the kernels derive from the device counter), with the
    model in training mode and no gradients; momenta and the training mode are restored afterwards, also when a forward
    raises.  Modules on the composed edited-list routes run torch's own BatchNorm under momentum None: right by
    construction.

        unpack(batch, device) -> (inputs, labels)   the trainers' callable (a list of modalities cannot go through torch's
                                                    `input = input[0]`); without it torch's convention holds: a list /
                                                    tuple batch means its first element, moved to `device` when given
        criterion, graph=True                       the forwards are replays of ONE private bmnas.graph.GraphedForward,
                                                    captured after the momenta are set and dropped at the end (a plan
                                                    captured under other momenta must not be used: value mode bakes the
                                                    scalar in); a ragged batch or a failed capture runs eagerly

    No host synchronisation per batch.  Not for data parallelism: every rank would see only its shard.
    -> dict(batches, replays, eager): how the forwards of this pass ran."""
    report = dict(batches=0, replays=0, eager=0)
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    if not bns:
        return report
    momenta = {m: m.momentum for m in bns}
    was_training = model.training
    fwd = None
    try:
        for m in bns:
            m.reset_running_stats()              # in place: NodeMixedOp's stacked views stay views
            m.momentum = None
        model.train()
        with torch.no_grad():
            for batch in loader:
                if unpack is not None:
                    inputs, labels = unpack(batch, device)
                else:
                    inputs, labels = (batch[0] if isinstance(batch, (list, tuple)) else batch), None
                    if device is not None:
                        inputs = inputs.to(device)
                report['batches'] += 1
                if graph and criterion is not None and labels is not None and fwd is not False:
                    if fwd is None:
                        from .graph import GraphedForward
                        fwd = GraphedForward.try_build(model, criterion, inputs, labels)
                    if fwd and fwd.matches(model, inputs, labels):
                        fwd(inputs, labels)
                        report['replays'] += 1
                        continue
                model(inputs)
                report['eager'] += 1
    finally:
        del fwd
        for m, mom in momenta.items():
            m.momentum = mom
        model.train(was_training)
    return report
