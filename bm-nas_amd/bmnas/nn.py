"""Drop-in nn.Module replacements for the two callers right after the fusion cell: the
central classifier (nn.Linear) and the criterion, both on the gfx950 kernels of
csrc/linear.hip.  Same constructor signatures, parameter names and state_dict keys as the torch
classes they subclass.  The criteria take class weights, pos_weight, label smoothing, ignore_index and
reduction 'mean' | 'sum' on the kernels (criterion_route says which calls); the combinations left
run the torch parent class after a one-time RuntimeWarning (bmnas.lib.note_off_path): nothing
leaves the HIP path silently."""
import torch
import torch.nn as nn

import contextlib

from . import lib
from .functions import (BCEWithLogitsCritFn, BCEWithLogitsFn, CrossEntropyCritFn, CrossEntropyFn, DeferredLossFn,
                        LinearFn)

_FUSED_CRITERION = [False]


@contextlib.contextmanager
def fused_criterion(on=True):
    """Inside this context a criterion applied to the logits of a fused head (FusionNetwork with its
    central classifier, csrc/head.hip) is evaluated by the head's backward launch instead of a
    launch of its own: the returned loss tensor is filled when backward has run.  For code that
    reads the loss only after backward — a captured training step (bmnas.graph.GraphedTrainStep
    turns it on), the benchmark step."""
    prev, _FUSED_CRITERION[0] = _FUSED_CRITERION[0], bool(on)
    try:
        yield
    finally:
        _FUSED_CRITERION[0] = prev


def _deferrable(input):
    head = getattr(input, '_bmnas_head', None)
    if _FUSED_CRITERION[0] and head is not None and torch.is_grad_enabled() and input.requires_grad:
        return head
    return None


class Linear(nn.Linear):
    """nn.Linear whose forward/backward run on the MFMA kernels when out_features <= 128,
    in_features % 16 == 0 and a bias is present (the central_classifier shapes)."""

    def forward(self, x):
        if (x.is_cuda and x.dim() == 2 and self.bias is not None and self.out_features <= 128
                and self.in_features % 16 == 0 and x.dtype == torch.float32):
            return LinearFn.apply(x, self.weight, self.bias)
        lib.note_off_path('bmnas.nn.Linear', f'input {tuple(x.shape)} {x.dtype} on {x.device}, out_features '
                          f'{self.out_features}, in_features {self.in_features}, bias {self.bias is not None}')
        return super().forward(x)


def _on_gpu(t):
    return t.device.type == 'cuda'


def _class_weight_ok(w, n_classes):
    """None, or what the kernels read by address: a contiguous 1-D fp32 device tensor with one entry per class."""
    return w is None or (w.dim() == 1 and w.shape[0] == n_classes and w.dtype == torch.float32 and _on_gpu(w)
                         and w.is_contiguous())


def _bare_ok(module, input, target):
    """The conditions under which the bare mean kernels ran before the options existed, unchanged: calls that took
    them then take them now."""
    if isinstance(module, nn.BCEWithLogitsLoss):
        return (_on_gpu(input) and module.weight is None and module.pos_weight is None and module.reduction == 'mean'
                and input.dtype == torch.float32 and target.dtype == torch.float32
                and tuple(input.shape) == tuple(target.shape))
    if isinstance(module, nn.CrossEntropyLoss):
        return (_on_gpu(input) and len(input.shape) == 2 and module.weight is None and module.reduction == 'mean'
                and module.label_smoothing == 0.0 and module.ignore_index == -100
                and target.dtype == torch.int64 and len(target.shape) == 1 and input.dtype == torch.float32)
    return False


def _criterion_plan(module, input, target):
    """-> None (the torch parent class runs), 'bare' (the kernels of the plain mean form: today's numbers) or 'crit'
    (the weighted / smoothed kernels, bmnas_criterion_t).  Reads shapes, dtypes and devices only."""
    if _bare_ok(module, input, target):
        return 'bare'
    if not (_on_gpu(input) and _on_gpu(target) and input.dtype == torch.float32 and len(input.shape) >= 1
            and module.reduction in ('mean', 'sum')):
        return None
    n_classes = input.shape[-1]
    if not _class_weight_ok(module.weight, n_classes):
        return None
    if isinstance(module, nn.BCEWithLogitsLoss):
        if not (target.dtype == torch.float32 and tuple(input.shape) == tuple(target.shape)
                and _class_weight_ok(module.pos_weight, n_classes)):
            return None
        return 'crit'
    if isinstance(module, nn.CrossEntropyLoss):
        # (class-index targets only: probability targets have the logits' dtype and shape)
        if not (len(input.shape) == 2 and target.dtype == torch.int64 and len(target.shape) == 1
                and target.shape[0] == input.shape[0] and 0.0 <= module.label_smoothing < 1.0):
            return None
        return 'crit'
    return None


def criterion_route(module, input, target):
    """'native': the call runs on the gfx950 kernels (csrc/linear.hip, or csrc/head.hip's backward launch inside
    fused_criterion()); 'torch': it warns once and runs the torch parent class.  A pure host decision over shapes,
    dtypes, devices and the module's options:

      BCEWithLogitsLoss   fp32 device logits (..., O) and targets of the same shape; `weight` / `pos_weight` absent or
                          contiguous 1-D fp32 device tensors of length O; reduction 'mean' | 'sum'.
      CrossEntropyLoss    fp32 device logits (b, O), int64 class-index targets (b); `weight` as above;
                          0 <= label_smoothing < 1; any ignore_index; reduction 'mean' | 'sum'.

    Everything else is 'torch': reduction='none', probability targets, weights of other shapes or dtypes, CPU tensors.
    The bare mean forms (no weight, no smoothing, ignore_index -100) are selected under exactly the conditions that
    selected them before the options existed (_bare_ok).
    A default-constructed CrossEntropyLoss() keeps the kernels of the bare mean form, which do NOT look for labels equal
    to its ignore_index of -100 (the reference's label sets hold none); give any other option, or another ignore_index,
    and ignored rows are honoured."""
    return 'torch' if _criterion_plan(module, input, target) is None else 'native'


def _crit_of(module, kind):
    return lib.Criterion(kind, weight=module.weight, pos_weight=getattr(module, 'pos_weight', None),
                         label_smoothing=getattr(module, 'label_smoothing', 0.0),
                         ignore_index=getattr(module, 'ignore_index', -100), reduction=module.reduction)


def relax_schedule_tau(tau_max, tau_min, epochs, epoch):
    """tau of epoch `epoch` on the exponential schedule tau_max * (tau_min / tau_max) ** (epoch / (epochs - 1)), formed
    in float64; epochs == 1 gives tau_max; epochs past the last hold tau_min."""
    if epochs == 1:
        return float(tau_max)
    e = min(max(int(epoch), 0), epochs - 1)
    return float(tau_max) * (float(tau_min) / float(tau_max)) ** (e / (epochs - 1))


class ArchRelaxation:
    """What the search hypernet softmaxes instead of its raw architecture tensors (FusionNetwork.set_relaxation):
         z = a / tau            an (annealed) temperature
         z = (a + G) / tau      gumbel=True: Gumbel-softmax sampling, fresh noise G every training step
    as ONE launch over all of them (bmnas.functions.ArchRelaxFn, csrc/relax.hip).  tau, the noise seed and the noise
    counter live in a small DEVICE block the launch reads by address, so a captured step honours a tau edited between
    replays and draws the noise of counter c, c + 1, ... on successive replays; nothing is frozen into a hipGraph.

    Noise is drawn iff `gumbel` and the owning module is in training mode; in eval mode z = a / tau and the counter
    stands still.  The stream is independent of the dropout stream (bmnas.cell.DROP): no dropout offset is consumed and
    the masks of a step are the same with and without the relaxation.  seed: None takes torch.initial_seed()."""

    def __init__(self, tau=1.0, gumbel=False, seed=None):
        self.gumbel = bool(gumbel)
        self.seed = int(torch.initial_seed() if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
        self.schedule = None                                      # (tau_max, tau_min, epochs)
        self.epoch = None
        self._state = torch.zeros(lib.RELAX_STATE_WORDS, dtype=torch.int64)     # moves to the device with its network
        signed = self.seed - (1 << 64) if self.seed >= (1 << 63) else self.seed
        self._state[1] = signed
        self._tau = None
        self.tau = tau

    # -- the device block ---------------------------------------------------------------------------------------------
    @property
    def state(self):
        """The int64 words of bmnas_arch_relax_state_t: tau (fp32 bits, low half of word 0) | seed | counter."""
        return self._state

    def to(self, device):
        """Move the block (before any capture: a captured launch holds its address)."""
        if self._state.device != torch.device(device):
            self._state = self._state.to(device)
        return self

    @property
    def tau(self):
        """The last value set (the host's mirror: reading it does not synchronise)."""
        return self._tau

    @tau.setter
    def tau(self, value):
        value = float(value)
        if not (value > 0.0 and value < float('inf')):
            raise ValueError(f'ArchRelaxation: tau must be a finite float > 0, got {value!r}')
        self._tau = value
        self._state.view(torch.float32)[0:1].fill_(value)         # one device fill, outside any replay

    @property
    def counter(self):
        """The noise counter, a one-element int64 view of the device block."""
        return self._state[2:3]

    def save_counter(self):
        return self.counter.clone()

    def restore_counter(self, t):
        self.counter.copy_(t, non_blocking=True)

    # -- schedule -----------------------------------------------------------------------------------------------------
    def set_schedule(self, tau_max, tau_min, epochs):
        tau_max, tau_min, epochs = float(tau_max), float(tau_min), int(epochs)
        if not (tau_min > 0.0 and tau_max < float('inf')):
            raise ValueError(f'ArchRelaxation: the schedule needs 0 < tau_min and a finite tau_max, got tau_min '
                             f'{tau_min!r}, tau_max {tau_max!r}')
        if tau_min > tau_max:
            raise ValueError(f'ArchRelaxation: tau_min {tau_min!r} > tau_max {tau_max!r} (the schedule anneals downwards)')
        if epochs < 1:
            raise ValueError(f'ArchRelaxation: the schedule needs epochs >= 1, got {epochs!r}')
        self.schedule = (tau_max, tau_min, epochs)
        return self

    def set_epoch(self, epoch):
        """tau of this epoch on the schedule (no schedule: tau stays).  -> tau."""
        self.epoch = int(epoch)
        if self.schedule is not None:
            self.tau = relax_schedule_tau(*self.schedule, self.epoch)
        return self.tau

    # -- state --------------------------------------------------------------------------------------------------------
    def state_dict(self):
        return dict(tau=self._tau, gumbel=self.gumbel, seed=self.seed, counter=self.counter.detach().cpu().clone(),
                    schedule=None if self.schedule is None else tuple(self.schedule), epoch=self.epoch)

    def load_state_dict(self, sd):
        self.gumbel = bool(sd['gumbel'])
        self.seed = int(sd['seed']) & 0xFFFFFFFFFFFFFFFF
        self._state[1:2].fill_(self.seed - (1 << 64) if self.seed >= (1 << 63) else self.seed)
        self.schedule = None if sd.get('schedule') is None else tuple(sd['schedule'])
        self.epoch = sd.get('epoch')
        self.tau = sd['tau']
        self.counter.copy_(torch.as_tensor(sd['counter'], dtype=torch.int64).reshape(1))

    # -- the launch ---------------------------------------------------------------------------------------------------
    def draws(self, training):
        return self.gumbel and bool(training)

    def __call__(self, training, *logits):
        """-> the tuple of z, one per tensor of `logits`, as ONE autograd node; with noise (and the counter moved on by
        one) iff gumbel and training."""
        from .functions import ArchRelaxFn
        dev = next((t.device for t in logits if t.is_cuda), None)
        if dev is None:
            raise RuntimeError('bmnas: the architecture relaxation needs its tensors on a HIP device; the fusion-cell '
                               'hot path runs only on the gfx950 kernels — there is no CPU fallback')
        self.to(dev)
        draw = self.draws(training)
        return ArchRelaxFn.apply(self._state, draw, draw, *logits)

    def peek(self, *logits, training=True):
        """The forward with the counter left where it is -> (z, noise): what the NEXT training step will hand to the
        softmax and the Gumbel noise it will draw (zeros without `gumbel` or in eval mode).  The audit export."""
        dev = next((t.device for t in logits if t.is_cuda), None)
        if dev is None:
            raise RuntimeError('bmnas: ArchRelaxation.peek needs tensors on a HIP device')
        self.to(dev)
        a = [t.detach().to(dev).float().contiguous() for t in logits]
        z = [torch.empty_like(t) for t in a]
        noise = [torch.zeros_like(t) for t in a]
        lib.arch_relax_fwd(a, z, noise, self._state, self.draws(training), False)
        return z, noise


class BCEWithLogitsLoss(nn.BCEWithLogitsLoss):
    def forward(self, input, target):
        plan = _criterion_plan(self, input, target)
        if plan is not None:
            crit = _crit_of(self, 'bce') if plan == 'crit' else None
            head = _deferrable(input)
            if head is not None:
                return DeferredLossFn.apply(input, target, head, 'bce', crit)
            if crit is not None:
                return BCEWithLogitsCritFn.apply(input, target, crit)
            return BCEWithLogitsFn.apply(input, target)
        lib.note_off_path('bmnas.nn.BCEWithLogitsLoss', f'input {tuple(input.shape)} {input.dtype} on {input.device}, '
                          f'target {tuple(target.shape)} {target.dtype}, reduction {self.reduction}')
        return super().forward(input, target)


class CrossEntropyLoss(nn.CrossEntropyLoss):
    def forward(self, input, target):
        plan = _criterion_plan(self, input, target)
        if plan is not None:
            crit = _crit_of(self, 'ce') if plan == 'crit' else None
            head = _deferrable(input)
            if head is not None:
                return DeferredLossFn.apply(input, target, head, 'ce', crit)
            if crit is not None:
                return CrossEntropyCritFn.apply(input, target, crit)
            return CrossEntropyFn.apply(input, target)
        lib.note_off_path('bmnas.nn.CrossEntropyLoss', f'input {tuple(input.shape)} {input.dtype} on {input.device}, '
                          f'target {tuple(target.shape)} {target.dtype}, reduction {self.reduction}')
        return super().forward(input, target)
