"""Shared pieces of the per-dataset search drivers (the reference repeats them three times in
{mmimdb,ntu,ego}_darts_searchable.py).  Not part of the reference's public surface."""
import contextlib

import torch
import torch.nn as nn
import torch.optim as op
from bmnas.optim import SGD, Adam     # torch.optim.Adam / SGD semantics, one HIP launch per step

import models.auxiliary.scheduler as sc
from bmnas import dist as bdist
from bmnas import nn as bnn

from .darts.architect import Architect
from .darts.model import Found_FusionNetwork
from .darts.model_search import FusionNetwork
from .plot_genotype import Plotter


def parallel_flag(args):
    """The reference's library reads args.parallel while two of its mains define
    --use_dataparallel; accept either."""
    return bool(getattr(args, 'parallel', getattr(args, 'use_dataparallel', False)))


def data_parallel_world(args=None):
    """Number of data-parallel replicas.  The reference turns nn.DataParallel on with
    `args.parallel` when several GPUs are visible (mmimdb_darts_searchable.py:36); here the
    replicas are processes, so the launch itself is the request: WORLD_SIZE > 1 (torchrun /
    torch.distributed.run) means data parallel, whatever the flag says — N independent full
    searches writing the same checkpoint directory are never what the launch meant."""
    return bdist.env_world()


def _class_vector(args, name, device):
    """args.<name> as an fp32 tensor of num_outputs entries, or None when the argument set has none."""
    values = getattr(args, name, None)
    if values is None:
        return None
    t = torch.as_tensor([float(v) for v in values], dtype=torch.float32, device=device)
    if t.numel() != args.num_outputs:
        raise ValueError(f'args.{name} has {t.numel()} entries, the task has {args.num_outputs} outputs')
    return t


def make_criterion(kind, args, device=None):
    """The search drivers' criterion: kind 'bce' (MM-IMDB, reference mmimdb_darts_searchable.py:22) or 'ce' (NTU, Ego).
    The reference's argument sets give the bare mean criterion, exactly as before.  Optional, all read with getattr:
      args.pos_weight       'bce': num_outputs floats, the weight of each genre's positive term
      args.class_weight     num_outputs floats, the per-class rescaling weight of either criterion
      args.label_smoothing  'ce': a float in [0, 1)
    The weight tensors are buffers of the criterion, which the hypernet holds as a submodule: they move with
    model.to(device) and are read by address by the gfx950 kernels (bmnas.nn.criterion_route)."""
    weight = _class_vector(args, 'class_weight', device)
    if kind == 'bce':
        return bnn.BCEWithLogitsLoss(weight=weight, pos_weight=_class_vector(args, 'pos_weight', device))
    if kind == 'ce':
        return bnn.CrossEntropyLoss(weight=weight, label_smoothing=float(getattr(args, 'label_smoothing', 0.0)))
    raise ValueError(f'criterion kind {kind!r}')


BACKBONE_DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}


def backbone_dtype_option(args):
    """args.backbone_dtype (optional; the reference's argument sets have none): 'bf16' or 'fp16' runs the backbones —
    and only them — under torch.autocast, so the reshape layers are handed half feature maps, which their pooling
    launch reads as they are (half the bytes of the step's largest tensors; the pooled tensors and everything behind
    them stay fp32).  Absent or None: the backbones run as they always did.  -> torch dtype or None."""
    value = getattr(args, 'backbone_dtype', None)
    if value is None:
        return None
    if value not in BACKBONE_DTYPES:
        from bmnas.lib import BmnasError
        raise BmnasError(f"args.backbone_dtype must be 'bf16', 'fp16' or absent / None, got {value!r}")
    return BACKBONE_DTYPES[value]


class HyperNetBase(nn.Module):
    """backbones (set by the subclass) -> reshape_layers -> fusion_net -> central_classifier.
    Attribute names are the reference's: trainers reach into .reshape_layers / .fusion_net."""

    param_group_order = ('reshape_layers', 'fusion_net', 'central_classifier')

    def _build_head(self, args, criterion, reshape_layers, num_input_nodes, num_keep_edges,
                    genotype=None, logger=None):
        self.args = args
        self._backbone_dtype = backbone_dtype_option(args)
        self.criterion = criterion
        self._criterion = criterion
        self.reshape_layers = reshape_layers
        self.multiplier = args.multiplier
        self.steps = args.steps
        self.parallel = parallel_flag(args)
        self.num_input_nodes = num_input_nodes
        self.num_keep_edges = num_keep_edges
        if genotype is None:
            self.fusion_net = FusionNetwork(steps=self.steps, multiplier=self.multiplier,
                                            num_input_nodes=num_input_nodes, num_keep_edges=num_keep_edges,
                                            args=args, criterion=criterion, logger=logger)
        else:
            self._genotype = genotype
            self.fusion_net = Found_FusionNetwork(steps=self.steps, multiplier=self.multiplier,
                                                  num_input_nodes=num_input_nodes,
                                                  num_keep_edges=num_keep_edges, args=args,
                                                  criterion=criterion, genotype=genotype)
        # nn.Linear subclass (same parameters / state_dict keys) running on the MFMA kernels
        self.central_classifier = bnn.Linear(args.C * args.L * self.multiplier, args.num_outputs)

    @staticmethod
    def make_reshape_layers(layer_cls, C_ins, args, genotype=None):
        """One reshape layer per backbone feature; a found net keeps only those its genotype
        uses (the others become parameter-free nn.ReLU placeholders, as in the reference)."""
        used = None if genotype is None else {e[1] for e in genotype.edges}
        layers = nn.ModuleList()
        for i, c_in in enumerate(C_ins):
            if used is None or i in used:
                layers.append(layer_cls(c_in, args.C, args.L, args))
            else:
                layers.append(nn.ReLU())
        return layers

    def backbone_autocast(self):
        """The context the forwards run their backbones in (never self.fuse): torch.autocast to args.backbone_dtype on
        the model's device, or nothing at all without the option."""
        dtype = getattr(self, '_backbone_dtype', None)
        if dtype is None:
            return contextlib.nullcontext()
        p = next(self.parameters(), None)
        return torch.autocast(device_type='cuda' if p is None else p.device.type, dtype=dtype)

    def reshape_input_features(self, input_features):
        # = [layer(f) for layer, f in zip(self.reshape_layers, input_features)], the conv stacks of all
        # modalities in one grouped set of launches (models.auxiliary.aux_models.reshape_all)
        import models.auxiliary.aux_models as aux
        return aux.reshape_all(list(self.reshape_layers), list(input_features))

    def fuse(self, raw_features):
        feats = self.reshape_input_features(list(raw_features))
        if hasattr(self.fusion_net, 'forward_classified'):        # search hypernet: K7 + classifier fused
            return self.fusion_net.forward_classified(feats, self.central_classifier)
        return self.central_classifier(self.fusion_net(feats))

    def genotype(self):
        if hasattr(self, '_genotype'):
            return self._genotype
        return self.fusion_net.genotype()

    def central_params(self):
        return [{'params': getattr(self, name).parameters()} for name in self.param_group_order]

    def _loss(self, input_features, labels):
        return self._criterion(self(input_features), labels)

    def arch_parameters(self):
        return self.fusion_net.arch_parameters()


def _make_optimizer(args, prefix, params, lr, weight_decay, max_grad_norm, betas=(0.9, 0.999)):
    """The weight (prefix '') or alpha (prefix 'arch_') optimizer of search_setup: bmnas.optim.Adam with the arguments it
    always had unless args.<prefix>optimizer says 'sgd'."""
    kind = getattr(args, prefix + 'optimizer', 'adam')
    if kind == 'adam':
        return Adam(params, lr=lr, betas=betas, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                    amsgrad=bool(getattr(args, prefix + 'amsgrad', False)),
                    decoupled_weight_decay=bool(getattr(args, prefix + 'decoupled_weight_decay', False)))
    if kind == 'sgd':
        return SGD(params, lr=lr, momentum=getattr(args, prefix + 'momentum', 0.9),
                   dampening=getattr(args, prefix + 'dampening', 0), weight_decay=weight_decay,
                   nesterov=bool(getattr(args, prefix + 'nesterov', False)), max_grad_norm=max_grad_norm)
    raise ValueError(f"args.{prefix}optimizer must be 'adam' or 'sgd', got {kind!r}")


def averaging_options(args, status):
    """Weight averaging of a found-stage run (optional; the reference's argument sets have none of these):
      args.ema_decay            a float in [0, 1]: an exponential moving average of the weights, updated after every weight
                                step and evaluated instead of the live weights — the usual last step of a retraining run
      args.swa_start            an epoch: stochastic weight averaging, one snapshot at the end of every epoch from this
                                one on (the scheduler is SGDR with warm restarts: a snapshot per restart is the SWA recipe)
      args.average_skip_frozen  default True: parameters with requires_grad=False (the frozen backbones) are copied once
                                and left out of later updates
    -> None when neither is set, else dict(decay, swa_start, skip_frozen).  Refused in a search (status != 'eval'):
    averaged weights would not belong to the current alphas."""
    decay, swa_start = getattr(args, 'ema_decay', None), getattr(args, 'swa_start', None)
    if decay is None and swa_start is None:
        return None
    if status != 'eval':
        raise ValueError("args.ema_decay / args.swa_start average the weights of a found-stage run (status 'eval') only: "
                         f"in a search (status {status!r}) the averaged weights would not belong to the current alphas")
    if decay is not None and swa_start is not None:
        raise ValueError('args.ema_decay and args.swa_start are two recipes over one averaged model: set one of them')
    if decay is not None:
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f'args.ema_decay must be in [0, 1], got {decay!r}')
    else:
        swa_start = int(swa_start)
        if swa_start < 0:
            raise ValueError(f'args.swa_start must be an epoch >= 0, got {swa_start!r}')
    return dict(decay=decay, swa_start=swa_start, skip_frozen=bool(getattr(args, 'average_skip_frozen', True)))


def update_bn_option(args, status, world=None):
    """args.swa_update_bn (optional, default False; needs args.ema_decay or args.swa_start): the averaged module's
    BatchNorm statistics are recomputed by bmnas.optim.update_bn — one cumulative pass over the training loader — before
    it is evaluated, instead of being averaged like weights (the step the SWA recipe ends with).  -> bool.  Refused in a
    search like the averaging options, and under data parallelism (world: the number of ranks; None: asks
    torch.distributed): every rank would see only its shard of the training data and the ranks' statistics would differ."""
    if not getattr(args, 'swa_update_bn', False):
        return False
    if status != 'eval':
        raise ValueError("args.swa_update_bn belongs to the weight averaging of a found-stage run (status 'eval'): "
                         f"refused in a search (status {status!r})")
    if getattr(args, 'ema_decay', None) is None and getattr(args, 'swa_start', None) is None:
        raise ValueError('args.swa_update_bn recomputes the BatchNorm statistics of the AVERAGED model: set '
                         'args.ema_decay or args.swa_start with it')
    if world is None:
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    if world > 1:
        raise ValueError(f'args.swa_update_bn is not available under data parallelism ({world} ranks): every rank would '
                         'see only its shard of the training loader, so the ranks would end with different statistics')
    return True


def device_stats_option(args, meter):
    """args.device_stats (optional, default False; the reference's argument sets have none): the trainer loop keeps its
    phase statistics — loss sum, accuracy or F1 counts — in one device accumulator tallied by ONE launch per batch
    (bmnas.metrics.PhaseStats; inside the replay where the batch is a captured gradient-free forward) instead of the
    aten launches of `loss_sum += ...; meter.update(...)`.  -> the PhaseStats that stands in for `meter` (kept ON the
    meter across run() / evaluate() calls: captured forwards hold its accumulator), or None — the option is absent or
    false, or the meter is not one of the loop's own (PhaseStats.from_meter): the loop then does what it always did."""
    if not getattr(args, 'device_stats', False):
        return None
    from bmnas.metrics import PhaseStats
    fresh = PhaseStats.from_meter(meter)
    if fresh is None:
        return None
    kept = meter.__dict__.get('_bmnas_phase_stats')
    if kept is not None and (kept.kind, kept.f1_type, kept.threshold) == (fresh.kind, fresh.f1_type, fresh.threshold):
        return kept
    meter.__dict__['_bmnas_phase_stats'] = fresh
    return fresh


def relaxation_option(args, status, num_epochs, world=None):
    """The relaxation of the architecture weights in a search (optional; the reference's argument sets have none of these
    and its softmax is the one at temperature 1):
      args.arch_tau      a float > 0 (default 1): the hypernet softmaxes a / tau
      args.arch_tau_min  with it tau anneals from arch_tau down to arch_tau_min over the run's epochs, exponentially
                         (bmnas.nn.ArchRelaxation.set_schedule; the loop calls set_epoch at the top of every epoch)
      args.arch_gumbel   bool: Gumbel-softmax sampling, softmax((a + G) / tau) with fresh noise every training step; the
                         noise seed is args.seed when present, else torch.initial_seed()
    -> a bmnas.nn.ArchRelaxation for FusionNetwork.set_relaxation, or None when none of them is set (the run is then what
    it always was).  Refused: a found-stage run (status 'eval': no architecture weights), args.unrolled (the + and - passes
    of the difference quotient would need the same draw — ArchRelaxation.save_counter / restore_counter exist for that,
    the step is not wired to them) and data parallelism (world: the number of ranks; None: asks torch.distributed and the
    environment — an idle replica of an uneven scatter skips its forward and its noise counter would fall behind)."""
    tau, tau_min = getattr(args, 'arch_tau', None), getattr(args, 'arch_tau_min', None)
    gumbel = bool(getattr(args, 'arch_gumbel', False))
    if tau is None and tau_min is None and not gumbel:
        return None
    if status == 'eval':
        raise ValueError("args.arch_tau / args.arch_tau_min / args.arch_gumbel relax the architecture weights of a search: "
                         "a found-stage run (status 'eval') has none")
    if bool(getattr(args, 'unrolled', False)):
        raise ValueError('args.arch_tau / args.arch_tau_min / args.arch_gumbel cannot be combined with args.unrolled (the '
                         'two passes of its difference quotient would need the same noise draw; not wired)')
    if world is None:
        import torch.distributed as dist
        world = max(data_parallel_world(args),
                    dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1)
    if world > 1:
        raise ValueError(f'args.arch_tau / args.arch_tau_min / args.arch_gumbel are not available under data parallelism '
                         f'({world} ranks): a replica that idles through a batch would fall behind in the noise counter')
    tau = 1.0 if tau is None else float(tau)
    seed = getattr(args, 'seed', None)
    relax = bnn.ArchRelaxation(tau=tau, gumbel=gumbel, seed=None if seed is None else int(seed))
    if tau_min is not None:
        relax.set_schedule(tau, float(tau_min), int(num_epochs))
    return relax


def make_averager(model, args, status):
    """-> (bmnas.optim.AveragedModel of `model`, its options), or (None, None) without the options.  use_buffers=True
    — averaged running statistics stand in for swa_utils.update_bn's cumulative pass — unless args.swa_update_bn asks
    for that pass (update_bn_option; opts['update_bn']): then the buffers are not averaged and the loop recomputes them
    with bmnas.optim.update_bn before the averaged module is evaluated."""
    opts = averaging_options(args, status)
    if opts is None:
        update_bn_option(args, status)           # (alone it is an error, not a silent no-op)
        return None, None
    opts['update_bn'] = update_bn_option(args, status)
    from bmnas.optim import AveragedModel
    return AveragedModel(model, decay=opts['decay'], use_buffers=not opts['update_bn'],
                         skip_frozen=opts['skip_frozen']), opts


def search_setup(model, args, criterion, device, num_batches_per_epoch, weight_decay):
    """Optimizers, scheduler, device placement, data parallelism and the Architect — the body of
    the reference's train_darts_model between model construction and the trainer call
    (mmimdb_darts_searchable.py:26-40).  nn.DataParallel is replaced by per-process replicas
    whose optimizers average gradients over RCCL right before step() (bmnas.dist)."""
    # args.grad_clip / args.arch_grad_clip (optional; the reference's argument sets have neither, DARTS ships
    # `--grad_clip 5`): the global gradient-norm clip of the weight / alpha step, inside the one-launch Adam step
    # (bmnas.optim.Adam(max_grad_norm=...): captured steps included; `.grad` stays unclipped)
    # args.amsgrad / args.decoupled_weight_decay and args.arch_amsgrad / args.arch_decoupled_weight_decay (optional; the
    # reference's argument sets have none of them): torch.optim.Adam's two switches for the weight / alpha optimizer —
    # the running maximum of the second moment, and AdamW's decay on the parameter instead of the gradient — in the same
    # one launch (bmnas_adam_multi_ex), captured steps included; absent, the optimizers are the ones they always were
    # args.optimizer / args.arch_optimizer in {'adam', 'sgd'} (optional, default 'adam'; the reference's argument sets have
    # neither): 'sgd' is DARTS' weight optimizer (models/search/darts/train_search.py:84-88), bmnas.optim.SGD with
    # args.momentum (default 0.9), args.dampening, args.nesterov — arch_momentum / arch_dampening / arch_nesterov for the
    # alpha optimizer — on one bmnas_sgd_multi launch; grad_clip / arch_grad_clip, the scheduler and bdist.attach apply
    # to it unchanged
    # args.unrolled (optional, DARTS' `--unrolled`, which the reference still parses at main_darts_found_ntu.py:48 and
    # models/search/darts/train_search.py:42) / args.unrolled_r (default 1e-2): the Architect runs DARTS' unrolled
    # second-order step (architect.Architect._step_unrolled) with the weight optimizer built here — its learning rate is
    # the step's eta, its weight_decay and momentum buffers enter the virtual step —, eagerly, single-process only; the
    # trainer loop then hands it one training batch per dev batch.  Absent: the first-order step, as it always was
    optimizer = _make_optimizer(args, '', model.central_params(), lr=args.eta_max, weight_decay=weight_decay,
                                max_grad_norm=getattr(args, 'grad_clip', None))
    scheduler = sc.LRCosineAnnealingScheduler(args.eta_max, args.eta_min, args.Ti, args.Tm,
                                              num_batches_per_epoch)
    arch_optimizer = _make_optimizer(args, 'arch_', model.arch_parameters(), lr=args.arch_learning_rate,
                                     weight_decay=args.arch_weight_decay,
                                     max_grad_norm=getattr(args, 'arch_grad_clip', None), betas=(0.5, 0.999))
    if data_parallel_world(args) > 1:
        # one process per GPU: the unchanged mains pass cuda:0 to every rank
        # (main_darts_searchable_mmimdb.py:86), so the rank's own device comes from LOCAL_RANK,
        # BEFORE the model moves; the trainer loops follow the model's device (_loop.run)
        _, local, _ = bdist.init_from_env()
        if torch.device(device).type == 'cuda':
            device = torch.device('cuda', local)
            torch.cuda.set_device(device)
    model.to(device)
    if data_parallel_world(args) > 1:
        bdist.broadcast_state(model, model.arch_parameters())
        bdist.attach(optimizer)
        bdist.attach(arch_optimizer)
    architect = Architect(model, args, criterion, arch_optimizer, network_optimizer=optimizer)
    return optimizer, scheduler, architect, Plotter(args)
