"""The epoch / phase loop shared by the three dataset trainers.

Behaviour follows the reference's train_searchable/{mmimdb,ntu,ego}.py: phase order, model.train()
in BOTH the train and dev phases of a search, Architect.step on every dev batch followed by a
no-grad forward for the metric, per-batch cosine schedule, best-dev checkpoint + genotype pickle.
Differences, all on the host side of the hot path:
  * the per-batch .item() / .cpu() syncs are gone: loss and metric statistics accumulate on the
    device and are read once per phase (same numbers, no stall per batch);
  * `parallel` means one process per GPU (bmnas.dist); statistics are summed over ranks and only
    rank 0 writes checkpoints — there is no `.module` indirection;
  * the weight step (forward + criterion + backward + Adam) and the Architect step are captured
    once and replayed as one hipGraph launch per batch (bmnas.graph.GraphedTrainStep); a ragged
    last batch, or a model that cannot be captured, runs the eager path.  On by default for
    single-process runs; `args.hip_graph` / BMNAS_HIP_GRAPH switch it (GraphedTrainStep.enabled);
  * the gradient-free passes — the metric forward of every dev batch after `architect.step`, the
    eval / test passes — are hipGraph replays too (bmnas.graph.GraphedForward, one graph per module
    mode and batch shape): issued eagerly that forward is host-bound, 0.55-0.86 ms against 0.11 ms;
  * optional, found-stage runs (status 'eval') only: weight averaging (models.search._common.averaging_options:
    args.ema_decay / args.swa_start / args.average_skip_frozen) on bmnas.optim.AveragedModel — an EMA updated after
    every weight step (inside the replay when the step is captured, eagerly on ragged batches) or an SWA snapshot at
    the end of every epoch from args.swa_start on; the phases that do not learn then evaluate the AVERAGED module and
    `best_test_averaged.pt` is saved next to `best_test_model.pt`.  args.swa_update_bn adds the step the SWA recipe
    ends with: the averaged module's BatchNorm statistics are not averaged but recomputed by one cumulative pass over
    the training loader (bmnas.optim.update_bn) before its first evaluation after the weights changed
    (run.stats['update_bn_passes']).  With no option set nothing changes;
  * optional: gradient accumulation (`accum_steps`: args.accum_steps = m > 1).  The weight steps of the learning phases
    hold m batches and take ONE optimizer step per group — the reference's `--batchsize 96 --parallel` step on fewer
    GPUs than the paper's: nn.DataParallel sums the mean-reduced gradients of its shards, here m micro-batches are
    combined with weights n_i / N (bmnas.optim.GradAccumulator, one bmnas_grad_combine_multi launch).  A full group
    of one shape is one replay of a GraphedTrainStep(accumulate=m); the ragged tail of a phase — fewer than m batches,
    or a shorter last one — is ONE eager accumulated step over what is there, never a run of single steps:
    ceil(batches / m) optimizer steps per phase.  The cosine scheduler still advances once per batch (the schedule's
    length is unchanged; a step runs with the rates after its group's last batch), the EMA updates once per optimizer
    step, `_observe('batch', ...)` fires per micro-batch, the architecture step stays one per dev batch.  BatchNorm
    running statistics advance once per MICRO-batch (nn.DataParallel keeps only replica 0's).  Absent or 1, the loop does
    what it does without it.
"""
import copy
import os

import torch
import torch.distributed as dist

import models.auxiliary.scheduler as sc
from models.search.darts.utils import count_parameters, save, save_pickle


def _world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _rank():
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _all_sum(t):
    if _world() > 1:
        from bmnas import dist as bdist
        bdist.all_reduce(t, dist.ReduceOp.SUM)
    return t


def _model_device(model, device):
    """Under data parallelism every rank's replica sits on its own GPU (search_setup places it by
    LOCAL_RANK) while the unchanged mains hand `cuda:0` to every rank: follow the model."""
    if _world() > 1:
        for p in model.parameters():
            return p.device
    return device


def _is_sharded(loader):
    from torch.utils.data.distributed import DistributedSampler
    return isinstance(getattr(loader, 'sampler', None), DistributedSampler)


def _shard_batch(inputs, labels):
    """A loader without a DistributedSampler yields the GLOBAL batch on every rank: keep this rank's contiguous slice,
    cut the way nn.DataParallel's scatter cuts it (mmimdb_darts_searchable.py:36-37; `bmnas.dist.uneven_bounds`:
    Tensor.chunk — ceil(n / world) samples per replica until the batch is used up, so the last replicas may get fewer
    or none).  The reference's loss is ONE mean over the n gathered outputs; a rank's mean over its own n_rank samples
    enters the gradient average with weight n_rank * world / n (`bmnas.dist.set_shard_weight`, applied by the reducer:
    eager steps scale the bucket, captured steps their loss — and are replayed only for the weight they were captured
    with).  A rank left without samples idles through the batch (`_idle_step`): zero gradients into the same
    collective, the same averaged update."""
    from bmnas import dist as bdist
    world, rank = _world(), _rank()
    n = labels.shape[0]
    start, length = bdist.uneven_bounds(n, rank, world)
    bdist.set_shard_weight(length * world / n if n else 1.0)
    cut = lambda t: t.narrow(0, start, length) if torch.is_tensor(t) and t.dim() > 0 else t
    if isinstance(inputs, (tuple, list)):
        inputs = type(inputs)(cut(t) for t in inputs)
    else:
        inputs = cut(inputs)
    return inputs, cut(labels)


def _weight():
    from bmnas import dist as bdist
    return bdist.shard_weight()


def _set_weight(w):
    from bmnas import dist as bdist
    bdist.set_shard_weight(w)


def _idle_step(optimizer):
    """This rank got no sample of the batch (uneven scatter): it still joins the step's ONE collective — with zero
    gradients, its shard weight is 0 — and applies the averaged gradients like every other rank."""
    for group in optimizer.param_groups:
        for p in group['params']:
            p.grad = torch.zeros_like(p)
    optimizer.step()


class AccuracyMeter:
    name = 'Acc'

    def reset(self, device):
        self.correct = torch.zeros((), device=device, dtype=torch.float64)

    def update(self, output, labels):
        self.correct += (output.argmax(1) == labels).sum()

    def compute(self, n):
        return float(_all_sum(self.correct.clone())) / n


class F1Meter:
    """weighted / macro / ... F1 of sigmoid(output) > threshold, like the reference's sklearn call."""

    def __init__(self, f1_type='weighted', th=0.3):
        self.f1_type, self.th = f1_type, th
        self.name = f'{f1_type} F1'

    def reset(self, device):
        self.preds, self.labels = [], []

    def update(self, output, labels):
        self.preds.append(torch.sigmoid(output) > self.th)
        self.labels.append(labels)

    def compute(self, n):
        from sklearn.metrics import f1_score
        y_pred = torch.cat(self.preds).cpu().numpy()
        y_true = torch.cat(self.labels).cpu().numpy()
        if _world() > 1:                       # gather every rank's shard on every rank
            objs = [None] * _world()
            dist.all_gather_object(objs, (y_pred, y_true))
            import numpy as np
            y_pred = np.concatenate([o[0] for o in objs])
            y_true = np.concatenate([o[1] for o in objs])
        return float(f1_score(y_true, y_pred, average=self.f1_type, zero_division=1))


def _tally(dstats, counters, loss_sum, meter, loss, output, labels, rode=False):
    """One batch into the phase statistics.  dstats None (args.device_stats absent or false, or a meter that is not the
    loop's own): the two statements the loop always had — loss_sum and meter are updated in place.  Else ONE tally
    through the bmnas.metrics.PhaseStats: `rode` — the replay that produced (loss, output) ended in the tally itself
    (_ForwardGraphs.tallied), nothing is issued; otherwise one launch behind the replay / eager step that reads the
    (static) loss and output tensors.  counters: run.stats / evaluate.stats."""
    if dstats is None:
        loss_sum += loss.detach().double() * labels.size(0)
        meter.update(output.detach(), labels)
        return
    if rode:
        counters['stat_in_replay'] += 1
        return
    before = dstats.launches, dstats.fallbacks
    dstats.update(loss.detach(), output.detach(), labels)
    counters['stat_launches'] += dstats.launches - before[0]
    counters['stat_fallbacks'] += dstats.fallbacks - before[1]


def fusion_params(model):
    n = sum(count_parameters(layer) for layer in model.reshape_layers)
    return n + count_parameters(model.fusion_net)


class _ForwardGraphs:
    """The gradient-free passes of the loops (metric pass of the dev phase, eval / test) as hipGraph replays
    (bmnas.graph.GraphedForward): one graph per (module mode, batch shape), at most three capture attempts; anything
    that does not fit — a ragged last batch, host tensors, a module that cannot be captured — stays eager."""

    def __init__(self, args, logger=None):
        from bmnas.graph import GraphedTrainStep
        self.on = GraphedTrainStep.enabled(args)
        self.graphs, self.attempts, self.logger = [], 0, logger
        self.replays = 0
        self.tallied = False         # whether the LAST replay tallied its batch itself (a graph built with stats=)

    def __deepcopy__(self, memo):
        """A deep copy of the model (bmnas.optim.AveragedModel) starts without graphs: these read the ORIGINAL's
        parameters, and a captured graph cannot be copied."""
        new = _ForwardGraphs.__new__(_ForwardGraphs)
        new.on, new.graphs, new.attempts, new.logger, new.replays = self.on, [], 0, self.logger, 0
        new.tallied = False
        return new

    @staticmethod
    def of(model, criterion, args, logger=None):
        """The graphs of (model, criterion), kept ON the model across run() / evaluate() calls: a capture costs three
        eager warm-ups, a rehearsal and a private pool — more than a short eval loader saves if every epoch's eval
        pass captured again.  (The graphs read the parameters in place: optimizer steps and load_state_dict are seen.)"""
        cache = model.__dict__.setdefault('_bmnas_forward_graphs', {})
        # keyed by id(), but the entry HOLDS its criterion: an id can be re-used by a new object once the old one is
        # freed (a criterion rebuilt per stage with another pos_weight), and a captured graph has its criterion baked
        # in — an entry whose criterion is not this very object is dropped together with its graphs' pools
        entry = cache.get(id(criterion))
        if entry is not None and entry[0] is not criterion:
            del cache[id(criterion)]
            entry = None
        if entry is None:
            entry = cache[id(criterion)] = (criterion, _ForwardGraphs(args, logger))
        fg = entry[1]
        from bmnas.graph import GraphedTrainStep
        fg.on = GraphedTrainStep.enabled(args)
        fg.replays = 0
        return fg

    def __call__(self, model, criterion, inputs, labels, stats=None):
        """-> (loss, output) from a replay, or None: run the pass eagerly.  stats (args.device_stats: a
        bmnas.metrics.PhaseStats): the graphs are built with it and end in its tally — `self.tallied` says whether the
        replay just taken did; a graph serves only the stats object it was built for (None: the graphs of always)."""
        self.tallied = False
        if not self.on:
            return None
        for g in self.graphs:
            if getattr(g, 'stats_for', None) is stats and g.matches(model, inputs, labels):
                self.replays += 1
                self.tallied = g.stats is not None
                return g(inputs, labels)
        if self.attempts >= 3:
            return None
        self.attempts += 1
        from bmnas.graph import GraphedForward
        if stats is None:
            g = GraphedForward.try_build(model, criterion, inputs, labels, self.logger)
        else:
            g = GraphedForward.try_build(model, criterion, inputs, labels, self.logger, stats=stats)
        if not g:
            return None
        g.stats_for = stats
        self.graphs.append(g)
        self.replays += 1
        self.tallied = g.stats is not None
        return g(inputs, labels)


def steps_per_replay(args):
    """How many weight steps the trainer captures into ONE hipGraph replay (`args.steps_per_replay`, else the environment
    variable BMNAS_STEPS_PER_REPLAY, else 1; at most 8).  With k > 1 the loop keeps k batches resident and replays a
    k-step graph — same batches, same order, same per-batch learning rates as the reference's one-by-one loop
    (train_searchable/mmimdb.py:73-113) —; a ragged tail of fewer than k batches runs as single steps."""
    v = getattr(args, 'steps_per_replay', None)
    if v is None:
        v = os.environ.get('BMNAS_STEPS_PER_REPLAY')
    try:
        k = int(v) if v is not None else 1
    except (TypeError, ValueError):
        k = 1
    return max(1, min(k, 8))


def accum_steps(args):
    """How many batches the learning phases accumulate into ONE optimizer step (`args.accum_steps`; absent, None or
    unreadable: 1; at most bmnas.lib.accum_max(), the parts one combine launch sums)."""
    v = getattr(args, 'accum_steps', None)
    try:
        m = int(v) if v is not None else 1
    except (TypeError, ValueError):
        m = 1
    if m <= 1:
        return 1
    from bmnas import lib
    return min(m, lib.accum_max())


def check_accum(args, world=None):
    """What `run` refuses at its start with args.accum_steps > 1: k steps per replay (each of the k steps would need its
    own group), the unrolled architecture step (it draws training batches of its own between weight steps), and data
    parallelism (one all-reduce per group is not built).  -> accum_steps(args)."""
    m = accum_steps(args)
    if m <= 1:
        return 1
    if steps_per_replay(args) > 1:
        raise ValueError(f'args.accum_steps = {m} cannot be combined with steps_per_replay = {steps_per_replay(args)} '
                         '(k optimizer steps per replay and m batches per optimizer step are two groupings of the '
                         'same batches: set one of them)')
    if bool(getattr(args, 'unrolled', False)):
        raise ValueError(f'args.accum_steps = {m} cannot be combined with args.unrolled (the unrolled architecture step '
                         'reads the weight optimizer between weight steps)')
    world = _world() if world is None else world
    if world > 1:
        raise ValueError(f'args.accum_steps = {m} is not available under data parallelism ({world} ranks): scale the '
                         'number of ranks, or accumulate in a single process')
    return m


def _set_relaxation(model, args, status, num_epochs):
    """args.arch_tau / args.arch_tau_min / args.arch_gumbel (models.search._common.relaxation_option, which refuses the
    combinations that are not built before anything moves) -> the bmnas.nn.ArchRelaxation now set on model.fusion_net, or
    None without the options: the model is then not touched.  A relaxation left on the network by an earlier run() is
    kept — captured steps hold the address of its device block — and takes the new settings; its noise counter goes on."""
    from models.search._common import data_parallel_world, relaxation_option
    relax = relaxation_option(args, status, num_epochs, world=max(_world(), data_parallel_world(args)))
    if relax is None:
        return None
    net = getattr(model, 'fusion_net', None)
    if not hasattr(net, 'set_relaxation'):
        raise ValueError('args.arch_tau / args.arch_tau_min / args.arch_gumbel need a search hypernet '
                         '(model.fusion_net.set_relaxation)')
    kept = net.relaxation
    if kept is None:
        net.set_relaxation(relax)
        return relax
    if kept.gumbel != relax.gumbel:
        model.__dict__.pop('_bmnas_forward_graphs', None)        # (whether noise is drawn is baked into a captured pass)
    settings = relax.state_dict()
    settings['counter'] = kept.counter
    kept.load_state_dict(settings)
    return kept


def _observe(event, **info):
    """tests/test_outer_loop_golden_gpu.py pins the loop against the reference's trainers through this hook
    (run.observer = callable(event, **info)); None in production: no host synchronisation is added."""
    obs = getattr(run, 'observer', None)
    if obs is not None:
        obs(event, **info)


def run(model, architect, criterion, optimizer, scheduler, dataloaders, dataset_sizes, device,
        num_epochs, logger, plotter, args, status, unpack, meter, eval_phases, better, task=None,
        nan_escape=False, init=None):
    """-> dict(best_dev, best_dev_genotype, best_test, best_test_genotype, last_genotype, nan_abort).
    init: what the first epoch's metric is compared with (the reference starts from best_f1 = init_f1 with `>`,
    train_searchable/mmimdb.py:19,162, and from best_acc = 0 with `>=`, ntu.py:18,135); None: always accepted."""
    m_accum = check_accum(args)              # (first: a refused combination moves nothing)
    relax = _set_relaxation(model, args, status, num_epochs)      # (args.arch_tau / arch_tau_min / arch_gumbel; else None)
    cosine = isinstance(scheduler, sc.LRCosineAnnealingScheduler)
    device = _model_device(model, device)
    from bmnas.graph import GraphedTrainStep
    use_graph = GraphedTrainStep.enabled(args)
    w_graph, w_attempts = None, 0
    k_steps = steps_per_replay(args) if use_graph else 1
    wk_graph, wk_attempts = None, 0
    f_graphs = _ForwardGraphs.of(model, criterion, args, logger)
    stats = run.stats = dict(graph_replays=0, eager_steps=0, forward_replays=0, k_step_replays=0)
    if relax is not None:                    # (without the options run.stats has the keys it always had)
        stats['relax_tau'] = relax.tau       # the last temperature set: the schedule's value of the current epoch
    # args.device_stats: the phase statistics in one device accumulator, one launch per batch (bmnas.metrics.PhaseStats);
    # None — the option absent, or a meter that is not the loop's own — and `tally` below is the two statements of always
    from models.search._common import device_stats_option
    dstats = device_stats_option(args, meter)
    if dstats is not None:                   # (without it run.stats has the keys it always had: read them with .get)
        stats.update(stat_launches=0,        # batches tallied by one eager launch behind their replay / eager step
                     stat_in_replay=0,       # ... by the captured forward's own last node: no host call
                     stat_fallbacks=0)       # ... by PhaseStats' torch restatement (tensors the launch does not take)
    # gradient accumulation (args.accum_steps = m > 1): the accumulate=m graph of the full groups and the accumulator of
    # the eager tails; absent or 1 none of this exists and nothing below changes
    wa_graph, wa_attempts, accumulator = None, 0, None
    if m_accum > 1:
        stats['accum_groups'] = 0            # optimizer steps taken over a group of held batches
        stats['accum_replays'] = 0           # ... of which as ONE replay of the accumulate=m graph
    # weight averaging (found-stage runs only; refused in a search): None without the options — and nothing below changes
    from models.search._common import make_averager
    averaged, avg_opts = make_averager(model, args, status)
    run.averaged = averaged          # (like run.stats: the caller's handle on the averaged model of this run)
    ema = averaged if averaged is not None and avg_opts['decay'] is not None else None     # updated after every step
    avg_graphs = _ForwardGraphs.of(averaged.module, criterion, args, logger) if averaged is not None else None
    if averaged is not None:
        stats['averaged_updates'] = 0
        stats['averaged_forwards'] = 0
    # args.swa_update_bn: the averaged module's BatchNorm statistics come from a cumulative pass over the training
    # loader (bmnas.optim.update_bn), taken before the first evaluation after its weights changed
    bn_pass = averaged is not None and avg_opts['update_bn']
    bn_pass_at = 0                   # stats['averaged_updates'] when the last pass ran
    if bn_pass:
        stats['update_bn_passes'] = 0
    # SWA: the phase after which an epoch's snapshot is taken — its last learning one (train and dev both learn here)
    swa_phase = ([ph for ph in eval_phases if ph in ('train', 'dev')] or [None])[-1] if averaged is not None else None
    best = dict(best_dev=None, best_dev_genotype=None, best_dev_epoch=0, best_test=None,
                best_test_genotype=None, best_test_epoch=0, last_genotype=None, nan_abort=False)
    # the unrolled architecture step (architect.unrolled) draws one training batch per dev batch from an iterator of its
    # own over the training loader, restarted when exhausted
    unrolled = status == 'search' and architect is not None and bool(getattr(architect, 'unrolled', False))
    train_iter = None

    def next_train():
        nonlocal train_iter
        for _ in range(2):
            if train_iter is None:
                train_iter = iter(dataloaders['train'])
            try:
                return unpack(next(train_iter), device)
            except StopIteration:
                train_iter = None
                stats['unrolled_train_restarts'] = stats.get('unrolled_train_restarts', 0) + 1
        raise RuntimeError('the training loader yields no batch')

    for epoch in range(num_epochs):
        logger.info('Epoch: {}'.format(epoch))
        logger.info('EXP: {}'.format(args.save))
        if relax is not None:
            stats['relax_tau'] = relax.set_epoch(epoch)      # one device fill, outside any replay (captured steps read it)
        phases = ['train', 'dev'] if status == 'search' else eval_phases
        for phase in phases:
            if phase == 'train':
                if not cosine:
                    scheduler.step()
                if architect is not None:
                    architect.log_learning_rate(logger)
                if relax is not None:
                    logger.info("Architecture Temperature: {}".format(relax.tau))
                model.train()
            elif phase == 'dev':
                if status == 'eval' and not cosine:
                    scheduler.step()
                model.train()                  # the reference keeps BN/dropout in train mode here
            else:
                model.eval()
            learn = phase == 'train' or (phase == 'dev' and status == 'eval')
            # a phase that does not learn evaluates the averaged weights, once there are any (SWA: from its first snapshot)
            use_avg = averaged is not None and not learn and stats['averaged_updates'] > 0
            net, net_graphs = (averaged.module, avg_graphs) if use_avg else (model, f_graphs)
            if use_avg and bn_pass and bn_pass_at != stats['averaged_updates']:
                from bmnas.optim import update_bn
                update_bn(dataloaders['train'], averaged.module, device, unpack=unpack, criterion=criterion)
                bn_pass_at = stats['averaged_updates']
                stats['update_bn_passes'] += 1
            if use_avg:
                averaged.module.eval()
            meter.reset(device)
            loss_sum = torch.zeros((), device=device, dtype=torch.float64)
            if dstats is not None:
                dstats.reset(device)
            seen = 0
            loader = dataloaders[phase]
            split = _world() > 1 and not _is_sharded(loader)
            if _world() > 1 and _is_sharded(loader):
                loader.sampler.set_epoch(epoch)          # a new shuffle per epoch, the same on every rank
            _set_weight(1.0)                             # (a shard weight belongs to ONE scattered batch: none carries over)
            def averaged_step(in_replay=False):
                """The EMA's update after a weight step — unless the replay that took the step held it."""
                if ema is not None:
                    if not in_replay:
                        ema.update_parameters(model)
                    stats['averaged_updates'] += 1

            def one_batch(inputs, labels):
                nonlocal w_graph, w_attempts, loss_sum
                # nothing of the previous batch's autograd graph may stay referenced while a step is
                # being captured (see GraphedTrainStep._live_graph_tensors)
                output = loss = None
                got = None
                if labels.size(0) == 0:
                    # an idle replica of an uneven scatter: no forward, the collectives of the batch only
                    if status == 'search' and phase in ('dev', 'test') and architect is not None:
                        _idle_step(architect.optimizer)
                    if learn:
                        if cosine:
                            scheduler.step()
                            scheduler.update_optimizer(optimizer)
                        _idle_step(optimizer)
                        averaged_step()
                    stats['idle_steps'] = stats.get('idle_steps', 0) + 1
                    return
                if status == 'search' and phase in ('dev', 'test') and architect is not None:
                    # (captured: the metric forward below rides at the end of the architecture step's replay — one
                    # batch copy and one hipGraph launch for both; None: it did not, evaluate it here)
                    if unrolled:
                        # DARTS' unrolled step (train_search.py:151: `architect.step(input, target, input_search,
                        # target_search, ...)`): one training batch beside the dev batch; eager, returns None — the
                        # metric forward below runs through f_graphs
                        x_train, y_train = next_train()
                        got = architect.step(inputs, labels, logger, input_train=x_train, target_train=y_train)
                        stats['unrolled_steps'] = stats.get('unrolled_steps', 0) + 1
                    else:
                        got = architect.step(inputs, labels, logger, metric=not learn and use_graph and f_graphs.on)
                if learn and use_graph:
                    if w_graph is None and w_attempts < 3:
                        w_attempts += 1
                        w_graph = GraphedTrainStep.try_build(model, criterion, optimizer, inputs, labels,
                                                             logger, averaged=ema) or None
                    if w_graph and w_graph.matches(inputs, labels):
                        if cosine:
                            scheduler.step()
                            scheduler.update_optimizer(optimizer)
                        loss, output = w_graph(inputs, labels)
                        averaged_step(in_replay=w_graph.averaged is not None)
                        _tally(dstats, stats, loss_sum, meter, loss, output, labels)
                        stats['graph_replays'] += 1
                        _observe('batch', epoch=epoch, phase=phase, loss=loss, output=output, optimizer=optimizer,
                                 learn=True, how='graph')
                        return
                if not learn:
                    # the metric pass: no gradients, one replay (the step above — architect.step in the dev phase —
                    # has already happened: this forward sees the updated alphas, like the reference's)
                    rode = False
                    if got is None:
                        if dstats is None:
                            got = net_graphs(net, criterion, inputs, labels)
                        else:
                            got = net_graphs(net, criterion, inputs, labels, stats=dstats)
                            rode = net_graphs.tallied
                        if use_avg:
                            stats['averaged_forwards'] += 1
                    else:
                        stats['merged_metric_replays'] = stats.get('merged_metric_replays', 0) + 1
                    if got is not None:
                        loss, output = got
                        _tally(dstats, stats, loss_sum, meter, loss, output, labels, rode)
                        stats['forward_replays'] += 1
                        _observe('batch', epoch=epoch, phase=phase, loss=loss, output=output, optimizer=optimizer,
                                 learn=False, how='graph')
                        return
                stats['eager_steps'] += 1
                optimizer.zero_grad()
                with torch.set_grad_enabled(learn):
                    output = net(inputs)
                    if isinstance(output, tuple):
                        output = output[-1]
                    loss = criterion(output, labels)
                    if learn:
                        if cosine:
                            scheduler.step()
                            scheduler.update_optimizer(optimizer)
                        loss.backward()
                        optimizer.step()
                        averaged_step()
                _tally(dstats, stats, loss_sum, meter, loss, output, labels)
                _observe('batch', epoch=epoch, phase=phase, loss=loss, output=output, optimizer=optimizer,
                         learn=learn, how='eager')

            def k_batches(batches):
                """k resident batches as ONE replay of a k-step graph (each step with the learning rate the scheduler gives
                its batch); anything that does not fit — no capture, another batch shape — runs batch by batch."""
                nonlocal wk_graph, wk_attempts, loss_sum
                x0, y0 = batches[0]
                if wk_graph is None and wk_attempts < 3:
                    wk_attempts += 1
                    wk_graph = GraphedTrainStep.try_build(model, criterion, optimizer, x0, y0, logger, k=k_steps,
                                                          averaged=ema) or None
                if not (wk_graph and all(wk_graph.matches(x_, y_) for x_, y_ in batches)):
                    for x_, y_ in batches:
                        one_batch(x_, y_)
                    return
                lrs = []
                for j, (x_, y_) in enumerate(batches):
                    if cosine:
                        scheduler.step()
                        scheduler.update_optimizer(optimizer)
                    lrs.append(wk_graph.stage(j, x_, y_))
                stats['k_step_replays'] += 1
                for (loss, output), (x_, y_), lr in zip(wk_graph.replay_staged(), batches, lrs):
                    averaged_step(in_replay=wk_graph.averaged is not None)
                    _tally(dstats, stats, loss_sum, meter, loss, output, y_)
                    stats['graph_replays'] += 1
                    # (lr: the rates THIS batch's step was staged with — the optimizer's own have moved on to the last
                    # batch of the group by now)
                    _observe('batch', epoch=epoch, phase=phase, loss=loss, output=output, optimizer=optimizer,
                             learn=True, how='graph', lr=lr)

            def accum_group(batches):
                """Up to m held batches as ONE optimizer step: a full group of one shape is a replay of the accumulate=m
                graph; anything else — the tail of a phase, no capture — is one eager accumulated step, the gradients
                of the micro-batches combined with weights n_i / N by the same bmnas.optim.GradAccumulator."""
                nonlocal wa_graph, wa_attempts, accumulator, loss_sum
                from bmnas.optim import GradAccumulator, accum_weights
                stats['accum_groups'] += 1
                x0, y0 = batches[0]
                flat = all(isinstance(x_, (list, tuple)) for x_, _ in batches)
                one_shape = flat and len(batches) == m_accum and all(
                    y_.shape == y0.shape and len(x_) == len(x0) and all(a.shape == b.shape for a, b in zip(x_, x0))
                    for x_, y_ in batches)
                if use_graph and one_shape:
                    if wa_graph is None and wa_attempts < 3:
                        wa_attempts += 1
                        wa_graph = GraphedTrainStep.try_build(model, criterion, optimizer, x0, y0, logger, averaged=ema,
                                                              accumulate=m_accum) or None
                    if wa_graph and wa_graph.matches_group(batches):
                        for j, (x_, y_) in enumerate(batches):
                            if cosine:
                                scheduler.step()
                                scheduler.update_optimizer(optimizer)
                            wa_graph.stage(j, x_, y_)        # (the step's scalars are fixed with the LAST micro-batch)
                        outs = wa_graph.replay_staged()
                        stats['accum_replays'] += 1
                        averaged_step(in_replay=wa_graph.averaged is not None)
                        for (loss, output), (x_, y_) in zip(outs, batches):
                            _tally(dstats, stats, loss_sum, meter, loss, output, y_)
                            stats['graph_replays'] += 1
                            _observe('batch', epoch=epoch, phase=phase, loss=loss, output=output, optimizer=optimizer,
                                     learn=True, how='graph')
                        return
                if accumulator is None:
                    accumulator = GradAccumulator(optimizer)
                accumulator.reset()
                targets = accumulator.tensors
                ws = accum_weights([y_.size(0) for _, y_ in batches], getattr(criterion, 'reduction', 'mean'))
                for (x_, y_), w_ in zip(batches, ws):
                    stats['eager_steps'] += 1
                    if cosine:
                        scheduler.step()
                        scheduler.update_optimizer(optimizer)
                    output = net(x_)
                    if isinstance(output, tuple):
                        output = output[-1]
                    loss = criterion(output, y_)
                    live = [t for t in targets if t.requires_grad]
                    got_g = iter(torch.autograd.grad(loss, live, allow_unused=True))
                    grads = [next(got_g) if t.requires_grad else None for t in targets]
                    accumulator.add([g if g is None else g.contiguous() for g in grads], w_)
                    _tally(dstats, stats, loss_sum, meter, loss, output, y_)
                    _observe('batch', epoch=epoch, phase=phase, loss=loss, output=output, optimizer=optimizer,
                             learn=True, how='eager')
                    output = loss = grads = got_g = None     # (no autograd graph may outlive the step: a later capture)
                accumulator.combine()
                optimizer.step()
                averaged_step()

            def k_arch_batches(batches):
                """The dev phase of a search: k (architecture step + metric forward) pairs as ONE replay."""
                nonlocal loss_sum
                outs = architect.step_k(batches, logger)
                if outs is None:
                    for x_, y_ in batches:
                        one_batch(x_, y_)
                    return
                stats['k_step_replays'] += 1
                for (loss, output), (x_, y_) in zip(outs, batches):
                    _tally(dstats, stats, loss_sum, meter, loss, output, y_)
                    stats['forward_replays'] += 1
                    stats['merged_metric_replays'] = stats.get('merged_metric_replays', 0) + 1
                    _observe('batch', epoch=epoch, phase=phase, loss=loss, output=output, optimizer=optimizer,
                             learn=False, how='graph')

            # which batches wait for a k-step replay: the weight steps of a learning phase; the (architecture step +
            # metric forward) pairs of a search's dev phase
            arch_phase = (status == 'search' and phase in ('dev', 'test') and architect is not None and not learn
                          and f_graphs.on and hasattr(architect, 'step_k') and not unrolled)
            group = k_batches if learn else (k_arch_batches if arch_phase else None)
            accumulating = learn and m_accum > 1         # (then k_steps == 1 and the world is one process: check_accum)
            hold_n = m_accum if accumulating else k_steps
            held, held_w = [], []                       # batches waiting for their k-step replay (+ their shard weights)

            def flush():
                # (a shard weight belongs to ITS batch: uneven scatters of different global sizes must not share a replay)
                nonlocal held, held_w
                if accumulating:
                    if held:                            # a full group, or the tail of the phase: ONE optimizer step
                        accum_group(held)
                elif len(held) == k_steps and len(set(held_w)) == 1:
                    _set_weight(held_w[0])
                    group(held)
                else:                                   # the ragged tail of a phase: single steps
                    for (x_, y_), w_ in zip(held, held_w):
                        _set_weight(w_)
                        one_batch(x_, y_)
                held, held_w = [], []

            for data in loader:
                inputs, labels = unpack(data, device)
                if split:
                    inputs, labels = _shard_batch(inputs, labels)
                seen += labels.size(0)
                if accumulating or (group is not None and k_steps > 1 and isinstance(inputs, (list, tuple))
                                    and labels.size(0)):
                    held.append((inputs, labels))
                    held_w.append(_weight())
                    if len(held) == hold_n:
                        flush()
                    continue
                w_now = _weight()
                flush()                                 # keep the batch order
                _set_weight(w_now)
                one_batch(inputs, labels)
            flush()
            _set_weight(1.0)
            if averaged is not None and ema is None and phase == swa_phase and epoch >= avg_opts['swa_start']:
                averaged.update_parameters(model)        # the SWA snapshot of this epoch: eager
                stats['averaged_updates'] += 1
            n = dataset_sizes[phase]
            if _world() > 1:
                # what the ranks processed together (a DistributedSampler pads; a split covers every sample)
                n = int(_all_sum(torch.tensor(float(seen), device=device, dtype=torch.float64)))
            if dstats is None:
                epoch_loss = float(_all_sum(loss_sum)) / n
                epoch_metric = meter.compute(n)
            else:                                        # one device-to-host read (summed over the ranks inside)
                epoch_loss = dstats.loss_sum() / n
                epoch_metric = dstats.compute(n)
            logger.info('{} Loss: {:.4f}, {}: {:.4f}'.format(phase, epoch_loss, meter.name, epoch_metric))
            logger.info('Fusion Model Params: {}'.format(fusion_params(model)))
            genotype = model.genotype()
            best['last_genotype'] = genotype
            logger.info(str(genotype))
            _observe('phase', epoch=epoch, phase=phase, loss=epoch_loss, metric=epoch_metric, genotype=genotype)
            if nan_escape and phase == 'train' and epoch_loss != epoch_loss:
                logger.info('Nan loss during training, escaping')
                model.eval()
                best['nan_abort'] = True
                return best
            for which, fname in (('dev', 'best_model.pt'), ('test', 'best_test_model.pt')):
                if phase != which or (which == 'dev' and status != 'search' and eval_phases[-1] != 'dev'):
                    continue
                key = 'best_' + which
                ref = best[key] if best[key] is not None else init
                if ref is None or better(epoch_metric, ref):
                    best[key] = epoch_metric
                    best[key + '_genotype'] = copy.deepcopy(genotype)
                    best[key + '_epoch'] = epoch
                    if _rank() == 0:
                        save(model, os.path.join(args.save, 'best', fname))
                        if averaged is not None and which == 'test':
                            # (torch.optim.swa_utils.AveragedModel's keys: `module.*` and `n_averaged`)
                            save(averaged, os.path.join(args.save, 'best', 'best_test_averaged.pt'))
                        save_pickle(best[key + '_genotype'],
                                    os.path.join(args.save, 'best', fname.replace('model.pt', 'genotype.pkl')))
        plotter.plot(best['last_genotype'], os.path.join(args.save, 'architectures', 'epoch_{}'.format(epoch)),
                     task=task)
        logger.info('Current best dev {}: {}, at training epoch: {}'.format(meter.name, best['best_dev'],
                                                                          best['best_dev_epoch']))
        logger.info('Current best test {}: {}, at training epoch: {}'.format(meter.name, best['best_test'],
                                                                           best['best_test_epoch']))
    return best


@torch.no_grad()
def evaluate(model, criterion, loader, n, device, logger, args, unpack, meter, phase='test'):
    model.eval()
    logger.info('EXP: {}'.format(args.save))
    device = _model_device(model, device)
    meter.reset(device)
    loss_sum = torch.zeros((), device=device, dtype=torch.float64)
    from models.search._common import device_stats_option
    dstats = device_stats_option(args, meter)            # (as in run: None without args.device_stats)
    counters = evaluate.stats = dict(stat_launches=0, stat_in_replay=0, stat_fallbacks=0)
    if dstats is not None:
        dstats.reset(device)
    split = _world() > 1 and not _is_sharded(loader)
    seen = 0
    f_graphs = _ForwardGraphs.of(model, criterion, args, logger)
    for data in loader:
        inputs, labels = unpack(data, device)
        if split:
            inputs, labels = _shard_batch(inputs, labels)
        seen += labels.size(0)
        if dstats is None:
            got = f_graphs(model, criterion, inputs, labels)
        else:
            got = f_graphs(model, criterion, inputs, labels, stats=dstats)
        if got is not None:
            loss, output = got
        else:
            output = model(inputs)
            if isinstance(output, tuple):
                output = output[-1]
            loss = criterion(output, labels)
        _tally(dstats, counters, loss_sum, meter, loss, output, labels, got is not None and f_graphs.tallied)
    evaluate.forward_replays = f_graphs.replays
    if _world() > 1:
        n = int(_all_sum(torch.tensor(float(seen), device=device, dtype=torch.float64)))
    if dstats is None:
        epoch_loss = float(_all_sum(loss_sum)) / n
        metric = meter.compute(n)
    else:
        epoch_loss = dstats.loss_sum() / n
        metric = dstats.compute(n)
    logger.info('{} Loss: {:.4f}, {}: {:.4f}'.format(phase, epoch_loss, meter.name, metric))
    logger.info('Fusion Model Params: {}'.format(fusion_params(model)))
    return metric
