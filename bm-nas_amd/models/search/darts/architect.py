"""The architecture step: first-order (reference models/search/darts/architect.py:9-29) and, with `args.unrolled`,
DARTS' unrolled second-order step — what the reference's callers still ask for (`architect.step(..., unrolled=
args.unrolled)`, models/search/darts/train_search.py:151) and its Architect no longer holds."""
import torch


class Architect(object):
    def __init__(self, model, args, criterion, optimizer, network_optimizer=None):
        self.network_weight_decay = args.weight_decay
        self.criterion = criterion
        self.model = model
        self.optimizer = optimizer
        # args.unrolled (DARTS' --unrolled): the second-order step of `_step_unrolled`; args.unrolled_r: the r of its
        # finite difference (R = r / ||v||, DARTS' 1e-2).  Off: nothing below differs and network_optimizer is not touched.
        self.unrolled = bool(getattr(args, 'unrolled', False))
        self.unrolled_r = getattr(args, 'unrolled_r', 1e-2)
        self.network_optimizer = network_optimizer
        self._unrolled = None                # bmnas.optim.UnrolledStep, built by the first unrolled step
        self.unrolled_steps = 0
        # forward + criterion + backward + Adam(alpha) as one hipGraph replay (GraphedTrainStep.enabled)
        from bmnas.graph import GraphedTrainStep
        self.use_graph = GraphedTrainStep.enabled(args)
        self._graph = None
        self._attempts = 0
        self.graph_replays = 0
        self._with_metric = False

    def log_learning_rate(self, logger):
        for group in self.optimizer.param_groups:
            logger.info("Architecture Learning Rate: {}".format(group['lr']))
            break

    def step(self, input_valid, target_valid, logger, metric=False, input_train=None, target_train=None):
        """metric=True (the trainer loop's dev phase): the caller will evaluate `criterion(model(input_valid),
        target_valid)` without gradients right after this step (train_searchable/mmimdb.py:66-84) — a captured step
        then carries that forward at its end and this returns (loss, output) of it; None: evaluate it yourself.
        input_train / target_train: a batch of the training split, needed (and read) by the unrolled step only, which
        runs eagerly and returns None."""
        if self.unrolled:
            return self._step_unrolled(input_valid, target_valid, input_train, target_train)
        if self.use_graph:
            if self._graph is None and self._attempts < 3:
                from bmnas.graph import GraphedTrainStep
                self._attempts += 1
                self._with_metric = bool(metric)
                g = False
                if metric:
                    g = GraphedTrainStep.try_build(self.model, self.criterion, self.optimizer, input_valid,
                                                   target_valid, logger, metric_forward=True)
                    self._with_metric = bool(g)
                if not g:
                    g = GraphedTrainStep.try_build(self.model, self.criterion, self.optimizer, input_valid,
                                                   target_valid, logger)
                self._graph = g or None
            if self._graph and self._graph.matches(input_valid, target_valid):
                out = self._graph(input_valid, target_valid)
                self.graph_replays += 1
                if self._with_metric:
                    # (the replay ran the metric forward whether or not this caller wants it: BatchNorm statistics and
                    # the dropout stream advanced as they do when the caller runs it, which it then must not do again)
                    return out[2], out[3]
                return None
        self.optimizer.zero_grad()
        self._backward_step(input_valid, target_valid)
        self.optimizer.step()
        return None

    def step_k(self, batches, logger):
        """k architecture steps, each followed by its metric forward (`step(..., metric=True)` k times), as ONE hipGraph
        replay over k resident batches — the dev phase of a search with the trainer's `steps_per_replay` = k.
        -> [(loss, output)] of the k metric forwards, or None: the caller takes the batches one by one."""
        if not self.use_graph:
            return None
        k = len(batches)
        from bmnas.graph import GraphedTrainStep
        gk = getattr(self, '_graph_k', None)
        if gk is None and getattr(self, '_attempts_k', 0) < 3:
            self._attempts_k = getattr(self, '_attempts_k', 0) + 1
            gk = self._graph_k = GraphedTrainStep.try_build(self.model, self.criterion, self.optimizer, batches[0][0],
                                                            batches[0][1], logger, metric_forward=True, k=k) or None
        if not gk or gk.k != k or not all(gk.matches(x, y) for x, y in batches):
            return None
        for j, (x, y) in enumerate(batches):
            gk.stage(j, x, y)
        self.graph_replays += k
        return [(o[2], o[3]) for o in gk.replay_staged()]

    def _backward_step(self, input_valid, target_valid):
        loss = self.criterion(self.model(input_valid), target_valid)
        loss.backward()

    def _loss(self, inputs, targets):
        out = self.model(inputs)
        if isinstance(out, tuple):
            out = out[-1]
        return self.criterion(out, targets)

    def _arch_grads(self, arch, inputs, targets):
        from bmnas import cell as K
        loss = self._loss(inputs, targets)
        with K.arch_grads_only(True):
            return torch.autograd.grad(loss, arch, allow_unused=True)

    def _step_unrolled(self, input_valid, target_valid, input_train, target_train):
        """DARTS' unrolled architecture step (Liu et al. 2019, eq. 7-8), eagerly, with the weight-side arithmetic on the
        kernels of bmnas.optim.UnrolledStep:
          1. g = grad_w L_train(w, alpha);  w' = w - eta (moment + g + wd w), w kept in a backup      (virtual_step)
          2. (dalpha, v) = grad_(alpha, w') L_val(w', alpha)
          3. w+ = w + R v, R = r / ||v||:  g+ = grad_alpha L_train(w+, alpha)                          (perturb)
          4. w- = w - R v:                 g- = grad_alpha L_train(w-, alpha)                          (perturb)
          5. w back from the backup                                                                   (restore)
          6. alpha.grad = dalpha - eta (g+ - g-) / (2 R);  optimizer.step()                           (combine)
        No `.grad` of a weight is written and the weight optimizer's state is only read.  The + and - passes see the
        same dropout masks (the counter-based offset of bmnas.cell.DROP and torch's CUDA generator are put back before
        the - pass; both advance normally afterwards): the difference quotient would otherwise measure mask noise
        amplified by 1 / (2 R).  All four passes run on the live model in its current mode, so BatchNorm running
        statistics and num_batches_tracked advance FOUR times per architecture step (DARTS: three times on the live
        model and once on its copy).  Data-parallel runs are refused: the step would need four reductions."""
        import torch.distributed as tdist
        from bmnas import cell as K, dist as bdist, lib
        from bmnas.optim import UnrolledStep
        if input_train is None or target_train is None:
            raise lib.BmnasError('Architect.step: the unrolled step needs a training batch (input_train, target_train)')
        if self.network_optimizer is None:
            raise lib.BmnasError('Architect: the unrolled step needs the network optimizer '
                                 '(Architect(..., network_optimizer=...))')
        world = max(bdist.env_world(), tdist.get_world_size() if tdist.is_available() and tdist.is_initialized() else 1)
        if world > 1:
            raise lib.BmnasError(f'Architect: the unrolled step is single-process (world size {world}: it would need four '
                                 'gradient reductions per step)')
        if self._unrolled is None:
            self._unrolled = UnrolledStep(self.network_optimizer, self.model.arch_parameters(), r=self.unrolled_r)
        us = self._unrolled
        us.eta()                                     # groups with different learning rates: refused before anything moves
        weights, arch = us.weights, us.arch
        loss = self._loss(input_train, target_train)
        with K.weight_grads_only(True):
            g = torch.autograd.grad(loss, weights, allow_unused=True)
        us.virtual_step(g)
        del g, loss
        try:
            loss = self._loss(input_valid, target_valid)
            both = torch.autograd.grad(loss, arch + weights, allow_unused=True)
            del loss
            dalpha, v = both[:len(arch)], both[len(arch):]
            us.perturb(v, +1)
            dev = arch[0].device
            drop_offset, rng = K.DROP.offset, torch.cuda.get_rng_state(dev)
            gp = self._arch_grads(arch, input_train, target_train)
            us.perturb(v, -1)
            K.DROP.offset = drop_offset
            torch.cuda.set_rng_state(rng, dev)
            gn = self._arch_grads(arch, input_train, target_train)
        finally:
            us.restore()
        dalpha = us.combine(dalpha, gp, gn)
        for a, d in zip(arch, dalpha):
            a.grad = d
        self.optimizer.step()
        self.unrolled_steps += 1
        return None
