"""Meta-training outer loop on the engine: one process per GPU, tasks sharded over ranks,
ONE all-reduce (RCCL over xGMI) of the flat meta-gradient per meta-iteration, then every
rank applies the identical fused RAdam step -- no parameter broadcast needed.

Replaces the reference's worker/main split:
  * task loop          `src/util/meta_run.py:109-238`  (K inner steps, meta frame,
                       `bptt_loss.backward()`, NaN guard `:209-211,226`)
  * gradient hand-off  `meta_run.py:237-238` (unsynchronised `+=` into shared CPU tensors)
                       -> deterministic device all-reduce
  * outer step         `src/train_meta.py:361-373` (average by meta_batch_size, optional
                       clip, RAdam with per-tensor groups `:110-127`, `clamp_init_lr`)
The flat state vector is [log_init_lr_* | model_init_*] in `MetaOptimizer.named_parameters()`
order (`meta_optim.py:65-66,78`), the reference's OIHW layout.  With a frozen encoder (the engine's
`train_from`, `train_encoder=False`) it holds the trainable tensors only -- the suffix of each part of the
engine's layout -- and so do the gradient, the all-reduce and the RAdam moments; the frozen init stays the
parent's weights.
"""
import math
import os

import torch

from .topology import neuron_lr_shape, trainable

# engines in flight on one GPU -> workgroups each plans its launches for (0 = the whole chip); measured on MI355X,
# 480x854 batch-1 tasks (profiles/r02_meta_wg_budget.txt); EOSVOS_META_WG_BUDGET overrides
CONCURRENT_WG_BUDGET = {1: 0, 2: 256, 3: 256, 4: 256}


class _on_stream:
    """Calls of an engine run under the torch stream it is bound to (a no-op for CPU stand-ins)."""

    def __init__(self, engine):
        self.ctx = torch.cuda.stream(engine.stream) if getattr(engine, 'stream', None) is not None else None

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


class MetaTrainer:
    def __init__(self, engine, dist=None, meta_batch_size=4, model_init_lr=1e-5, log_init_lr_lr=1e-5,
                 model_init_weight_decay=1e-3, grad_clip=None, max_lr=None, lr_hierarchy_level='NEURON',
                 use_log_init_lr=False, loss_func='cross_entropy', learn_model_init=True, freeze_encoder=False,
                 extra_engines=(), comm=None):
        """`extra_engines`: more engines on the SAME GPU (each built on its own torch stream): the tasks of one
        meta-iteration are then dealt over all of them and run concurrently -- a batch-1 task leaves CUs idle in its
        tails and small grids that a second and third task fill (measured: 3 engines 1.17x the task rate of 1)."""
        self.eng = engine
        self.engines = [engine] + list(extra_engines)
        # `comm`: an `engine.RcclComm` -- the exchange then goes through the library's own `eosvos_allreduce_sum` (a host
        # without torch.distributed); default: `dist.all_reduce` (backend nccl = RCCL)
        self.comm = comm
        # engines that share the GPU plan each launch for part of the chip (`eosvos_set_wg_budget`): less K splitting,
        # fewer parked partial tiles; the other tasks' launches fill the remaining CUs
        self.wg_budget = int(os.environ.get('EOSVOS_META_WG_BUDGET', CONCURRENT_WG_BUDGET.get(min(len(self.engines), 4), 0)))
        self._apply_wg_budget()
        self.level, self.use_log = lr_hierarchy_level, bool(use_log_init_lr)
        self.n_lr_full = engine.lr_store_count(lr_hierarchy_level)   # NotImplementedError for unknown levels
        # frozen encoder: the learned tensors are tr[nf:] (topology.frozen_tensors); nf = 0 without one
        self.train_from = int(getattr(engine, 'train_from', 0))
        tr_all = trainable(engine.encoder)
        nf = self.train_from
        self._tr = tr_all[nf:]
        self.n_param = sum(math.prod(s) for _, s in self._tr) if nf else engine.n_param
        self._frozen_init = None
        for e in self.engines[1:]:                 # the extra engines of a frozen-encoder model end their backward where it does
            if int(getattr(e, 'train_from', 0)) != self.train_from:
                e.set_trainable_from(self.train_from)
        if lr_hierarchy_level == 'NEURON':
            self.n_lr = sum(math.prod(neuron_lr_shape(s)) for _, s in self._tr)
        elif lr_hierarchy_level == 'TENSOR':
            self.n_lr = len(self._tr)
        elif lr_hierarchy_level == 'PARAM':
            self.n_lr = self.n_param
        if not nf or lr_hierarchy_level == 'SINGLE':
            self.n_lr = self.n_lr_full
        engine.set_loss(loss_func)
        self.loss_func = loss_func
        self.dist = dist
        self.meta_batch_size = meta_batch_size
        self.model_init_lr, self.log_init_lr_lr = model_init_lr, log_init_lr_lr
        self.wd, self.grad_clip, self.max_lr = model_init_weight_decay, grad_clip, max_lr
        # `learn_model_init: False`: model_init_* are no Parameters (meta_optim.py:76-78) -- no meta-gradient, no RAdam
        # step, not in the state dict.  `freeze_encoder` (train_meta.py:120-121): lr = 0 for every learned tensor whose
        # name contains 'backbone' (log_init_lr_backbone-* and model_init_backbone-*).
        self.learn_model_init, self.freeze_encoder = bool(learn_model_init), bool(freeze_encoder)
        tr = self._tr
        nb = sum(1 for n_, _ in tr if n_.startswith('backbone'))
        assert all(n_.startswith('backbone') for n_, _ in tr[:nb])      # the backbone tensors come first
        self._backbone_param = sum(math.prod(s) for _, s in tr[:nb])
        if lr_hierarchy_level == 'NEURON':
            self._backbone_lr = sum(math.prod(neuron_lr_shape(s)) for _, s in tr[:nb])
        elif lr_hierarchy_level == 'PARAM':
            self._backbone_lr = self._backbone_param
        else:
            self._backbone_lr = 0            # one `log_init_lr` Parameter: its name has no 'backbone'
        n = self.n_lr + self.n_param
        dev = engine.device
        self.state = torch.zeros(n, device=dev)
        self.grad = torch.zeros(n, device=dev)
        self.task_grad = torch.zeros(self.n_lr_full + engine.n_param, device=dev)    # engine layout (eosvos_meta_grad)
        self.exp_avg = torch.zeros(n, device=dev)
        self.exp_avg_sq = torch.zeros(n, device=dev)
        self.step = 0
        self.skipped_tasks = 0
        # One launch for the whole outer step (`eosvos_outer_step`) where the engine offers it: NEURON level, and the state
        # vector holding the init part (learn_model_init) or only the lr state.  The extra engines then READ the first
        # engine's learned init / lr (`eosvos_alias_state`): nothing is uploaded per engine after a step.
        # EOSVOS_NO_FUSED_OUTER=1: the separate RAdam / clamp / zero / upload calls (A/B, and what the CPU stand-in runs).
        # (not with a frozen encoder: the fused step keeps the engine's full layout, the subset goes through eosvos_radam_step)
        self.fused_outer = (hasattr(engine, 'outer_step') and lr_hierarchy_level == 'NEURON' and not self.train_from and
                            os.environ.get('EOSVOS_NO_FUSED_OUTER', '0') != '1')
        if self.fused_outer:
            for e in self.engines[1:]:
                e.alias_state(engine)

    # ---- state ------------------------------------------------------------------------
    def load_state(self, model_state, lrs):
        """model_state: reference-style model state dict; lrs: the learned lr state in the reference's
        layout for the hierarchy level (list of per-tensor tensors for NEURON / PARAM, one (G,1) / (1,1)
        tensor for TENSOR / SINGLE; log values with `use_log_init_lr`)."""
        names = [n for n, _ in self._tr]
        dev = self.eng.device
        lrs = list(lrs) if isinstance(lrs, (list, tuple)) else [lrs]
        self.state[:self.n_lr] = torch.cat([l.reshape(-1).float() for l in lrs]).to(dev)
        self.state[self.n_lr:] = torch.cat([model_state[n].reshape(-1).float() for n in names]).to(dev)
        frozen = trainable(self.eng.encoder)[:self.train_from]
        self._frozen_init = (torch.cat([model_state[n].reshape(-1).float() for n, _ in frozen]).to(dev) if frozen else None)
        self._model_state = model_state          # (frozen norm statistics + the init of engines built later for other frame sizes)
        self._drop_pool()
        for e in self.engines:
            with _on_stream(e):
                e.set_loss(self.loss_func)
                e.load_model_state(model_state)
                e.set_lr_state(self.level, self.use_log, self._engine_lr())
        self._mode_check_pending = True      # the first meta-iteration decides the matrix mode for every rank's engines together

    def state_dict(self):
        """`meta_optim_state_dict` of the reference checkpoints (train_meta.py:277-286)."""
        out, off = {}, 0
        tr = self._tr
        if self.level in ('SINGLE', 'TENSOR'):              # one `log_init_lr` Parameter, meta_optim.py:27-42
            out['log_init_lr'] = self.state[:self.n_lr].view(self.n_lr, 1)
            off = self.n_lr
        else:
            for n, shape in tr:
                s = tuple(shape) if self.level == 'PARAM' else neuron_lr_shape(shape)
                k = math.prod(s)
                out['log_init_lr_' + n.replace('.', '-')] = self.state[off:off + k].view(s)
                off += k
        if not self.learn_model_init:
            return out
        for n, shape in tr:
            k = math.prod(shape)
            out['model_init_' + n.replace('.', '-')] = self.state[off:off + k].view(shape)
            off += k
        return out

    # ---- engines for other frame sizes --------------------------------------------------------------
    # The reference feeds every video at its native size (no resize in its data layer): DAVIS 480p sequences are 854 or 910 wide,
    # YouTube-VOS is mostly 1280 x 720 -- the tasks of one meta-batch differ in size.  An engine is built for one size, so the
    # trainer keeps a small pool of engine sets keyed by (H, W); they READ the first engine's learned state (`eosvos_alias_state`)
    # or are uploaded with it after every outer step, carry the same frozen norm statistics, loss, budget and matrix mode.
    MAX_POOLED_SIZES = int(os.environ.get('EOSVOS_META_ENGINE_SIZES', '6'))

    def _all_engines(self):
        return self.engines + [e for es in getattr(self, '_pool', {}).values() for e in es]

    def _drop_pool(self):
        for es in getattr(self, '_pool', {}).values():
            for e in es:
                e.close()
        self._pool, self._pool_use = {}, []

    def _new_engine(self, height, width):
        eng = self.eng
        on_gpu = getattr(eng, 'stream', None) is not None
        kw = dict(norm=getattr(eng, 'norm', 'bn'))
        if on_gpu:
            with torch.cuda.stream(torch.cuda.Stream(eng.device)):
                e = type(eng)(eng.encoder, height, width, eng.max_batch, str(eng.device), side_stream=False, **kw)
        else:
            e = type(eng)(eng.encoder, height, width, eng.max_batch, **kw)
        with _on_stream(e):
            if on_gpu:
                e.stream.wait_stream(eng.stream)
            e.set_loss(self.loss_func)
            if self.train_from:
                e.set_trainable_from(self.train_from)
            e.load_model_state(self._model_state)
            e.set_lr_state(self.level, self.use_log, self._engine_lr())
            if self.fused_outer:
                e.alias_state(eng)
            elif getattr(e, 'verify_matrix_mode', None) is not None:
                e.set_init(self._engine_init(), verify=False)
            else:
                e.set_init(self._engine_init())
            if getattr(e, 'verify_matrix_mode', None) is not None:      # one matrix mode per trainer (the first engine's verdict)
                e.set_engine_matrix_mode(getattr(eng, '_own_mode', None))
                e._verify_pending = e._step_check_pending = False
            if hasattr(e, 'set_wg_budget'):
                e.set_wg_budget(self.wg_budget)
        return e

    def _engines_for(self, height, width, want):
        """Up to `want` engines for frames of this size (the trainer's own for its primary size)."""
        if (height, width) == (self.eng.height, self.eng.width):
            return self.engines
        if not hasattr(self, '_pool'):
            self._pool, self._pool_use = {}, []
        key = (height, width)
        es = self._pool.setdefault(key, [])
        if key in self._pool_use:
            self._pool_use.remove(key)
        self._pool_use.append(key)
        while len(self._pool_use) > self.MAX_POOLED_SIZES:              # least recently used size goes
            for e in self._pool.pop(self._pool_use.pop(0)):
                e.close()
        while len(es) < max(1, min(want, len(self.engines))):
            try:
                es.append(self._new_engine(height, width))
            except Exception:
                # out of device memory with engine sets of other frame sizes pooled: release those and try once more
                others = [k for k in self._pool if k != key]
                if not others:
                    raise
                for k in others:
                    for e in self._pool.pop(k):
                        e.close()
                    if k in self._pool_use:
                        self._pool_use.remove(k)
                es.append(self._new_engine(height, width))
        return es

    def _push_state(self):
        for k, e in enumerate(self._all_engines()):
            with _on_stream(e):
                if k and getattr(e, 'stream', None) is not None:
                    e.stream.wait_stream(self.eng.stream)       # the outer step wrote the state on the first engine's stream
                e.set_lr_state(self.level, self.use_log, self._engine_lr())
                if getattr(e, 'verify_matrix_mode', None) is not None:
                    e.set_init(self._engine_init(), verify=False)      # one outer step away from a state the guard has seen
                else:
                    e.set_init(self._engine_init())

    def _engine_lr(self):
        """The lr state in the engine's layout (frozen encoder: the learned lrs are its suffix; the frozen rows are inert)."""
        lr = self.state[:self.n_lr]
        if self.n_lr == self.n_lr_full:
            return lr
        return torch.cat([torch.zeros(self.n_lr_full - self.n_lr, device=lr.device), lr])

    def _engine_init(self):
        """The init in the engine's layout: the parent's frozen weights, then the learned ones."""
        init = self.state[self.n_lr:]
        return init if self._frozen_init is None else torch.cat([self._frozen_init, init])

    def _add_task(self, tg):
        """self.grad += the learned part of a task gradient in the engine's layout."""
        if not self.train_from:
            self.grad.add_(tg)
            return
        nl, nlf = self.n_lr, self.n_lr_full
        self.grad[:nl].add_(tg[nlf - nl:nlf])
        self.grad[nl:].add_(tg[tg.numel() - self.n_param:])

    # ---- one task ---------------------------------------------------------------------
    def run_task(self, x_train, y_train, x_meta, y_meta, inner_steps=5, bptt_epochs=None, multi_step_bptt_loss=None, eng=None):
        """Returns the (last) meta loss.  Adds the task's meta-gradient into self.grad unless a meta loss is NaN
        (meta_run.py:209-211,226: skipped tasks contribute zeros but the average still divides by
        meta_batch_size).  `bptt_epochs` < inner_steps = truncated BPTT (`:187-221`): every bptt_epochs steps the
        meta frame is back-propagated and `meta_optim.reset(keep_state=True)` detaches the parameters AND the
        state lr (`meta_optim.py:145-151`), so only the first segment leaves gradients on the learned init / lr;
        the later segments are still run (inner steps, meta loss, NaN check) but need no backward here.
        `multi_step_bptt_loss` = per-step weights of the meta loss (`:154-177`)."""
        eng = eng or self.eng
        if multi_step_bptt_loss:
            assert inner_steps == len(multi_step_bptt_loss)             # meta_run.py:156
        bptt = bptt_epochs or inner_steps
        eng.meta_task_begin()
        self.task_grad.zero_()
        first_segment, meta_loss = True, float('nan')

        def meta_frame(weight, boundary):
            if first_segment:
                return eng.meta_grad(x_meta, y_meta, self.task_grad, weight=weight, init_grad=self.learn_model_init,
                                     new_segment=boundary)
            eng.forward(x_meta, want_logits=False)                     # detached segment: loss value only
            return float(eng.loss(self.loss_func, y_meta))

        if inner_steps == 0:                                           # meta frame at the learned init only
            meta_loss = meta_frame(1.0, True)
        for epoch in range(1, inner_steps + 1):
            eng.finetune_step(x_train, y_train, accumulate=first_segment, sync_loss=False)
            boundary = epoch % bptt == 0 or epoch == inner_steps
            evaluated = bool(multi_step_bptt_loss) or boundary
            if multi_step_bptt_loss:
                meta_loss = meta_frame(multi_step_bptt_loss[epoch - 1], boundary)
            elif boundary:
                meta_loss = meta_frame(1.0, True)
            if evaluated and math.isnan(meta_loss):
                break
            if boundary:
                first_segment = False
        if math.isnan(meta_loss):
            self.skipped_tasks += 1
        else:
            self._add_task(self.task_grad)
        return meta_loss

    # ---- one meta-iteration --------------------------------------------------------------
    def _apply_wg_budget(self):
        """(Re)apply the budget: the first engine is the model's and an evaluation in between may have changed it.
        Engines that run side by side also give up their side stream (one queue each: `eosvos_set_side_stream`)."""
        for e in self._all_engines():
            if hasattr(e, 'set_wg_budget'):
                e.set_wg_budget(self.wg_budget)
            if len(self.engines) > 1 and hasattr(e, 'set_side_stream') and os.environ.get('EOSVOS_INFLIGHT_SIDE_STREAM', '0') != '1':
                e.set_side_stream(False)

    def run_tasks_concurrent(self, tasks, inner_steps, engines=None):
        """The default schedule (one meta frame after `inner_steps` steps) for several tasks at once, task i on engine
        i % n: every call is enqueued without waiting, one synchronisation at the end.  NaN tasks are skipped as in
        run_task.  Returns the meta losses."""
        engines = engines or self.engines
        n = len(engines)
        self._apply_wg_budget()
        if len(getattr(self, '_task_grads', [])) < n:
            self._task_grads = [torch.zeros_like(self.task_grad) for _ in range(n)]
        losses = []
        for base in range(0, len(tasks), n):
            group = tasks[base:base + n]
            out = []
            for e, tg, _ in zip(engines, self._task_grads, group):
                with _on_stream(e):
                    if getattr(e, 'stream', None) is not None:
                        e.stream.wait_stream(self.eng.stream)
                    e.meta_task_begin()
                    tg.zero_()
            for _ in range(inner_steps):
                for e, (xt, yt, _, _) in zip(engines, group):
                    with _on_stream(e):
                        e.finetune_step(xt, yt, accumulate=True, sync_loss=False)
            for e, tg, (_, _, xm, ym) in zip(engines, self._task_grads, group):
                with _on_stream(e):
                    out.append(e.meta_grad(xm, ym, tg, init_grad=self.learn_model_init, new_segment=True, sync=False))
            for e, tg, l in zip(engines, self._task_grads, out):
                e.synchronize()
                l = float(l)
                if math.isnan(l):
                    self.skipped_tasks += 1
                else:
                    self._add_task(tg)
                losses.append(l)
        return losses

    def _collective_mode_check(self, local_tasks):
        """The f16x3 range guard (`Engine.verify_matrix_mode`: forward pass AND one fine-tune step of the loaded state in f16x3
        against the exact-split mode) for a trainer: run once, on the first engine with this rank's first task, at the first
        meta-iteration after `load_state`; the verdict is all-reduced (MAX) so that EVERY engine of EVERY rank ends in the same
        mode -- ranks in different modes would average gradients of slightly different functions.  Every rank takes part in
        the collective whether it has a task or not (all ranks call `meta_iteration` equally often)."""
        self._mode_check_pending = False
        real = [e for e in self._all_engines() if getattr(e, 'verify_matrix_mode', None) is not None]
        flag, checked = 0, False
        # an engine of this rank that already left f16x3 (an earlier lazy guard, or the caller) IS a fall-back: the other ranks
        # must follow it, or the ranks would average gradients of two slightly different functions
        from .engine import get_matrix_mode as _process_mode
        if _process_mode() == 'f16x3' and any(e.matrix_mode != 'f16x3' for e in real):
            flag = 1
        if real and local_tasks and getattr(real[0], '_verify_pending', False):
            from .engine import _guard_enabled
            if _guard_enabled() and real[0].matrix_mode == 'f16x3':
                xt, yt = local_tasks[0][0], local_tasks[0][1]
                ve = self._engines_for(int(xt.shape[-2]), int(xt.shape[-1]), 1)[0]      # (an engine of the first task's frame size)
                if ve is not self.eng and getattr(ve, 'stream', None) is not None:
                    ve.stream.wait_stream(self.eng.stream)
                with _on_stream(ve):
                    flag = max(flag, int(ve.verify_matrix_mode(xt, yt) != 'f16x3'))
                    if ve is not self.eng:
                        ve.synchronize()
                checked = True
                real = [e for e in self._all_engines() if getattr(e, 'verify_matrix_mode', None) is not None]
        if self.comm is not None:
            t = torch.tensor([float(flag)], device=self.state.device)
            es = getattr(self.eng, 'stream', None)
            cur = torch.cuda.current_stream(self.state.device) if self.state.is_cuda else None
            if es is not None and cur is not None and es != cur:
                es.wait_stream(cur)             # t was written on the current stream
            with _on_stream(self.eng):
                self.eng.allreduce_sum(t, self.comm)
                self.eng.synchronize()
            flag = int(float(t.item()) > 0.0)
        elif self.dist is not None and self.dist.is_initialized():
            t = torch.tensor([flag], device=self.state.device, dtype=torch.int32)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            flag = int(t.item())
        collective = self.comm is not None or (self.dist is not None and self.dist.is_initialized())
        for e in real:
            if flag and e.matrix_mode == 'f16x3':
                e.set_engine_matrix_mode('bf16x6')
            # the verdict is final for every rank that took part in the collective -- also for one that had no task to check
            # with (it adopts what the ranks with tasks found; a lazy check of its own later could leave it alone in bf16x6).
            # Without a collective a task-less trainer keeps its engines' lazy check.
            if checked or flag or collective:
                e._verify_pending = e._step_check_pending = False
        return flag

    def meta_iteration(self, local_tasks, inner_steps=5, bptt_epochs=None, multi_step_bptt_loss=None):
        """local_tasks: this rank's share of the meta-batch: [(x_train, y_train, x_meta, y_meta)]."""
        if getattr(self, '_mode_check_pending', False):
            self._collective_mode_check(local_tasks)
        default_schedule = not multi_step_bptt_loss and (bptt_epochs or inner_steps) == inner_steps and inner_steps > 0
        for t in local_tasks:
            if t[0].shape[0] > self.eng.max_batch or t[2].shape[0] > self.eng.max_batch:
                raise ValueError(f'task batch {t[0].shape[0]} / {t[2].shape[0]} exceeds the engines\' max_batch {self.eng.max_batch}')
        prof = getattr(self, 'profile', None)       # bench.py: {'tasks_ms', 'allreduce_ms', 'outer_step_ms'} summed over calls
        tick = self._tick if prof is not None else (lambda: 0.0)
        t0 = tick()
        self._apply_wg_budget()                     # an evaluation in between may have changed the first engine's budget
        # runs of consecutive tasks with one frame size (the usual case: all of them), each on the engines of that size; the tasks'
        # gradients enter self.grad in task order either way
        losses, i = [], 0
        while i < len(local_tasks):
            hw = tuple(local_tasks[i][0].shape[-2:])
            j = i
            while j < len(local_tasks) and tuple(local_tasks[j][0].shape[-2:]) == hw:
                j += 1
            run = local_tasks[i:j]
            engines = self._engines_for(hw[0], hw[1], len(run))
            # every run is ordered after the one before it (they share self.grad / the task-gradient buffers) and after the
            # caller's stream: the current stream waited for the previous run's engines below, this run's engines -- the first
            # engine included, whose stream need not be the current one -- wait for the current stream
            if self.state.is_cuda:
                cur = torch.cuda.current_stream(self.state.device)
                for e in engines:
                    es = getattr(e, 'stream', None)
                    if es is not None and es != cur:
                        es.wait_stream(cur)
            if len(engines) > 1 and len(run) > 1 and default_schedule:
                losses += self.run_tasks_concurrent(run, inner_steps, engines)
                if self.state.is_cuda:          # (run_tasks_concurrent ends with every engine synchronised; the wait records the order)
                    for e in engines:
                        if getattr(e, 'stream', None) is not None:
                            torch.cuda.current_stream(self.state.device).wait_stream(e.stream)
            else:
                e0 = engines[0]
                if e0 is not self.eng and getattr(e0, 'stream', None) is not None:
                    e0.stream.wait_stream(self.eng.stream)                  # the learned state was written on the first engine's stream
                with _on_stream(e0):
                    losses += [self.run_task(*t, inner_steps=inner_steps, bptt_epochs=bptt_epochs,
                                             multi_step_bptt_loss=multi_step_bptt_loss, eng=e0) for t in run]
                if self.state.is_cuda and getattr(e0, 'stream', None) is not None:
                    torch.cuda.current_stream(self.state.device).wait_stream(e0.stream)
            i = j
        t1 = tick()
        if self.comm is not None:
            # the library's own collective, on the first engine's stream (ordered after the tasks: the streams were joined above)
            es = getattr(self.eng, 'stream', None)
            cur = torch.cuda.current_stream(self.state.device) if self.state.is_cuda else None
            if es is not None and cur is not None and es != cur:
                es.wait_stream(cur)
            with _on_stream(self.eng):
                self.eng.allreduce_sum(self.grad, self.comm)
        elif self.dist is not None and self.dist.is_initialized():
            # sum over ranks, one 161 MB message (also with ONE rank: the collective, its device binding and its stream
            # ordering are then the code that runs on a node -- tests/test_gpu_nccl.py)
            self.dist.all_reduce(self.grad)
        t2 = tick()
        self.outer_step()
        if prof is not None:
            t3 = tick()
            prof['tasks_ms'] = prof.get('tasks_ms', 0.0) + 1e3 * (t1 - t0)
            prof['allreduce_ms'] = prof.get('allreduce_ms', 0.0) + 1e3 * (t2 - t1)
            prof['outer_step_ms'] = prof.get('outer_step_ms', 0.0) + 1e3 * (t3 - t2)
            prof['iterations'] = prof.get('iterations', 0) + 1
        return losses

    def _tick(self):
        """Wall clock after everything queued so far has finished (profiling passes only: it drains the GPU)."""
        import time
        for e in self._all_engines():
            e.synchronize()
        if self.state.is_cuda:
            torch.cuda.synchronize(self.state.device)
        return time.perf_counter()

    def outer_step(self):
        eng = self.eng
        self.step += 1
        nl = self.n_lr
        scale = 1.0 / self.meta_batch_size
        clip = float(self.grad_clip) if self.grad_clip is not None else 0.0
        fl, fp = (self._backbone_lr, self._backbone_param) if self.freeze_encoder else (0, 0)
        if self.use_log:                                    # clamp_init_lr, meta_optim.py:116-133
            lo, hi = -33.0, float('inf') if self.max_lr is None else math.log(self.max_lr)
        else:
            lo, hi = 0.0, float('inf') if self.max_lr is None else float(self.max_lr)
        # the gradient was summed by torch on the CURRENT stream; the engine's kernels run on ITS stream (the same one for an
        # engine built on the default stream, a different one for engines built for side-by-side work)
        es = getattr(eng, 'stream', None)
        cur = torch.cuda.current_stream(self.state.device) if self.state.is_cuda else None
        if es is not None and cur is not None and es != cur:
            es.wait_stream(cur)
        if self.fused_outer:
            n = nl + (eng.n_param if self.learn_model_init else 0)
            with _on_stream(eng):
                eng.outer_step(self.state[:n], self.grad[:n], self.exp_avg[:n], self.exp_avg_sq[:n], nl, self.learn_model_init,
                               self.step, self.log_init_lr_lr, self.model_init_lr, self.wd, grad_scale=scale, grad_clip=clip,
                               lr_lo=lo, lr_hi=hi, use_log=self.use_log, frozen_lr=fl, frozen_param=fp)
                if not self.learn_model_init:
                    self.grad[n:].zero_()               # the init part of the task gradients is not a Parameter: dropped
            if es is not None and cur is not None and es != cur:
                cur.wait_stream(es)
            return
        ranges = []                                          # (lo, hi, lr, weight decay): the reference's per-tensor groups
        if fl:
            ranges.append((0, fl, 0.0, 0.0))
        ranges.append((fl, nl, self.log_init_lr_lr, 0.0))
        if self.learn_model_init:
            if fp:
                ranges.append((nl, nl + fp, 0.0, self.wd))
            ranges.append((nl + fp, self.state.numel(), self.model_init_lr, self.wd))
        with _on_stream(eng):
            for a, b, lr, wd in ranges:
                eng.radam_step(self.state[a:b], self.grad[a:b], self.exp_avg[a:b], self.exp_avg_sq[a:b],
                               lr, wd, self.step, grad_scale=scale, grad_clip=clip)
            eng.clamp(self.state[:nl], lo, hi)
        if es is not None and cur is not None and es != cur:
            cur.wait_stream(es)
        self.grad.zero_()
        self._push_state()


def shard_tasks(n_tasks, rank, world):
    """Rank r of R takes tasks {r, r+R, ...} (`meta_run.py:39`)."""
    return list(range(rank, n_tasks, world))
