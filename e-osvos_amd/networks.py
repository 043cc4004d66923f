"""Drop-in for `src/networks/deeplabv3plus.py::DeepLabV3Plus` on the MI355X engine.

Same constructor arguments and call surface as the reference class (`deeplabv3plus.py:104-178,
259-301`): `model(inputs) -> [logits]`, `train_without_dropout()`, `eval()`, `train()`,
`to(device)`, `state_dict()/load_state_dict()` with the torchvision key names (374 keys),
`named_parameters()`, `parameters()`, `zero_grad()`.  The arithmetic runs in libeosvos.so; the
tensors kept here are the reference-layout (OIHW) *initial* weights and the frozen norm
statistics.  The engine is created lazily at the first forward (it needs the frame size) and
re-created when the frame size changes (DAVIS 480p frames are not all 854 wide).

Only the mode the fine-tuning loops use is implemented: BatchNorm in eval mode with frozen
affine (`batch_norm.accum_stats False`, `cfgs/meta.yaml:72-75`) and Dropout off; anything
else raises NotImplementedError (no silent fallback).  `train_encoder=False` (`cfgs/meta.yaml:71`)
freezes the backbone as the reference does (V3+: all but layer4, `deeplabv3plus.py:144-146`; V3: all of it,
`deeplabv3.py:53-54`): those tensors report `requires_grad == False` and every engine of the model ends its
backward pass at the boundary (`eosvos_set_trainable_from`).
"""
from collections import OrderedDict

import torch

from . import _ffi
from .engine import Engine
from .topology import conv_infos, frozen_tensors, model_state_keys, norm_layers, trainable, trainable_from


class _Param:
    """Minimal stand-in for torch.nn.Parameter as the reference loops use it: a tensor view with
    `.requires_grad`, `.grad`, `.data`."""

    def __init__(self, name, tensor, requires_grad):
        self.name, self.data, self.requires_grad, self.grad = name, tensor, requires_grad, None

    def numel(self):
        return self.data.numel()

    @property
    def shape(self):
        return self.data.shape

    @property
    def device(self):
        return self.data.device


class DeepLabV3Plus:
    def __init__(self, backbone, num_classes, batch_norm=None, train_encoder=True,
                 replace_batch_with_group_norms=False, max_batch=3, device='cuda:0'):
        if backbone not in ('resnet50', 'resnet101', 'deeplabv3_resnet50', 'deeplabv3_resnet101'):
            raise NotImplementedError(backbone)
        if backbone.startswith('deeplabv3_') and replace_batch_with_group_norms:
            raise NotImplementedError('plain DeepLabV3 has no GroupNorm variant (networks/deeplabv3.py)')
        if num_classes != 1:
            raise NotImplementedError('num_classes != 1')
        if batch_norm is not None and (batch_norm.get('accum_stats') or batch_norm.get('learn_weight')
                                       or batch_norm.get('learn_bias')):
            raise NotImplementedError('only frozen BatchNorm (accum_stats/learn_* False) is implemented')
        self._ctor = dict(backbone=backbone, num_classes=num_classes, batch_norm=batch_norm, train_encoder=train_encoder,
                          replace_batch_with_group_norms=replace_batch_with_group_norms)
        self.encoder = backbone
        self.norm = 'gn' if replace_batch_with_group_norms else 'bn'
        self.device = torch.device(device)
        self.max_batch = max_batch
        self.training = True
        self._dropout_off = False
        self.engine = None
        self._dirty = True                     # python-side state newer than the engine's
        self._lr_flat = None
        tr = trainable(backbone)
        self._names = [n for n, _ in tr]
        self._shapes = [s for _, s in tr]
        n_param = sum(int(torch.Size(s).numel()) for s in self._shapes)
        self._flat = torch.zeros(n_param)     # learned init, reference layout
        self._views = OrderedDict()
        off = 0
        for n, s in tr:
            k = int(torch.Size(s).numel())
            self._views[n] = self._flat[off:off + k].view(s)
            off += k
        self._norm = OrderedDict()
        for p, c in norm_layers(backbone):
            self._norm[p + '.weight'] = torch.ones(c)
            self._norm[p + '.bias'] = torch.zeros(c)
            if self.norm == 'bn':
                self._norm[p + '.running_mean'] = torch.zeros(c)
                self._norm[p + '.running_var'] = torch.ones(c)
                self._norm[p + '.num_batches_tracked'] = torch.zeros((), dtype=torch.long)
        self._train_from = trainable_from(backbone, train_encoder)         # first trainable conv (0: all of them)
        nf = frozen_tensors(backbone, train_encoder)
        self._params = OrderedDict((n, _Param(n, v, i >= nf)) for i, (n, v) in enumerate(self._views.items()))
        self._train_names = self._names[nf:]       # what MetaOptimizer learns (`meta_optim.py:46-78`): the requires_grad tensors

    # ---- nn.Module-like surface ---------------------------------------------------------
    def to(self, device):
        self.device = torch.device(device)
        return self

    def train(self, mode=True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def train_without_dropout(self):
        self.train()
        self._dropout_off = True

    def zero_grad(self):
        for p in self._params.values():
            p.grad = None

    def named_parameters(self):
        for n, p in self._params.items():
            yield n, p
        for k, v in self._norm.items():
            if k.endswith('.weight') or k.endswith('.bias'):
                yield k, _Param(k, v, False)

    def parameters(self):
        return (p for _, p in self.named_parameters())

    def state_dict(self):
        """Current (possibly fine-tuned) weights in the reference key order."""
        cur = self._flat
        if self.engine is not None and not self._dirty:
            cur = self.engine.get_params().cpu()
        out = OrderedDict()
        off = 0
        views = {}
        for n, s in zip(self._names, self._shapes):
            k = int(torch.Size(s).numel())
            views[n] = cur[off:off + k].view(s).clone()
            off += k
        for k in model_state_keys(self.encoder, self.norm):
            out[k] = views[k] if k in views else self._norm[k].clone()
        return out

    def load_state_dict(self, sd, strict=True):
        keys = model_state_keys(self.encoder, self.norm)
        if strict:
            missing = [k for k in keys if k not in sd]
            if missing:
                raise KeyError(f'missing keys in state_dict: {missing[:5]}...')
        for k in keys:
            if k not in sd:
                continue
            if k in self._views:
                self._views[k].copy_(sd[k])
            else:
                self._norm[k] = sd[k].detach().clone().cpu()
        self._dirty = True

    def spawn(self):
        """A second model with the same construction and learned state and its own (lazily built) engine -- for work
        that runs beside this one on the same GPU (the objects of a sequence, `evaluate.object_workers`)."""
        m = type(self)(max_batch=self.max_batch, device=str(self.device), **self._ctor)
        m._flat.copy_(self._flat)
        m._norm = OrderedDict((k, v.clone()) for k, v in self._norm.items())
        m.training, m._dropout_off = self.training, self._dropout_off
        return m

    def copy_state_from(self, other):
        """Take `other`'s learned init and frozen norm statistics (a spawned worker re-synchronised with its parent after
        the parent loaded another checkpoint: `evaluate_dataset` per dataset key, reference `evaluate.py:46-50`)."""
        if (self._flat.shape == other._flat.shape and torch.equal(self._flat, other._flat.to(self._flat.device)) and
                list(self._norm) == list(other._norm) and all(torch.equal(v, other._norm[k].to(v.device)) for k, v in self._norm.items())):
            return                          # nothing changed since the last copy: no re-upload, no new range-guard run
        self._flat.copy_(other._flat)
        self._norm = OrderedDict((k, v.clone()) for k, v in other._norm.items())
        self._dirty = True

    def set_side_stream(self, on):
        """`eosvos_set_side_stream` of this model's engine, now and whenever the engine is rebuilt (False while it runs
        beside other engines: `evaluate.run_objects_in_flight`)."""
        self.side_stream = bool(on)
        if self.engine is not None and hasattr(self.engine, 'set_side_stream'):
            self.engine.set_side_stream(self.side_stream)

    def set_wg_budget(self, workgroups):
        """`eosvos_set_wg_budget` of this model's engine, now and whenever the engine is rebuilt."""
        self.wg_budget = int(workgroups)
        if self.engine is not None and hasattr(self.engine, 'set_wg_budget'):      # (CPU stand-ins of the tests have none)
            self.engine.set_wg_budget(self.wg_budget)

    # ---- engine plumbing --------------------------------------------------------------------
    def _ensure_engine(self, height, width, batch):
        e = self.engine
        if e is None or e.height != height or e.width != width or batch > e.max_batch:
            carry = None
            if e is not None:
                # A new frame size / larger batch needs a new engine.  Fine-tuned weights travel with it; state that
                # cannot (the FIRST_STEP snapshot, the sum_k g_k of a running meta task) makes it an error instead of
                # silently restarting from the learned init.
                if e.in_meta_task and e.steps_since_reset > 0:
                    raise _ffi.EosvosError('frame size / batch changed in the middle of a meta task (sum_k g_k would be lost): '
                                           'size max_batch for the largest batch of the task up front')
                if e.has_snapshot:
                    raise _ffi.EosvosError('frame size / batch changed while a first-step snapshot is held (online adaptation): '
                                           'size max_batch for the adaptation batches up front')
                if e.steps_since_reset > 0 and not self._dirty:
                    carry = e.get_params()
                self._park_engine(e)
            want_side = getattr(self, 'side_stream', True)
            parked = self.__dict__.setdefault('_engine_cache', {}).pop((height, width), None)
            if parked is not None and (parked.max_batch < max(batch, self.max_batch) or getattr(parked, '_built_with_side', True) != want_side):
                parked.close()
                parked = None
            if parked is not None:           # the engine this model used for that frame size before (state re-uploaded below)
                self.engine = parked
                parked.steps_since_reset, parked.has_snapshot, parked.in_meta_task = 0, False, False
            else:
                kw = {} if want_side else {'side_stream': False}
                try:
                    self.engine = Engine(self.encoder, height, width, max(batch, self.max_batch), str(self.device), norm=self.norm, **kw)
                except _ffi.EosvosError:
                    # out of device memory with engines of other frame sizes parked (4-17 GB each): let them go and try once more
                    cache = self.__dict__.get('_engine_cache', {})
                    if not cache:
                        raise
                    for pe in cache.values():
                        pe.close()
                    cache.clear()
                    self.engine = Engine(self.encoder, height, width, max(batch, self.max_batch), str(self.device), norm=self.norm, **kw)
                self.engine._built_with_side = want_side
                if self._train_from:
                    self.engine.set_trainable_from(self._train_from)
            if getattr(self, 'wg_budget', 0) and hasattr(self.engine, 'set_wg_budget'):
                self.engine.set_wg_budget(self.wg_budget)
            if not getattr(self, 'side_stream', True) and hasattr(self.engine, 'set_side_stream'):
                self.engine.set_side_stream(False)
            self.max_batch = max(batch, self.max_batch)
            self._dirty = True
            if carry is not None:
                self.push_state()
                self.engine.set_params(carry)
                self.engine.steps_since_reset = 1
        if self._dirty:
            self.push_state()
        if getattr(self, '_pending_task_begin', False):
            self.engine.meta_task_begin()
            if getattr(self, '_pending_task_eval', False):      # reset() was followed by eval(): an evaluation fine-tune
                self.engine.in_meta_task = False
            self._pending_task_begin = self._pending_task_eval = False
        return self.engine

    ENGINE_CACHE = 2        # engines of other frame sizes kept for the next sequence of that size (creation costs ~0.5 s, 4-17 GB each)

    def _park_engine(self, e):
        """Videos come at their native sizes (854 / 910 x 480, 1280 x 720 ...): the engine of the size just left is kept, the least
        recently parked one beyond ENGINE_CACHE is closed."""
        cache = self.__dict__.setdefault('_engine_cache', {})
        old = cache.pop((e.height, e.width), None)
        if old is not None and old is not e:
            old.close()
        cache[(e.height, e.width)] = e
        while len(cache) > self.ENGINE_CACHE:
            cache.pop(next(iter(cache))).close()

    def _build_view_engine(self, height, width, batch):
        kw = {} if getattr(self, 'side_stream', True) else {'side_stream': False}
        return Engine(self.encoder, height, width, batch, str(self.device), norm=self.norm, **kw)

    def _view_engine(self, height, width, batch):
        """The engine that scores the height x width views of test-time augmentation (`tta.ViewSet`).  It lives BESIDE the live
        engine (`_ensure_engine` would replace that one, and refuses to while a first-step snapshot is held, which online
        adaptation always has): built on first use with this model's norm statistics, kept per size, and released by
        `close_parked_engines`.  Its weights are the caller's business (`ViewSet.sync`: the live engine's current ones)."""
        views = self.__dict__.setdefault('_view_engines', {})
        v = views.get((height, width))
        if v is not None and (v.max_batch < batch or getattr(v, 'h', True) is None):
            v.close()
            v = None
        if v is None:
            v = views[(height, width)] = self._build_view_engine(height, width, batch)
            v._norm_pushes = None
            if self._train_from and hasattr(v, 'set_trainable_from'):
                v.set_trainable_from(self._train_from)
            if getattr(self, 'wg_budget', 0) and hasattr(v, 'set_wg_budget'):
                v.set_wg_budget(self.wg_budget)
        pushes = self.__dict__.get('_push_count', 0)
        if v._norm_pushes != pushes:          # norm statistics as of the last push_state (the weights come from ViewSet.sync)
            nl = norm_layers(self.encoder)
            cat = lambda suf: torch.cat([self._norm[p + suf].reshape(-1).float() for p, _ in nl])
            if self.norm == 'gn':
                g = cat('.weight')
                v.set_norm(g, cat('.bias'), torch.zeros_like(g), torch.ones_like(g))
            else:
                v.set_norm(cat('.weight'), cat('.bias'), cat('.running_mean'), cat('.running_var'))
            v._norm_pushes = pushes
        return v

    def close_parked_engines(self):
        """Release the engines parked for other frame sizes and the view engines of test-time augmentation (keeps the live
        one)."""
        for e in self.__dict__.get('_engine_cache', {}).values():
            e.close()
        self.__dict__['_engine_cache'] = {}
        for e in self.__dict__.get('_view_engines', {}).values():
            e.close()
        self.__dict__['_view_engines'] = {}

    def close_engines(self):
        self.close_parked_engines()
        if self.engine is not None:
            self.engine.close()
            self.engine = None
            self._dirty = True

    def push_state(self):
        """Upload init weights / norm statistics (/ learning rates) to the engine; theta <- init."""
        e = self.engine
        e.set_init(self._flat)
        nl = norm_layers(self.encoder)
        cat = lambda suf: torch.cat([self._norm[p + suf].reshape(-1).float() for p, _ in nl])
        if self.norm == 'gn':
            g = cat('.weight')
            e.set_norm(g, cat('.bias'), torch.zeros_like(g), torch.ones_like(g))
        else:
            e.set_norm(cat('.weight'), cat('.bias'), cat('.running_mean'), cat('.running_var'))
        if self._lr_flat is not None:
            level, use_log = getattr(self, '_lr_mode', ('NEURON', False))
            lr = self._lr_flat
            if self._train_from:          # the learned lrs of the trainable tensors are the suffix of the engine's layout
                lr = torch.cat([torch.zeros(e.lr_store_count(level) - lr.numel(), dtype=lr.dtype, device=lr.device), lr])
            e.set_lr_state(level, use_log, lr)
        self._dirty = False
        self.__dict__['_push_count'] = self.__dict__.get('_push_count', 0) + 1

    def __call__(self, inputs):
        if self.training and not self._dropout_off:
            raise NotImplementedError('training-mode Dropout is not implemented: call train_without_dropout() '
                                      '(evaluate.py:213, meta_run.py:130) or eval()')
        if not inputs.is_cuda:
            raise _ffi.EosvosError('inputs must live on the GPU (no CPU path)')
        b, _, h, w = inputs.shape
        e = self._ensure_engine(h, w, b)
        logits = e.forward(inputs.contiguous().float())
        logits._eosvos_engine = e          # lets compute_loss / MetaOptimizer.step find the engine
        return [logits]

    forward = __call__


class DeepLabV3(DeepLabV3Plus):
    """Drop-in for `src/networks/deeplabv3.py::DeepLabV3` (`init_parent_model(architecture='DeepLabV3')`,
    `helper_func.py:343-344`): same constructor (`backbone, num_classes, batch_norm=None, train_encoder=True`), output
    stride 8, DeepLabHead (ASPP[12, 24, 36] -> 3x3 conv + BN + ReLU -> 1x1 conv), logits resized x8.  The reference class
    lacks `train_without_dropout()` (its loops call it, so it cannot run there at this commit); here
    it exists with the DeepLabV3+ meaning: frozen BatchNorm (`deeplabv3.py:56-62`) and Dropout off."""

    def __init__(self, backbone, num_classes, batch_norm=None, train_encoder=True, max_batch=3, device='cuda:0'):
        super().__init__('deeplabv3_' + backbone if not backbone.startswith('deeplabv3_') else backbone, num_classes,
                         batch_norm=batch_norm, train_encoder=train_encoder, replace_batch_with_group_norms=False,
                         max_batch=max_batch, device=device)
        self._ctor = dict(backbone=backbone, num_classes=num_classes, batch_norm=batch_norm, train_encoder=train_encoder)


def conv_names(encoder='resnet50'):
    return [c.name for c in conv_infos(encoder)]
