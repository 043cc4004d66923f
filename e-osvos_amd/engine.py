"""Python handle on one `eosvos_engine` (one per process / GPU, like the reference's one
model per process, `src/util/helper_func.py:499-512`).

torch-ROCm is used for device memory and streams only; every arithmetic call goes through
the C-ABI of include/eosvos.h.
"""
import collections
import ctypes
import functools

import torch

from . import _ffi, bootstrap, boundary, cldice, loss_sum, potts, surface
from .loss_names import (BY_KEYWORD, FAMILIES, LOSS_KINDS, resolve_cap, resolve_loss,  # noqa: F401  (their home; callers import them
                         resolve_name, resolve_radius)                                  # from here)
from .topology import ARCH_ID, norm_layers, trainable


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _optr(t):
    return _ptr(t) if t is not None else None


def _chunks(n, step):
    """(f, g) of every run of at most `step` frames of n, in order."""
    return ((f, min(f + step, n)) for f in range(0, n, step))


def _keep_flags(keep, n):
    """One byte per frame, 1 for the frame indices of `keep` (indices outside [0, n) are ignored)."""
    flags = bytearray(n)
    for f in keep:
        if 0 <= int(f) < n:
            flags[int(f)] = 1
    return flags


def _relu_bits(t):
    """ReLU mask bytes of t (..., C), the form the engine's data gradients read: bit j of byte q = (channel 4q + j > 0)."""
    if t is None:
        return None
    m = (t > 0).to(torch.uint8).reshape(*t.shape[:-1], -1, 4)
    return (m[..., 0] | (m[..., 1] << 1) | (m[..., 2] << 2) | (m[..., 3] << 3)).contiguous()


def _ld(t):
    """Leading dimension (elements per pixel) of a pixel-major view with unit channel stride whose images are P pixels apart."""
    if t is None:
        return 0
    assert t.stride(-1) == 1 and t.stride(0) == t[0].numel() // t.shape[-1] * t.stride(-2), 'not a pixel-major view'
    return t.stride(-2)


def _dev_f32(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _touched(*tensors):
    """The library wrote these caller tensors through raw pointers: bump their in-place version counters, so that code which
    keys a cache on `tensor._version` (MetaOptimizer.load_state_dict's skip of an unchanged state) sees the change."""
    for t in tensors:
        if t is not None:
            torch.autograd.graph.increment_version(t)


LR_LEVELS = {'NEURON': 0, 'TENSOR': 1, 'SINGLE': 2, 'PARAM': 3}      # include/eosvos.h EOSVOS_LR_*
# One resolved `loss_func`: the ctypes arrays of its n kinds and weights, whether the engine combines them (a spelling with
# '+' or '*') or runs kinds[0]'s own launches alone, and the fraction / radius / cap the spelling or its keyword carries (None:
# the engine's current value stays), the (radius or None, dilation or None) of a `potts` term (None without one), and the depth a
# `cldice` term carries (None: the engine's stays).
LossSpec = collections.namedtuple('LossSpec', 'n kinds weights combine fraction radius cap window depth')


@functools.lru_cache(maxsize=64, typed=True)
def _resolve(name, fraction, radius, cap=None, window=None, depth=None):
    """A sum spelling (`loss_sum.resolve_terms`) or a plain name (`loss_names.resolve_name`, one term of weight 1) as a
    LossSpec, kept per spelling: splitting and checking one takes ~10 us on the host, which a loss whose launches take 30 us
    would otherwise pay on every evaluation (`profiles/loss_sum_time.txt`); a spelling that raises is not kept."""
    combine = loss_sum.is_sum(name)
    if combine:
        kinds, weights, _, knobs = loss_sum.resolve_terms(name, fraction=fraction, radius=radius, cap=cap, window=window, depth=depth)
    else:
        kind, knobs = resolve_name(name, fraction, radius, cap, window, depth)
        kinds, weights = [kind], [1.0]
    n = len(kinds)
    return LossSpec(n, (ctypes.c_int * n)(*kinds), (ctypes.c_float * n)(*weights), combine, *knobs)


# the order `_loss_spec` has always applied a spelling's knobs in: depth, window, cap, fraction, radius
_APPLIED = (*reversed(FAMILIES[2:]), *FAMILIES[:2])


def check_ignore(ignore):
    """The void label of a loss (`ignore=` of networks/loss_lovasz.py:78-126) as a float: finite and outside [0, 1], so that no
    target can take it."""
    v = float(ignore)
    if v != v or v in (float('inf'), float('-inf')) or 0.0 <= v <= 1.0:
        raise ValueError(f'ignore={ignore!r}: the void label must be finite and outside [0, 1]')
    return v


def set_matrix_mode(mode):
    """'f16x3' (default), 'bf16x6' or 'f32': how the convolutions' fp32 contractions use the matrix cores (process-wide; include/eosvos.h)."""
    _ffi.check(_ffi.load().eosvos_set_matrix_mode({'f32': 0, 'bf16x6': 1, 'f16x3': 2}[mode]))


def get_matrix_mode():
    return {0: 'f32', 1: 'bf16x6', 2: 'f16x3'}[_ffi.load().eosvos_get_matrix_mode()]


# f16x3 range guard (see Engine.verify_matrix_mode): absolute / relative logit difference against the exact-split mode above
# which the ENGINE falls back to bf16x6.  A tenth of the north_star logit tolerance; measured differences between the two
# modes: 1e-5 on the benign synthetic state, 1e-5 on the heavy-tailed one of fixture G19 (profiles/r04_g19_margins.txt).
GUARD_ABS_TOL, GUARD_REL_TOL = 1e-4, 1e-4
# ... and of ONE fine-tune step: relative loss difference, and per trainable tensor max |delta_f16x3 - delta_bf16x6| of the
# parameter update (= lr * gradient) against GUARD_STEP_TOL * max |delta_bf16x6| + GUARD_PARAM_TOL * max |parameter| -- the
# second term because the update is observed THROUGH the fp32 parameters: one step moves a weight by 40 ... 150 of its ulps, so
# updates that differ by one ulp of the weight differ by 1/38 ... 1/150 of themselves (measured on every fixture state; 1e-6 =
# 8 ulps of the tensor's largest weight, and the parity tests hold parameters to 3e-6 of their maximum after T steps).
# Measured between the two modes: loss 2e-7, update <= 3e-4 of a tensor's maximum (ReLU-gate flips on the heavy-tailed state).
# A third term allows for ReLU-gate flips: a pre-activation within rounding of 0 is gated differently by the two modes, which
# moves a whole pixel's contribution in or out of every weight gradient downstream of it -- 1 / (pixels of the map) of the
# tensor's update, percents on the stride-16 maps of small frames (6 x 10 at 96 x 160: measured 2.6e-2), 1e-4 at 480 x 854.
# The tolerance is GUARD_STEP_TOL + GUARD_FLIP_PIXELS / (batch x pixels of the stride-16 map): the step half of the guard is a
# detector of GROSS range failures in the backward pass (an out-of-envelope state is wrong by O(1), see
# tests/test_gpu_heavy_tailed.py); the fine accuracy of the mode is what the reference fixtures G15 / G19 / G20 / G21 pin.
GUARD_LOSS_REL_TOL, GUARD_STEP_TOL, GUARD_PARAM_TOL, GUARD_FLIP_PIXELS = 1e-4, 5e-3, 1e-6, 4.0
GUARD_LOG = []                       # (reason, max difference) of every fallback this process took
_MODE_IDS = {'f32': 0, 'bf16x6': 1, 'f16x3': 2}
_MODE_NAMES = {v: k for k, v in _MODE_IDS.items()}


def _guard_enabled():
    import os
    return os.environ.get('EOSVOS_MODE_GUARD', '1') != '0'


_POOL_WARMED = []


def warm_stream_pool(device):
    """ROCm deals HIP streams onto a few hardware queues (four by default): the first streams get a queue each, later ones
    the least-referenced queue, and engines that run side by side lose a quarter of their rate when two of their streams
    share a queue (tools/stream_queue_probe.py, profiles/r03_stream_queue_probe.txt: 4 engines at batch 1, 207 vs 263
    iterations/s).  torch hands out its 32 pooled streams in order; four consecutive ones sit on four different queues
    EXCEPT among the first three of the pool, which are dealt while the queue pool is still filling.  So the pool is
    instantiated, and its first three streams are burnt, before this package creates any stream of its own."""
    if _POOL_WARMED or not torch.cuda.is_available():
        return
    _POOL_WARMED.extend(torch.cuda.Stream(device) for _ in range(3))


class Engine:
    def __init__(self, encoder='resnet50', height=480, width=854, max_batch=3, device='cuda:0', norm='bn', side_stream=True):
        """`side_stream=False`: an engine that will run beside others (one queue each, `eosvos_set_side_stream`) is built
        without the second stream in the first place -- which hardware queue / pipe a stream lands on depends on every
        stream created before it, and engines whose queues share a pipe run at three quarters of their rate."""
        if not torch.cuda.is_available():
            raise _ffi.EosvosError('no GPU visible: the e-osvos_amd engine has no CPU path')
        self.lib = _ffi.load()
        self.encoder = encoder
        self.norm = norm
        if norm not in ('bn', 'gn'):
            raise NotImplementedError(norm)
        self.arch = ARCH_ID[encoder]
        self.device = torch.device(device)
        self.height, self.width, self.max_batch = height, width, max_batch
        self.n_param = int(self.lib.eosvos_param_count(self.arch))
        self.n_lr = int(self.lib.eosvos_lr_count(self.arch))
        self.n_norm = int(self.lib.eosvos_norm_count(self.arch))
        self.lr_level, self.lr_log = 'NEURON', False
        self.n_lr_store = self.n_lr
        torch.cuda.set_device(self.device)
        warm_stream_pool(self.device)
        self.stream = torch.cuda.current_stream(self.device)
        h = ctypes.c_void_p()
        _ffi.check(self.lib.eosvos_create_ex(ctypes.byref(h), self.arch, 1 if norm == 'gn' else 0, height, width, max_batch,
                                             self.device.index or 0, ctypes.c_void_p(self.stream.cuda_stream),
                                             0 if side_stream else 1))          # EOSVOS_CREATE_NO_SIDE_STREAM
        self.h = h
        self.train_from = 0                # eosvos_set_trainable_from
        self._loss = torch.zeros(1, device=self.device)
        # host-side view of the engine's state (networks.DeepLabV3Plus carries it across an engine re-creation)
        self.steps_since_reset, self.has_snapshot, self.in_meta_task = 0, False, False

    def close(self):
        if getattr(self, 'h', None):
            self.lib.eosvos_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state ----------------------------------------------------------------------
    def set_init(self, flat, verify=True):
        """`verify=False`: a state that evolves in small steps from one the range guard has seen (the outer loop's upload)."""
        flat = _dev_f32(flat, self.device)
        assert flat.numel() == self.n_param
        _ffi.check(self.lib.eosvos_set_init(self.h, _ptr(flat)))
        self.synchronize()
        self.steps_since_reset = 0
        if verify:
            self._new_state_for_guard()      # new weights: the f16x3 range guard looks at the next forward

    def set_lr(self, flat):
        flat = _dev_f32(flat, self.device)
        assert flat.numel() == self.n_lr
        _ffi.check(self.lib.eosvos_set_lr(self.h, _ptr(flat)))
        self.lr_level, self.lr_log, self.n_lr_store = 'NEURON', False, self.n_lr
        self.synchronize()

    def lr_store_count(self, level):
        return int(self.lib.eosvos_lr_store_count(self.arch, LR_LEVELS[level]))

    def set_lr_state(self, level, use_log, flat):
        """Learned lr state at `lr_hierarchy_level` (flat, reference tensor order), optionally log(lr)."""
        if level not in LR_LEVELS:
            raise NotImplementedError(level)            # meta_optim.py:68-69
        flat = _dev_f32(flat, self.device)
        n = self.lr_store_count(level)
        assert flat.numel() == n, (flat.numel(), n)
        _ffi.check(self.lib.eosvos_set_lr_state(self.h, LR_LEVELS[level], int(bool(use_log)), _ptr(flat)))
        self.lr_level, self.lr_log, self.n_lr_store = level, bool(use_log), n
        self.synchronize()

    def set_loss(self, name, ignore=None, fraction=None, radius=None, cap=None, window=None, depth=None):
        """Loss of finetune_step / meta_grad (`loss_func`, helper_func.py:28-56) and its void label (None: every pixel counts).
        `bootstrapped_cross_entropy_<P>` or `fraction=` also set the engine's bootstrap fraction, `boundary_f_<r>` /
        `cross_entropy_and_boundary_f_<r>` or `radius=` its boundary radius, `surface_<L>` or `cap=` its surface cap,
        `potts_<r>` / `potts_<r>x<d>` or `window=` its potts window, `cldice_<k>` or `depth=` its cldice depth (see
        `_loss_spec`).  A sum spelling
        (`0.5*lovasz_hinge+boundary_f_4`, `loss_sum.py`) selects `eosvos_set_loss_sum`; a single name returns to one kind."""
        try:
            spec = self._loss_spec(name, fraction, radius, cap, window, depth)
        except KeyError:
            raise NotImplementedError(name) from None   # helper_func.py:55-56
        v = None if ignore is None else check_ignore(ignore)
        if spec.combine:
            _ffi.check(self.lib.eosvos_set_loss_sum(self.h, spec.n, spec.kinds, spec.weights))
        else:
            _ffi.check(self.lib.eosvos_set_loss(self.h, spec.kinds[0]))
        _ffi.check(self.lib.eosvos_set_loss_ignore(self.h, int(v is not None), v or 0.0))

    def set_loss_bootstrap(self, fraction):
        """The fraction of `bootstrapped_cross_entropy` for every later evaluation on this engine (`eosvos_set_loss_bootstrap`;
        0.25 on a new engine)."""
        _ffi.check(self.lib.eosvos_set_loss_bootstrap(self.h, bootstrap.check_fraction(fraction)))

    def _set_whole(self, keyword, value):
        """A whole-number knob for every later evaluation on this engine, by its family's entry point: 0 for the frame-size
        default, otherwise what the family's check lets through (a bool is no 0)."""
        family = BY_KEYWORD[keyword]
        _ffi.check(getattr(self.lib, 'eosvos_' + family.setter)(self.h, 0 if value == 0 and not isinstance(value, bool)
                                                                 else family.check(value)))

    def set_loss_boundary(self, radius):
        """The window radius of `boundary_f` / `cross_entropy_and_boundary_f` for every later evaluation on this engine
        (`eosvos_set_loss_boundary`): 1 .. 16, or 0 for the frame-size default `boundary.default_radius(H, W)`, which a new
        engine has."""
        self._set_whole('radius', radius)

    def set_loss_surface(self, cap):
        """The distance cap of `surface` for every later evaluation on this engine (`eosvos_set_loss_surface`): 1 .. 4095, or
        0 for the frame-size default `surface.default_cap(H, W)`, which a new engine has.  The default is untuned."""
        self._set_whole('cap', cap)

    def set_loss_cldice(self, depth):
        """The depth (the number of erosions of the soft skeleton) of `cldice` for every later evaluation on this engine
        (`eosvos_set_loss_cldice`): 1 .. 16, or 0 for the frame-size default `cldice.default_depth(H, W)`, which a new engine
        has.  The default is untuned."""
        self._set_whole('depth', depth)

    def set_loss_potts(self, window=None, dilation=None, sigma_xy=None, sigma_rgb=None):
        """Window radius (1 .. 7), dilation (1 .. 4, radius * dilation <= 16) and sigmas (finite, > 0) of `potts` for every
        later evaluation on this engine (`eosvos_set_loss_potts`).  None keeps what the engine has, 0 returns to the default
        (3, 2, radius * dilation, 0.1), which a new engine has.  The defaults are untuned."""
        now = dict(getattr(self, '_potts', None) or {'window': 0, 'dilation': 0, 'sigma_xy': 0.0, 'sigma_rgb': 0.0})
        for key, v in (('window', window), ('dilation', dilation), ('sigma_xy', sigma_xy), ('sigma_rgb', sigma_rgb)):
            if v is None:
                continue
            if v == 0 and not isinstance(v, bool):
                now[key] = 0
            elif key == 'window':
                now[key] = potts.check_window(v)
            elif key == 'dilation':
                now[key] = potts.check_window(1, v)[1]
            else:
                now[key] = potts.check_sigma(key, v)
        potts.check_window(now['window'] or potts.DEFAULT_WINDOW, now['dilation'] or potts.DEFAULT_DILATION)
        _ffi.check(self.lib.eosvos_set_loss_potts(self.h, now['window'], now['dilation'], now['sigma_xy'], now['sigma_rgb']))
        self._potts = now

    def _loss_spec(self, name, fraction=None, radius=None, cap=None, window=None, depth=None):
        """The LossSpec of a spelled `loss_func` (`_resolve`); a fraction, radius, cap, window or depth carried by the spelling or
        the keyword becomes the engine's before the call that follows."""
        spec = _resolve(name, fraction, radius, cap, window, depth)
        for family in _APPLIED:
            knob = getattr(spec, family.keyword)
            args = knob if isinstance(knob, tuple) else (knob,)      # (potts carries a pair; (None, None) asks for nothing)
            if any(a is not None for a in args):
                getattr(self, family.setter)(*args)
        return spec

    def _loss_on_forward(self, spec, masks, ignore, out):
        """The spec on the last forward: eosvos_loss, eosvos_loss_ignore with a void label, or eosvos_loss_sum."""
        b = masks.shape[0]
        if spec.combine:
            _ffi.check(self.lib.eosvos_loss_sum(self.h, spec.n, spec.kinds, spec.weights, _ptr(masks), b, int(ignore is not None),
                                                ignore or 0.0, _optr(out)))
        elif ignore is None:
            _ffi.check(self.lib.eosvos_loss(self.h, spec.kinds[0], _ptr(masks), b, _optr(out)))
        else:
            _ffi.check(self.lib.eosvos_loss_ignore(self.h, spec.kinds[0], _ptr(masks), b, ignore, _optr(out)))

    def _loss_on_tensors(self, spec, logits, masks, ignore, out, grad=None):
        """The spec on caller tensors, the elements one set: eosvos_loss_tensors, eosvos_loss_tensors_ignore with a void label,
        or eosvos_loss_sum_tensors -- the one that hands a gradient back, so with `grad` a single kind goes there too, as the
        sum of one term of weight 1, which has that kind's bits."""
        n = logits.numel()
        if spec.combine or grad is not None:
            _ffi.check(self.lib.eosvos_loss_sum_tensors(self.h, spec.n, spec.kinds, spec.weights, _ptr(logits), _ptr(masks), n,
                                                        int(ignore is not None), ignore or 0.0, _ptr(out), _optr(grad)))
        elif ignore is None:
            _ffi.check(self.lib.eosvos_loss_tensors(self.h, spec.kinds[0], _ptr(logits), _ptr(masks), n, _ptr(out)))
        else:
            _ffi.check(self.lib.eosvos_loss_tensors_ignore(self.h, spec.kinds[0], _ptr(logits), _ptr(masks), n, ignore, _ptr(out)))

    def set_norm(self, gamma, beta, mean, var, eps=1e-5):
        ts = [_dev_f32(t, self.device) for t in (gamma, beta, mean, var)]
        assert all(t.numel() == self.n_norm for t in ts)
        _ffi.check(self.lib.eosvos_set_norm(self.h, *[_ptr(t) for t in ts], ctypes.c_float(eps)))
        self.synchronize()
        self._new_state_for_guard()          # new norm statistics: same

    def load_model_state(self, state_dict, lrs=None):
        """Convenience: reference-style model state dict (+ list of NEURON lr tensors)."""
        names = [n for n, _ in trainable(self.encoder)]
        self.set_init(torch.cat([state_dict[n].reshape(-1).float() for n in names]))
        nl = norm_layers(self.encoder)
        cat = lambda suf: torch.cat([state_dict[p + suf].reshape(-1).float() for p, _ in nl])
        if self.norm == 'gn':       # GroupNorm shares only the affine (no running statistics in the state dict)
            g = cat('.weight')
            self.set_norm(g, cat('.bias'), torch.zeros_like(g), torch.ones_like(g))
        else:
            self.set_norm(cat('.weight'), cat('.bias'), cat('.running_mean'), cat('.running_var'))
        if lrs is not None:
            self.set_lr(torch.cat([l.reshape(-1).float() for l in lrs]))

    def reset(self):
        _ffi.check(self.lib.eosvos_reset(self.h))
        # theta <- init starts a new object / task: the first-step snapshot of the previous one is dead
        self.steps_since_reset, self.in_meta_task, self.has_snapshot = 0, False, False

    def get_params(self):
        out = torch.empty(self.n_param, device=self.device)
        _ffi.check(self.lib.eosvos_get_params(self.h, _ptr(out)))
        if torch.cuda.current_stream(self.device) != self.stream:
            self.synchronize()            # the export ran on the engine's stream: a caller on another stream must not read it early
        return out

    def set_params(self, flat):
        flat = _dev_f32(flat, self.device)
        _ffi.check(self.lib.eosvos_set_params(self.h, _ptr(flat)))
        self.synchronize()

    def snapshot(self):
        _ffi.check(self.lib.eosvos_snapshot_params(self.h))
        self.has_snapshot = True

    def restore(self):
        _ffi.check(self.lib.eosvos_restore_params(self.h))

    # ---- hot loop -------------------------------------------------------------------
    def _check_stream(self):
        """The engine launches on the stream that was current when it was built; tensors the caller produces or
        consumes on another torch stream would be unordered with those launches."""
        if torch.cuda.current_stream(self.device) != self.stream:
            raise _ffi.EosvosError('the current torch stream is not the stream this engine is bound to: call it under '
                                   '`with torch.cuda.stream(engine.stream)` (or build the engine on this stream)')

    def _check_images(self, images):
        self._check_stream()
        assert images.is_cuda and images.dtype == torch.float32 and images.is_contiguous()
        b, c, h, w = images.shape
        assert c == 3 and h == self.height and w == self.width and 1 <= b <= self.max_batch, images.shape
        return b

    # ---- matrix mode of this engine / f16x3 range guard -------------------------------------
    @property
    def matrix_mode(self):
        """The mode this engine's contractions run in: its own (`set_engine_matrix_mode`) or the process-wide one."""
        return _MODE_NAMES[self.lib.eosvos_get_engine_matrix_mode(self.h)]

    def set_engine_matrix_mode(self, mode):
        """'f16x3' / 'bf16x6' / 'f32' for THIS engine only (`eosvos_set_engine_matrix_mode`); None: follow the process-wide mode."""
        _ffi.check(self.lib.eosvos_set_engine_matrix_mode(self.h, -1 if mode is None else _MODE_IDS[mode]))
        self._own_mode = mode
        self._guard_fell_back = False        # (set again by _fall_back: only a guard-made bf16x6 is undone by the next state)

    def plan_fingerprint(self):
        """(forward, backward) launch-plan hashes of the last passes (`eosvos_plan_fingerprint`)."""
        out = (ctypes.c_uint64 * 2)()
        _ffi.check(self.lib.eosvos_plan_fingerprint(self.h, out))
        return int(out[0]), int(out[1])

    def _new_state_for_guard(self):
        """A new state was loaded: the range guard looks at the next forward.  An engine that sits in bf16x6 because the guard
        moved it there for the PREVIOUS state (not because the caller chose the mode) follows the process-wide mode again
        and is checked afresh -- a parked engine / a long-lived object worker would otherwise stay in the slower exact mode
        for every later checkpoint and sequence."""
        if getattr(self, '_guard_fell_back', False):
            self._guard_fell_back = False
            self.set_engine_matrix_mode(None)
        self._verify_pending = True

    def _fall_back(self, reason, diff, scale):
        import warnings
        self.set_engine_matrix_mode('bf16x6')
        self._guard_fell_back = True
        GUARD_LOG.append((reason, diff))
        warnings.warn(f'e-osvos_amd: {reason}: {diff:.3g} (scale {scale:.3g}) for this state / input: the dynamic range inside an '
                      'operand tensor exceeds what one power-of-two scale per tensor covers.  This engine continues in the '
                      'bf16x6 matrix mode.', RuntimeWarning)
        return 'bf16x6'

    def verify_matrix_mode(self, images, masks=None, loss_kind=None):
        """Range guard of the default matrix mode.  f16x3 runs every fp32 contraction on the fp16 matrix cores under ONE
        power-of-two scale per operand tensor: elements more than ~2^-18 below their tensor's largest magnitude keep fewer
        bits (absolute error floor 2^-40 of that maximum).  Reference-generated fixtures cover benign and heavy-tailed
        (BatchNorm statistics over 4-6 decades, G19) states; for anything outside, this check runs the ACTUAL weights / norm
        statistics / input in f16x3 and in the exact-split mode (bf16x6: no range assumption):
          * the forward pass: logits must agree to GUARD_ABS_TOL + GUARD_REL_TOL * max|logit| (and be finite in both or neither);
          * with `masks` (round 5): ONE whole fine-tune step -- loss to GUARD_LOSS_REL_TOL and, per trainable tensor, the
            parameter update (lr x gradient: the backward pass's operands have the wider dynamic range) to GUARD_STEP_TOL (+ an
            allowance for ReLU-gate flips, see GUARD_FLIP_PIXELS) of the tensor's largest update; the weights are put back
            afterwards.
        If either differs, THIS ENGINE moves to bf16x6 (`eosvos_set_engine_matrix_mode`; other engines and the process-wide
        mode are untouched) with a RuntimeWarning and an entry in GUARD_LOG.  Runs automatically at the first forward /
        fine-tune step after new weights or norm statistics were set (EOSVOS_MODE_GUARD=0 disables); costs two forward passes
        (+ two steps) per loaded state.  A process group is NOT consulted here (the call is lazy, ranks may differ in how
        often they get here); `MetaTrainer` makes the decision collective for its ranks.  Returns the mode in effect."""
        if self.matrix_mode != 'f16x3':
            self._verify_pending = self._step_check_pending = False
            return self.matrix_mode
        own = getattr(self, '_own_mode', None)
        b = self._check_images(images)
        a = torch.empty(b, 1, self.height, self.width, device=self.device)
        ref = torch.empty_like(a)
        try:
            _ffi.check(self.lib.eosvos_forward(self.h, _ptr(images), b, _ptr(a)))
            self.set_engine_matrix_mode('bf16x6')
            _ffi.check(self.lib.eosvos_forward(self.h, _ptr(images), b, _ptr(ref)))
        finally:
            self.set_engine_matrix_mode(own)                 # (an exception leaves the check pending: nothing was decided)
        self._verify_pending = False
        fin_a, fin_r = bool(torch.isfinite(a).all()), bool(torch.isfinite(ref).all())
        scale = float(ref[torch.isfinite(ref)].abs().max()) if bool(torch.isfinite(ref).any()) else 0.0
        diff = float((a - ref).abs().max()) if (fin_a and fin_r) else float('inf')
        if (fin_r and not fin_a) or (fin_a and fin_r and diff > GUARD_ABS_TOL + GUARD_REL_TOL * scale):
            self._step_check_pending = False
            return self._fall_back('f16x3 logits differ from the exact-split mode', diff, scale)
        if masks is None:
            return 'f16x3'
        return self._verify_step(images, masks, loss_kind)

    def _verify_step(self, images, masks, loss_kind=None, ignore=None):
        """The fine-tune-step half of the guard (see verify_matrix_mode): one step in each split mode from the same weights.
        `loss_kind` None: the fused step with the engine's own loss and void label; otherwise that loss with `ignore`."""
        self._step_check_pending = False
        own = getattr(self, '_own_mode', None)
        b = images.shape[0]
        p0 = self.get_params()
        got = {}
        try:
            for mode in ('f16x3', 'bf16x6'):
                self.set_engine_matrix_mode(mode)
                if loss_kind is None:
                    _ffi.check(self.lib.eosvos_finetune_step(self.h, _ptr(images), _ptr(masks), b, 0, None))
                else:
                    _ffi.check(self.lib.eosvos_forward(self.h, _ptr(images), b, None))
                    self._loss_on_forward(self._loss_spec(loss_kind), masks, ignore, None)
                    _ffi.check(self.lib.eosvos_backward_step(self.h, 0))
                loss = torch.empty(1, device=self.device)
                _ffi.check(self.lib.eosvos_last_loss(self.h, _ptr(loss)))
                got[mode] = (loss, self.get_params())
                _ffi.check(self.lib.eosvos_set_params(self.h, _ptr(p0)))
        finally:
            self.set_engine_matrix_mode(own)
        (la, pa), (lb, pb) = got['f16x3'], got['bf16x6']
        la, lb = float(la), float(lb)
        fin_a, fin_b = bool(torch.isfinite(pa).all()) and la == la, bool(torch.isfinite(pb).all()) and lb == lb
        if fin_b and not fin_a:
            return self._fall_back('f16x3 fine-tune step is not finite, the exact-split mode\'s is', float('inf'), abs(lb))
        if not (fin_a and fin_b):
            return 'f16x3'                                       # not finite in either mode: nothing a mode change repairs
        if abs(la - lb) > GUARD_LOSS_REL_TOL * max(1.0, abs(lb)):
            return self._fall_back('f16x3 loss differs from the exact-split mode', abs(la - lb), abs(lb))
        db = (pb - p0).abs()
        err = (pa - pb).abs()                                    # = |delta_f16x3 - delta_bf16x6|
        sizes = []
        for _, shape in trainable(self.encoder):
            n = 1
            for d in shape:
                n *= d
            sizes.append(n)
        e_max = torch.stack([t.max() for t in err.split(sizes)])
        d_max = torch.stack([t.max() for t in db.split(sizes)])
        p_max = torch.stack([t.max() for t in p0.abs().split(sizes)])
        step_tol = GUARD_STEP_TOL + GUARD_FLIP_PIXELS / (b * ((self.height + 15) // 16) * ((self.width + 15) // 16))
        tol = step_tol * d_max + GUARD_PARAM_TOL * p_max
        ratio = e_max / tol.clamp_min(1e-30)
        worst = int(ratio.argmax())
        self.last_step_check = {'worst_tensor': trainable(self.encoder)[worst][0], 'ratio_to_tolerance': float(ratio[worst]),
                                'update_diff': float(e_max[worst]), 'largest_update': float(d_max[worst]), 'loss_rel': abs(la - lb) / max(1.0, abs(lb))}
        if float(ratio[worst]) > 1.0:
            return self._fall_back(f'f16x3 parameter update of {trainable(self.encoder)[worst][0]} differs from the exact-split mode',
                                   float(e_max[worst]), float(d_max[worst]))
        return 'f16x3'

    def _guard(self, images, masks=None, want_step=False):
        """First forward / step after a state load: the forward half at once; the step half with `masks` (finetune_step) or,
        for callers that go forward -> loss -> backward_step separately, deferred to backward_step (`_step_check_pending`)."""
        if getattr(self, '_verify_pending', False) and _guard_enabled():
            mode = self.verify_matrix_mode(images, masks)
            if masks is None and want_step and mode == 'f16x3':
                self._step_check_pending = True
                self._chk_images, self._chk_masks, self._chk_kind, self._chk_ignore = images, None, None, None

    def forward(self, images, want_logits=True):
        b = self._check_images(images)
        self._guard(images, want_step=True)
        if getattr(self, '_step_check_pending', False):
            self._chk_images, self._chk_masks = images, None      # (the forward whose loss / backward_step may follow)
        out = torch.empty(b, 1, self.height, self.width, device=self.device) if want_logits else None
        _ffi.check(self.lib.eosvos_forward(self.h, _ptr(images), b, _ptr(out) if want_logits else None))
        return out

    def loss_bce(self, masks):
        assert masks.is_cuda and masks.dtype == torch.float32 and masks.is_contiguous()
        loss = torch.empty(1, device=self.device)
        _ffi.check(self.lib.eosvos_loss_bce(self.h, _ptr(masks), masks.shape[0], _ptr(loss)))
        if getattr(self, '_step_check_pending', False):
            self._chk_masks, self._chk_kind, self._chk_ignore = masks, 'cross_entropy', None
        return loss

    def loss(self, kind, masks, ignore=None, fraction=None, radius=None, cap=None, window=None, depth=None):
        """kind: a compute_loss name (helper_func.py:28-56, see LOSS_KINDS); leaves dL/dlogits.  `ignore`: the void label --
        pixels whose mask equals it are in no sum, count or ranking and get gradient 0 (`eosvos_loss_ignore`).  `fraction`:
        of `bootstrapped_cross_entropy`, `radius`: of the boundary kinds, `cap`: of `surface`, `window`: of `potts` (which
        reads the frames of the last forward and not the masks), `depth`: of `cldice`, as in `set_loss`.  A sum spelling
        evaluates the weighted sum of its terms (`eosvos_loss_sum`); `last_loss_terms` then gives the terms' own values."""
        spec = self._loss_spec(kind, fraction, radius, cap, window, depth)
        ignore = None if ignore is None else check_ignore(ignore)
        assert masks.is_cuda and masks.dtype == torch.float32 and masks.is_contiguous()
        out = torch.empty(1, device=self.device)
        self._loss_on_forward(spec, masks, ignore, out)
        if getattr(self, '_step_check_pending', False):
            self._chk_masks, self._chk_kind, self._chk_ignore = masks, kind, ignore
        return out

    def loss_of(self, kind, logits, masks, ignore=None, fraction=None, radius=None, cap=None, depth=None):
        """Value of a compute_loss loss on arbitrary device tensors (one sample of a batch for
        `batch_average: False`); no gradient is kept.  `ignore`: as in `loss` (`eosvos_loss_tensors_ignore`); `fraction`: of
        `bootstrapped_cross_entropy`, `radius`: of the boundary kinds, `cap`: of `surface`, `depth`: of `cldice`, as in `set_loss`.  The
        boundary kinds, `surface` and `cldice` need the frame's shape: they take one image of the engine's H * W elements only
        (`boundary_f`, `surface_loss` and `cldice_loss` below take any shape).  `potts` is refused: no frames travel with the tensors (`potts_loss` takes them)."""
        logits, masks = logits.contiguous(), masks.contiguous()
        assert logits.is_cuda and masks.is_cuda and logits.numel() == masks.numel()
        out = torch.empty(1, device=self.device)
        self._loss_on_tensors(self._loss_spec(kind, fraction, radius, cap, None, depth), logits, masks,
                              None if ignore is None else check_ignore(ignore), out)
        return out

    def loss_grad_of(self, name, logits, masks, ignore=None, fraction=None, radius=None, cap=None, depth=None):
        """(loss, dL/dlogits of the logits' shape) of a single kind or a sum on arbitrary device tensors, the elements one set
        as in `loss_of` (`eosvos_loss_sum_tensors`; a single kind is the sum of one term of weight 1, which has that kind's
        bits).  At most the engine's largest batch of pixels; the engine's own gradient is untouched.  A `potts` term is refused
        as in `loss_of`."""
        logits, masks = logits.contiguous(), masks.contiguous()
        assert logits.is_cuda and masks.is_cuda and logits.dtype == masks.dtype == torch.float32
        assert logits.numel() == masks.numel()
        v = None if ignore is None else check_ignore(ignore)
        out, grad = torch.empty(1, device=self.device), torch.empty_like(logits)
        try:
            spec = self._loss_spec(name, fraction, radius, cap, None, depth)
        except KeyError:
            raise NotImplementedError(f"loss_func='{name}'") from None
        self._loss_on_tensors(spec, logits, masks, v, out, grad)
        return out, grad

    def last_loss_terms(self):
        """The unweighted values of the terms of the last sum evaluated on this engine, in spelled order
        (`eosvos_last_loss_terms`): by `loss` / `loss_of` / `loss_grad_of`, or by `finetune_step` / `meta_grad` under a sum."""
        out, n = torch.empty(loss_sum.MAX_TERMS, device=self.device), ctypes.c_int(0)
        _ffi.check(self.lib.eosvos_last_loss_terms(self.h, _ptr(out), ctypes.byref(n)))
        if torch.cuda.current_stream(self.device) != self.stream:
            self.synchronize()
        return out[:n.value].tolist()

    def boundary_f(self, logits, masks, radius=None, ignore=None, combined=False):
        """`boundary_f` (or with `combined` `cross_entropy_and_boundary_f`) of device tensors (B, H, W) or (H, W) of any frame
        size that fits the engine's scratch (`eosvos_boundary_f`); `radius` None: that shape's default.  Returns (loss,
        dL/dlogits of the logits' shape); the engine's own gradient is untouched."""
        logits, masks = logits.contiguous(), masks.contiguous()
        assert logits.is_cuda and masks.is_cuda and logits.dtype == masks.dtype == torch.float32 and logits.shape == masks.shape
        assert logits.dim() in (2, 3)
        b = logits.shape[0] if logits.dim() == 3 else 1
        h, w = logits.shape[-2:]
        v = None if ignore is None else check_ignore(ignore)
        out, grad = torch.empty(1, device=self.device), torch.empty_like(logits)
        _ffi.check(self.lib.eosvos_boundary_f(self.h, _ptr(logits), _ptr(masks), b, h, w,
                                              0 if radius is None else boundary.check_radius(radius), int(bool(combined)),
                                              int(v is not None), v or 0.0, _ptr(out), _ptr(grad)))
        return out, grad

    def _frame_args(self, maps, keyword, value, ignore):
        """(images, H, W, the family's knob as the library takes it (0: the shape's default), the void label as a ctypes pointer
        or None) of (B, H, W) / (H, W)."""
        assert maps.is_cuda and maps.dtype == torch.float32 and maps.is_contiguous() and maps.dim() in (2, 3)
        v = None if ignore is None else ctypes.byref(ctypes.c_float(check_ignore(ignore)))
        return (maps.shape[0] if maps.dim() == 3 else 1, *maps.shape[-2:], 0 if value is None else BY_KEYWORD[keyword].check(value), v)

    def surface_loss(self, logits, masks, cap=None, ignore=None):
        """`surface` of device tensors (B, H, W) or (H, W) of any frame size up to 4096 a side (`eosvos_surface_loss`); `cap`
        None: that shape's default `surface.default_cap(H, W)`.  Returns (loss, dL/dlogits of the logits' shape); the
        engine's own gradient is untouched."""
        self._check_stream()
        logits, masks = logits.contiguous(), masks.contiguous()
        assert logits.is_cuda and logits.dtype == torch.float32 and logits.shape == masks.shape
        b, h, w, cap, v = self._frame_args(masks, 'cap', cap, ignore)
        out, grad = torch.empty(1, device=self.device), torch.empty_like(logits)
        _ffi.check(self.lib.eosvos_surface_loss(self.h, _ptr(logits), _ptr(masks), b, h, w, cap, v, _ptr(out), _ptr(grad)))
        return out, grad

    def surface_weights(self, masks, cap=None, ignore=None):
        """(c, w) of rules 1 and 2 of `surface.py` for device targets (B, H, W) or (H, W) (`eosvos_surface_weights`): the capped
        squared distances to the other class as int32 and the weights as float32, of the targets' shape."""
        self._check_stream()
        masks = masks.contiguous()
        b, h, w, cap, v = self._frame_args(masks, 'cap', cap, ignore)
        c, wt = torch.empty(masks.shape, dtype=torch.int32, device=self.device), torch.empty_like(masks)
        _ffi.check(self.lib.eosvos_surface_weights(self.h, _ptr(masks), b, h, w, cap, v, _ptr(c), _ptr(wt)))
        return c, wt

    def cldice_loss(self, logits, masks, depth=None, ignore=None):
        """`cldice` of device tensors (B, H, W) or (H, W) of any frame size up to 4096 a side (`eosvos_cldice_loss`); `depth`
        None: that shape's default `cldice.default_depth(H, W)` (untuned).  Returns (loss, dL/dlogits of the logits' shape);
        the engine's own gradient is untouched."""
        self._check_stream()
        logits, masks = logits.contiguous(), masks.contiguous()
        assert logits.is_cuda and logits.dtype == torch.float32 and logits.shape == masks.shape
        b, h, w, depth, v = self._frame_args(masks, 'depth', depth, ignore)
        out, grad = torch.empty(1, device=self.device), torch.empty_like(logits)
        _ffi.check(self.lib.eosvos_cldice_loss(self.h, _ptr(logits), _ptr(masks), b, h, w, depth, v, _ptr(out), _ptr(grad)))
        return out, grad

    def soft_skeleton(self, maps, depth, ignore=None, masks=None):
        """The soft skeleton S (rules 1 and 2 of `cldice.py`) of device maps in [0, 1], (B, H, W) or (H, W)
        (`eosvos_soft_skeleton`), of the maps' shape: 0 at void pixels, which are where `masks` (None: the maps themselves)
        equal `ignore`.  The debugging and visualisation view of the selection chain."""
        self._check_stream()
        maps = maps.contiguous()
        b, h, w, depth, v = self._frame_args(maps, 'depth', depth, ignore)
        if masks is not None:
            masks = masks.contiguous()
            assert masks.is_cuda and masks.dtype == torch.float32 and masks.shape == maps.shape
        out = torch.empty_like(maps)
        _ffi.check(self.lib.eosvos_soft_skeleton(self.h, _ptr(maps), None if masks is None else _ptr(masks), b, h, w, depth, v,
                                                 _ptr(out)))
        return out

    def potts_loss(self, logits, frames, window=None, dilation=None, sigma_xy=None, sigma_rgb=None):
        """`potts` of device logits (B, H, W) or (H, W) against their frames (B, 3, H, W) or (3, H, W), any frame size up to
        4096 a side (`eosvos_potts_loss`).  None: the defaults of `potts.py` (3, 2, window * dilation, 0.1; untuned), not the
        engine's own settings.  Returns (loss, dL/dlogits of the logits' shape); the engine's own gradient is untouched."""
        self._check_stream()
        logits, frames = logits.contiguous(), frames.contiguous()
        assert logits.is_cuda and frames.is_cuda and logits.dtype == frames.dtype == torch.float32 and logits.dim() in (2, 3)
        b = logits.shape[0] if logits.dim() == 3 else 1
        h, w = logits.shape[-2:]
        assert frames.numel() == 3 * logits.numel() and tuple(frames.shape[-3:]) == (3, h, w)
        r, d = potts.check_window(potts.DEFAULT_WINDOW if window is None else window,
                                  potts.DEFAULT_DILATION if dilation is None else dilation)
        sxy = 0.0 if sigma_xy is None else potts.check_sigma('sigma_xy', sigma_xy)
        srgb = 0.0 if sigma_rgb is None else potts.check_sigma('sigma_rgb', sigma_rgb)
        out, grad = torch.empty(1, device=self.device), torch.empty_like(logits)
        _ffi.check(self.lib.eosvos_potts_loss(self.h, _ptr(logits), _ptr(frames), b, h, w, r, d, sxy, srgb, _ptr(out), _ptr(grad)))
        return out, grad

    def loss_of_framed(self, name, logits, masks, frames, ignore=None):
        """`loss_of` for callers that hold the frames of their logits (`run_frames`' per-frame metric): a spelling without a
        `potts` term goes to `loss_of` as it is.  With one, every other term is `loss_of`'s, the `potts` term is `potts_loss`
        on `frames` (N, 3, H, W) with the engine's window and sigmas (a suffix sets them first, as everywhere), and the values
        are combined by the sum's rule (`loss_sum.py`: fp32 products and sums, in spelled order)."""
        terms = loss_sum.parse(name)
        if not any(potts.parse(t)[0] in potts.KINDS for _, t in terms):
            return self.loss_of(name, logits, masks, ignore=ignore)
        self._loss_spec(name)
        q = {k: (v or None) for k, v in (getattr(self, '_potts', None) or {}).items()}
        acc = None
        for w, t in terms:
            if potts.parse(t)[0] in potts.KINDS:
                v = self.potts_loss(logits.reshape(-1, *frames.shape[-2:]), frames, **q)[0]
            else:
                v = self.loss_of(t, logits, masks, ignore=ignore)
            v = v * torch.tensor(w, dtype=torch.float32, device=v.device)
            acc = v if acc is None else acc + v
        return acc

    def propagation_targets(self, probs, lo, hi, ignore, counts=True):
        """Pseudo-label targets of online adaptation with an uncertainty band (`eosvos_propagation_targets`): probs (F, ...)
        device fp32 -> (targets of the same shape: 1 where p >= hi, 0 where p < lo, `ignore` between; the number of 1s per frame
        as a list of ints after ONE host read, or None with counts=False)."""
        self._check_stream()
        probs = probs.contiguous()
        assert probs.is_cuda and probs.dtype == torch.float32 and probs.dim() >= 2
        if not 0.0 <= lo < hi <= 1.0:
            raise ValueError(f'propagation_targets: needs 0 <= lo < hi <= 1, got {lo!r}, {hi!r}')
        f = probs.shape[0]
        out = torch.empty_like(probs)
        n_pos = (ctypes.c_int64 * f)() if counts else None
        _ffi.check(self.lib.eosvos_propagation_targets(self.h, _ptr(probs), f, probs[0].numel(), lo, hi, check_ignore(ignore),
                                                       _ptr(out), n_pos))
        return out, ([int(v) for v in n_pos] if counts else None)

    def _check_maps(self, who, t, name):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == self.device and t.dtype == torch.float32):
            raise ValueError(f'{who}: {name} must be an fp32 tensor on {self.device}')
        if t.dim() == 4 and t.shape[1] == 1:
            t = t[:, 0]
        if t.dim() != 3 or t.shape[0] < 1 or min(t.shape[1:]) < 1 or max(t.shape[1:]) > 4096:
            raise ValueError(f'{who}: {name} must be (N, 1, H, W) or (N, H, W) with 1 <= H, W <= 4096, got {tuple(t.shape)}')
        return t.contiguous()

    def distance_sq(self, probs, threshold, invert=False, limit=4095):
        """Capped squared Euclidean distance to the nearest seed (`eosvos_distance_sq`, rule 1 of `adapt.py`): probs (N, 1, H, W)
        or (N, H, W) fp32 on the engine's device, any H, W <= 4096; seeds = {probs >= threshold}, or its complement with
        `invert`.  Returns min(D^2, limit^2 + 1) as int32 of the shape of `probs`.  Nothing waits for the GPU."""
        from . import adapt
        limit = adapt._check_limit('distance_sq', limit)
        if threshold != threshold:
            raise ValueError('distance_sq: the threshold is NaN')
        maps = self._check_maps('distance_sq', probs, 'probs')
        self._check_stream()
        n, h, w = maps.shape
        out = torch.empty(n, h, w, dtype=torch.int32, device=self.device)
        for f, g in _chunks(n, adapt.frames_per_call(h, w)):
            _ffi.check(self.lib.eosvos_distance_sq(self.h, _ptr(maps[f:g]), g - f, h, w, threshold, int(bool(invert)), limit,
                                                   _ptr(out[f:g])))
        return out.view(probs.shape)

    def adapt_targets(self, probs, anchors, lo, hi, params, ignore, counts=True):
        """Distance-gated pseudo-label targets of online adaptation (`eosvos_adapt_targets`, rules 2-6 of `adapt.py`): probs and
        anchors (F, 1, H, W) or (F, H, W) fp32 -- frame i's own probabilities and those of the frame before it -- -> (targets
        of the shape of `probs`: the band's rule with 0 wherever the pixel is farther than `neg_dist` from the eroded anchor
        {anchors >= hi}; the number of 1s per frame as a list of ints after ONE host read per chunk of frames under
        `adapt.SCRATCH_CAP`, or None with counts=False)."""
        from . import adapt
        p = adapt.check(params)
        if not p['neg_dist']:
            raise ValueError('adapt_targets: neg_dist=0 means "off" for the distance gate; pass a value in [1, 4095]')
        if not 0.0 <= lo < hi <= 1.0:
            raise ValueError(f'adapt_targets: needs 0 <= lo < hi <= 1, got {lo!r}, {hi!r}')
        x, a = self._check_maps('adapt_targets', probs, 'probs'), self._check_maps('adapt_targets', anchors, 'anchors')
        if x.shape != a.shape:
            raise ValueError(f'adapt_targets: probs {tuple(x.shape)} and anchors {tuple(a.shape)} must share one shape')
        ignore = check_ignore(ignore)
        self._check_stream()
        n, h, w = x.shape
        out = torch.empty_like(x)
        n_pos = []
        for f, g in _chunks(n, adapt.frames_per_call(h, w, p['erode'])):
            host = (ctypes.c_int64 * (g - f))() if counts else None
            _ffi.check(self.lib.eosvos_adapt_targets(self.h, _ptr(x[f:g]), _ptr(a[f:g]), g - f, h, w, lo, hi, hi, p['erode'],
                                                     p['neg_dist'], ignore, _ptr(out[f:g]), host))
            if counts:
                n_pos.extend(int(v) for v in host)
        return out.view(probs.shape), (n_pos if counts else None)

    def bce(self, logits, masks):
        """Mean BCE-with-logits of arbitrary device tensors (no gradient kept)."""
        logits, masks = logits.contiguous(), masks.contiguous()
        loss = torch.empty(1, device=self.device)
        _ffi.check(self.lib.eosvos_bce(self.h, _ptr(logits), _ptr(masks), logits.numel(), _ptr(loss), None))
        return loss

    def backward_step(self, accumulate=False):
        self._check_stream()
        if getattr(self, '_step_check_pending', False):
            # deferred step half of the range guard (callers that go forward -> loss -> backward_step): one step per split mode
            # from the current weights, then the forward + loss of THIS step again in the mode that stays
            x, m, kind = getattr(self, '_chk_images', None), getattr(self, '_chk_masks', None), getattr(self, '_chk_kind', None)
            ign = getattr(self, '_chk_ignore', None)      # the check repeats the caller's loss, void label included
            self._step_check_pending = False
            self._chk_images = self._chk_masks = None
            if not accumulate and x is not None and m is not None and m.shape[0] == x.shape[0] and _guard_enabled():
                self._verify_step(x, m, kind, ign)
                _ffi.check(self.lib.eosvos_forward(self.h, _ptr(x), x.shape[0], None))
                self._loss_on_forward(self._loss_spec(kind), m, ign, None)
        _ffi.check(self.lib.eosvos_backward_step(self.h, int(accumulate)))
        self.steps_since_reset += 1

    def finetune_step(self, images, masks, accumulate=False, sync_loss=True):
        b = self._check_images(images)
        assert masks.is_cuda and masks.is_contiguous() and masks.shape[0] == b
        self._guard(images, None if accumulate else masks)      # (a meta task's accumulating steps: the forward half only)
        self._step_check_pending = False
        self.steps_since_reset += 1
        if sync_loss:
            l = ctypes.c_float()
            _ffi.check(self.lib.eosvos_finetune_step(self.h, _ptr(images), _ptr(masks), b, int(accumulate),
                                                     ctypes.byref(l)))
            return l.value
        _ffi.check(self.lib.eosvos_finetune_step(self.h, _ptr(images), _ptr(masks), b, int(accumulate), None))
        return None

    def last_loss(self):
        """Loss of the last forward + loss (a `finetune_step` included) as a 1-element device tensor."""
        out = torch.empty(1, device=self.device)
        _ffi.check(self.lib.eosvos_last_loss(self.h, _ptr(out)))
        if torch.cuda.current_stream(self.device) != self.stream:
            self.synchronize()
        return out

    def keep_grads(self, on=True):
        _ffi.check(self.lib.eosvos_keep_grads(self.h, int(on)))

    def get_grads(self):
        out = torch.empty(self.n_param, device=self.device)
        _ffi.check(self.lib.eosvos_get_grads(self.h, _ptr(out)))
        if torch.cuda.current_stream(self.device) != self.stream:
            self.synchronize()
        return out

    def debug_gsum(self):
        """`eosvos_debug_gsum`: copy of the gradient sum of the accumulating steps since `meta_task_begin`, flat OIHW as
        `get_grads` (per-link tests)."""
        out = torch.empty(self.n_param, device=self.device)
        _ffi.check(self.lib.eosvos_debug_gsum(self.h, _ptr(out)))
        if torch.cuda.current_stream(self.device) != self.stream:
            self.synchronize()
        return out

    def infer(self, images):
        b = self._check_images(images)
        self._guard(images)
        out = torch.empty(b, 1, self.height, self.width, device=self.device)
        _ffi.check(self.lib.eosvos_infer(self.h, _ptr(images), b, _ptr(out)))
        return out

    # ---- test-time augmentation (mirrored / rescaled views, see tta.py) ------------------------
    def infer_view(self, images, mirror=False):
        """`eosvos_infer_view`: the inference forward of `infer` on the frames as they are or mirrored left-right (the layout
        pass flips them on the way in); the logits stay in the engine for `tta_accumulate`."""
        b = self._check_images(images)
        self._guard(images)
        _ffi.check(self.lib.eosvos_infer_view(self.h, _ptr(images), b, int(bool(mirror))))
        return b

    def tta_accumulate(self, acc, weight, mirror=False, first=False):
        """`eosvos_tta_accumulate`: acc (B, 1, H, W) (+)= weight * sigmoid(bilinear_{align_corners=False}(un-mirrored logits of
        this engine's last forward)), one launch; `first` stores instead of adding.  Returns acc."""
        self._check_stream()
        assert acc.is_cuda and acc.dtype == torch.float32 and acc.is_contiguous() and acc.dim() == 4 and acc.shape[1] == 1, acc.shape
        _ffi.check(self.lib.eosvos_tta_accumulate(self.h, self.height, self.width, acc.shape[0], int(bool(mirror)), float(weight),
                                                  int(bool(first)), _ptr(acc), acc.shape[2], acc.shape[3]))
        return acc

    def resize_frames(self, frames, height, width):
        """`eosvos_resize_frames`: (B, C, h, w) device fp32 -> (B, C, height, width), bilinear with align_corners=False."""
        self._check_stream()
        assert frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous() and frames.dim() == 4, frames.shape
        b, c, h, w = frames.shape
        out = torch.empty(b, c, int(height), int(width), device=self.device)
        _ffi.check(self.lib.eosvos_resize_frames(self.h, _ptr(frames), b, c, h, w, int(height), int(width), _ptr(out)))
        return out

    # ---- object-centred zoom pass (a second look at a crop around the object, see zoom.py) -----
    def _check_zoom(self, who, t, name, dtype=torch.float32, shape=None):
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f'{who}: {name} must be a contiguous {dtype} tensor on {self.device}')
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f'{who}: {name} must be {tuple(shape)}, got {tuple(t.shape)}')

    def zoom_boxes(self, probs, params):
        """`eosvos_zoom_boxes` (`zoom.py`, rules 1-5): first-pass probabilities (N, 1, H, W) or (N, H, W) fp32 on the engine's
        device, any H, W <= 4096 -> boxes (N, 5) int32 on the device: valid, y0, x0, bh, bw.  Nothing waits for the GPU."""
        from . import zoom
        p = zoom.check(params)
        if p['max_zoom'] == 0:
            raise ValueError('zoom_boxes: max_zoom=0 means "off" for the zoom pass; pass a number in [1, 4]')
        self._check_zoom('zoom_boxes', probs, 'probs')
        if probs.dim() == 4 and probs.shape[1] == 1:
            probs = probs[:, 0]
        if probs.dim() != 3 or probs.shape[0] < 1 or min(probs.shape[1:]) < 1 or max(probs.shape[1:]) > zoom.MAX_SIDE:
            raise ValueError(f'zoom_boxes: probs must be (N, 1, H, W) or (N, H, W) with 1 <= H, W <= {zoom.MAX_SIDE}, got '
                             f'{tuple(probs.shape)}')
        self._check_stream()
        n, h, w = probs.shape
        boxes = torch.empty(n, 5, dtype=torch.int32, device=self.device)
        _ffi.check(self.lib.eosvos_zoom_boxes(self.h, _ptr(probs), n, h, w, p['threshold'], p['min_pixels'], zoom.q16(p['margin']),
                                              p['margin_px'], zoom.q16(p['min_zoom']), zoom.q16(p['max_zoom']), _ptr(boxes)))
        return boxes

    def zoom_crop(self, frames, boxes, out=None):
        """`eosvos_zoom_crop` (`zoom.py`, rule 6): frames (B, C, H, W) fp32 cut to their boxes (B, 5) int32 and magnified to
        H x W; an invalid frame is copied.  Returns `out` (a new tensor without it)."""
        self._check_zoom('zoom_crop', frames, 'frames')
        if frames.dim() != 4:
            raise ValueError(f'zoom_crop: frames must be (B, C, H, W), got {tuple(frames.shape)}')
        self._check_zoom('zoom_crop', boxes, 'boxes', torch.int32, (frames.shape[0], 5))
        out = torch.empty_like(frames) if out is None else out
        self._check_zoom('zoom_crop', out, 'out', shape=frames.shape)
        self._check_stream()
        b, c, h, w = frames.shape
        _ffi.check(self.lib.eosvos_zoom_crop(self.h, _ptr(frames), _ptr(boxes), b, c, h, w, _ptr(out)))
        return out

    def zoom_accumulate(self, boxes, pz, view_weight, mirror=False, first=False):
        """`eosvos_zoom_accumulate` (`zoom.py`, rule 8): pz (B, 1, H, W) inside each valid box (+)= view_weight *
        sigmoid(bilinear(un-mirrored logits of this engine's last forward -> bh x bw)); `first` stores instead of adding.
        Everything outside the boxes keeps its bits.  Returns pz."""
        self._check_zoom('zoom_accumulate', pz, 'pz')
        if pz.dim() != 4 or tuple(pz.shape[1:]) != (1, self.height, self.width) or not 1 <= pz.shape[0] <= self.max_batch:
            raise ValueError(f'zoom_accumulate: pz must be (B <= {self.max_batch}, 1, {self.height}, {self.width}), got '
                             f'{tuple(pz.shape)}')
        self._check_zoom('zoom_accumulate', boxes, 'boxes', torch.int32, (pz.shape[0], 5))
        self._check_stream()
        _ffi.check(self.lib.eosvos_zoom_accumulate(self.h, _ptr(boxes), pz.shape[0], int(bool(mirror)), float(view_weight),
                                                   int(bool(first)), _ptr(pz)))
        return pz

    def zoom_blend(self, boxes, pz, probs, weight, feather):
        """`eosvos_zoom_blend` (`zoom.py`, rule 9): probs (B, 1, H, W) = probs + (weight * ramp) * (pz - probs) inside valid
        boxes, IN PLACE; invalid frames and pixels outside the boxes are not written.  Returns probs."""
        self._check_zoom('zoom_blend', probs, 'probs')
        if probs.dim() != 4 or probs.shape[1] != 1:
            raise ValueError(f'zoom_blend: probs must be (B, 1, H, W), got {tuple(probs.shape)}')
        self._check_zoom('zoom_blend', pz, 'pz', shape=probs.shape)
        self._check_zoom('zoom_blend', boxes, 'boxes', torch.int32, (probs.shape[0], 5))
        self._check_stream()
        b, _, h, w = probs.shape
        _ffi.check(self.lib.eosvos_zoom_blend(self.h, _ptr(boxes), b, h, w, float(weight), int(feather), _ptr(pz), _ptr(probs)))
        return probs

    # ---- lucid first-frame synthesis (object and background moved independently, see lucid.py) -----
    def lucid_plate(self, frame, mask, dilate):
        """`eosvos_lucid_plate` (`lucid.py`, rules 1-5): frame (C, H, W) and mask (1, H, W) or (H, W), fp32 on the engine's
        device, any H, W <= 4096 -> the plate (C, H, W): the frame with the mask (grown by `dilate`) filled from the push-pull
        pyramid.  Nothing waits for the GPU."""
        from . import lucid
        if isinstance(dilate, bool) or not isinstance(dilate, int) or not 0 <= dilate <= lucid.MAX_DILATE:
            raise ValueError(f'lucid_plate: dilate={dilate!r}: an integer in [0, {lucid.MAX_DILATE}]')
        c, h, w = self._check_lucid('lucid_plate', frame, mask)
        self._check_stream()
        plate = torch.empty_like(frame)
        _ffi.check(self.lib.eosvos_lucid_plate(self.h, _ptr(frame), _ptr(mask), c, h, w, dilate, _ptr(plate)))
        return plate

    def _check_lucid(self, who, frame, mask, plate=None):
        from . import lucid
        self._check_zoom(who, frame, 'frame')
        if frame.dim() != 3 or frame.shape[0] < 1 or min(frame.shape[1:]) < 1 or max(frame.shape[1:]) > lucid.MAX_SIDE:
            raise ValueError(f'{who}: frame must be (C, H, W) with 1 <= H, W <= {lucid.MAX_SIDE}, got {tuple(frame.shape)}')
        self._check_zoom(who, mask, 'mask')
        if tuple(mask.shape) not in ((1, *frame.shape[1:]), tuple(frame.shape[1:])):
            raise ValueError(f'{who}: mask must be (1, H, W) or (H, W) of the frame\'s size, got {tuple(mask.shape)}')
        if plate is not None:
            self._check_zoom(who, plate, 'plate', shape=frame.shape)
        return tuple(int(v) for v in frame.shape)

    def lucid_compose(self, frame, mask, plate, params, read_counts=True):
        """`eosvos_lucid_compose` (`lucid.py`, rules 6-9): ONE launch for the samples params = [{'flip', 'Bi', 'Oi'}] (at most
        16; the matrices are the inverse ones, 6 doubles each) -> (images (S, C, H, W), labels (S, 1, H, W) of 0 / 1, counts:
        a list of S ints after one host read, or None without `read_counts`, when nothing waits for the GPU)."""
        from . import lucid
        c, h, w = self._check_lucid('lucid_compose', frame, mask, plate)
        n = len(params)
        if not 1 <= n <= lucid.MAX_SAMPLES_PER_LAUNCH:
            raise ValueError(f'lucid_compose: between 1 and {lucid.MAX_SAMPLES_PER_LAUNCH} samples per call, got {n}')
        flips = (ctypes.c_int32 * n)(*[int(bool(p['flip'])) for p in params])
        mats = (ctypes.c_double * (12 * n))(*[float(v) for p in params for v in tuple(p['Bi']) + tuple(p['Oi'])])
        if len(mats) != 12 * n:
            raise ValueError('lucid_compose: every sample needs two matrices of 6 numbers')
        self._check_stream()
        images = torch.empty(n, c, h, w, device=self.device)
        labels = torch.empty(n, 1, h, w, device=self.device)
        counts = (ctypes.c_int32 * n)() if read_counts else None
        _ffi.check(self.lib.eosvos_lucid_compose(self.h, _ptr(frame), _ptr(mask), _ptr(plate), c, h, w, n, flips, mats, _ptr(images),
                                                 _ptr(labels), counts))
        return images, labels, (list(counts) if read_counts else None)

    def lucid_compose_layers(self, frame, ids, plate, samples, target_id=1, read_counts=True, want_ids=False):
        """`eosvos_lucid_compose_layers` (`lucid_layers.py`, rules L2-L5): ONE launch for the samples = [{'flip', 'Bi', 'layers':
        [(id, Oi), ...] back to front}] (at most 8 samples of at most 8 layers; the matrices are the inverse ones, 6 doubles
        each) over the id map `ids` (H, W) uint8 -> (images (S, C, H, W), labels (S, 1, H, W): 1 where the visible layer carries
        `target_id`, counts: per sample the list of its layers' visible pixel counts after one host read, or None without
        `read_counts`, when nothing waits for the GPU; ids_out (S, H, W) uint8 with `want_ids`, else None)."""
        from . import lucid_layers as ll
        self._check_zoom('lucid_compose_layers', frame, 'frame')
        if frame.dim() != 3 or frame.shape[0] < 1 or min(frame.shape[1:]) < 1 or max(frame.shape[1:]) > ll.MAX_SIDE:
            raise ValueError(f'lucid_compose_layers: frame must be (C, H, W) with 1 <= H, W <= {ll.MAX_SIDE}, got {tuple(frame.shape)}')
        self._check_zoom('lucid_compose_layers', ids, 'ids', torch.uint8, frame.shape[1:])
        self._check_zoom('lucid_compose_layers', plate, 'plate', shape=frame.shape)
        c, h, w = (int(v) for v in frame.shape)
        n = len(samples)
        if not 1 <= n <= ll.MAX_SAMPLES_PER_LAUNCH:
            raise ValueError(f'lucid_compose_layers: between 1 and {ll.MAX_SAMPLES_PER_LAUNCH} samples per call, got {n}')
        if isinstance(target_id, bool) or not isinstance(target_id, int) or not 1 <= target_id <= 255:
            raise ValueError(f'lucid_compose_layers: target_id={target_id!r}: an integer in [1, 255]')
        flips = (ctypes.c_int32 * n)(*[int(bool(p['flip'])) for p in samples])
        n_layers = (ctypes.c_int32 * n)(*[len(p['layers']) for p in samples])
        layer_ids = (ctypes.c_uint8 * (ll.MAX_LAYERS * n))()
        mats = (ctypes.c_double * (6 * (1 + ll.MAX_LAYERS) * n))()
        for s, p in enumerate(samples):
            layers = list(p['layers'])
            if not 1 <= len(layers) <= ll.MAX_LAYERS:
                raise ValueError(f'lucid_compose_layers: between 1 and {ll.MAX_LAYERS} layers per sample, got {len(layers)}')
            rows = [tuple(p['Bi'])] + [tuple(oi) for _, oi in layers]
            if any(len(r) != 6 for r in rows):
                raise ValueError('lucid_compose_layers: every matrix has 6 numbers')
            for k, (i, _) in enumerate(layers):
                if isinstance(i, bool) or not isinstance(i, int) or not 1 <= i <= 255:
                    raise ValueError(f'lucid_compose_layers: layer id {i!r}: an integer in [1, 255]')
                layer_ids[s * ll.MAX_LAYERS + k] = i
            for k, r in enumerate(rows):
                for j, v in enumerate(r):
                    mats[(s * (1 + ll.MAX_LAYERS) + k) * 6 + j] = float(v)
        self._check_stream()
        images = torch.empty(n, c, h, w, device=self.device)
        labels = torch.empty(n, 1, h, w, device=self.device)
        ids_out = torch.empty(n, h, w, dtype=torch.uint8, device=self.device) if want_ids else None
        counts = (ctypes.c_int32 * (ll.MAX_LAYERS * n))() if read_counts else None
        _ffi.check(self.lib.eosvos_lucid_compose_layers(self.h, _ptr(frame), _ptr(ids), _ptr(plate), c, h, w, n, flips, n_layers,
                                                        layer_ids, mats, target_id, _ptr(images), _ptr(labels), _optr(ids_out),
                                                        counts))
        per_sample = [list(counts[s * ll.MAX_LAYERS:s * ll.MAX_LAYERS + n_layers[s]]) for s in range(n)] if read_counts else None
        return images, labels, per_sample, ids_out

    def merge_labels(self, probs):
        """probs: (n_obj, H, W) device fp32 -> (H, W) uint8.  `evaluate.py:322-326`."""
        probs = probs.contiguous()
        n_obj = probs.shape[0]
        n_pix = probs[0].numel()
        out = torch.empty(probs.shape[1:], dtype=torch.uint8, device=self.device)
        _ffi.check(self.lib.eosvos_merge_labels(self.h, _ptr(probs), n_obj, n_pix, _ptr(out)))
        return out

    def davis_counts(self, pred, gt, n_obj, bound_th=0.008):
        """DAVIS J / F counts of label maps (`eosvos_davis_counts`; evaluate.py:345-359, helper_func.py:444-458).
        pred, gt: (N, H, W) uint8 tensors on the engine's device, any H and W (W <= 4096).  Returns an (N, n_obj, 6) int64
        numpy array: inter, union, n_fg, n_gt, fg_match, gt_match per frame and object (`data.measures_from_counts`)."""
        import numpy as np
        from .data import davis_bound_pix
        if pred.dtype != torch.uint8 or gt.dtype != torch.uint8 or pred.dim() != 3 or pred.shape != gt.shape:
            raise ValueError('davis_counts: pred and gt must be (N, H, W) uint8 tensors of one shape')
        if pred.device != self.device or gt.device != self.device:
            raise ValueError(f'davis_counts: the label maps must be on {self.device}')
        n, h, w = pred.shape
        pred, gt = pred.contiguous(), gt.contiguous()
        counts = np.empty((n, n_obj, 6), dtype=np.int64)
        _ffi.check(self.lib.eosvos_davis_counts(self.h, _ptr(pred), _ptr(gt), n, h, w, n_obj, davis_bound_pix(bound_th, h, w),
                                                counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return counts

    def crf_labels(self, images, probs, iterations=5, radius=5, dilation=2, w_appearance=10.0, w_smooth=3.0, theta_alpha=8.0,
                   theta_beta=0.05, theta_gamma=3.0, return_q=False):
        """Local dense-CRF refinement of the merge (`eosvos_crf_labels`; beside evaluate.py:322-326, the model: `crf.py`).
        images (N, 3, H, W), probs (N, n_obj, H, W): device fp32 of any H and W -> label maps (N, H, W) uint8, with `return_q`
        also Q^T (N, n_obj + 1, H, W).  iterations = 0 is `merge_labels`.  Nothing waits for the GPU; the frames go through in
        chunks that keep the engine's scratch under `crf.SCRATCH_CAP`."""
        from . import crf
        p = crf.check(dict(iterations=iterations, radius=radius, dilation=dilation, w_appearance=w_appearance, w_smooth=w_smooth,
                           theta_alpha=theta_alpha, theta_beta=theta_beta, theta_gamma=theta_gamma))
        crf._check_tensors(images, probs)
        self._check_stream()
        for t in (images, probs):
            if t.device != self.device or t.dtype != torch.float32:
                raise ValueError(f'crf_labels: images and probs must be fp32 tensors on {self.device}')
        images, probs = images.contiguous(), probs.contiguous()
        n, n_obj, h, w = probs.shape
        out = torch.empty(n, h, w, dtype=torch.uint8, device=self.device)
        q = torch.empty(n, n_obj + 1, h, w, device=self.device) if return_q else None
        for f, g in _chunks(n, crf.frames_per_call(n_obj, h, w)):
            _ffi.check(self.lib.eosvos_crf_labels(self.h, _ptr(images[f:g]), _ptr(probs[f:g]), g - f, n_obj, h, w, p['iterations'],
                                                  p['radius'], p['dilation'], p['w_appearance'], p['w_smooth'], p['theta_alpha'],
                                                  p['theta_beta'], p['theta_gamma'], _ptr(out[f:g]), _optr(q[f:g] if return_q else None)))
        return (out, q) if return_q else out

    def _check_label_maps(self, who, labels, prev=None):
        from . import components
        components._check_maps(who, labels, prev)
        for t in (labels, prev):
            if t is not None and (not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.uint8):
                raise ValueError(f'{who}: the label maps must be uint8 tensors on {self.device}')

    def label_components(self, labels, connectivity=8):
        """Component ids of label maps (`eosvos_label_components`; the rules: `components.py`).  labels (N, H, W) uint8 on the
        engine's device, any H and W within the limits -> (N, H, W) int32: 1 + the smallest y * W + x of the pixel's component,
        0 on background.  Nothing waits for the GPU; the frames go through in chunks under `components.SCRATCH_CAP`."""
        from . import components
        if connectivity not in (4, 8):
            raise ValueError(f'label_components: connectivity={connectivity!r}: 4 or 8')
        self._check_label_maps('label_components', labels)
        self._check_stream()
        labels = labels.contiguous()
        n, h, w = labels.shape
        ids = torch.empty(n, h, w, dtype=torch.int32, device=self.device)
        for f, g in _chunks(n, components.frames_per_call(h, w)):
            _ffi.check(self.lib.eosvos_label_components(self.h, _ptr(labels[f:g]), g - f, h, w, connectivity, _ptr(ids[f:g])))
        return ids

    def filter_components(self, labels, connectivity=8, min_area=0, min_rel_area=0.0, largest_only=False, gate=0, prev=None,
                          keep=(), return_removed=False):
        """The component filter of `components.py` (`eosvos_filter_components`).  labels (N, H, W) uint8 on the engine's
        device in frame order, prev (H, W) uint8 or None, keep: frame indices copied unchanged -> filtered maps (N, H, W) uint8;
        with `return_removed` also the pixels zeroed per frame as an (N,) int64 numpy array (this waits for the GPU).  The frames
        go through in chunks under `components.SCRATCH_CAP`; a chunk's last filtered frame is the `prev` of the next."""
        import numpy as np
        from . import components
        p = components.check(dict(connectivity=connectivity, min_area=min_area, min_rel_area=min_rel_area,
                                  largest_only=largest_only, gate=gate))
        self._check_label_maps('filter_components', labels, prev)
        self._check_stream()
        labels = labels.contiguous()
        n, h, w = labels.shape
        flags = _keep_flags(keep, n)
        out = torch.empty_like(labels)
        removed = np.zeros(n, dtype=np.int64)
        rem_p = ctypes.POINTER(ctypes.c_int64)
        prev = prev.contiguous() if prev is not None else None
        for f, g in _chunks(n, components.frames_per_call(h, w)):
            _ffi.check(self.lib.eosvos_filter_components(
                self.h, _ptr(labels[f:g]), g - f, h, w, p['connectivity'], p['min_area'], components.rel_q16(p['min_rel_area']),
                int(p['largest_only']), p['gate'], _optr(prev), bytes(flags[f:g]), _ptr(out[f:g]),
                removed[f:g].ctypes.data_as(rem_p) if return_removed else None))
            prev = out[g - 1]
        return (out, removed) if return_removed else out

    def fill_holes(self, labels, connectivity=8, max_area=0, max_rel_area=1.0, prev_overlap=0.0, prev=None, keep=(),
                   return_filled=False):
        """The hole filler of `holes.py` (`eosvos_fill_holes`).  labels (N, H, W) uint8 on the engine's device in frame order,
        prev (H, W) uint8 or None, keep: frame indices copied unchanged -> filled maps (N, H, W) uint8; with `return_filled`
        also the pixels filled per frame as an (N,) int64 numpy array (this waits for the GPU).  The frames go through in chunks
        under `holes.SCRATCH_CAP`; a chunk's last filled frame is the `prev` of the next."""
        import numpy as np
        from . import holes
        p = holes.check(dict(connectivity=connectivity, max_area=max_area, max_rel_area=max_rel_area, prev_overlap=prev_overlap))
        self._check_label_maps('fill_holes', labels, prev)
        self._check_stream()
        labels = labels.contiguous()
        n, h, w = labels.shape
        flags = _keep_flags(keep, n)
        out = torch.empty_like(labels)
        filled = np.zeros(n, dtype=np.int64)
        fill_p = ctypes.POINTER(ctypes.c_int64)
        prev = prev.contiguous() if prev is not None else None
        for f, g in _chunks(n, holes.frames_per_call(h, w)):
            _ffi.check(self.lib.eosvos_fill_holes(
                self.h, _ptr(labels[f:g]), g - f, h, w, p['connectivity'], p['max_area'], holes.rel_q16(p['max_rel_area']),
                holes.overlap_q16(p['prev_overlap']), _optr(prev), bytes(flags[f:g]), _ptr(out[f:g]),
                filled[f:g].ctypes.data_as(fill_p) if return_filled else None))
            prev = out[g - 1]
        return (out, filled) if return_filled else out

    def _check_rgb(self, who, rgb, labels=None):
        from . import snap
        for t in (rgb, labels):
            if t is not None and (not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.uint8):
                raise ValueError(f'{who}: rgb and labels must be uint8 tensors on {self.device}')
        snap._check_rgb(who, rgb, labels)

    def superpixels(self, rgb, step=16, iterations=5, compactness=10):
        """Integer SLIC superpixels (`eosvos_superpixels`; the rules: `snap.py`).  rgb (N, 3, H, W) uint8 on the engine's device
        (`snap.quantise` makes it from fp32 frames), any H and W within the limits -> ids (N, H, W) int32, the cluster
        cy * gx + cx of every pixel.  Nothing waits for the GPU; the frames go through in chunks under `snap.SCRATCH_CAP`."""
        from . import snap
        p = snap.check(dict(step=step, iterations=iterations, compactness=compactness))
        if p['step'] == 0:
            raise ValueError('superpixels: step=0 means "off" for the snapping stage; pass a step in [4, 64]')
        self._check_rgb('superpixels', rgb)
        self._check_stream()
        rgb = rgb.contiguous()
        n, _, h, w = rgb.shape
        ids = torch.empty(n, h, w, dtype=torch.int32, device=self.device)
        for f, g in _chunks(n, snap.frames_per_call(0, h, w, p['step'])):
            _ffi.check(self.lib.eosvos_superpixels(self.h, _ptr(rgb[f:g]), g - f, h, w, p['step'], p['iterations'], p['compactness'],
                                                   _ptr(ids[f:g])))
        return ids

    def snap_labels(self, rgb, labels, n_obj=255, step=16, iterations=5, compactness=10, min_share=0.5, keep=(),
                    return_changed=False):
        """The superpixel snapping of `snap.py` (`eosvos_snap_labels`).  rgb (N, 3, H, W) and labels (N, H, W) uint8 on the
        engine's device, n_obj: labels above it neither vote nor change, keep: frame indices copied unchanged -> snapped maps
        (N, H, W) uint8; with `return_changed` also the pixels changed per frame as an (N,) int64 numpy array (this waits for the
        GPU).  step 0 copies.  The frames go through in chunks under `snap.SCRATCH_CAP`."""
        import numpy as np
        from . import snap
        p = snap.check(dict(step=step, iterations=iterations, compactness=compactness, min_share=min_share))
        n_obj = snap._check_n_obj(n_obj)
        self._check_rgb('snap_labels', rgb, labels)
        self._check_stream()
        rgb, labels = rgb.contiguous(), labels.contiguous()
        n, h, w = labels.shape
        changed = np.zeros(n, dtype=np.int64)
        if p['step'] == 0:
            return (labels.clone(), changed) if return_changed else labels.clone()
        flags = _keep_flags(keep, n)
        out = torch.empty_like(labels)
        changed_p = ctypes.POINTER(ctypes.c_int64)
        for f, g in _chunks(n, snap.frames_per_call(n_obj, h, w, p['step'])):
            _ffi.check(self.lib.eosvos_snap_labels(
                self.h, _ptr(rgb[f:g]), _ptr(labels[f:g]), g - f, h, w, n_obj, p['step'], p['iterations'], p['compactness'],
                snap.share_q16(p['min_share']), bytes(flags[f:g]), _ptr(out[f:g]),
                changed[f:g].ctypes.data_as(changed_p) if return_changed else None))
        return (out, changed) if return_changed else out

    def block_motion(self, rgb, block=8, radius=16, bias=2, prev_rgb=None):
        """Block vectors between consecutive frames (`eosvos_block_motion`; the rules: `motion.py`).  rgb (N, 3, H, W) uint8 on the
        engine's device in frame order (`snap.quantise` makes it from fp32 frames), prev_rgb (3, H, W) uint8 or None: the frame
        before the first -> mv (N, by, bx, 2) int8, (dy, dx) per block; without `prev_rgb` the first frame gets zeros.  Nothing
        waits for the GPU; the frames go through in chunks under `motion.SCRATCH_CAP`, a chunk's last frame is the `prev_rgb`
        of the next."""
        from . import motion
        p = motion.check(dict(block=block, radius=radius, bias=bias))
        if p['block'] == 0:
            raise ValueError('block_motion: block=0 means "off" for the motion compensation; pass 8 or 16')
        self._check_rgb('block_motion', rgb, None)
        if prev_rgb is not None and (not isinstance(prev_rgb, torch.Tensor) or prev_rgb.device != self.device or prev_rgb.dtype != torch.uint8):
            raise ValueError(f'block_motion: prev_rgb must be a uint8 tensor on {self.device}')
        motion._check_rgb('block_motion', rgb, prev_rgb)
        self._check_stream()
        rgb = rgb.contiguous()
        n, _, h, w = rgb.shape
        mv = torch.empty((n,) + motion.grid(h, w, p['block']) + (2,), dtype=torch.int8, device=self.device)
        prev = prev_rgb.contiguous() if prev_rgb is not None else None
        for f, g in _chunks(n, motion.frames_per_call(h, w)):
            _ffi.check(self.lib.eosvos_block_motion(self.h, _ptr(rgb[f:g]), _optr(prev), g - f, h, w, p['block'], p['radius'], p['bias'],
                                                    _ptr(mv[f:g])))
            prev = rgb[g - 1]
        return mv

    def warp_labels(self, labels, mv, block):
        """Label maps warped by block vectors (`eosvos_warp_labels`; `motion.py`, rule 7).  labels (N, H, W) uint8 and mv
        (N, by, bx, 2) int8 on the engine's device -> (N, H, W) uint8, out(y, x) = labels(y + dy, x + dx) with the vector of the
        pixel's block; frame n is warped by mv[n].  Nothing waits for the GPU."""
        from . import motion
        self._check_label_maps('warp_labels', labels)
        if not isinstance(mv, torch.Tensor) or mv.device != self.device or mv.dtype != torch.int8:
            raise ValueError(f'warp_labels: mv must be an int8 tensor on {self.device}')
        motion._check_mv('warp_labels', labels, mv, block)
        self._check_stream()
        labels, mv = labels.contiguous(), mv.contiguous()
        n, h, w = labels.shape
        out = torch.empty_like(labels)
        _ffi.check(self.lib.eosvos_warp_labels(self.h, _ptr(labels), _ptr(mv), n, h, w, block, _ptr(out)))
        return out

    # ---- meta-training ----------------------------------------------------------------
    def meta_task_begin(self):
        _ffi.check(self.lib.eosvos_meta_task_begin(self.h))
        self.steps_since_reset, self.in_meta_task, self.has_snapshot = 0, True, False

    def meta_grad(self, images, masks, flat_meta_grad, weight=1.0, init_grad=True, new_segment=False, sync=True):
        """ADDS weight * task meta-gradient into flat_meta_grad ([lr state | init]); returns the meta loss.
        weight / init_grad / new_segment: `multi_step_bptt_loss` and truncated BPTT (include/eosvos.h).
        sync=False: nothing waits for the GPU; returns a device tensor holding the meta loss (concurrent tasks)."""
        b = self._check_images(images)
        assert flat_meta_grad.numel() == self.n_lr_store + self.n_param and flat_meta_grad.is_cuda
        flags = (1 if init_grad else 0) | (2 if new_segment else 0)
        if not sync:
            _ffi.check(self.lib.eosvos_meta_grad_ex(self.h, _ptr(images), _ptr(masks), b, _ptr(flat_meta_grad), None,
                                                    float(weight), flags))
            out = torch.empty(1, device=self.device)
            _ffi.check(self.lib.eosvos_last_loss(self.h, _ptr(out)))
            _touched(flat_meta_grad)
            return out
        l = ctypes.c_float()
        _ffi.check(self.lib.eosvos_meta_grad_ex(self.h, _ptr(images), _ptr(masks), b, _ptr(flat_meta_grad),
                                                ctypes.byref(l), float(weight), flags))
        _touched(flat_meta_grad)
        return l.value

    def radam_step(self, param, grad, exp_avg, exp_avg_sq, lr, weight_decay, step, grad_scale=1.0,
                   grad_clip=0.0, betas=(0.9, 0.999), eps=1e-8):
        _ffi.check(self.lib.eosvos_radam_step(self.h, _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq),
                                              param.numel(), lr, weight_decay, betas[0], betas[1], eps, step,
                                              grad_scale, grad_clip))
        _touched(param, exp_avg, exp_avg_sq)

    def clamp(self, param, lo, hi):
        _ffi.check(self.lib.eosvos_clamp(self.h, _ptr(param), param.numel(), lo, hi))
        _touched(param)

    def outer_step(self, state, grad, exp_avg, exp_avg_sq, n_lr, learn_model_init, step, lr_lr, init_lr, weight_decay,
                   grad_scale=1.0, grad_clip=0.0, lr_lo=0.0, lr_hi=float('inf'), use_log=False, frozen_lr=0, frozen_param=0,
                   betas=(0.9, 0.999), eps=1e-8):
        """`eosvos_outer_step`: scale + clip + RAdam (both parameter groups) + lr clamp + grad zero in one launch that also
        leaves the new learned state in this engine (effective lr, init = current weights).  NEURON level only."""
        self._check_stream()
        for t in (state, grad, exp_avg, exp_avg_sq):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == state.numel()
        assert state.numel() == n_lr + (self.n_param if learn_model_init else 0) and n_lr == self.n_lr
        _ffi.check(self.lib.eosvos_outer_step(self.h, _ptr(state), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), n_lr,
                                              int(bool(learn_model_init)), int(step), lr_lr, init_lr, weight_decay, betas[0], betas[1],
                                              eps, grad_scale, grad_clip, lr_lo, lr_hi, int(bool(use_log)), int(frozen_lr),
                                              int(frozen_param)))
        _touched(state, grad, exp_avg, exp_avg_sq)
        self.lr_level, self.lr_log, self.n_lr_store = 'NEURON', bool(use_log), self.n_lr
        if learn_model_init:
            self.steps_since_reset = 0

    def set_trainable_from(self, conv_idx):
        """`eosvos_set_trainable_from`: convs [0, conv_idx) are frozen (`topology.trainable_from`; 0 trains everything).  Weight
        entries keep the full layout; the frozen part of the meta-gradient / gradients is left untouched / zero."""
        _ffi.check(self.lib.eosvos_set_trainable_from(self.h, int(conv_idx)))
        self.train_from = int(conv_idx)

    def alias_state(self, src):
        """`eosvos_alias_state`: this engine reads `src`'s learned init and per-neuron lr from now on (engines that run the
        tasks of one meta-batch side by side); `src` must stay alive as long as this engine."""
        _ffi.check(self.lib.eosvos_alias_state(self.h, src.h))
        self._alias_of = src              # keeps `src` alive

    def unalias_state(self):
        """`eosvos_unalias_state`: own buffers again, holding the state this engine has been reading."""
        _ffi.check(self.lib.eosvos_unalias_state(self.h))
        self._alias_of = None

    def allreduce_sum(self, flat, comm):
        """`eosvos_allreduce_sum`: in-place all-reduce(sum) of a flat device tensor over the RCCL communicator `comm` (an
        `RcclComm`), asynchronous on this engine's stream -- the exchange step of meta-training for hosts that do not run
        torch.distributed (`src/util/meta_run.py:237-238` + `src/train_meta.py:361-366` in the reference)."""
        self._check_stream()
        assert flat.is_cuda and flat.dtype == torch.float32 and flat.is_contiguous()
        _ffi.check(self.lib.eosvos_allreduce_sum(self.h, _ptr(flat), flat.numel(), comm.handle))
        _touched(flat)

    def synchronize(self):
        _ffi.check(self.lib.eosvos_synchronize(self.h))

    def set_wg_budget(self, workgroups):
        """Workgroups a launch plans for (`eosvos_set_wg_budget`): 0 = the whole chip (an engine alone on the GPU),
        256 for engines that run beside each other.  Returns the budget in effect."""
        r = self.lib.eosvos_set_wg_budget(self.h, int(workgroups))
        if r < 0:
            _ffi.check(1)
        return r

    def set_side_stream(self, on):
        """`eosvos_set_side_stream`: False for engines that run side by side (one queue each); returns the state in effect."""
        r = self.lib.eosvos_set_side_stream(self.h, int(bool(on)))
        if r < 0:
            _ffi.check(1)
        return bool(r)

    def time_hot_kernel(self, batch, reps=20):
        ms, fl = ctypes.c_float(), ctypes.c_double()
        _ffi.check(self.lib.eosvos_time_hot_kernel(self.h, batch, reps, ctypes.byref(ms), ctypes.byref(fl)))
        return ms.value, fl.value

    def bench_conv(self, conv_idx, kind, batch, reps=10):
        """(ms, TFLOP/s) of one layer's fwd (0) / dgrad (1) / wgrad (2) launch."""
        ms, fl = ctypes.c_float(), ctypes.c_double()
        _ffi.check(self.lib.eosvos_bench_conv(self.h, conv_idx, kind, batch, reps, ctypes.byref(ms), ctypes.byref(fl)))
        return ms.value, fl.value / (ms.value * 1e-3) / 1e12

    def profile_launches(self, on=True):
        """HIP events around every matrix-core kernel launch (on its own stream) from now on."""
        _ffi.check(self.lib.eosvos_profile_launches(self.h, int(on)))

    def profile_read(self):
        """{kernel symbol: (launches, total ms, total executed fp32-equivalent FLOPs)} since profile_launches(True)."""
        mx = 32
        names = ctypes.create_string_buffer(64 * mx)
        counts, ms, fl, n = (ctypes.c_int64 * mx)(), (ctypes.c_double * mx)(), (ctypes.c_double * mx)(), ctypes.c_int()
        _ffi.check(self.lib.eosvos_profile_read(self.h, mx, names, counts, ms, fl, ctypes.byref(n)))
        return {names.raw[64 * i:64 * i + 64].split(b'\0')[0].decode(): (int(counts[i]), float(ms[i]), float(fl[i]))
                for i in range(n.value)}

    PLAN_LOG_FIELDS = ('kernel_id', 'kmajor', 'bn', 'tiles', 'ksteps', 'deep', 'dp_q', 'per', 'nwg', 'splitk', 'tprefix', 'torder',
                       'fixup', 'budget')          # include/eosvos.h EOSVOS_PLAN_LOG_FIELDS

    def plan_log(self, on=True):
        """Record how every tiled-conv launch is planned from now on (host bookkeeping for the tests; clears the log)."""
        _ffi.check(self.lib.eosvos_test_conv_plan_log(self.h, int(on)))

    def plan_log_read(self):
        """The launches since plan_log(True), in order: one dict per launch with 'kernel' (symbol) and PLAN_LOG_FIELDS
        (include/eosvos.h eosvos_test_conv_plan_log_read).  Raises when more launches ran than the log keeps."""
        mx, nf = 16, len(self.PLAN_LOG_FIELDS)
        names = ctypes.create_string_buffer(64 * mx)
        fields, n = (ctypes.c_int * (mx * nf))(), ctypes.c_int()
        _ffi.check(self.lib.eosvos_test_conv_plan_log_read(self.h, mx, names, fields, ctypes.byref(n)))
        if n.value > mx:
            raise _ffi.EosvosError(f'plan log: {n.value} launches, {mx} kept')
        out = []
        for i in range(n.value):
            rec = {'kernel': names.raw[64 * i:64 * i + 64].split(b'\0')[0].decode()}
            rec.update(zip(self.PLAN_LOG_FIELDS, (int(v) for v in fields[i * nf:(i + 1) * nf])))
            out.append(rec)
        return out

    def mfma_probe(self, iters=20000):
        """Sustained fp32 MFMA TFLOP/s of this device (register-only calibration kernel)."""
        ms, fl = ctypes.c_float(), ctypes.c_double()
        _ffi.check(self.lib.eosvos_mfma_probe(self.h, iters, ctypes.byref(ms), ctypes.byref(fl)))
        return fl.value / (ms.value * 1e-3) / 1e12

    def debug_tensor(self, name):
        """Copy of a named internal NHWC buffer as a (B,C,H,W) tensor (parity tests)."""
        ptr = ctypes.c_void_p()
        dims = (ctypes.c_int64 * 4)()
        _ffi.check(self.lib.eosvos_debug_tensor(self.h, name.encode(), ctypes.byref(ptr), dims))
        b, h, w, c = [int(d) for d in dims]
        n = b * h * w * c
        out = torch.empty(n, device=self.device)
        self.synchronize()
        import ctypes as _c
        hip = _c.CDLL('libamdhip64.so')
        rc = hip.hipMemcpy(_c.c_void_p(out.data_ptr()), ptr, _c.c_size_t(n * 4), 3)  # device to device
        if rc != 0:
            raise _ffi.EosvosError(f'hipMemcpy failed ({rc})')
        return out.view(b, h, w, c).permute(0, 3, 1, 2).contiguous()

    # ---- low-level op tests --------------------------------------------------------------
    def test_conv(self, x_nhwc, w_oihw, scale, bias, res, relu, stride, dil, pad):
        B, H, W, Cin = x_nhwc.shape
        Cout, _, k, _ = w_oihw.shape
        Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
        Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
        y = torch.empty(B, Ho, Wo, Cout, device=self.device)
        p = lambda t: _ptr(t) if t is not None else None
        _ffi.check(self.lib.eosvos_test_conv(self.h, _ptr(x_nhwc), _ptr(w_oihw), p(scale), p(bias), p(res),
                                             int(relu), B, H, W, Cin, Cout, k, stride, dil, pad, _ptr(y)))
        return y

    ALGOS = {'auto': 0, 'direct': 1, 'wino_f2': 2, 'wino_f4': 3}          # include/eosvos.h EOSVOS_ALGO_*

    def test_conv_algo(self, algo, x_nhwc, w_oihw, scale, bias, res, relu, stride, dil, pad):
        """One conv through the production forward path with the algorithm forced."""
        B, H, W, Cin = x_nhwc.shape
        Cout, _, k, _ = w_oihw.shape
        Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
        Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
        y = torch.full((B, Ho, Wo, Cout), float('nan'), device=self.device)          # an element no workgroup wrote stays NaN
        p = lambda t: _ptr(t) if t is not None else None
        _ffi.check(self.lib.eosvos_test_conv_algo(self.h, self.ALGOS[algo], _ptr(x_nhwc), _ptr(w_oihw), p(scale), p(bias),
                                                  p(res), int(relu), B, H, W, Cin, Cout, k, stride, dil, pad, _ptr(y)))
        return y

    def test_conv_bwd_algo(self, algo, x_nhwc, w_oihw, g_nhwc, stride, dil, pad, scale=None, mask=None):
        """(dx, dw) through the production weight- / data-gradient paths with the algorithm forced; dx = 0 where mask (NHWC
        like x) is <= 0, passed to the engine as mask bytes."""
        B, H, W, Cin = x_nhwc.shape
        Cout, _, k, _ = w_oihw.shape
        dx = torch.full_like(x_nhwc, float('nan'))          # an element no workgroup wrote stays NaN
        dw = torch.full_like(w_oihw, float('nan'))
        m8 = _relu_bits(mask)
        _ffi.check(self.lib.eosvos_test_conv_bwd_algo(self.h, self.ALGOS[algo], _ptr(x_nhwc), _ptr(w_oihw), _ptr(g_nhwc),
                                                      _optr(scale), _optr(m8), B, H, W, Cin, Cout, k, stride, dil, pad, _ptr(dx),
                                                      _ptr(dw)))
        return dx, dw

    def test_conv_bwd(self, x_nhwc, w_oihw, g_nhwc, stride, dil, pad):
        B, H, W, Cin = x_nhwc.shape
        Cout, _, k, _ = w_oihw.shape
        dx = torch.empty_like(x_nhwc)
        dw = torch.empty_like(w_oihw)
        _ffi.check(self.lib.eosvos_test_conv_bwd(self.h, _ptr(x_nhwc), _ptr(w_oihw), _ptr(g_nhwc), B, H, W, Cin,
                                                 Cout, k, stride, dil, pad, _ptr(dx), _ptr(dw)))
        return dx, dw

    @staticmethod
    def _view(t, C, shape):
        """eosvos_view of `t`: a (B, h, w, C) NHWC tensor, or (view, base) with `view` a channel slice of the contiguous NHWC
        tensor `base` (the key: absmax slot and mask bytes are kept per tensor).  Refuses anything that is not inside its base."""
        v = _ffi.View()
        if t is None:
            return v
        view, base = t if isinstance(t, tuple) else (t, None)
        B, h, w = shape
        ld = view.stride(2)
        assert view.dtype == torch.float32 and tuple(view.shape) == (B, h, w, C), (tuple(view.shape), (B, h, w, C))
        assert view.stride() == (h * w * ld, w * ld, ld, 1) and ld >= C and ld % 4 == 0, view.stride()
        v.p, v.ld = view.data_ptr(), ld
        if base is None:
            assert view.is_contiguous() or view._base is not None, 'a strided view needs its base tensor'
            if view._base is not None:
                b0 = view._base
                off = (view.data_ptr() - b0.data_ptr()) // 4
                assert 0 <= off and off + (B * h * w - 1) * ld + C <= b0.numel(), 'view outside its storage'
        else:
            assert base.dtype == torch.float32 and base.is_contiguous() and tuple(base.shape) == (B, h, w, ld), tuple(base.shape)
            off = (view.data_ptr() - base.data_ptr()) // 4
            assert 0 <= off <= ld - C and off % 4 == 0, off
            v.key, v.ldkey = base.data_ptr(), ld
        return v

    def test_conv_views(self, algo, w_oihw, stride, dil, pad, shape, scale=None, bias=None, x=None, y=None, res=None, relu=False,
                        y_m8=None, g=None, gx=None, add=None, accum=False, mask_c0=0, gx_m8=None, want_dw=False, fwd_slices=1):
        """One conv through the production conv_fwd / conv_dgrad / conv_wgrad with every operand a view (include/eosvos.h
        eosvos_test_conv_views): `shape` = (B, H, W) of the conv input; an operand is an NHWC tensor (its pixel stride is the
        pitch) or a (view, base) pair.  Passes: forward when `y` is given (written in place; y_m8 = uint8 (B, Ho, Wo, ld / 4) mask
        bytes of the whole y tensor), data gradient when `gx` is given (in place; gx_m8 = uint8 (B, H, W, ld / 4)), weight
        gradient when want_dw.  fwd_slices = n > 1: n forwards in one absmax phase, the i-th reading the next Cin channels of x's
        base and writing the next Cout channels of y's.  Returns {'dw', 'y_slot', 'gx_slot', 'x_slot', 'g_slot'}: slots as (bit
        pattern of the committed max, trusted); x_slot / g_slot: the whole-tensor slot a keyed source view ran under."""
        B, H, W = shape
        Cout, Cin, k, _ = w_oihw.shape
        Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
        Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
        a = _ffi.ConvViews()
        a.algo, a.B, a.H, a.W, a.Cin, a.Cout, a.k, a.stride, a.dil, a.pad = self.ALGOS[algo], B, H, W, Cin, Cout, k, stride, dil, pad
        assert w_oihw.is_contiguous() and w_oihw.dtype == torch.float32
        a.w_oihw = w_oihw.data_ptr()
        for name, t in (('scale', scale), ('bias', bias)):
            if t is not None:
                assert t.is_contiguous() and t.dtype == torch.float32 and t.numel() == Cout
                setattr(a, name, t.data_ptr())
        a.passes = (_ffi.VIEWS_FWD if y is not None else 0) | (_ffi.VIEWS_DGRAD if gx is not None else 0) | (_ffi.VIEWS_WGRAD if want_dw else 0)
        a.x, a.y, a.res = self._view(x, Cin, (B, H, W)), self._view(y, Cout, (B, Ho, Wo)), self._view(res, Cout, (B, Ho, Wo))
        a.g, a.gx, a.add = self._view(g, Cout, (B, Ho, Wo)), self._view(gx, Cin, (B, H, W)), self._view(add, Cin, (B, H, W))
        a.relu, a.accum, a.mask_c0, a.fwd_slices = int(relu), int(accum), int(mask_c0), int(fwd_slices)
        if fwd_slices > 1:
            for vw, C in ((a.x, Cin), (a.y, Cout)):
                assert vw.key and (vw.p - vw.key) // 4 + fwd_slices * C <= vw.ldkey, 'fwd_slices: past the base tensor'
        if y_m8 is not None:
            assert y_m8.dtype == torch.uint8 and y_m8.is_contiguous() and tuple(y_m8.shape) == (B, Ho, Wo, a.y.ld // 4), tuple(y_m8.shape)
            a.y_m8 = y_m8.data_ptr()
        if gx_m8 is not None:
            assert gx_m8.dtype == torch.uint8 and gx_m8.is_contiguous() and tuple(gx_m8.shape) == (B, H, W, a.gx.ld // 4), tuple(gx_m8.shape)
            a.gx_m8 = gx_m8.data_ptr()
        dw = torch.full_like(w_oihw, float('nan')) if want_dw else None
        if dw is not None:
            a.dw_oihw = dw.data_ptr()
        torch.cuda.synchronize(self.device)
        _ffi.check(self.lib.eosvos_test_conv_views(self.h, ctypes.byref(a)))
        return {'dw': dw, 'y_slot': (int(a.slot_bits[0]), bool(a.slot_valid[0])), 'gx_slot': (int(a.slot_bits[1]), bool(a.slot_valid[1])),
                'x_slot': (int(a.src_slot_bits[0]), bool(a.src_slot_valid[0])), 'g_slot': (int(a.src_slot_bits[1]), bool(a.src_slot_valid[1]))}

    def test_aspp_dgrad(self, g_cat, l4_m8, g_l4, force_fallback=False):
        """The ASPP branches' data gradient into d(layer4 output) as the backward pass runs it (include/eosvos.h
        eosvos_test_aspp_dgrad), with this engine's weights: g_cat (B, h16, w16, 1280), l4_m8 uint8 (B, h16, w16, 512), g_l4
        (B, h16, w16, 2048) updated in place.  Returns (merged_ran, (slot bits, trusted))."""
        B, h, w, _ = g_cat.shape
        ptr, dims = ctypes.c_void_p(), (ctypes.c_int64 * 4)()
        _ffi.check(self.lib.eosvos_debug_tensor(self.h, b'g_cat', ctypes.byref(ptr), dims))
        assert (h, w) == (int(dims[1]), int(dims[2])) and 1 <= B <= self.max_batch, ((B, h, w), list(dims))      # the engine's own buffers
        assert g_cat.is_contiguous() and g_cat.dtype == torch.float32 and g_cat.shape[3] == 1280
        assert g_l4.is_contiguous() and g_l4.dtype == torch.float32 and tuple(g_l4.shape) == (B, h, w, 2048)
        assert l4_m8.is_contiguous() and l4_m8.dtype == torch.uint8 and tuple(l4_m8.shape) == (B, h, w, 512)
        merged, bits, valid = ctypes.c_int(), ctypes.c_uint(), ctypes.c_int()
        torch.cuda.synchronize(self.device)
        _ffi.check(self.lib.eosvos_test_aspp_dgrad(self.h, B, _ptr(g_cat), _ptr(l4_m8), _ptr(g_l4), int(force_fallback),
                                                   ctypes.byref(merged), ctypes.byref(bits), ctypes.byref(valid)))
        return bool(merged.value), (int(bits.value), bool(valid.value))

    # Op-level entries of misc_kernels.hip (include/eosvos.h) on device tensors.  Pixel-major (B, P, C) / (B, H, W, C) views with
    # unit channel stride; the pixel stride is the leading dimension, so a channel slice of a wider buffer may be passed.
    def test_groupnorm(self, z, gamma, beta, eps=1e-5, res=None, relu=False, y=None, m8=None):
        """GroupNorm(16, C) forward of z (B, P, C) into y (default: a new (B, P, C)); returns (y, stats (B, 16, 2) = mean /
        rstd).  m8 (uint8 (B, P, >= C / 4)) receives the ReLU mask bits (relu only)."""
        B, P, C = z.shape
        y = torch.empty(B, P, C, device=self.device) if y is None else y
        stats = torch.empty(B, 16, 2, device=self.device)
        _ffi.check(self.lib.eosvos_test_groupnorm(self.h, 0, _ptr(z), _ld(z), None, 0, _ptr(gamma), _ptr(beta), _optr(res),
                                                  _ld(res), int(relu), B, P, C, float(eps), _ptr(y), _ld(y), _ptr(stats), _optr(m8),
                                                  _ld(m8)))
        return y, stats

    def test_groupnorm_bwd(self, z, g, gamma, stats):
        """dL/dz of that forward (without ReLU / residual) given g = dL/d(gn output) (B, P, C); overwrites z and returns it."""
        B, P, C = z.shape
        _ffi.check(self.lib.eosvos_test_groupnorm(self.h, 1, _ptr(z), _ld(z), _ptr(g), _ld(g), _ptr(gamma), None, None, 0, 0,
                                                  B, P, C, 0.0, None, 0, _ptr(stats), None, 0))
        return z

    def test_maxpool(self, x, gy=None):
        """max_pool2d(3, 2, 1) of a dense x (B, H, W, C): (y, argmax bytes, gx or None)."""
        B, H, W, C = x.shape
        assert x.is_contiguous() and (gy is None or gy.is_contiguous())
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty(B, Ho, Wo, C, device=self.device)
        idx = torch.empty(B, Ho, Wo, C, dtype=torch.uint8, device=self.device)
        gx = torch.empty_like(x) if gy is not None else None
        _ffi.check(self.lib.eosvos_test_maxpool(self.h, _ptr(x), B, H, W, C, _ptr(y), _ptr(idx), _optr(gy), _optr(gx)))
        return y, idx, gx

    def test_resize(self, align_corners, x=None, y=None, gy=None, gx=None, mask=None):
        """Bilinear resize x (B, hin, win, C) -> y (B, hout, wout, C) and / or its backward gy -> gx (zero where mask <= 0,
        passed to the engine as mask bytes: C % 4 == 0); the caller provides every tensor."""
        (B, hin, win, C), (hout, wout) = (x if x is not None else gx).shape, (y if y is not None else gy).shape[1:3]
        m8 = _relu_bits(mask)
        _ffi.check(self.lib.eosvos_test_resize(self.h, int(align_corners), hin, win, hout, wout, B, C, _optr(x), _ld(x), _optr(y),
                                               _ld(y), _optr(gy), _ld(gy), _optr(gx), _ld(gx), _optr(m8), _ld(m8)))

    def test_aspp_pool(self, x, w, a=None, bias=None, y=None, m8=None, gy=None):
        """ASPP image pooling of x (B, P, K) with w (N, K): dict of v, pool, y (default (B, P, N)) and, given gy (B, P, N),
        gpool, gv, dw, gx."""
        B, P, K = x.shape
        N = w.shape[0]
        dev = self.device
        r = {'v': torch.empty(B, K, device=dev), 'pool': torch.empty(B, N, device=dev),
             'y': y if y is not None else torch.empty(B, P, N, device=dev)}
        if gy is not None:
            r.update(gpool=torch.empty(B, N, device=dev), gv=torch.empty(B, K, device=dev), dw=torch.empty(N, K, device=dev),
                     gx=torch.empty(B, P, K, device=dev))
        q = lambda k: _optr(r.get(k))
        _ffi.check(self.lib.eosvos_test_aspp_pool(self.h, B, P, K, N, _ptr(w), _optr(a), _optr(bias), _ptr(x), _ld(x), q('v'),
                                                  q('pool'), q('y'), _ld(r['y']), _optr(m8), _ld(m8), _optr(gy), _ld(gy),
                                                  q('gpool'), q('gv'), q('dw'), q('gx'), K))
        return r

    def test_head(self, x, w, bias, g=None):
        """1-channel classifier of a dense x (P, C): (y (P,), gx or None, dw (C + 1,) = weight and bias gradient, or None)."""
        P, C = x.shape
        assert x.is_contiguous()
        y = torch.empty(P, device=self.device)
        gx = torch.empty_like(x) if g is not None else None
        dw = torch.empty(C + 1, device=self.device) if g is not None else None
        _ffi.check(self.lib.eosvos_test_head(self.h, _ptr(x), _ptr(w), _ptr(bias), P, C, _ptr(y), _optr(g), _optr(gx), _optr(dw)))
        return y, gx, dw


class RcclComm:
    """An RCCL communicator owned through the C-ABI (`eosvos_comm_*`, include/eosvos.h): one rank per GPU.  Rank 0 makes
    `RcclComm.unique_id()` (128 bytes) and hands it to the other ranks by the host's own means; constructing the communicator
    is collective over all `world_size` ranks."""

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        _ffi.check(_ffi.load().eosvos_comm_unique_id(buf))
        return buf.raw

    def __init__(self, world_size, rank, unique_id, device=0):
        assert len(unique_id) == 128
        self.world_size, self.rank = world_size, rank
        h = ctypes.c_void_p()
        self._id = ctypes.create_string_buffer(unique_id, 128)
        _ffi.check(_ffi.load().eosvos_comm_init_rank(ctypes.byref(h), world_size, self._id, rank, int(device)))
        self.handle = h

    def close(self):
        if getattr(self, 'handle', None):
            _ffi.check(_ffi.load().eosvos_comm_destroy(self.handle))
            self.handle = None
