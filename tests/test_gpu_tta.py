"""Test-time augmentation (`eosvos_amd/tta.py`): the mirrored forward (`eosvos_infer_view`), the fused view -> accumulator
kernel (`eosvos_tta_accumulate`), the frame resize (`eosvos_resize_frames`) and `run_frames` / `evaluate_sequence` with
`tta=`.  Needs an MI355X: pytest -m gpu.

Tolerances are not fixed numbers.  `_fp32_error` evaluates the expression under test in fp32 with torch on the CPU and takes
its largest difference from the fp64 value; the kernel is allowed twice that, and every case prints both (`pytest -s`;
`tools/tta_time.py` records them in profiles/tta_time.txt)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eosvos_amd import _ffi, synthetic, topology
from eosvos_amd.engine import Engine

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SMALL = (96, 160)
MODES = ('f32', 'bf16x6', 'f16x3')
# h x w -> H x W of test 2: identity, up, down, odd sizes (73 x 122 = round(0.75 * 97) x round(0.75 * 163))
PAIRS = [((96, 160), (96, 160)), ((72, 120), (96, 160)), ((120, 200), (96, 160)), ((73, 122), (97, 163))]
W3 = float(np.float32(1.0 / 3.0))            # the weight as the fp32 the kernel receives
TTA6 = {'flip': True, 'scales': [0.75, 1.0, 1.25]}

_ENGINES = {}


def _engine(h, w):
    """One engine per frame size for the whole module (batch <= 2, synthetic state, theta = init)."""
    if (h, w) not in _ENGINES:
        e = Engine('resnet50', h, w, max_batch=2, device=DEV)
        e.load_model_state(synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50'))
        _ENGINES[(h, w)] = e
    return _ENGINES[(h, w)]


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- 1. the mirrored forward --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('batch', [1, 2])
@pytest.mark.parametrize('size', [(97, 163), (96, 160)])
def test_mirrored_forward_equals_forward_of_the_flipped_frame(size, batch, mode):
    eng = _engine(*size)
    x = synthetic.synthetic_frames(batch, *size, seed=11)[0].to(DEV)
    eng.set_engine_matrix_mode(mode)
    eng.reset()         # a mode change goes with a weight (re)load, as in tests/shape_sweep.py: the per-mode weight caches are remade
    try:
        a, b = eng.forward(x), eng.forward(x)
        assert torch.equal(_bits(a), _bits(b)), 'two plain forwards of one input differ'       # else the bound below is not 0
        ref = eng.forward(torch.flip(x, [3]).contiguous())
        eng.infer_view(x, mirror=True)
        got = eng.debug_tensor('logits')[:batch]
    finally:
        eng.set_engine_matrix_mode(None)
    assert not torch.equal(_bits(ref), _bits(a))                                               # the flip matters at all
    assert torch.equal(_bits(got), _bits(ref))


def test_plain_view_is_the_inference_forward():
    eng = _engine(*SMALL)
    x = synthetic.synthetic_frames(2, *SMALL, seed=12)[0].to(DEV)
    probs = eng.infer(x)
    fp = eng.plan_fingerprint()
    logits = eng.debug_tensor('logits')[:2]
    eng.infer_view(x, mirror=False)
    assert torch.equal(_bits(eng.debug_tensor('logits')[:2]), _bits(logits))
    assert eng.plan_fingerprint()[0] == fp[0]
    eng.infer_view(x, mirror=True)
    assert eng.plan_fingerprint()[0] == fp[0]                       # the mirrored view runs the launch plan of eosvos_infer
    acc = torch.empty_like(probs)
    eng.infer_view(x, mirror=False)
    eng.tta_accumulate(acc, 1.0, mirror=False, first=True)
    assert torch.equal(_bits(acc), _bits(probs))                    # identity size, weight 1: eosvos_infer's bits


# ---- 2. the accumulate kernel against fp64 ------------------------------------------------------------------------------
def _expr(logits, out_hw, mirror, dtype):
    """sigmoid(F.interpolate(un-mirrored logits, out_hw, bilinear, align_corners=False)) on the CPU in `dtype`."""
    u = logits.detach().cpu().to(dtype)
    if mirror:
        u = torch.flip(u, [3])
    return torch.sigmoid(F.interpolate(u, out_hw, mode='bilinear', align_corners=False))


def _fp32_error(logits, out_hw, mirror):
    """(fp64 value, largest error of the same expression in fp32)."""
    r64 = _expr(logits, out_hw, mirror, torch.float64)
    return r64, float((_expr(logits, out_hw, mirror, torch.float32).double() - r64).abs().max())


@functools.lru_cache(maxsize=None)
def _view_case(hw, HW, mirror):
    """The logits an engine of size hw leaves for a view (mirrored input when `mirror`), and their fp64 reference at HW."""
    eng = _engine(*hw)
    x = synthetic.synthetic_frames(2, *hw, seed=21 + hw[0])[0].to(DEV)
    eng.infer_view(x, mirror=mirror)
    logits = eng.debug_tensor('logits')[:2]
    return (x, logits) + _fp32_error(logits, HW, mirror)


@pytest.mark.parametrize('first', [True, False])
@pytest.mark.parametrize('mirror', [False, True])
@pytest.mark.parametrize('hw,HW', PAIRS)
def test_accumulate_against_fp64(hw, HW, mirror, first):
    x, logits, r64, err32 = _view_case(hw, HW, mirror)
    eng = _engine(*hw)
    eng.infer_view(x, mirror=mirror)                               # (another case may have used this engine since)
    prior = torch.rand(2, 1, *HW, generator=torch.Generator().manual_seed(5)) * (2.0 / 3.0)
    acc = prior.to(DEV)
    eng.tta_accumulate(acc, W3, mirror=mirror, first=first)
    want = W3 * r64 + (0.0 if first else prior.double())
    got = float((acc.cpu().double() - want).abs().max())
    print(f'tta_accumulate {hw[0]}x{hw[1]} -> {HW[0]}x{HW[1]} mirror={int(mirror)} first={int(first)}: '
          f'torch fp32 error {err32:.3e}, kernel error {got:.3e}, allowed {2 * err32:.3e}')
    assert err32 > 0
    assert got <= 2 * err32
    if hw == HW:                                                    # identity size: sigmoid of the logit itself
        sg = torch.sigmoid((torch.flip(logits, [3]) if mirror else logits).cpu().double())
        assert float((acc.cpu().double() - (W3 * sg + (0.0 if first else prior.double()))).abs().max()) <= 2 * err32


# ---- 3. end to end ------------------------------------------------------------------------------------------------------
BN_CFG = {'accum_stats': False, 'learn_weight': False, 'learn_bias': False}
MO_CFG = dict(init_lr=1e-3, learn_model_init=True, second_order_gradients=False, lr_hierarchy_level='NEURON',
              use_log_init_lr=False, max_lr=None)


def _meta_state():
    sd = synthetic.synthetic_state('resnet50')
    out = {}
    for (n, _), lr in zip(topology.trainable('resnet50'), synthetic.synthetic_lrs('resnet50')):
        out['log_init_lr_' + n.replace('.', '-')] = lr.clone()
    for n, _ in topology.trainable('resnet50'):
        out['model_init_' + n.replace('.', '-')] = sd[n].clone()
    return sd, out


@pytest.fixture(scope='module')
def model_and_optim():
    from eosvos_amd.helper_func import init_parent_model
    from eosvos_amd.meta_optim import MetaOptimizer
    model, _ = init_parent_model(architecture='DeepLabV3Plus', encoder='resnet50', train_encoder=True,
                                 decoder_norm_layer='BatchNorm2d', replace_batch_with_group_norms=False, batch_norm=BN_CFG,
                                 roi_pool_output_sizes=None, eval_augment_rpn_proposals_mode=None, box_nms_thresh=None,
                                 maskrcnn_loss=None)
    sd, msd = _meta_state()
    model.load_state_dict(sd)
    mo = MetaOptimizer(model, **MO_CFG)
    yield model, mo, msd
    model.close_engines()


def test_run_frames_with_six_views_equals_the_composed_pipeline(model_and_optim):
    from eosvos_amd.helper_func import run_frames
    model, mo, msd = model_and_optim
    mo.load_state_dict(msd)
    mo.reset()
    x, y = synthetic.synthetic_frames(2, *SMALL, seed=41)
    xg, yg = x.to(DEV), y.to(DEV)
    main = model._ensure_engine(*SMALL, 2)
    p_init = run_frames(model, xg, tta=TTA6)[2]
    main.finetune_step(xg, yg)
    p = run_frames(model, xg, tta=TTA6)[2]
    assert p.shape == (2, 1, *SMALL)
    assert float((p - p_init).abs().max()) > 1e-6                  # the views saw the fine-tuned weights ...
    theta = main.get_params()
    total, err_max = torch.zeros(2, 1, *SMALL, dtype=torch.float64), 0.0
    for s in TTA6['scales']:
        h, w = int(round(SMALL[0] * s)), int(round(SMALL[1] * s))
        eng = main if s == 1.0 else _engine(h, w)
        xs = xg if s == 1.0 else main.resize_frames(xg, h, w)
        if s != 1.0:
            ref_xs = F.interpolate(x.double(), (h, w), mode='bilinear', align_corners=False)
            e32 = float((F.interpolate(x, (h, w), mode='bilinear', align_corners=False).double() - ref_xs).abs().max())
            assert float((xs.cpu().double() - ref_xs).abs().max()) <= 2 * e32    # twice torch's own fp32 error, as in test 2
            eng.set_params(theta)
        for mirror in (False, True):
            logits = eng.forward(torch.flip(xs, [3]).contiguous() if mirror else xs)
            r64, e32 = _fp32_error(logits, SMALL, mirror)
            total += r64 / 6.0
            err_max = max(err_max, e32)
        if s != 1.0:
            eng.reset()                                            # theta <- init for the other tests of the module
    got = float((p.cpu().double() - total).abs().max())
    # a convex combination of six views, each within twice its own fp32 error (test 2): within twice the largest of them
    print(f'run_frames, 6 views: largest torch fp32 error of a view {err_max:.3e}, error {got:.3e}, allowed {2 * err_max:.3e}')
    assert got <= 2 * err_max
    # ... and the fine-tuned ones exactly: the same composition from the initial weights is far outside that bound
    assert float((p_init.cpu().double() - total).abs().max()) > 2 * err_max
    mo.reset()


# ---- 4. off means off ---------------------------------------------------------------------------------------------------
NEUTRAL = {'flip': False, 'scales': [1.0]}


def test_off_means_off(model_and_optim, monkeypatch):
    from eosvos_amd import config
    from eosvos_amd.evaluate import evaluate_sequence
    from eosvos_amd.helper_func import run_frames
    model, mo, msd = model_and_optim
    mo.load_state_dict(msd)
    mo.reset()
    x, y = synthetic.synthetic_frames(2, *SMALL, seed=43)
    xg, yg = x.to(DEV), y.to(DEV)
    eng = model._ensure_engine(*SMALL, 1)
    today = torch.cat([eng.infer(xg[i:i + 1].contiguous()) for i in range(2)])       # the calls run_frames makes today
    fp = eng.plan_fingerprint()
    run_frames(model, xg, tta=TTA6)
    with monkeypatch.context() as mp:
        def no_view(*a, **k):
            raise AssertionError('a test-time augmentation call on the plain path')
        for name in ('infer_view', 'tta_accumulate', 'resize_frames'):
            mp.setattr(Engine, name, no_view)
        runs = [run_frames(model, xg, yg), run_frames(model, xg, yg, tta=None), run_frames(model, xg, yg, tta=NEUTRAL)]
        for losses, accs, probs in runs:
            assert torch.equal(_bits(probs), _bits(today))
            assert torch.equal(losses, runs[0][0]) and torch.equal(accs, runs[0][1])
        assert model.engine.plan_fingerprint() == fp                # unchanged after a run with views in between
        cfg = config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS-OnA', 'num_epochs.eval=2', 'eval_online_adapt.num_epochs=1',
                                'eval_online_adapt.step=2'])
        frames, gt = synthetic.synthetic_frames(1, *SMALL, seed=3)
        seq = torch.cat([torch.roll(frames, shifts=4 * i, dims=3) for i in range(4)]).to(DEV)
        outs = [evaluate_sequence(model, mo, msd, seq, [gt[0]], cfg, **kw) for kw in ({}, {'tta': None}, {'tta': NEUTRAL})]
        for labels, probs, hist in outs[1:]:
            assert torch.equal(labels, outs[0][0]) and hist == outs[0][2]
            assert torch.equal(_bits(probs[0]), _bits(outs[0][1][0]))
    on = evaluate_sequence(model, mo, msd, seq, [gt[0]], cfg, tta={'flip': True, 'scales': [1.0]})
    assert on[1][0].shape == outs[0][1][0].shape and not torch.equal(on[1][0], outs[0][1][0])      # and on means on
    model.close_parked_engines()
    assert model.__dict__['_view_engines'] == {}
    mo.reset()


# ---- 5. bad arguments ---------------------------------------------------------------------------------------------------
def test_bad_arguments_return_errors_without_launching():
    eng = _engine(*SMALL)
    lib, h = eng.lib, eng.h
    x = synthetic.synthetic_frames(1, *SMALL, seed=5)[0].to(DEV)
    eng.infer_view(x)
    acc = torch.full((1, 1, *SMALL), 7.0, device=DEV)
    small = torch.full((1, 3, 8, 8), 7.0, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    H, W = SMALL
    bad = [
        lambda: lib.eosvos_infer_view(None, P(x), 1, 0),
        lambda: lib.eosvos_infer_view(h, None, 1, 0),
        lambda: lib.eosvos_infer_view(h, P(x), 0, 0),
        lambda: lib.eosvos_infer_view(h, P(x), eng.max_batch + 1, 0),
        lambda: lib.eosvos_tta_accumulate(None, H, W, 1, 0, 1.0, 1, P(acc), H, W),
        lambda: lib.eosvos_tta_accumulate(h, H, W, 1, 0, 1.0, 1, None, H, W),
        lambda: lib.eosvos_tta_accumulate(h, H, W, 0, 0, 1.0, 1, P(acc), H, W),
        lambda: lib.eosvos_tta_accumulate(h, H, W, eng.max_batch + 1, 0, 1.0, 1, P(acc), H, W),
        lambda: lib.eosvos_tta_accumulate(h, 0, W, 1, 0, 1.0, 1, P(acc), H, W),
        lambda: lib.eosvos_tta_accumulate(h, H, W, 1, 0, 1.0, 1, P(acc), H, 0),
        lambda: lib.eosvos_tta_accumulate(h, H - 1, W, 1, 0, 1.0, 1, P(acc), H, W),          # not the engine's frame size
        lambda: lib.eosvos_tta_accumulate(h, H, W, 1, 0, float('nan'), 1, P(acc), H, W),
        lambda: lib.eosvos_resize_frames(None, P(small), 1, 3, 8, 8, 8, 8, P(small)),
        lambda: lib.eosvos_resize_frames(h, None, 1, 3, 8, 8, 8, 8, P(small)),
        lambda: lib.eosvos_resize_frames(h, P(small), 1, 3, 8, 8, 8, 8, None),
        lambda: lib.eosvos_resize_frames(h, P(small), 0, 3, 8, 8, 8, 8, P(small)),
        lambda: lib.eosvos_resize_frames(h, P(small), 1, 0, 8, 8, 8, 8, P(small)),
        lambda: lib.eosvos_resize_frames(h, P(small), 1, 3, 0, 8, 8, 8, P(small)),
        lambda: lib.eosvos_resize_frames(h, P(small), 1, 3, 8, 8, 8, 0, P(small)),
    ]
    for i, call in enumerate(bad):
        assert call() == 1, i
        assert lib.eosvos_last_error().decode(), i
    torch.cuda.synchronize()
    assert bool((acc == 7.0).all()) and bool((small == 7.0).all())              # nothing was written
    with pytest.raises(_ffi.EosvosError):
        _ffi.check(lib.eosvos_tta_accumulate(h, H, W, 0, 0, 1.0, 1, P(acc), H, W))
