"""The object-centred zoom pass on the MI355X (`eosvos_amd/zoom.py`): the box kernel against the numpy twin bit for bit, the
cut / put-back / blend kernels against fp64, and `run_frames` / `evaluate_sequence` with `zoom=`.  Needs an MI355X:
pytest -m gpu.

Tolerances are not fixed numbers (the yardstick of tests/test_gpu_tta.py).  `_fp32_error` evaluates the expression under test
in fp32 with torch on the CPU and takes its largest difference from the fp64 value; the kernel is allowed twice that, and
every case prints both (`pytest -s`; `tools/zoom_time.py` records them in profiles/zoom_time.txt)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import zoom_ref  # noqa: E402

from eosvos_amd import _ffi, synthetic, topology, zoom  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SMALL, ODD = (96, 160), (97, 163)
SENTINEL = 7.0

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


def _dev_boxes(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


def _fp32_error(expr):
    """(fp64 value, largest error of the same expression in fp32) of expr(dtype)."""
    r64 = expr(torch.float64)
    return r64, float((expr(torch.float32).double() - r64).abs().max())


def _inside(boxes, shape):
    """Boolean (B, 1, H, W): the pixels inside valid boxes."""
    m = torch.zeros(shape, dtype=torch.bool)
    for f, (valid, y0, x0, bh, bw) in enumerate(boxes):
        if valid:
            m[f, :, y0:y0 + bh, x0:x0 + bw] = True
    return m


# ---- 1. boxes: bit-equal to the numpy twin ------------------------------------------------------------------------------
def mixed_frames(H, W):
    """Three frames of mixed validity: a small blob (valid), nothing (empty), a blob too large to magnify by min_zoom."""
    return np.stack([zoom_ref.frame(H, W, (H // 3, H // 3 + 3, W // 2, W // 2 + 3)), zoom_ref.frame(H, W),
                     zoom_ref.frame(H, W, (2, H - 3, 3, W - 4))])


def device_boxes_of_all_cases(eng):
    """{name: boxes as a list} of every case of tests/zoom_ref.py and of the three-frame calls, from the device."""
    out = {}
    for name, p0, prm in zoom_ref.cases():
        out[name] = eng.zoom_boxes(torch.from_numpy(p0)[None].to(DEV), prm).cpu().tolist()
    for H, W in zoom_ref.SIZES:
        out[f'{H}x{W} three frames'] = eng.zoom_boxes(torch.from_numpy(mixed_frames(H, W)).to(DEV), zoom_ref.BASE).cpu().tolist()
    return out


def host_boxes_of_all_cases():
    out = {name: zoom.boxes_host(p0[None], prm).tolist() for name, p0, prm in zoom_ref.cases()}
    for H, W in zoom_ref.SIZES:
        out[f'{H}x{W} three frames'] = zoom.boxes_host(mixed_frames(H, W), zoom_ref.BASE).tolist()
    return out


def test_boxes_are_bit_equal_to_the_numpy_twin():
    got, want = device_boxes_of_all_cases(_engine(*SMALL)), host_boxes_of_all_cases()
    assert want['anchor'] == [list(zoom_ref.ANCHOR)]
    for H, W in zoom_ref.SIZES:
        assert [b[0] for b in want[f'{H}x{W} three frames']] == [1, 0, 0]
    for name in want:
        assert got[name] == want[name], name
    again = device_boxes_of_all_cases(_engine(*SMALL))                 # the record is re-initialised by every call
    assert again == got


CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from eosvos_amd.engine import Engine
import test_gpu_zoom as T
eng = Engine('resnet50', 96, 160, max_batch=1, device='cuda:0')
out = T.device_boxes_of_all_cases(eng)
eng.close()
print(json.dumps(out))
'''


def test_nan_filled_buffers_give_the_same_boxes():
    """The same calls in a process whose engine buffers (the bound records included) start out as NaN words, and in one that
    gets the allocator's pages as they come: a kernel that trusts a record nothing initialised would differ."""
    want = host_boxes_of_all_cases()
    for fill in (None, '7fc00000'):
        env = dict(os.environ, EOSVOS_MODE_GUARD='0')
        env.pop('EOSVOS_DEBUG_FILL', None)
        if fill:
            env['EOSVOS_DEBUG_FILL'] = fill
        p = subprocess.run([sys.executable, '-c', CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
        assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        assert json.loads(lines[-1]) == want, fill


# ---- 2. the cut ---------------------------------------------------------------------------------------------------------
CROP_CASES = [
    ('corner', SMALL, [(1, 0, 0, 32, 54)]),
    ('far corner', SMALL, [(1, 64, 106, 32, 54)]),
    ('interior', SMALL, [(1, 29, 49, 32, 54)]),
    ('odd sizes', ODD, [(1, 13, 21, 41, 69)]),
    ('batch 2, different boxes', ODD, [(1, 0, 94, 33, 69), (1, 50, 7, 47, 79)]),
    ('batch 2, one invalid', SMALL, [(0, 0, 0, 96, 160), (1, 10, 20, 48, 80)]),
]


@pytest.mark.parametrize('name,hw,boxes', CROP_CASES, ids=[c[0] for c in CROP_CASES])
def test_crop_against_fp64(name, hw, boxes):
    eng = _engine(*SMALL)                                              # the cut is not tied to the engine's frame size
    x = synthetic.synthetic_frames(len(boxes), *hw, seed=31 + hw[0])[0]
    got = eng.zoom_crop(x.to(DEV), _dev_boxes(boxes)).cpu()
    r64, err32 = _fp32_error(lambda dt: zoom.crop_host(x, boxes, dt))
    err = float((got.double() - r64).abs().max())
    print(f'zoom_crop {name} {hw[0]}x{hw[1]}: torch fp32 error {err32:.3e}, kernel error {err:.3e}, allowed {2 * err32:.3e}')
    assert err32 > 0
    assert err <= 2 * err32
    for f, b in enumerate(boxes):
        if not b[0]:
            assert torch.equal(_bits(got[f]), _bits(x[f]))             # an invalid frame is copied through bit for bit
        else:
            assert not torch.equal(got[f], x[f])


# ---- 3. the put-back ----------------------------------------------------------------------------------------------------
ACC_CASES = [(SMALL, [(1, 29, 49, 32, 54), (0, 0, 0, 96, 160)]), (SMALL, [(1, 0, 0, 48, 80), (1, 64, 106, 32, 54)]),
             (ODD, [(1, 13, 21, 41, 69), (1, 50, 7, 47, 79)])]
WV = 0.5                                                               # the view weight of a flip pair, exact in fp32


@pytest.mark.parametrize('first', [True, False])
@pytest.mark.parametrize('mirror', [False, True])
@pytest.mark.parametrize('hw,boxes', ACC_CASES, ids=['interior+invalid', 'corners', 'odd sizes'])
def test_accumulate_against_fp64(hw, boxes, mirror, first):
    eng = _engine(*hw)
    x = synthetic.synthetic_frames(2, *hw, seed=21 + hw[0])[0].to(DEV)
    eng.infer_view(x, mirror=mirror)
    logits = eng.debug_tensor('logits')[:2]
    prior = torch.rand(2, 1, *hw, generator=torch.Generator().manual_seed(5)) * 0.5 if not first else \
        torch.full((2, 1, *hw), SENTINEL)
    pz = prior.to(DEV)
    eng.zoom_accumulate(_dev_boxes(boxes), pz, WV, mirror=mirror, first=first)
    got = pz.cpu()

    def expr(dt):
        return WV * zoom.put_back_host([(logits, mirror)], boxes, dt) + (0.0 if first else prior.to(dt))
    r64, err32 = _fp32_error(expr)
    inside = _inside(boxes, got.shape)
    err = float((got.double() - r64)[inside].abs().max())
    print(f'zoom_accumulate {hw[0]}x{hw[1]} mirror={int(mirror)} first={int(first)}: torch fp32 error {err32:.3e}, kernel error '
          f'{err:.3e}, allowed {2 * err32:.3e}')
    assert err32 > 0
    assert err <= 2 * err32
    assert torch.equal(_bits(got)[~inside], _bits(prior)[~inside])     # outside the boxes and in invalid frames: untouched
    assert bool(inside.any()) and not torch.equal(got[inside], prior[inside])


# ---- 4. the blend -------------------------------------------------------------------------------------------------------
BLEND_CASES = [('top-left corner', [(1, 0, 0, 32, 54), (0, 0, 0, 96, 160)]), ('interior', [(1, 29, 49, 32, 54), (1, 64, 106, 32, 54)]),
               ('whole frame', [(1, 0, 0, 96, 160), (1, 0, 20, 96, 100)])]


@pytest.mark.parametrize('feather', [0, 8])
@pytest.mark.parametrize('name,boxes', BLEND_CASES, ids=[c[0] for c in BLEND_CASES])
def test_blend_against_fp64(name, boxes, feather):
    eng = _engine(*SMALL)
    x = synthetic.synthetic_frames(2, *SMALL, seed=17)[0].to(DEV)
    p0 = eng.infer(x)
    pz = torch.rand(2, 1, *SMALL, generator=torch.Generator().manual_seed(9)).to(DEV)
    weight = 0.7
    out = eng.zoom_blend(_dev_boxes(boxes), pz, p0.clone(), weight, feather).cpu()
    r64, err32 = _fp32_error(lambda dt: zoom.blend_host(p0, pz, boxes, weight, feather, dt))
    err = float((out.double() - r64).abs().max())
    print(f'zoom_blend {name} feather={feather}: torch fp32 error {err32:.3e}, kernel error {err:.3e}, allowed {2 * err32:.3e}')
    assert err32 > 0
    assert err <= 2 * err32
    inside = _inside(boxes, out.shape)
    assert torch.equal(_bits(out)[~inside], _bits(p0)[~inside])        # invalid frames and pixels outside the boxes: p0's bits
    assert not torch.equal(out[inside], p0.cpu()[inside])
    if name == 'top-left corner':                                      # no ramp on the two sides that are frame borders
        f = zoom.ramp_host(boxes[0], *SMALL, feather)
        assert float(f[0, 0]) == 1.0 and (feather == 0 or float(f[-1, 0]) == 1.0 / (feather + 1) == float(f[0, -1]))
        w32 = float(np.float32(weight))
        assert abs(float(out[0, 0, 0, 0]) - (float(p0[0, 0, 0, 0]) + w32 * (float(pz[0, 0, 0, 0]) - float(p0[0, 0, 0, 0])))) <= 1e-6


# ---- 5. end to end ------------------------------------------------------------------------------------------------------
BN_CFG = {'accum_stats': False, 'learn_weight': False, 'learn_bias': False}
MO_CFG = dict(init_lr=1e-3, learn_model_init=True, second_order_gradients=False, lr_hierarchy_level='NEURON',
              use_log_init_lr=False, max_lr=None)
FLIP = {'flip': True, 'scales': [1.0]}


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


def _zoom_at_least_2(p0, base):
    """`base` with a threshold under which frame 0 of p0 (N, 1, H, W) has a valid box of at most half the frame's height: the
    value of its k-th largest pixel, for the largest k of a few that does it.  k = 1 (the maximum itself) is one pixel, whose
    box is the max_zoom floor."""
    a = p0.detach().cpu().numpy()
    top = np.sort(a[0].ravel())[::-1]
    for k in (256, 128, 64, 32, 16, 8, 4, 2, 1):
        thr = float(top[k - 1])
        if not 0 < thr < 1:
            continue
        z = dict(base, threshold=thr)
        box = zoom.boxes_host(a, z)[0]
        if box[0] == 1 and 2 * box[3] <= a.shape[2]:
            return z
    raise AssertionError('no threshold gives frame 0 a box at zoom >= 2')


def test_zoom_one_is_the_plain_path_bit_for_bit(model_and_optim):
    from eosvos_amd.helper_func import run_frames
    model, mo, msd = model_and_optim
    mo.load_state_dict(msd)
    mo.reset()
    x, y = synthetic.synthetic_frames(2, *SMALL, seed=43)
    xg, yg = x.to(DEV), y.to(DEV)
    plain = run_frames(model, xg, yg)
    fp = model.engine.plan_fingerprint()
    thr = float(plain[2].amax(dim=(1, 2, 3)).min().item())             # every frame has a pixel at or above it
    one = {'max_zoom': 1, 'min_zoom': 1, 'threshold': min(max(thr, 1e-6), 1 - 1e-6), 'min_pixels': 1, 'weight': 0.5, 'feather': 8}
    boxes = zoom.boxes_host(plain[2], one)
    assert boxes.tolist() == [[1, 0, 0, *SMALL]] * 2                   # non-empty first-pass masks: the box is the whole frame
    losses, accs, probs = run_frames(model, xg, yg, zoom=one)
    assert torch.equal(_bits(probs), _bits(plain[2])) and torch.equal(accs, plain[1])
    assert model.engine.plan_fingerprint() == fp


def test_run_frames_with_zoom_and_flip_equals_the_composed_pipeline(model_and_optim):
    from eosvos_amd.helper_func import run_frames
    model, mo, msd = model_and_optim
    mo.load_state_dict(msd)
    mo.reset()
    x, y = synthetic.synthetic_frames(2, *SMALL, seed=41)
    xg, yg = x.to(DEV), y.to(DEV)
    main = model._ensure_engine(*SMALL, 2)
    main.finetune_step(xg, yg)
    p0 = run_frames(model, xg, tta=FLIP)[2]                            # the first pass: the mean over the flip pair
    Z = _zoom_at_least_2(p0, {'max_zoom': 4, 'min_zoom': 2, 'min_pixels': 1, 'margin': 0.25, 'margin_px': 2, 'weight': 0.5,
                              'feather': 4})
    p = run_frames(model, xg, tta=FLIP, zoom=Z)[2]
    assert p.shape == (2, 1, *SMALL)
    boxes = zoom.boxes_host(p0, Z)
    assert boxes[0, 0] == 1 and 2 * boxes[0, 3] <= SMALL[0]
    assert main.zoom_boxes(p0, Z).cpu().tolist() == boxes.tolist()
    total, err_max = torch.empty(2, 1, *SMALL, dtype=torch.float64), 0.0
    for i in range(2):                                                 # run_frames scores one frame at a time
        bx = boxes[i:i + 1]
        view = main.zoom_crop(xg[i:i + 1].contiguous(), _dev_boxes(bx.tolist()))
        logits = [(main.forward(torch.flip(view, [3]).contiguous() if m else view), m) for m in (False, True)]
        pz64, e_pz = _fp32_error(lambda dt: zoom.put_back_host(logits, bx, dt))
        out64, e_bl = _fp32_error(lambda dt: zoom.blend_host(p0[i:i + 1], pz64, bx, Z['weight'], Z['feather'], dt))
        total[i:i + 1] = out64
        err_max = max(err_max, e_pz, e_bl)
    got = float((p.cpu().double() - total).abs().max())
    # the blend is a convex combination of p0 (exact: the same bits) and pz (within twice its fp32 error, test 3), evaluated
    # within twice its own fp32 error (test 4): within twice the larger of the two
    print(f'run_frames, zoom + flip: largest torch fp32 error of a component {err_max:.3e}, error {got:.3e}, allowed {2 * err_max:.3e}')
    assert err_max > 0
    assert got <= 2 * err_max
    assert float((p - p0).abs().max()) > 2 * err_max                   # the second look changed the prediction at all
    # the zoomed views saw the fine-tuned weights: the same call from the initial ones is far outside that bound
    mo.reset()
    p_init = run_frames(model, xg, tta=FLIP, zoom=Z)[2]
    assert float((p_init.cpu().double() - total).abs().max()) > 2 * err_max


def test_evaluate_sequence_on_and_off(model_and_optim, monkeypatch):
    from eosvos_amd import config
    from eosvos_amd.evaluate import evaluate_sequence
    model, mo, msd = model_and_optim
    mo.load_state_dict(msd)
    mo.reset()
    cfg = config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS-OnA', 'num_epochs.eval=2', 'eval_online_adapt.num_epochs=1',
                            'eval_online_adapt.step=2'])
    frames, gt = synthetic.synthetic_frames(1, *SMALL, seed=3)
    seq = torch.cat([torch.roll(frames, shifts=4 * i, dims=3) for i in range(4)]).to(DEV)
    with monkeypatch.context() as mp:
        def no_zoom(*a, **k):
            raise AssertionError('a zoom call on the plain path')
        for name in ('zoom_boxes', 'zoom_crop', 'zoom_accumulate', 'zoom_blend'):
            mp.setattr(Engine, name, no_zoom)
        outs = [evaluate_sequence(model, mo, msd, seq, [gt[0]], cfg, **kw) for kw in ({}, {'zoom': None}, {'zoom': {'max_zoom': 0}})]
    for labels, probs, hist in outs[1:]:
        assert torch.equal(labels, outs[0][0]) and hist == outs[0][2]
        assert torch.equal(_bits(probs[0]), _bits(outs[0][1][0]))
    # frame 1 is the first frame inferred, after the same fine-tuning: its first pass is the plain run's
    Z = _zoom_at_least_2(outs[0][1][0][1:2].unsqueeze(1), {'max_zoom': 4, 'min_zoom': 1.5, 'min_pixels': 1, 'margin': 0.25,
                                                          'margin_px': 2, 'weight': 0.5, 'feather': 4})
    on = evaluate_sequence(model, mo, msd, seq, [gt[0]], cfg, zoom=Z)
    assert on[1][0].shape == outs[0][1][0].shape and torch.equal(_bits(on[1][0][0]), _bits(outs[0][1][0][0]))     # the train frame
    assert not torch.equal(on[1][0][1], outs[0][1][0][1])
    assert bool(torch.isfinite(on[1][0]).all())
    mo.reset()


# ---- 6. bad arguments ---------------------------------------------------------------------------------------------------
def test_bad_arguments_return_errors_without_launching():
    eng = _engine(*SMALL)
    lib, h = eng.lib, eng.h
    H, W = SMALL
    x = synthetic.synthetic_frames(1, *SMALL, seed=5)[0].to(DEV)
    eng.infer_view(x)
    probs = torch.full((1, 1, H, W), 0.75, device=DEV)
    pz = torch.full((1, 1, H, W), SENTINEL, device=DEV)
    out = torch.full((1, 3, H, W), SENTINEL, device=DEV)
    boxes = torch.full((1, 5), 77, dtype=torch.int32, device=DEV)
    good = _dev_boxes([(1, 0, 0, 32, 54)])
    P = lambda t: ctypes.c_void_p(t.data_ptr())                        # noqa: E731
    Q = 65536
    zb = lambda **k: lib.eosvos_zoom_boxes(*[k.get(n, d) for n, d in (                               # noqa: E731
        ('e', h), ('probs', P(probs)), ('n', 1), ('H', H), ('W', W), ('thr', 0.5), ('minpix', 16), ('margin', Q // 2), ('px', 8),
        ('minz', 3 * Q // 2), ('maxz', 3 * Q), ('boxes', P(boxes)))])
    bad = [
        lambda: zb(e=None), lambda: zb(probs=None), lambda: zb(boxes=None), lambda: zb(n=0), lambda: zb(n=65536), lambda: zb(H=0),
        lambda: zb(W=0), lambda: zb(H=4097), lambda: zb(W=4097), lambda: zb(thr=0.0), lambda: zb(thr=1.0), lambda: zb(thr=float('nan')),
        lambda: zb(minpix=0), lambda: zb(margin=-1), lambda: zb(margin=4 * Q + 1), lambda: zb(px=-1), lambda: zb(px=257),
        lambda: zb(maxz=Q - 1), lambda: zb(maxz=4 * Q + 1), lambda: zb(minz=Q - 1), lambda: zb(minz=3 * Q + 1),
        lambda: lib.eosvos_zoom_crop(None, P(x), P(good), 1, 3, H, W, P(out)),
        lambda: lib.eosvos_zoom_crop(h, None, P(good), 1, 3, H, W, P(out)),
        lambda: lib.eosvos_zoom_crop(h, P(x), None, 1, 3, H, W, P(out)),
        lambda: lib.eosvos_zoom_crop(h, P(x), P(good), 1, 3, H, W, None),
        lambda: lib.eosvos_zoom_crop(h, P(x), P(good), 0, 3, H, W, P(out)),
        lambda: lib.eosvos_zoom_crop(h, P(x), P(good), 1, 0, H, W, P(out)),
        lambda: lib.eosvos_zoom_crop(h, P(x), P(good), 1, 3, 0, W, P(out)),
        lambda: lib.eosvos_zoom_crop(h, P(x), P(good), 1, 3, H, 4097, P(out)),
        lambda: lib.eosvos_zoom_accumulate(None, P(good), 1, 0, 1.0, 1, P(pz)),
        lambda: lib.eosvos_zoom_accumulate(h, None, 1, 0, 1.0, 1, P(pz)),
        lambda: lib.eosvos_zoom_accumulate(h, P(good), 1, 0, 1.0, 1, None),
        lambda: lib.eosvos_zoom_accumulate(h, P(good), 0, 0, 1.0, 1, P(pz)),
        lambda: lib.eosvos_zoom_accumulate(h, P(good), eng.max_batch + 1, 0, 1.0, 1, P(pz)),
        lambda: lib.eosvos_zoom_accumulate(h, P(good), 1, 0, float('nan'), 1, P(pz)),
        lambda: lib.eosvos_zoom_accumulate(h, P(good), 1, 0, float('inf'), 1, P(pz)),
        lambda: lib.eosvos_zoom_blend(None, P(good), 1, H, W, 0.5, 8, P(pz), P(probs)),
        lambda: lib.eosvos_zoom_blend(h, None, 1, H, W, 0.5, 8, P(pz), P(probs)),
        lambda: lib.eosvos_zoom_blend(h, P(good), 1, H, W, 0.5, 8, None, P(probs)),
        lambda: lib.eosvos_zoom_blend(h, P(good), 1, H, W, 0.5, 8, P(pz), None),
        lambda: lib.eosvos_zoom_blend(h, P(good), 0, H, W, 0.5, 8, P(pz), P(probs)),
        lambda: lib.eosvos_zoom_blend(h, P(good), 1, 0, W, 0.5, 8, P(pz), P(probs)),
        lambda: lib.eosvos_zoom_blend(h, P(good), 1, H, 4097, 0.5, 8, P(pz), P(probs)),
        lambda: lib.eosvos_zoom_blend(h, P(good), 1, H, W, 0.0, 8, P(pz), P(probs)),
        lambda: lib.eosvos_zoom_blend(h, P(good), 1, H, W, 1.5, 8, P(pz), P(probs)),
        lambda: lib.eosvos_zoom_blend(h, P(good), 1, H, W, float('nan'), 8, P(pz), P(probs)),
        lambda: lib.eosvos_zoom_blend(h, P(good), 1, H, W, 0.5, -1, P(pz), P(probs)),
        lambda: lib.eosvos_zoom_blend(h, P(good), 1, H, W, 0.5, 65, P(pz), P(probs)),
    ]
    for i, call in enumerate(bad):
        assert call() == 1, i
        assert lib.eosvos_last_error().decode(), i
    torch.cuda.synchronize()
    assert bool((probs == 0.75).all()) and bool((pz == SENTINEL).all()) and bool((out == SENTINEL).all())       # nothing was written
    assert bool((boxes == 77).all())
    with pytest.raises(_ffi.EosvosError):
        _ffi.check(zb(n=0))
    for call in (lambda: eng.zoom_boxes(probs, {'max_zoom': 0}), lambda: eng.zoom_boxes(probs.cpu(), {'max_zoom': 3}),
                 lambda: eng.zoom_boxes(probs, {'max_zoom': 5}), lambda: eng.zoom_crop(x, boxes.long()),
                 lambda: eng.zoom_accumulate(good, pz[:, :, :-1].contiguous(), 1.0),
                 lambda: eng.zoom_blend(good, pz, probs[:, :, 1:].contiguous(), 0.5, 8)):
        with pytest.raises(ValueError):
            call()
