"""Local dense-CRF refinement on the MI355X (`eosvos_crf_labels`, csrc/crf_kernels.hip), all through the C-ABI, against the
torch twin `eosvos_amd.crf.refine_host` in fp64.  Needs an MI355X: pytest -m gpu.

Tolerances are not fixed numbers.  Per case, err32 is the largest difference between `refine_host` evaluated in fp32 and in
fp64 on the CPU; the device is allowed 4 x err32 -- 4, not the 2 of tests/test_gpu_tta.py, because the kernel adds up to 224
neighbour terms in another order than torch and uses another exp.  Every case prints both (`pytest -s`; tools/crf_time.py
records them in profiles/crf_time.txt)."""
import ctypes
import functools
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

import crf_ref  # noqa: E402

from eosvos_amd import _ffi, crf, synthetic  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# (H, W, n_obj, radius, dilation): small windows, the default window, more labels than one LDS chunk of 4, a window larger than
# the frame, a frame without any neighbour, and halo 16 with label chunks of 3 at sizes that are no multiple of the 32 x 8 tile
CASES = [(37, 53, 3, 2, 1), (48, 64, 2, 3, 2), (40, 70, 1, 5, 2), (33, 65, 5, 1, 3), (7, 9, 2, 5, 2), (2, 2, 1, 2, 2),
         (97, 163, 9, 4, 4)]
ITERS = [5, 1]


def P(**kw):
    return dict(crf.DEFAULTS, **kw)


@pytest.fixture(scope='module')
def eng():
    e = Engine('resnet50', 96, 160, max_batch=1, device=DEV)        # lends its stream and scratch; frames are of any size
    yield e
    e.close()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def abi(eng, images, probs, params, want_q=True):
    """`eosvos_crf_labels` as it is: device tensors in, (labels, Q^T or None) out."""
    n, n_obj, h, w = probs.shape
    labels = torch.full((n, h, w), 255, dtype=torch.uint8, device=DEV)
    q = torch.full((n, n_obj + 1, h, w), -7.0, device=DEV) if want_q else None
    p = crf.check(params)
    _ffi.check(eng.lib.eosvos_crf_labels(eng.h, _ptr(images), _ptr(probs), n, n_obj, h, w, p['iterations'], p['radius'],
                                         p['dilation'], p['w_appearance'], p['w_smooth'], p['theta_alpha'], p['theta_beta'],
                                         p['theta_gamma'], _ptr(labels), _ptr(q)))
    eng.synchronize()
    return labels, q


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def special_probs(n_obj, h, w, seed):
    """Random probabilities with the threshold itself, the seeded 2 * GT and exact ties between objects written in."""
    probs = torch.rand(2, n_obj, h, w, generator=torch.Generator().manual_seed(seed))
    probs[0, :, 0, :9] = 0.5
    probs[0, 0, 1, :9] = 0.5
    probs[0, :, 2, :9] = 2.0
    probs[0, -1, 3, :9] = 2.0
    probs[1, :, 4, :] = probs[1, 0, 4, :].clone()
    probs[1, :, 5, :9] = 0.49999997
    probs[1, :, 6, :9] = 0.0
    return probs


@functools.lru_cache(maxsize=None)
def case(h, w, n_obj, r, d, T, n_frames=1):
    """(images, probs, parameters, fp64 labels, fp64 Q, err32) of one case; computed once, never changed."""
    images, probs = crf_ref.scene(h, w, n_obj, seed=100 + h + w + n_obj, n_frames=n_frames)
    params = P(iterations=T, radius=r, dilation=d)
    lab64, q64 = crf.refine_host(images, probs, params, dtype=torch.float64)
    _, q32 = crf.refine_host(images, probs, params, dtype=torch.float32)
    return images, probs, params, lab64, q64, float((q32.double() - q64).abs().max())


# ---- 1. zero iterations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_obj', [1, 3])
@pytest.mark.parametrize('h,w', [(33, 65), (97, 163)])
def test_zero_iterations_is_merge_labels_bit_for_bit(eng, h, w, n_obj):
    probs = special_probs(n_obj, h, w, seed=h + n_obj).to(DEV)
    images = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(1)).to(DEV)
    want = torch.stack([eng.merge_labels(probs[f]) for f in range(2)])
    labels, q = abi(eng, images, probs, P(iterations=0))
    assert torch.equal(labels, want)
    assert torch.equal(abi(eng, images, probs, P(iterations=0), want_q=False)[0], want)
    _, q64 = crf.refine_host(images.cpu(), probs.cpu(), P(iterations=0))
    # Q^0 = s_l / sum(s) <= 1: 1 - m, the n_obj additions of the sum and the division round once each, half an ulp = 2^-24 relative
    assert float((q.cpu().double() - q64).abs().max()) <= (n_obj + 2) * 2.0 ** -24


# ---- 2. / 3. Q^T and the labels against fp64 ----------------------------------------------------------------------------
@pytest.mark.parametrize('T', ITERS)
@pytest.mark.parametrize('h,w,n_obj,r,d', CASES)
def test_q_against_fp64(eng, h, w, n_obj, r, d, T):
    images, probs, params, _, q64, err32 = case(h, w, n_obj, r, d, T)
    _, q = abi(eng, images.to(DEV), probs.to(DEV), params)
    got = float((q.cpu().double() - q64).abs().max())
    print(f'crf Q {h}x{w} n_obj={n_obj} r={r} d={d} T={T}: torch fp32 error {err32:.3e}, kernel error {got:.3e}, '
          f'allowed {4 * err32:.3e}')
    assert err32 > 0
    assert got <= 4 * err32


@pytest.mark.parametrize('T', ITERS)
@pytest.mark.parametrize('h,w,n_obj,r,d', CASES)
def test_labels_against_fp64(eng, h, w, n_obj, r, d, T):
    images, probs, params, lab64, q64, err32 = case(h, w, n_obj, r, d, T)
    labels, _ = abi(eng, images.to(DEV), probs.to(DEV), params)
    top = q64.topk(2, dim=1).values
    close = (top[:, 0] - top[:, 1]) < 2 * (4 * err32)               # the two largest fp64 values within twice test 2's tolerance
    frac = float(close.double().mean())
    print(f'crf labels {h}x{w} n_obj={n_obj} r={r} d={d} T={T}: {frac:.4%} of the pixels undecided in fp64')
    assert frac <= 0.001
    assert torch.equal(labels.cpu()[~close], lab64[~close])


def test_frames_of_one_call_are_independent(eng):
    images, probs, params, lab64, q64, err32 = case(48, 64, 2, 3, 2, 5, n_frames=3)
    labels, q = abi(eng, images.to(DEV), probs.to(DEV), params)
    assert float((q.cpu().double() - q64).abs().max()) <= 4 * err32
    for f in range(3):
        one_l, one_q = abi(eng, images[f:f + 1].to(DEV), probs[f:f + 1].to(DEV), params)
        assert torch.equal(one_l[0], labels[f]) and torch.equal(_bits(one_q[0]), _bits(q[f]))
    assert not torch.equal(labels[0], labels[1])


# ---- 4. determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,n_obj,r,d', [(48, 64, 2, 3, 2), (97, 163, 9, 4, 4)])
def test_two_calls_give_identical_bits(eng, h, w, n_obj, r, d):
    images, probs, params = case(h, w, n_obj, r, d, 5)[:3]
    a = abi(eng, images.to(DEV), probs.to(DEV), params)
    b = abi(eng, images.to(DEV), probs.to(DEV), params)
    assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert torch.equal(abi(eng, images.to(DEV), probs.to(DEV), params, want_q=False)[0], a[0])     # q_out = NULL: the same labels


# ---- 5. it does something -----------------------------------------------------------------------------------------------
def test_refinement_moves_more_than_one_percent_of_the_labels(eng):
    images, probs, params = case(48, 64, 2, 3, 2, 5)[:3]
    labels, _ = abi(eng, images.to(DEV), probs.to(DEV), params)
    plain = eng.merge_labels(probs[0].to(DEV))
    moved = float((labels[0] != plain).float().mean())
    print(f'crf 48x64 n_obj=2 r=3 d=2 T=5: {moved:.2%} of the labels differ from merge_labels')
    assert moved > 0.01


# ---- 6. rejections ------------------------------------------------------------------------------------------------------
def test_rejections_launch_nothing_and_leave_the_engine_usable(eng):
    images, probs, params, lab64 = case(48, 64, 2, 3, 2, 5)[:4]
    xi, xp = images.to(DEV), probs.to(DEV)
    labels = torch.full((1, 48, 64), 255, dtype=torch.uint8, device=DEV)
    q = torch.full((1, 3, 48, 64), -7.0, device=DEV)
    lib, h = eng.lib, eng.h
    nan, inf = float('nan'), float('inf')

    def call(e=h, im=xi, pr=xp, n=1, n_obj=2, H=48, W=64, T=5, r=3, d=2, wa=10.0, ws=3.0, ta=8.0, tb=0.05, tg=3.0, lab=labels):
        return lib.eosvos_crf_labels(e, _ptr(im), _ptr(pr), n, n_obj, H, W, T, r, d, wa, ws, ta, tb, tg, _ptr(lab), _ptr(q))
    bad = [dict(T=-1), dict(T=21), dict(r=0), dict(r=8), dict(d=0), dict(d=5), dict(r=6, d=3), dict(r=5, d=4),
           dict(wa=-1.0), dict(ws=-0.5), dict(wa=nan), dict(ws=inf), dict(ta=0.0), dict(tb=-0.05), dict(tg=0.0), dict(ta=nan),
           dict(tb=inf), dict(tg=nan), dict(n_obj=0), dict(n_obj=256), dict(e=None), dict(im=None), dict(pr=None),
           dict(lab=None), dict(H=0), dict(W=0), dict(n=-1)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert lib.eosvos_last_error().decode().startswith('crf_labels'), kw
    eng.synchronize()
    assert bool((labels == 255).all()) and bool((q == -7.0).all())                # nothing was written
    assert call() == 0                                                            # a valid call right after succeeds
    eng.synchronize()
    assert torch.equal(labels.cpu(), lab64)
    with pytest.raises(_ffi.EosvosError, match='crf_labels'):
        _ffi.check(call(r=0))
    # one call may take 512 MB of scratch: more is reported before any launch, and the engine goes on
    big_i, big_p = torch.zeros(1, 3, 1024, 1024, device=DEV), torch.zeros(1, 63, 1024, 1024, device=DEV)
    big_l = torch.full((1, 1024, 1024), 255, dtype=torch.uint8, device=DEV)
    assert lib.eosvos_crf_labels(h, _ptr(big_i), _ptr(big_p), 1, 63, 1024, 1024, 1, 1, 1, 10.0, 3.0, 8.0, 0.05, 3.0, _ptr(big_l), None) != 0
    assert b'512 MB' in lib.eosvos_last_error()
    eng.synchronize()
    assert bool((big_l == 255).all())
    assert torch.equal(abi(eng, xi, xp, params)[0].cpu(), lab64)
    with pytest.raises(ValueError):
        eng.crf_labels(xi, xp, radius=9)
    with pytest.raises(ValueError):
        eng.crf_labels(xi, xp[:, :, :40])


# ---- 7. NaN -------------------------------------------------------------------------------------------------------------
def test_a_nan_probability_stays_inside_its_window(eng):
    images, probs, params = case(48, 64, 2, 3, 2, 1)[:3]
    clean_l, clean_q = abi(eng, images.to(DEV), probs.to(DEV), params)
    dirty = probs.clone()
    dirty[0, 1, 20, 30] = float('nan')
    lab, q = abi(eng, images.to(DEV), dirty.to(DEV), params)
    outside = torch.ones(48, 64, dtype=torch.bool)
    outside[20 - 6:20 + 7, 30 - 6:30 + 7] = False                   # the window: radius 3 x dilation 2 around the pixel
    assert torch.equal(_bits(q[0][:, outside.to(DEV)]), _bits(clean_q[0][:, outside.to(DEV)]))
    assert torch.equal(lab[0][outside.to(DEV)], clean_l[0][outside.to(DEV)])
    assert not torch.equal(_bits(q), _bits(clean_q))                 # (the NaN did arrive)


CHILD = r'''
import hashlib, json, sys
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from eosvos_amd.engine import Engine
import test_gpu_crf as T
eng = Engine('resnet50', 96, 160, max_batch=1, device='cuda:0')
out = {}
for c in ((48, 64, 2, 3, 2), (33, 65, 5, 1, 3), (7, 9, 2, 5, 2)):
    images, probs = T.crf_ref.scene(*c[:3], seed=100 + c[0] + c[1] + c[2])
    lab, q = T.abi(eng, images.cuda(), probs.cuda(), T.P(iterations=2, radius=c[3], dilation=c[4]))
    out[str(c)] = [hashlib.sha256(lab.cpu().numpy().tobytes()).hexdigest(), hashlib.sha256(q.cpu().numpy().tobytes()).hexdigest()]
eng.close()
print(json.dumps(out))
'''


def test_nan_filled_buffers_give_the_same_bits():
    """The same calls in a process whose engine buffers (the CRF scratch included) start out as NaN words, and in one that
    gets the allocator's pages as they come: a kernel that reads a slot nothing wrote would differ."""
    res = []
    for fill in (None, '7fc00000'):
        env = dict(os.environ, EOSVOS_MODE_GUARD='0')
        env.pop('EOSVOS_DEBUG_FILL', None)
        if fill:
            env['EOSVOS_DEBUG_FILL'] = fill
        p = subprocess.run([sys.executable, '-c', CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
        assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        res.append(json.loads(lines[-1]))
    assert res[0] == res[1], res


# ---- 8. end to end ------------------------------------------------------------------------------------------------------
BN_CFG = {'accum_stats': False, 'learn_weight': False, 'learn_bias': False}
MO_CFG = dict(init_lr=1e-3, learn_model_init=True, second_order_gradients=False, lr_hierarchy_level='NEURON',
              use_log_init_lr=False, max_lr=None)


def test_evaluate_sequence_with_crf(monkeypatch):
    from eosvos_amd import config, topology
    from eosvos_amd.evaluate import evaluate_sequence
    from eosvos_amd.helper_func import init_parent_model
    from eosvos_amd.meta_optim import MetaOptimizer
    model, _ = init_parent_model(architecture='DeepLabV3Plus', encoder='resnet50', train_encoder=True,
                                 decoder_norm_layer='BatchNorm2d', replace_batch_with_group_norms=False, batch_norm=BN_CFG,
                                 roi_pool_output_sizes=None, eval_augment_rpn_proposals_mode=None, box_nms_thresh=None,
                                 maskrcnn_loss=None)
    sd = synthetic.synthetic_state('resnet50')
    msd = {}
    for (n, _), lr in zip(topology.trainable('resnet50'), synthetic.synthetic_lrs('resnet50')):
        msd['log_init_lr_' + n.replace('.', '-')] = lr.clone()
    for n, _ in topology.trainable('resnet50'):
        msd['model_init_' + n.replace('.', '-')] = sd[n].clone()
    model.load_state_dict(sd)
    mo = MetaOptimizer(model, **MO_CFG)
    try:
        cfg = config.parse_cli(['num_epochs.eval=2'])
        frames, gt = synthetic.synthetic_frames(1, 96, 160, seed=3)
        seq = torch.cat([torch.roll(frames, shifts=4 * i, dims=3) for i in range(4)]).to(DEV)
        gts = [gt[0], 1.0 - gt[0]]
        today = evaluate_sequence(model, mo, msd, seq, gts, cfg)
        fp = model.engine.plan_fingerprint()
        with monkeypatch.context() as mp:
            def no_crf(*a, **k):
                raise AssertionError('a CRF call on the plain path')
            mp.setattr(Engine, 'crf_labels', no_crf)
            for kw in ({'crf': None}, {'crf': P(iterations=0)}):
                off = evaluate_sequence(model, mo, msd, seq, gts, cfg, **kw)
                assert torch.equal(off[0], today[0]) and off[2] == today[2]
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(off[1], today[1]))
        on = evaluate_sequence(model, mo, msd, seq, gts, cfg, crf=crf.DEFAULTS)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(on[1], today[1]))
        assert model.engine.plan_fingerprint() == fp                # no matrix kernel: the conv plans did not move
        stack = torch.stack(on[1], dim=1)
        want = model.engine.crf_labels(seq, stack, **crf.DEFAULTS)
        assert on[0].dtype == torch.uint8 and on[0].shape == (4, 96, 160)
        assert torch.equal(on[0][1:], want[1:])
        assert torch.equal(on[0][0], model.engine.merge_labels(stack[0])) and torch.equal(on[0][0], today[0][0])
    finally:
        model.close_engines()
