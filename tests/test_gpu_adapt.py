"""The distance gate of online adaptation on the MI355X (`eosvos_amd/adapt.py`, csrc/edt_kernels.hip): `Engine.distance_sq` and
`Engine.adapt_targets` against the numpy twins bit for bit (the twins are held to plain loops by tests/test_adapt_host.py), the
independence from what scratch and outputs held before, the C entries' refusals, and `finetune_object` with `adapt=`.
Needs an MI355X: pytest -m gpu.

Everything here is integers (and targets out of {0, 1, ignore}): every comparison is exact.  The shapes are the smallest at
which the kernels can go wrong: one pixel, one row, one column, rows narrower and wider than the 256-thread row tile (300: more
than one pass, no multiple of 4 or 64), several frames per call."""
import ctypes

import numpy as np
import pytest
import torch

import adapt_ref as R
from eosvos_amd import adapt, synthetic
from eosvos_amd.engine import Engine

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SMALL = (96, 160)
SIZES = [(1, 1), (1, 70), (70, 1), (17, 241), (33, 65), (67, 130), (97, 300)]
LIMITS = [1, 2, 7, 64, 400]
GROUPS = [R.PATTERNS[i:i + 3] for i in range(0, 9, 3)] + [R.PATTERNS[8:11]]     # 3 frames per call, every pattern in one


@pytest.fixture(scope='module')
def eng():
    e = Engine('resnet50', *SMALL, max_batch=1, device=DEV)                      # the entries are not tied to its frame size
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def frames_of(group, h, w):
    return np.stack([R.pattern(name, h, w) for name in group])


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def fill_scratch(e, byte=0xFF):
    """Every byte of the engine's grow-only scratch becomes `byte`."""
    p, dims = ctypes.c_void_p(), (ctypes.c_int64 * 4)()
    assert e.lib.eosvos_debug_tensor(e.h, b'ccl_scratch', ctypes.byref(p), dims) == 0
    assert p.value and dims[3] > 0
    e.synchronize()
    assert ctypes.CDLL('libamdhip64.so').hipMemset(p, byte, ctypes.c_size_t(dims[3] * 4)) == 0
    assert ctypes.CDLL('libamdhip64.so').hipDeviceSynchronize() == 0


# ---- rule 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('invert', [False, True], ids=['ge', 'not_ge'])
@pytest.mark.parametrize('hw', SIZES, ids=[f'{h}x{w}' for h, w in SIZES])
def test_distance_sq_equals_the_twin(eng, hw, invert):
    for group in GROUPS:
        p = frames_of(group, *hw)
        with np.errstate(invalid='ignore'):
            ge = p >= np.float32(R.T)
        seeds = ~ge if invert else ge
        pd = dev(p)
        for limit in LIMITS:
            got = eng.distance_sq(pd, R.T, invert=invert, limit=limit)
            assert got.dtype == torch.int32 and got.shape == pd.shape
            assert np.array_equal(got.cpu().numpy().astype(np.int64), adapt.distance_sq_host(seeds, limit)), (group, limit)
    one = eng.distance_sq(pd[:1, None], R.T, invert=invert, limit=7)          # (N, 1, H, W) keeps its shape
    assert one.shape == (1, 1) + tuple(hw) and torch.equal(one[0, 0], eng.distance_sq(pd[:1], R.T, invert=invert, limit=7)[0])


def test_distance_sq_does_not_depend_on_what_the_buffers_held(eng):
    """The C entry into an output and a scratch that hold 0xFF bytes, after calls of other sizes and limits used both."""
    h, w = 97, 300
    p = frames_of(('blobs', 'sparse', 'nans'), h, w)
    pd = dev(p)
    for limit, invert in ((400, False), (7, True)):
        first = eng.distance_sq(pd, R.T, invert=invert, limit=limit)
        eng.distance_sq(dev(frames_of(('full', 'empty', 'centre'), 67, 130)), R.T, limit=64)
        fill_scratch(eng)
        out = torch.full((3, h, w), -1, dtype=torch.int32, device=DEV)         # 0xFF bytes
        assert eng.lib.eosvos_distance_sq(eng.h, ptr(pd), 3, h, w, R.T, int(invert), limit, ptr(out)) == 0
        assert torch.equal(out, first)
        with np.errstate(invalid='ignore'):
            ge = p >= np.float32(R.T)
        assert np.array_equal(out.cpu().numpy().astype(np.int64), adapt.distance_sq_host(~ge if invert else ge, limit))


# ---- rules 2-6 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nans', [False, True], ids=['finite', 'nans'])
@pytest.mark.parametrize('band', [(0.0, 0.5), (0.3, 0.7)], ids=['scalar', 'band'])
@pytest.mark.parametrize('neg', [5, 40])
@pytest.mark.parametrize('erode', [0, 3])
def test_adapt_targets_equals_the_twin(eng, erode, neg, band, nans):
    prm = {'neg_dist': neg, 'erode': erode}
    total = 0
    for h, w in ((67, 130), (97, 300)):
        probs, anchors = R.three_frames(h, w, nans)
        want, n_want = adapt.targets_host(probs, anchors, band[0], band[1], prm, R.IGN)
        got, n_got = eng.adapt_targets(dev(probs), dev(anchors), band[0], band[1], prm, R.IGN)
        assert got.shape == (3, h, w) and np.array_equal(bits(got), bits(want))
        assert n_got == n_want.tolist() and n_want[1] == 0
        total += sum(n_got)
        assert np.array_equal(bits(got[1]), bits(R.band_rule(probs[1], *band)))    # no anchor: the base rule's map
        # into targets and a scratch that hold 0xFF bytes, no host read: the same bits
        fill_scratch(eng)
        out = torch.full((3, 1, h, w), float('nan'), device=DEV)
        out.view(torch.int32).fill_(-1)
        again, none = eng.adapt_targets(dev(probs)[:, None], dev(anchors)[:, None], band[0], band[1], prm, R.IGN, counts=False)
        assert none is None and again.shape == (3, 1, h, w) and np.array_equal(bits(again[:, 0]), bits(want))
        assert eng.lib.eosvos_adapt_targets(eng.h, ptr(dev(probs)), ptr(dev(anchors)), 3, h, w, band[0], band[1], band[1], erode, neg,
                                            R.IGN, ptr(out), None) == 0
        assert np.array_equal(bits(out[:, 0]), bits(want))
    assert total > 0                                                           # the case has positives to count


def test_adapt_targets_far_blob_and_lost_anchor(eng):
    """The case the stage exists for, at a size the row pass takes in two tiles: the look-alike becomes 0, the object stays 1;
    an anchor that erosion removes leaves count 0 and the band's map."""
    h, w = 40, 300
    probs = np.full((2, h, w), 0.1, dtype=np.float32)
    probs[:, 10:30, 20:60] = 0.95
    probs[:, 12:20, 270:290] = 0.95
    anchors = np.zeros((2, h, w), dtype=np.float32)
    anchors[0, 10:30, 16:56] = 1
    anchors[1, 10:13, 16:56] = 1                     # three rows: gone under erode 2
    prm = {'neg_dist': 30, 'erode': 2}
    got, n = eng.adapt_targets(dev(probs), dev(anchors), 0.3, 0.7, prm, R.IGN)
    want, n_want = adapt.targets_host(probs, anchors, 0.3, 0.7, prm, R.IGN)
    assert np.array_equal(bits(got), bits(want)) and n == n_want.tolist() == [800, 0]
    g = got.cpu().numpy()
    assert (g[0, 10:30, 20:60] == 1).all() and (g[0, 12:20, 270:290] == 0).all() and (g[1, 12:20, 270:290] == 1).all()


# ---- the C entries' refusals ------------------------------------------------------------------------------------------------
NAN = float('nan')
BAD_DISTANCE = {  # (n_frames, h, w, threshold, invert, limit)
    'no frame': (0, 4, 6, 0.5, 0, 3), 'too many frames': (65536, 4, 6, 0.5, 0, 3), 'height 0': (1, 0, 6, 0.5, 0, 3),
    'width 0': (1, 4, 0, 0.5, 0, 3), 'height 4097': (1, 4097, 6, 0.5, 0, 3), 'width 4097': (1, 4, 4097, 0.5, 0, 3),
    'limit 0': (1, 4, 6, 0.5, 0, 0), 'limit -1': (1, 4, 6, 0.5, 1, -1), 'limit 4096': (1, 4, 6, 0.5, 0, 4096), 'NaN threshold': (1, 4, 6, NAN, 0, 3),
}
BAD_TARGETS = {  # (n_frames, h, w, lo, hi, anchor_thr, erode, neg_dist, ignore)
    'no frame': (0, 4, 6, 0.3, 0.7, 0.7, 0, 3, 255.0), 'too many frames': (65536, 4, 6, 0.3, 0.7, 0.7, 0, 3, 255.0),
    'height 0': (1, 0, 6, 0.3, 0.7, 0.7, 0, 3, 255.0), 'width 4097': (1, 4, 4097, 0.3, 0.7, 0.7, 0, 3, 255.0),
    'neg_dist 0': (1, 4, 6, 0.3, 0.7, 0.7, 0, 0, 255.0), 'neg_dist 4096': (1, 4, 6, 0.3, 0.7, 0.7, 0, 4096, 255.0),
    'erode -1': (1, 4, 6, 0.3, 0.7, 0.7, -1, 3, 255.0), 'erode 256': (1, 4, 6, 0.3, 0.7, 0.7, 256, 3, 255.0),
    'lo > hi': (1, 4, 6, 0.7, 0.3, 0.7, 0, 3, 255.0), 'lo == hi': (1, 4, 6, 0.5, 0.5, 0.5, 0, 3, 255.0),
    'lo < 0': (1, 4, 6, -0.1, 0.5, 0.5, 0, 3, 255.0), 'hi > 1': (1, 4, 6, 0.5, 1.5, 0.5, 0, 3, 255.0), 'NaN lo': (1, 4, 6, NAN, 0.5, 0.5, 0, 3, 255.0),
    'NaN hi': (1, 4, 6, 0.3, NAN, 0.5, 0, 3, 255.0), 'NaN anchor threshold': (1, 4, 6, 0.3, 0.7, NAN, 0, 3, 255.0),
    'ignore 0.5': (1, 4, 6, 0.3, 0.7, 0.7, 0, 3, 0.5), 'ignore 1': (1, 4, 6, 0.3, 0.7, 0.7, 0, 3, 1.0), 'NaN ignore': (1, 4, 6, 0.3, 0.7, 0.7, 0, 3, NAN),
    'inf ignore': (1, 4, 6, 0.3, 0.7, 0.7, 0, 3, float('inf')),
}


@pytest.mark.parametrize('name', list(BAD_DISTANCE))
def test_distance_sq_refuses_bad_arguments(eng, name):
    n, h, w, thr, inv, limit = BAD_DISTANCE[name]
    p = torch.full((4, 6), 0.9, device=DEV)
    out = torch.full((4, 6), -7, dtype=torch.int32, device=DEV)
    assert eng.lib.eosvos_distance_sq(eng.h, ptr(p), n, h, w, thr, inv, limit, ptr(out)) != 0
    assert b'distance_sq' in eng.lib.eosvos_last_error()
    eng.synchronize()
    assert bool((out == -7).all())


def test_null_pointers_are_refused(eng):
    p = torch.full((4, 6), 0.9, device=DEV)
    out = torch.full((4, 6), -7, dtype=torch.int32, device=DEV)
    tgt = torch.full((4, 6), -7.0, device=DEV)
    assert eng.lib.eosvos_distance_sq(eng.h, None, 1, 4, 6, 0.5, 0, 3, ptr(out)) != 0
    assert eng.lib.eosvos_distance_sq(eng.h, ptr(p), 1, 4, 6, 0.5, 0, 3, None) != 0
    assert eng.lib.eosvos_distance_sq(None, ptr(p), 1, 4, 6, 0.5, 0, 3, ptr(out)) != 0
    for probs, anchors, targets in ((None, ptr(p), ptr(tgt)), (ptr(p), None, ptr(tgt)), (ptr(p), ptr(p), None)):
        assert eng.lib.eosvos_adapt_targets(eng.h, probs, anchors, 1, 4, 6, 0.3, 0.7, 0.7, 0, 3, 255.0, targets, None) != 0
    eng.synchronize()
    assert bool((out == -7).all()) and bool((tgt == -7).all())


@pytest.mark.parametrize('name', list(BAD_TARGETS))
def test_adapt_targets_refuses_bad_arguments(eng, name):
    n, h, w, lo, hi, thr, erode, neg, ign = BAD_TARGETS[name]
    p = torch.full((4, 6), 0.9, device=DEV)
    out = torch.full((4, 6), -7.0, device=DEV)
    counts = (ctypes.c_int64 * 1)(-7)
    assert eng.lib.eosvos_adapt_targets(eng.h, ptr(p), ptr(p), n, h, w, lo, hi, thr, erode, neg, ign, ptr(out), counts) != 0
    assert eng.lib.eosvos_last_error()
    eng.synchronize()
    assert bool((out == -7).all()) and counts[0] == -7


def test_the_wrappers_raise_before_the_library(eng):
    p = torch.full((1, 4, 6), 0.9, device=DEV)
    for kw in (dict(limit=0), dict(limit=4096), dict(limit=2.0)):
        with pytest.raises(ValueError):
            eng.distance_sq(p, 0.5, **kw)
    with pytest.raises(ValueError):
        eng.distance_sq(p, NAN)
    with pytest.raises(ValueError):
        eng.distance_sq(p.cpu(), 0.5)
    with pytest.raises(ValueError):
        eng.distance_sq(p[0, 0], 0.5)
    for args in ((0.7, 0.3, {'neg_dist': 3}, 255.0), (0.3, 0.7, {'neg_dist': 0}, 255.0), (0.3, 0.7, {'neg_dist': 3, 'erode': 256}, 255.0),
                 (0.3, 0.7, {'neg_dist': 3}, 0.5)):
        with pytest.raises(ValueError):
            eng.adapt_targets(p, p, *args)
    with pytest.raises(ValueError):
        eng.adapt_targets(p, p[:, :2], 0.3, 0.7, {'neg_dist': 3}, 255.0)


# ---- online adaptation ------------------------------------------------------------------------------------------------------
BN_CFG = {'accum_stats': False, 'learn_weight': False, 'learn_bias': False}
MO_CFG = dict(init_lr=1e-3, learn_model_init=True, second_order_gradients=False, lr_hierarchy_level='NEURON',
              use_log_init_lr=False, max_lr=None)


def test_online_adaptation_with_the_distance_gate(monkeypatch):
    """step 2, 2 + 2 + 2 iterations, 7 frames (two adaptation rounds) on the small engine of test_gpu_loss_ignore.py.  Every
    inferred map is replaced by the object where the ground truth has it plus a confident look-alike far away, so the gate has
    something to reject.  Off (no keyword, None, neg_dist 0): the same bits.  On: round 0 is the same, the later rounds are not."""
    from eosvos_amd import evaluate, topology
    from eosvos_amd.helper_func import init_parent_model
    from eosvos_amd.meta_optim import MetaOptimizer
    model, _ = init_parent_model(architecture='DeepLabV3Plus', encoder='resnet50', train_encoder=True,
                                 decoder_norm_layer='BatchNorm2d', replace_batch_with_group_norms=False, batch_norm=BN_CFG,
                                 roi_pool_output_sizes=None, eval_augment_rpn_proposals_mode=None, box_nms_thresh=None,
                                 maskrcnn_loss=None)
    sd, lrs = synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50')
    msd = {}
    for (n, _), lr in zip(topology.trainable('resnet50'), lrs):
        msd['log_init_lr_' + n.replace('.', '-')] = lr.clone()
    for n, _ in topology.trainable('resnet50'):
        msd['model_init_' + n.replace('.', '-')] = sd[n].clone()
    model.load_state_dict(sd)
    mo = MetaOptimizer(model, **MO_CFG)
    H, W, N = SMALL[0], SMALL[1], 7
    frames, gt = synthetic.synthetic_frames(1, H, W, seed=3)
    seq = torch.cat([torch.roll(frames, shifts=4 * i, dims=3) for i in range(N)]).to(DEV)
    obj = gt[0, 0].numpy() > 0
    prm = {'neg_dist': 12, 'erode': 1}
    d = adapt.distance_sq_host(obj, 60)
    cy, cx = np.unravel_index(int(np.argmax(d)), d.shape)
    y0, x0 = min(max(cy - 4, 0), H - 8), min(max(cx - 4, 0), W - 8)
    assert obj.sum() > 9 and d[y0:y0 + 8, x0:x0 + 8].min() > (prm['neg_dist'] + 1) ** 2      # the look-alike lies beyond the gate
    assert adapt.eroded_host(gt[0, 0].numpy(), 0.5, prm['erode']).any()                      # and erosion leaves an anchor
    planted = torch.full((N, 1, H, W), 0.1)
    planted[:, 0, torch.from_numpy(obj)] = 0.95
    planted[2::2, 0, y0:y0 + 8, x0:x0 + 8] = 0.95                                            # the propagated frames: 2 and 4
    planted = planted.to(DEV)
    real_infer, real_targets, calls = Engine.infer, Engine.adapt_targets, []

    def infer(self, x):
        real_infer(self, x)
        which = [int(torch.nonzero((seq.view(N, -1) == xi.view(1, -1)).all(1))[0]) for xi in x]
        return planted[which].clone()
    monkeypatch.setattr(Engine, 'infer', infer)

    def spy(self, probs, anchors, lo, hi, params, ignore, counts=True):
        out = real_targets(self, probs, anchors, lo, hi, params, ignore, counts)
        calls.append((probs.shape[0], out[1]))
        return out
    monkeypatch.setattr(Engine, 'adapt_targets', spy)
    cfg = {'eval_online_adapt': {'step': 2, 'reset_model_mode': 'FIRST_STEP', 'num_epochs': 2, 'min_prop': 0.5},
           'data_cfg': {'batch_sizes': {'train': 3}, 'random_train_transform': False}, 'num_epochs': {'eval': 2},
           'loss_func': 'cross_entropy', 'seed': 1}
    try:
        for min_prop in (0.5, [0.3, 0.7]):
            cfg['eval_online_adapt']['min_prop'] = min_prop
            base, hist_base = evaluate.finetune_object(model, mo, msd, seq, gt[0], cfg)
            assert [len(h) for h in hist_base] == [2, 2, 2]
            for off in (None, {'neg_dist': 0, 'erode': 3}):
                same, hist_same = evaluate.finetune_object(model, mo, msd, seq, gt[0], cfg, adapt=off)
                assert torch.equal(same, base) and hist_same == hist_base and not calls
            on, hist_on = evaluate.finetune_object(model, mo, msd, seq, gt[0], cfg, adapt=prm)
            assert calls == [(1, [int(obj.sum())])] * 2                    # one call per adaptation round, the look-alike not counted
            calls.clear()
            assert hist_on[0] == hist_base[0] and torch.equal(on, base)     # round 0 knows no gate (and every map is planted)
            assert np.isfinite(np.concatenate(hist_on)).all()
            assert hist_on[1] != hist_base[1] and hist_on[2] != hist_base[2]
    finally:
        if model.engine is not None:
            model.engine.close()
