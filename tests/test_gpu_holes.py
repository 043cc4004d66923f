"""Hole filling on the MI355X (`eosvos_fill_holes`, csrc/ccl_kernels.hip) against the numpy twin of `eosvos_amd/holes.py`.
Integer arithmetic on both sides: every output is compared bit for bit.  Needs an MI355X: pytest -m gpu.

The kernels' tile is 64 wide and 16 high, so the sizes are: 1 x 1, 5 x 7 (inside a tile), 16 x 64 (one tile exactly), 17 x 65
(one pixel over the tile in each direction), 33 x 130 and 97 x 161 (several tiles, no multiple of the tile)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import components_ref  # noqa: E402
import holes_ref as ref  # noqa: E402

from eosvos_amd import _ffi, components, holes, synthetic  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = [(1, 1), (5, 7), (ref.TILE_H, ref.TILE_W), (ref.TILE_H + 1, ref.TILE_W + 1), (33, 130), (97, 161)]
ANY = 1 << 24                          # max_area: no limit beside max_rel_area


def P(**kw):
    return dict(holes.DEFAULTS, **kw)


@pytest.fixture(scope='module')
def eng():
    e = Engine('resnet50', 96, 160, max_batch=1, device=DEV)        # lends its stream and scratch; frames are of any size
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def pattern_case(h, w):
    """(maps (K, H, W), names); computed once, never changed."""
    pats = ref.patterns(h, w)
    return np.stack(list(pats.values())), tuple(pats)


@functools.lru_cache(maxsize=None)
def punched_case(h, w, p):
    """(three punched frames, prev: a punched map of another seed)."""
    return np.stack([ref.punched(h, w, p, seed=10 * k + int(p * 10)) for k in range(3)]), ref.punched(h, w, p, seed=99)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_as_twin(eng, labels, params, prev=None, keep=(), msg=''):
    want, want_filled = holes.fill_host(labels, params, prev=prev, keep=keep, return_filled=True)
    got, filled = eng.fill_holes(dev(labels), prev=None if prev is None else dev(prev), keep=keep, return_filled=True, **params)
    assert got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=msg)
    np.testing.assert_array_equal(filled, want_filled, err_msg=msg)
    return want, want_filled


# ---- patterns -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('h,w', SIZES)
def test_patterns_equal_the_twin(eng, h, w, connectivity):
    maps, names = pattern_case(h, w)
    want, filled = same_as_twin(eng, maps, P(connectivity=connectivity, max_area=ANY))
    same_as_twin(eng, maps, P(connectivity=connectivity, max_area=3))
    count = dict(zip(names, filled))
    k = names.index
    assert count['empty'] == 0 and count['full'] == 0 and np.array_equal(want[k('full')], maps[k('full')])
    if 'ring' in count:
        assert count['ring'] > 0 and bool((want[k('ring')][1:h - 1, 1:w - 1] == 1).all())
        assert count['ring_at_border'] == 0 and count['between_two'] == 0 and count['corridor_open'] == 0
        assert count['corner_leak'] == (3 if connectivity == 8 else 0)
        assert count['corridor'] == int((maps[k('corridor')] == 0).sum()) and bool((want[k('corridor')] == 1).all())
    if 'nested' in count:
        nested = want[k('nested')]
        assert count['nested'] == 1 and nested[5, 5] == 2 and not nested[2, 2:9].any()      # the moat has two labels: it stays
    if 'seam_xy' in count:
        assert (count['seam_x'], count['seam_y'], count['seam_xy']) == (4, 8, 16)


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('p', [0.1, 0.3, 0.5])
@pytest.mark.parametrize('h,w', [(33, 130), (97, 161)])
def test_punched_stripes_equal_the_twin_in_every_outcome_class(eng, h, w, p, connectivity):
    labels, prev = punched_case(h, w, p)
    params = P(connectivity=connectivity, max_area=4, max_rel_area=0.002, prev_overlap=0.5)
    want, want_filled = holes.fill_host(labels, params, prev=prev, return_filled=True)
    by_rule, by_rule_filled, classes = ref.fill_ref(labels, params, prev=prev)
    np.testing.assert_array_equal(want, by_rule)                     # the classes below are the twin's
    np.testing.assert_array_equal(want_filled, by_rule_filled)
    print(f'{h} x {w}, p {p}, connectivity {connectivity}: {classes}')
    assert all(classes[c] > 0 for c in ref.CLASSES), classes         # a case that takes one branch only proves nothing
    same_as_twin(eng, labels, params, prev=prev)
    same_as_twin(eng, labels, params)                                # no R for the first frame
    same_as_twin(eng, labels, dict(params, prev_overlap=0.0), prev=prev)       # all frames in one launch set


# ---- exact thresholds ---------------------------------------------------------------------------------------------------
def test_thresholds_are_exact(eng):
    m = np.zeros((2, 20, 80), dtype=np.uint8)
    ref._ring(m[0], 2, 60, 6, 70, 1)                                 # hole 2 x 8 = 16 pixels over x = 64, ring of 24
    ref._ring(m[1], 2, 60, 6, 71, 1)                                 # hole 2 x 9 = 18
    m[1, 3, 61] = 1                                                  # ... = 17 pixels
    out = same_as_twin(eng, m, P(max_area=16))[0]
    assert out[0, 3:5, 61:69].all() and not out[1, 4, 61:70].any()   # A == max_area fills, A == max_area + 1 does not
    m = np.zeros((2, 20, 80), dtype=np.uint8)
    ref._ring(m[0], 2, 62, 6, 66, 1)                                 # hole 2 x 2 = 4, ring of 12
    m[0, 10, 0:4] = 1                                                # S = 16: A * 65536 == rq * S at max_rel_area = 0.25
    ref._ring(m[1], 2, 60, 5, 67, 1)                                 # hole 1 x 5 = 5, ring of 16: one pixel more
    assert (m[0] == 1).sum() == 16 and (m[1] == 1).sum() == 16 and holes.rel_q16(0.25) * 16 == 4 * 65536
    out = same_as_twin(eng, m, P(max_area=ANY, max_rel_area=0.25))[0]
    assert out[0, 3:5, 63:65].all() and not out[1, 3, 61:66].any()
    out = same_as_twin(eng, m, P(max_area=ANY, max_rel_area=0.25 - 2.0 ** -16))[0]
    assert not out[0, 3:5, 63:65].any()
    m = np.zeros((1, 20, 80), dtype=np.uint8)
    ref._ring(m[0], 2, 62, 6, 66, 1)                                 # A = 4
    prev = np.zeros((20, 80), dtype=np.uint8)
    prev[3, 63:65] = 1                                               # C = 2
    out = same_as_twin(eng, m, P(max_area=4, prev_overlap=0.5), prev=prev)[0]
    assert out[0, 3:5, 63:65].all()
    prev[3, 64] = 0                                                  # C = 1
    prev[15, 15] = 1
    out = same_as_twin(eng, m, P(max_area=4, prev_overlap=0.5), prev=prev)[0]
    assert not out[0, 3:5, 63:65].any()


# ---- the chain ----------------------------------------------------------------------------------------------------------
def test_chain_reads_the_filled_frame_before(eng, monkeypatch):
    labels, prev, keep, real, (sy0, sy1, sx0, sx1) = ref.chain()
    params = P(max_area=16, prev_overlap=0.5)
    want = same_as_twin(eng, labels, params, prev=prev, keep=keep)[0]
    for f, (y0, y1, x0, x1) in enumerate(real):
        assert not want[f, y0:y1, x0:x1].any()                       # the real hole stays open in every frame
    assert (want[2:4, sy0:sy1, sx0:sx1] == 1).all()                  # the spurious hole fills in both frames
    assert not labels[2:4, sy0:sy1, sx0:sx1].any()
    unfilled_R = holes.fill_host(labels[3:4], params, prev=labels[2])[0]
    assert not unfilled_R[sy0:sy1, sx0:sx1].any()                    # with the unfilled input as R it would stay open:
    assert not np.array_equal(unfilled_R, want[3])                   # the test tells the two apart
    assert not want[:, -4, 4:6].any()                                # the keep frame has label 2 with its hole: it stays
    np.testing.assert_array_equal(want[0], labels[0])                # the keep frame
    same_as_twin(eng, labels, params, prev=None, keep=keep)
    same_as_twin(eng, labels, params, prev=np.where(prev == 1, 9, prev).astype(np.uint8), keep=())    # label 1 absent from R
    free = same_as_twin(eng, labels, params, prev=prev, keep=())[0]
    assert (free[:, -4, 4:6] == 2).all()                             # label 2 is absent from `prev`: rule inactive, filled at once
    same_as_twin(eng, labels, dict(params, connectivity=4), prev=prev, keep=keep)
    monkeypatch.setattr(holes, 'frames_per_call', lambda h, w: 2)    # chunks: the last filled frame is handed over
    got = eng.fill_holes(dev(labels), prev=dev(prev), keep=keep, **params)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


# ---- scratch ------------------------------------------------------------------------------------------------------------
def test_scratch_is_shared_and_stale_scratch_does_not_show(eng):
    big, prev_big = punched_case(97, 161, 0.3)
    small, names = pattern_case(33, 130)
    params = P(max_area=ANY, prev_overlap=0.5)
    same_as_twin(eng, big, params, prev=prev_big)                    # the larger call first
    want = same_as_twin(eng, small, params)[0]                       # back to back on the same scratch
    for k in range(len(names)):
        got = eng.fill_holes(dev(small[k:k + 1]), **params)          # a batch equals single-frame calls (no prev: no rule 4)
        single = holes.fill_host(small[k:k + 1], params)
        np.testing.assert_array_equal(got.cpu().numpy(), single, err_msg=names[k])
    off = dict(params, prev_overlap=0.0)
    batch = eng.fill_holes(dev(small), **off)
    for k in range(len(names)):
        assert torch.equal(eng.fill_holes(dev(small[k:k + 1]), **off)[0], batch[k]), names[k]
    # interleaved with the component filter and the id map on the same engine
    cmaps = np.stack(list(components_ref.patterns(33, 130).values()))
    cpar = dict(components.DEFAULTS, largest_only=True, min_area=2)
    x, c = dev(big), dev(cmaps)
    a1 = eng.fill_holes(x, prev=dev(prev_big), **params)
    f1 = eng.filter_components(c, **cpar)
    a2 = eng.fill_holes(dev(small), **params)
    i1 = eng.label_components(c, 8)
    a3 = eng.fill_holes(x, prev=dev(prev_big), **params)
    assert torch.equal(a1, a3)
    np.testing.assert_array_equal(a1.cpu().numpy(), holes.fill_host(big, params, prev=prev_big))
    np.testing.assert_array_equal(a2.cpu().numpy(), want)
    np.testing.assert_array_equal(f1.cpu().numpy(), components.filter_host(cmaps, cpar))
    np.testing.assert_array_equal(i1.cpu().numpy(), components.label_host(cmaps, 8))


# ---- rejections ---------------------------------------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def test_limits_are_refused_without_a_launch(eng):
    maps = pattern_case(33, 130)[0][:3]
    x = dev(maps)
    out = torch.full((3, 33, 130), 77, dtype=torch.uint8, device=DEV)
    lib, h = eng.lib, eng.h

    def fill(e=h, lab=x, n=3, H=33, W=130, conn=8, max_area=ANY, q=65536, oq=0, o=out):
        return lib.eosvos_fill_holes(e, _ptr(lab), n, H, W, conn, max_area, q, oq, None, None, _ptr(o), None)
    # arguments only: the geometry is refused before anything is read, so the buffers need not have the size that is named
    for kw in (dict(conn=6), dict(conn=0), dict(H=4097, W=1), dict(H=1, W=4097), dict(H=4096, W=4096), dict(H=0), dict(W=0),
               dict(n=-1), dict(n=65536), dict(max_area=-1), dict(max_area=ANY + 1), dict(q=-1), dict(q=65537), dict(oq=-1),
               dict(oq=65537), dict(e=None), dict(lab=None), dict(o=None), dict(n=65535, H=480, W=854)):
        assert fill(**kw) != 0, kw
        assert lib.eosvos_last_error().decode().startswith('fill_holes'), kw
    assert 'cap' in lib.eosvos_last_error().decode()                 # the last one: more than 512 MB of scratch
    eng.synchronize()
    assert bool((out == 77).all())                                   # nothing was written
    with pytest.raises(_ffi.EosvosError, match='fill_holes'):
        _ffi.check(fill(conn=6))
    assert fill() == 0                                               # a valid call right after succeeds
    eng.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), holes.fill_host(maps, P(max_area=ANY)))
    assert fill(max_area=0) == 0                                     # off: a copy
    eng.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), maps)
    for bad in (dict(connectivity=6), dict(max_rel_area=1.5), dict(max_area=-1), dict(prev_overlap=-0.5)):
        with pytest.raises(ValueError):
            eng.fill_holes(x, **bad)
    with pytest.raises(ValueError):
        eng.fill_holes(x.cpu(), max_area=4)
    with pytest.raises(ValueError):
        eng.fill_holes(x.int(), max_area=4)
    with pytest.raises(ValueError):
        eng.fill_holes(x, max_area=4, prev=x[0, :, :100])


# ---- end to end ---------------------------------------------------------------------------------------------------------
BN_CFG = {'accum_stats': False, 'learn_weight': False, 'learn_bias': False}
MO_CFG = dict(init_lr=1e-3, learn_model_init=True, second_order_gradients=False, lr_hierarchy_level='NEURON',
              use_log_init_lr=False, max_lr=None)


def test_evaluate_sequence_with_holes(monkeypatch):
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
            def no_fill(*a, **k):
                raise AssertionError('a hole-filling call on the plain path')
            mp.setattr(Engine, 'fill_holes', no_fill)
            for kw in ({'holes': None}, {'holes': P()}, {'holes': P(max_area=9, max_rel_area=0.0)}):
                off = evaluate_sequence(model, mo, msd, seq, gts, cfg, **kw)
                assert torch.equal(off[0], today[0]) and off[2] == today[2]
                assert all(torch.equal(a, b) for a, b in zip(off[1], today[1]))
        cpar = dict(components.DEFAULTS, min_area=3, gate=8)
        cleaned = evaluate_sequence(model, mo, msd, seq, gts, cfg, components=cpar)
        params = P(max_area=ANY, prev_overlap=0.25)
        on = evaluate_sequence(model, mo, msd, seq, gts, cfg, components=cpar, holes=params)
        assert all(torch.equal(a, b) for a, b in zip(on[1], today[1]))
        assert model.engine.plan_fingerprint() == fp                # no matrix kernel: the conv plans did not move
        want = holes.fill_host(cleaned[0].cpu().numpy(), params, keep=(0,))
        assert on[0].dtype == torch.uint8 and on[0].shape == (4, 96, 160)
        np.testing.assert_array_equal(on[0].cpu().numpy(), want)
        assert torch.equal(on[0][0], today[0][0])                    # the train frame passes unchanged
        alone = evaluate_sequence(model, mo, msd, seq, gts, cfg, holes=params)
        np.testing.assert_array_equal(alone[0].cpu().numpy(), holes.fill_host(today[0].cpu().numpy(), params, keep=(0,)))
    finally:
        model.close_engines()
