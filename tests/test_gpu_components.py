"""Connected components and the component filter on the MI355X (`eosvos_label_components`, `eosvos_filter_components`,
csrc/ccl_kernels.hip) against the numpy twin of `eosvos_amd/components.py`.  Integer arithmetic on both sides: every output is
compared bit for bit.  Needs an MI355X: pytest -m gpu.

The kernels' tile is 64 wide and 16 high (`components_ref.TILE_W`, `TILE_H`), so the sizes are: 1 x 1, 5 x 7 (inside a tile),
16 x 64 (one tile exactly), 17 x 65 (one pixel over the tile in each direction), 33 x 130 and 97 x 161 (several tiles, no
multiple of the tile)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import components_ref as ref  # noqa: E402

from eosvos_amd import _ffi, components, synthetic  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = [(1, 1), (5, 7), (ref.TILE_H, ref.TILE_W), (ref.TILE_H + 1, ref.TILE_W + 1), (33, 130), (97, 161)]
FILTERS = [dict(min_area=3), dict(min_rel_area=0.25), dict(largest_only=True), dict(largest_only=True, connectivity=4),
           dict(min_area=2, min_rel_area=0.1, connectivity=4)]


def P(**kw):
    return dict(components.DEFAULTS, **kw)


@pytest.fixture(scope='module')
def eng():
    e = Engine('resnet50', 96, 160, max_batch=1, device=DEV)        # lends its stream and scratch; frames are of any size
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def pattern_case(h, w, connectivity):
    """(maps (K, H, W), names, ids of the twin); computed once, never changed."""
    pats = ref.patterns(h, w)
    maps = np.stack(list(pats.values()))
    return maps, tuple(pats), components.label_host(maps, connectivity)


@functools.lru_cache(maxsize=None)
def chain_case():
    return ref.chain(40, 160, 10, 12)          # the object drifts over the seam at x = 64, the distractor sits beyond x = 128


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- labelling ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('h,w', SIZES)
def test_ids_equal_the_twin_on_every_pattern(eng, h, w, connectivity):
    maps, names, want = pattern_case(h, w, connectivity)
    ids = eng.label_components(dev(maps), connectivity).cpu().numpy()
    assert ids.dtype == np.int32
    for k, name in enumerate(names):
        np.testing.assert_array_equal(ids[k], want[k], err_msg=name)


def test_a_batch_equals_single_frame_calls_and_stale_scratch_does_not_show(eng):
    big, _, want_big = pattern_case(97, 161, 8)
    small, names, want_small = pattern_case(33, 130, 8)
    assert np.array_equal(eng.label_components(dev(big), 8).cpu().numpy(), want_big)        # the larger call first
    four = [names.index(n) for n in ('serpentine', 'spiral', 'noise_0.5', 'seam_quadrants')]
    batch = eng.label_components(dev(small[four]), 8).cpu().numpy()                        # back to back on the same scratch
    np.testing.assert_array_equal(batch, want_small[four])
    for k, i in enumerate(four):
        np.testing.assert_array_equal(eng.label_components(dev(small[i:i + 1]), 8).cpu().numpy()[0], batch[k])
    params = P(largest_only=True, min_area=2)
    got = eng.filter_components(dev(big), **params).cpu().numpy()
    np.testing.assert_array_equal(got, components.filter_host(big, params))
    got = eng.filter_components(dev(small[four]), **params)
    np.testing.assert_array_equal(got.cpu().numpy(), components.filter_host(small[four], params))
    for k, i in enumerate(four):
        assert torch.equal(eng.filter_components(dev(small[i:i + 1]), **params)[0], got[k])


# ---- the filter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(5, 7), (ref.TILE_H + 1, ref.TILE_W + 1), (97, 161)])
def test_area_rules_equal_the_twin_on_every_pattern(eng, h, w):
    maps = pattern_case(h, w, 8)[0]
    for kw in FILTERS:
        params = P(**kw)
        want, want_removed = components.filter_host(maps, params, return_removed=True)
        got, removed = eng.filter_components(dev(maps), return_removed=True, **params)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=str(kw))
        np.testing.assert_array_equal(removed, want_removed, err_msg=str(kw))


@pytest.mark.parametrize('kw', [dict(gate=10), dict(gate=10, largest_only=True), dict(gate=9, min_area=150),
                                dict(gate=10, connectivity=4, min_rel_area=1.0), dict(gate=63), dict(gate=1)])
def test_gate_chain_equals_the_twin(eng, kw, monkeypatch):
    labels, prev, keep = chain_case()
    params = P(**kw)
    for pv, kp in ((prev, keep), (None, keep), (prev, ())):
        want, want_removed = components.filter_host(labels, params, prev=pv, keep=kp, return_removed=True)
        got, removed = eng.filter_components(dev(labels), prev=None if pv is None else dev(pv), keep=kp, return_removed=True,
                                             **params)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'{kw} prev={pv is not None} keep={kp}')
        np.testing.assert_array_equal(removed, want_removed)
    want = components.filter_host(labels, params, prev=prev, keep=keep)
    if kw in (dict(gate=10), dict(gate=10, largest_only=True)):      # the gate first: the smaller object survives, the distractor goes
        for f in (0, 1):
            assert not want[f, :12, -24:].any() and np.array_equal(want[f, :, :-24], labels[f, :, :-24])
        assert not (want[2] == 1).any() and np.array_equal(want[4], labels[4])
    monkeypatch.setattr(components, 'frames_per_call', lambda h, w: 2)                      # chunks: prev is handed over
    got = eng.filter_components(dev(labels), prev=dev(prev), keep=keep, **params)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_gate_on_noise_with_many_labels_equals_the_twin(eng):
    rng = np.random.default_rng(7)
    labels = np.stack([ref.noise(33, 130, d, seed=40 + i) for i, d in enumerate((0.1, 0.2, 0.35, 0.1))])
    labels[1][labels[1] == 3] = 200                                  # a label that comes and goes
    labels[3, :, 100:] = np.where(rng.random((33, 30)) < 0.3, 255, 0)
    prev = ref.noise(33, 130, 0.02, seed=3)
    for kw in (dict(gate=2), dict(gate=3, connectivity=4, min_area=2), dict(gate=5, largest_only=True)):
        want, want_removed = components.filter_host(labels, P(**kw), prev=prev, return_removed=True)
        got, removed = eng.filter_components(dev(labels), prev=dev(prev), return_removed=True, **P(**kw))
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=str(kw))
        np.testing.assert_array_equal(removed, want_removed)
        assert 0 < int(removed.sum()) < int((labels != 0).sum())


def test_relative_area_boundary_and_the_largest_only_tie(eng):
    m = np.zeros((1, 40, 200), dtype=np.uint8)
    m[0, 0, 0:128] = 1                                               # Amax = 128, over two tiles
    m[0, 2, 60:92] = 1                                               # A = 32: A * 65536 == q * Amax at min_rel_area = 0.25 exactly
    m[0, 4, 60:91] = 1                                               # A = 31: below
    m[0, 20, 60:188] = 1                                             # a second component of Amax pixels, with the larger id
    for params in (P(min_rel_area=0.25), P(min_rel_area=0.25 + 2.0 ** -16), P(largest_only=True)):
        got = eng.filter_components(dev(m), **params).cpu().numpy()
        np.testing.assert_array_equal(got, components.filter_host(m, params))
    at = eng.filter_components(dev(m), **P(min_rel_area=0.25)).cpu().numpy()
    assert at[0, 2, 60:92].all() and not at[0, 4].any() and at[0, 0, :128].all() and at[0, 20, 60:188].all()
    above = eng.filter_components(dev(m), **P(min_rel_area=0.25 + 2.0 ** -16)).cpu().numpy()
    assert not above[0, 2].any() and above[0, 0, :128].all()
    tie = eng.filter_components(dev(m), **P(largest_only=True)).cpu().numpy()
    assert tie[0, 0, :128].all() and not tie[0, 1:].any()            # the tie goes to the smaller id


# ---- rejections ---------------------------------------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def test_limits_are_refused_without_a_launch(eng):
    maps = pattern_case(33, 130, 8)[0][:2]
    x = dev(maps)
    out = torch.full((2, 33, 130), 77, dtype=torch.uint8, device=DEV)
    ids = torch.full((2, 33, 130), -5, dtype=torch.int32, device=DEV)
    lib, h = eng.lib, eng.h

    def flt(e=h, lab=x, n=2, H=33, W=130, conn=8, min_area=0, q=0, largest=1, gate=0, o=out):
        return lib.eosvos_filter_components(e, _ptr(lab), n, H, W, conn, min_area, q, largest, gate, None, None, _ptr(o), None)

    def lbl(e=h, lab=x, n=2, H=33, W=130, conn=8, o=ids):
        return lib.eosvos_label_components(e, _ptr(lab), n, H, W, conn, _ptr(o))
    # arguments only: the geometry is refused before anything is read, so the buffers need not have the size that is named
    for kw in (dict(gate=64), dict(gate=-1), dict(conn=6), dict(conn=0), dict(H=4097, W=1), dict(H=1, W=4097), dict(H=4096, W=4096),
               dict(H=0), dict(W=0), dict(n=-1), dict(n=65536), dict(min_area=-1), dict(q=-1), dict(q=65537), dict(e=None),
               dict(lab=None), dict(o=None)):
        assert flt(**kw) != 0, kw
        assert lib.eosvos_last_error().decode().startswith('filter_components'), kw
    for kw in (dict(conn=6), dict(H=4097, W=1), dict(H=4096, W=4096), dict(H=0), dict(n=-1), dict(e=None), dict(lab=None), dict(o=None)):
        assert lbl(**kw) != 0, kw
        assert lib.eosvos_last_error().decode().startswith('label_components'), kw
    eng.synchronize()
    assert bool((out == 77).all()) and bool((ids == -5).all())       # nothing was written
    with pytest.raises(_ffi.EosvosError, match='filter_components'):
        _ffi.check(flt(gate=64))
    assert flt() == 0 and lbl() == 0                                 # valid calls right after succeed
    eng.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), components.filter_host(maps, P(largest_only=True)))
    np.testing.assert_array_equal(ids.cpu().numpy(), components.label_host(maps, 8))
    for bad in (dict(gate=64), dict(connectivity=6), dict(min_rel_area=1.5), dict(min_area=-1)):
        with pytest.raises(ValueError):
            eng.filter_components(x, **bad)
    with pytest.raises(ValueError):
        eng.filter_components(x.cpu(), largest_only=True)
    with pytest.raises(ValueError):
        eng.label_components(x.int())
    with pytest.raises(ValueError):
        eng.filter_components(x, gate=1, prev=x[0, :, :100])


# ---- end to end ---------------------------------------------------------------------------------------------------------
BN_CFG = {'accum_stats': False, 'learn_weight': False, 'learn_bias': False}
MO_CFG = dict(init_lr=1e-3, learn_model_init=True, second_order_gradients=False, lr_hierarchy_level='NEURON',
              use_log_init_lr=False, max_lr=None)


def test_evaluate_sequence_with_components(monkeypatch):
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
            def no_filter(*a, **k):
                raise AssertionError('a component call on the plain path')
            mp.setattr(Engine, 'filter_components', no_filter)
            mp.setattr(Engine, 'label_components', no_filter)
            for kw in ({'components': None}, {'components': P()}):
                off = evaluate_sequence(model, mo, msd, seq, gts, cfg, **kw)
                assert torch.equal(off[0], today[0]) and off[2] == today[2]
                assert all(torch.equal(a, b) for a, b in zip(off[1], today[1]))
        params = P(largest_only=True, gate=8)
        on = evaluate_sequence(model, mo, msd, seq, gts, cfg, components=params)
        assert all(torch.equal(a, b) for a, b in zip(on[1], today[1]))
        assert model.engine.plan_fingerprint() == fp                # no matrix kernel: the conv plans did not move
        want = components.filter_host(today[0].cpu().numpy(), params, keep=(0,))
        assert on[0].dtype == torch.uint8 and on[0].shape == (4, 96, 160)
        np.testing.assert_array_equal(on[0].cpu().numpy(), want)
        assert torch.equal(on[0][0], today[0][0])                    # the train frame passes unchanged
    finally:
        model.close_engines()
