"""Host-side checks of the distance gate of online adaptation (`eosvos_amd/adapt.py`, no GPU): the numpy twins against the plain
loops of tests/adapt_ref.py bit for bit, the properties the rules imply, `check` / `active` / `parse_cli`, and -- on the
recording stand-in engine of test_loss_ignore_host.py -- that the off path calls nothing new and the on path makes one
`adapt_targets` call per adaptation round with the right anchors."""
import os
import re

import numpy as np
import pytest
import torch

import adapt_ref as R
import test_loss_ignore_host as L
from eosvos_amd import adapt, config, evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 70), (70, 1), (17, 41), (33, 65)]
LIMITS = [1, 2, 7, 64, 100]                        # 100: larger than both sides of every size


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- rule 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('invert', [False, True], ids=['ge', 'not_ge'])
@pytest.mark.parametrize('hw', SIZES, ids=[f'{h}x{w}' for h, w in SIZES])
def test_distance_twin_equals_the_plain_loops(hw, invert):
    for name in R.PATTERNS:
        p = R.pattern(name, *hw)
        seeds = R.seeds_of(p, R.T, invert)
        with np.errstate(invalid='ignore'):
            ge = p >= np.float32(R.T)
        assert np.array_equal(seeds, ~ge if invert else ge), name           # the predicate of the twins' callers
        d2 = R.distance_sq_all_pairs(seeds)
        for limit in LIMITS:
            got = adapt.distance_sq_host(seeds, limit)
            assert got.dtype == np.int64 and got.shape == seeds.shape
            assert np.array_equal(got, R.distance_sq(seeds, limit, d2)), (name, limit)


def test_the_patterns_are_what_they_say():
    h, w = 33, 65
    n = {name: int((R.pattern(name, h, w) >= R.T).sum()) for name in R.PATTERNS}
    assert n['empty'] == 0 and n['full'] == h * w and n['centre'] == 1 and all(n[f'corner{c}'] == 1 for c in ('00', '0w', 'h0', 'hw'))
    assert 0 < n['sparse'] < 20 and 0 < n['blobs'] < h * w and 0 < n['blob_far_blob'] < h * w
    assert np.isnan(R.pattern('nans', h, w)).any() and np.array_equal(bits(R.pattern('blobs', h, w, 3)), bits(R.pattern('blobs', h, w, 3)))


@pytest.mark.parametrize('name', ['sparse', 'blobs', 'blob_far_blob'])
def test_distance_properties(name):
    seeds = R.pattern(name, 33, 65) >= R.T
    for limit in (2, 7, 100):
        d = adapt.distance_sq_host(seeds, limit)
        assert np.array_equal(d == 0, seeds)                                # 0 exactly on the seeds
        assert d.max() <= limit * limit + 1 and d.min() >= 0
        assert np.array_equal(adapt.distance_sq_host(seeds[:, ::-1], limit), d[:, ::-1])
        assert np.array_equal(adapt.distance_sq_host(seeds[::-1], limit), d[::-1])
        assert np.array_equal(adapt.distance_sq_host(seeds.T, limit), d.T)
    stack = np.stack([seeds, ~seeds, np.zeros_like(seeds)])                # leading dimensions are independent frames
    both = adapt.distance_sq_host(stack, 7)
    assert np.array_equal(both[0], adapt.distance_sq_host(seeds, 7)) and np.array_equal(both[1], adapt.distance_sq_host(~seeds, 7))
    assert (both[2] == 50).all()                                            # no seed: L^2 + 1 everywhere


@pytest.mark.parametrize('bad', [0, -1, 4096, 2.0, True, None])
def test_bad_limits_raise(bad):
    with pytest.raises(ValueError):
        adapt.distance_sq_host(np.ones((3, 3), dtype=bool), bad)


# ---- rules 2-6 ------------------------------------------------------------------------------------------------------------
CASES = [(erode, neg, band, nans) for erode in (0, 2) for neg in (3, 10) for band in ((0.0, 0.5), (0.3, 0.7)) for nans in (False, True)]


@pytest.mark.parametrize('erode,neg,band,nans', CASES)
def test_targets_twin_equals_the_plain_loops(erode, neg, band, nans):
    probs, anchors = R.three_frames(17, 41, nans)
    want, n_want = R.targets(probs, anchors, band[0], band[1], neg, erode)
    got, n_got = adapt.targets_host(probs, anchors, band[0], band[1], {'neg_dist': neg, 'erode': erode}, R.IGN)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    assert n_got.dtype == np.int64 and n_got.tolist() == n_want and n_want[1] == 0
    assert np.array_equal(bits(got[1]), bits(R.band_rule(probs[1], *band)))            # rule 6: no anchor, the base rule's map
    got4, n4 = adapt.targets_host(probs[:, None], anchors[:, None], band[0], band[1], {'neg_dist': neg, 'erode': erode}, R.IGN)
    assert got4.shape == (3, 1, 17, 41) and np.array_equal(bits(got4[:, 0]), bits(got)) and n4.tolist() == n_want


def test_erode_zero_keeps_the_anchor_and_erosion_ignores_the_border():
    a = R.pattern('blobs', 33, 65)
    assert np.array_equal(adapt.eroded_host(a, R.T, 0), a >= np.float32(R.T))
    for erode in (1, 3):
        assert np.array_equal(adapt.eroded_host(a, R.T, erode), R.eroded(a, R.T, erode))
    cut = np.zeros((9, 12), dtype=np.float32)
    cut[:, :6] = 1                                   # an object cut by three borders: eroded from its one inner edge only
    E = adapt.eroded_host(cut, 0.5, 2)
    assert E[:, :4].all() and not E[:, 4:].any()


def test_a_distance_beyond_the_diagonal_is_the_band_rule():
    probs, anchors = R.three_frames(17, 41, nans=True)
    for band in ((0.0, 0.5), (0.3, 0.7)):
        got, n = adapt.targets_host(probs, anchors, band[0], band[1], {'neg_dist': 45}, R.IGN)       # 45^2 > 16^2 + 40^2
        want = R.band_rule(probs, *band)
        assert np.array_equal(bits(got), bits(want))
        assert n.tolist() == [int((want[0] == 1).sum()), 0, int((want[2] == 1).sum())] and n[0] > 0 and n[2] > 0


def test_an_anchor_eroded_away_counts_nothing():
    probs = np.full((1, 12, 20), 0.9, dtype=np.float32)
    anchors = np.zeros((1, 12, 20), dtype=np.float32)
    anchors[0, 4:7, 3:17] = 1                        # three rows thick: gone under erode 2, alive under erode 1
    out, n = adapt.targets_host(probs, anchors, 0.3, 0.7, {'neg_dist': 2, 'erode': 2}, R.IGN)
    assert n.tolist() == [0] and (out == 1).all()    # the base rule's map, and a count that drops the frame
    out, n = adapt.targets_host(probs, anchors, 0.3, 0.7, {'neg_dist': 2, 'erode': 1}, R.IGN)
    assert n[0] > 0 and (out[0, 5, 4:16] == 1).all() and (out[0, 0] == 0).all() and n[0] == int((out == 1).sum())


def test_the_far_confident_blob_becomes_negative():
    h, w = 24, 60
    probs = np.full((1, h, w), 0.1, dtype=np.float32)
    probs[0, 8:16, 5:15] = 0.95                      # the object, where it was
    probs[0, 10:14, 50:56] = 0.95                    # a look-alike 35 pixels away
    probs[0, 8:16, 15:18] = 0.6                      # an uncertain rim
    anchors = np.zeros((1, h, w), dtype=np.float32)
    anchors[0, 8:16, 4:14] = 1
    for lo, hi in ((0.0, 0.7), (0.3, 0.7)):
        out, n = adapt.targets_host(probs, anchors, lo, hi, {'neg_dist': 12, 'erode': 1}, R.IGN)
        assert (out[0, 8:16, 5:15] == 1).all() and (out[0, 10:14, 50:56] == 0).all() and (out[0, 8:16, 15:18] == R.IGN).all()
        assert n.tolist() == [80]
        # near and unsure: negative under the band, void under the scalar form (nothing near is negative)
        assert out[0, 0, 5] == (R.IGN if lo == 0.0 else 0)
        off = R.band_rule(probs, lo, hi)
        assert (off[0, 10:14, 50:56] == 1).all()     # what the rounds were trained on without the gate


def test_bad_arguments_of_the_twin_raise():
    x = np.zeros((1, 4, 4), dtype=np.float32)
    for kw in ({'neg_dist': 0}, {'neg_dist': 3, 'erode': 256}, {'neg_dist': 3, 'gate': 1}):
        with pytest.raises(ValueError):
            adapt.targets_host(x, x, 0.3, 0.7, kw, R.IGN)
    with pytest.raises(ValueError):
        adapt.targets_host(x, x, 0.7, 0.3, {'neg_dist': 3}, R.IGN)
    with pytest.raises(ValueError):
        adapt.targets_host(x, x[:, :2], 0.3, 0.7, {'neg_dist': 3}, R.IGN)


# ---- parameters and the command line ------------------------------------------------------------------------------------------
def test_check_and_active():
    assert adapt.DEFAULTS == {'neg_dist': 0, 'erode': 0} == config.ADAPT['eval_adapt']
    assert adapt.check({}) == adapt.DEFAULTS and adapt.check({'neg_dist': 4095, 'erode': 255}) == {'neg_dist': 4095, 'erode': 255}
    assert not adapt.active(None) and not adapt.active({}) and not adapt.active({'neg_dist': 0}) and not adapt.active({'erode': 9})
    assert adapt.active({'neg_dist': 1}) and adapt.active({'neg_dist': 220, 'erode': 15})
    for bad in ({'neg_dist': -1}, {'neg_dist': 4096}, {'neg_dist': 2.0}, {'neg_dist': True}, {'erode': 256}, {'erode': -1},
                {'erode': '3'}, {'dist': 3}, [220, 15], 220):
        with pytest.raises(ValueError):
            adapt.check(bad)
        with pytest.raises(ValueError):
            adapt.active(bad)
    assert adapt.band_of(0.5, None) == (0.0, 0.5) and adapt.band_of(1, None) == (0.0, 1.0) and adapt.band_of([0.3, 0.7], (0.3, 0.7)) == (0.3, 0.7)
    for bad in (0, 0.0, -0.1, 1.5, float('nan'), True, 'a'):
        with pytest.raises(ValueError):
            adapt.band_of(bad, None)
    assert adapt.frames_per_call(480, 854) >= 2 and adapt.frames_per_call(4096, 4096, 15) == 10 and adapt.frames_per_call(1, 1) == 65535


def test_parse_cli_adds_the_group_only_when_asked():
    plain = config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS-OnA'])
    assert 'eval_adapt' not in plain and 'eval_adapt' not in config.BASE
    assert sorted(config.BASE['eval_online_adapt']) == ['min_prop', 'num_epochs', 'reset_model_mode', 'step']
    cfg = config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS-OnA', 'eval_adapt.neg_dist=220', 'eval_adapt.erode=15'])
    assert cfg['eval_adapt'] == {'neg_dist': 220, 'erode': 15}
    rest = {k: v for k, v in cfg.items() if k != 'eval_adapt'}
    assert rest == plain                                                    # nothing leaks into BASE's keys or the other groups
    assert config.ADAPT['eval_adapt'] == {'neg_dist': 0, 'erode': 0}        # the group's defaults are copied, not edited
    assert config.parse_cli(['e-OSVOS-OnA', 'eval_adapt.erode=3'])['eval_adapt'] == {'neg_dist': 0, 'erode': 3}
    other = config.parse_cli(['e-OSVOS-OnA', 'eval_lucid.samples=1'])
    assert 'eval_adapt' not in other


@pytest.mark.parametrize('bad', ['eval_adapt.neg_dist=4096', 'eval_adapt.neg_dist=-1', 'eval_adapt.neg_dist=2.5', 'eval_adapt.erode=256',
                                 'eval_adapt.neg_dist=true'])
def test_parse_cli_rejects_bad_values(bad):
    with pytest.raises(ValueError):
        config.parse_cli(['e-OSVOS-OnA', bad])


def test_parse_cli_rejects_unknown_keys_and_a_gate_without_adaptation():
    with pytest.raises(KeyError):
        config.parse_cli(['e-OSVOS-OnA', 'eval_adapt.radius=3'])
    with pytest.raises(ValueError, match='no consumer'):
        config.parse_cli(['e-OSVOS', 'eval_adapt.neg_dist=220'])            # eval_online_adapt.step is 0
    with pytest.raises(ValueError, match='no consumer'):
        config.parse_cli(['eval_adapt.neg_dist=220', 'eval_adapt.erode=15'])
    assert config.parse_cli(['eval_adapt.neg_dist=220', 'eval_online_adapt.step=5'])['eval_adapt']['neg_dist'] == 220


# ---- online adaptation on the recording stand-in engine -----------------------------------------------------------------------
class GateEngine(L.StubEngine):
    """The stand-in engine of test_loss_ignore_host.py with the new entry point: records the call, answers with the twin."""

    def adapt_targets(self, probs, anchors, lo, hi, params, ignore, counts=True):
        self.calls.append(('adapt_targets', lo, hi, dict(params), ignore, probs.clone(), anchors.clone()))
        out, n = adapt.targets_host(probs, anchors, lo, hi, params, ignore)
        return torch.from_numpy(out), [int(c) for c in n]


H, W, N = 8, 16, 10                                  # step 3, batch 3: round 1 propagates frames 3 and 2, round 2 frames 6 and 5


def sequence_probs():
    p = torch.full((N, 1, H, W), 0.1)
    p[1, 0, 2:6, 0:4] = 0.9                          # frame 1: the object at the left (the anchor of frame 2)
    p[2, 0, 2:6, 1:5] = 0.9                          # frame 2: the object, one column on ...
    p[2, 0, 2:6, 12:16] = 0.9                        # ... and a look-alike 8 columns from the anchor
    p[2, 0, 0, :3] = torch.tensor([0.3, 0.7, 0.5])
    p[3] = 0.4                                       # frame 3: no positive under 0.5 or 0.7
    p[4, 0, 2:6, 2:6] = 0.9
    p[5] = 0.2                                       # frame 5: the object is lost: no positive, and no anchor for frame 6
    p[6, 0, 2:6, 3:7] = 0.9                          # frame 6: confident, but nothing to anchor it
    return p


def run(min_prop, engine_cls=GateEngine, **kw):
    probs = sequence_probs()
    eng = engine_cls(probs)
    frames = torch.arange(N, dtype=torch.float32).view(N, 1, 1, 1).expand(N, 3, H, W).contiguous()
    gt = torch.zeros(1, H, W)
    gt[0, 2:6, 0:3] = 1
    cfg = {'eval_online_adapt': {'step': 3, 'reset_model_mode': 'FIRST_STEP', 'num_epochs': 2, 'min_prop': min_prop},
           'data_cfg': {'batch_sizes': {'train': 3}}, 'num_epochs': {'eval': 2}, 'loss_func': 'dice', 'seed': 1}
    masks, hist = evaluate.finetune_object(L.StubModel(eng), L.StubMetaOptim(), {}, frames, gt, cfg, **kw)
    return eng, masks, hist, probs, gt


def same_log(a, b):
    assert len(a) == len(b)
    for ca, cb in zip(a, b):
        assert len(ca) == len(cb)
        for va, vb in zip(ca, cb):
            assert torch.equal(va, vb) if isinstance(va, torch.Tensor) else va == vb


@pytest.mark.parametrize('min_prop', [0.5, [0.3, 0.7]], ids=['scalar', 'band'])
def test_off_calls_nothing_new(min_prop):
    ref, masks, hist, _, _ = run(min_prop)
    assert len(hist) == 3 and any(c[0] == 'loss' and c[2].shape[0] > 1 for c in ref.calls)
    for off in (None, {'neg_dist': 0}, {'neg_dist': 0, 'erode': 5}, {}):
        eng, m, h, _, _ = run(min_prop, adapt=off)
        assert not [c for c in eng.calls if c[0] == 'adapt_targets']
        same_log(eng.calls, ref.calls)                                      # the same calls with the same batches
        assert torch.equal(m, masks) and h == hist


@pytest.mark.parametrize('min_prop,band', [(0.5, (0.0, 0.5)), ([0.3, 0.7], (0.3, 0.7))], ids=['scalar', 'band'])
def test_on_makes_one_call_per_adaptation_round(min_prop, band):
    params = {'neg_dist': 4, 'erode': 0}
    eng, masks, hist, probs, gt = run(min_prop, adapt=params)
    calls = [c for c in eng.calls if c[0] == 'adapt_targets']
    assert len(hist) == 3 and len(calls) == 2                               # one per adaptation round
    assert not [c for c in eng.calls if c[0] == 'propagation_targets']
    seeded = probs.clone()
    seeded[0] = 2 * gt
    for c, fs in zip(calls, ([3, 2], [6, 5])):
        assert c[1:5] == (band[0], band[1], params, evaluate.PROPAGATION_IGNORE)
        assert torch.equal(c[5], seeded[fs]) and torch.equal(c[6], seeded[[f - 1 for f in fs]])       # the anchors: frames f - 1
    losses = [c for c in eng.calls if c[0] == 'loss']
    n0, n1 = len(hist[0]), len(hist[1])
    r0, r1, r2 = losses[:n0], losses[n0:n0 + n1], losses[n0 + n1:]
    assert all(c[3] is None for c in r0)
    # round 1: frame 3 has no positive and is dropped, frame 2 joins with its look-alike as a negative
    assert r1 and all(c[3] == evaluate.PROPAGATION_IGNORE and c[2].shape[0] == 2 for c in r1)
    t = r1[0][2]
    assert torch.equal(t[0], gt.view(1, H, W))                              # rule 8: the train frame's ground truth
    assert (t[1, 0, 2:6, 1:5] == 1).all() and (t[1, 0, 2:6, 12:16] == 0).all()
    want, n_want = R.targets(seeded[[3, 2], 0].numpy(), seeded[[2, 1], 0].numpy(), band[0], band[1], 4, 0)
    ones = 16 + (2 if band[0] == 0.0 else 1)                                # the object, and 0.7 (with 0.5 under the scalar) of row 0
    assert n_want == [0, ones] and int((t[1] == 1).sum()) == ones and np.array_equal(bits(t[1, 0].numpy()), bits(want[1]))
    # round 2: frame 5 has no positive, frame 6 no anchor: the train frame alone, the plain loss
    assert r2 and all(c[3] is None and c[2].shape[0] == 1 for c in r2)
    # without the gate the look-alike is a positive target of round 1 and frame 6 joins round 2
    off, _, _, _, _ = run(min_prop)
    plain = [c for c in off.calls if c[0] == 'loss']
    assert (plain[n0][2][1, 0, 2:6, 12:16] == 1).all() and plain[-1][2].shape[0] == 2


def test_on_uses_the_twin_on_an_engine_without_the_entry_point():
    eng, masks, hist, probs, gt = run([0.3, 0.7], engine_cls=L.StubEngine, adapt={'neg_dist': 4})
    assert not [c for c in eng.calls if c[0] == 'propagation_targets']
    losses = [c for c in eng.calls if c[0] == 'loss']
    t = losses[len(hist[0])][2]
    assert t.shape[0] == 2 and (t[1, 0, 2:6, 12:16] == 0).all() and t[1, 0, 0, :3].tolist() == [255.0, 1.0, 255.0]


@pytest.mark.parametrize('bad', [0, 0.0, 1.5])
def test_a_scalar_the_gate_cannot_use_raises_before_any_engine_work(bad):
    eng = GateEngine(torch.zeros(5, 1, 4, 6))
    cfg = {'eval_online_adapt': {'step': 2, 'reset_model_mode': 'FIRST_STEP', 'num_epochs': 2, 'min_prop': bad},
           'data_cfg': {'batch_sizes': {'train': 3}}, 'num_epochs': {'eval': 2}}
    gen = evaluate.finetune_object_steps(L.StubModel(eng), L.StubMetaOptim(), {}, torch.zeros(5, 3, 4, 6), torch.zeros(1, 4, 6), cfg,
                                         adapt={'neg_dist': 3})
    with pytest.raises(ValueError):
        next(gen)
    assert not eng.calls
    gen = evaluate.finetune_object_steps(L.StubModel(eng), L.StubMetaOptim(), {}, torch.zeros(5, 3, 4, 6), torch.zeros(1, 4, 6), cfg,
                                         adapt={'neg_dist': 0})
    next(gen)                                                                # off: the scalar is today's business


def test_the_keyword_travels_only_when_set():
    from eosvos_amd import eval_options
    assert eval_options.travelling({'adapt': None}) == {} and eval_options.travelling({'adapt': {'neg_dist': 3}}) == {'adapt': {'neg_dist': 3}}
    import inspect
    for fn in (evaluate.finetune_object, evaluate.finetune_object_steps, evaluate.run_objects_in_flight, evaluate.evaluate_sequence,
               evaluate.evaluate_dataset):
        # the functions take the groups through one `**groups` checked against the table: `adapt` is accepted, and optional
        assert inspect.signature(fn).parameters['groups'].kind is inspect.Parameter.VAR_KEYWORD, fn.__name__
        assert eval_options.split(fn.__name__, {}) == ({}, {}) and eval_options.split(fn.__name__, {'adapt': None}, merge=False) == ({}, {})
        assert eval_options.split(fn.__name__, {'adapt': {'neg_dist': 3}}, merge=False) == ({'adapt': {'neg_dist': 3}}, {})
    assert eval_options.from_cfg({'eval_adapt': None}) == {} and eval_options.from_cfg({'eval_adapt': {'neg_dist': 3}}) == {'adapt': {'neg_dist': 3}}
    for name in ('eval_worker.py', 'train_meta.py'):
        assert '**eval_options.from_cfg(cfg)' in open(os.path.join(ROOT, 'e-osvos_amd', name)).read(), name


def test_entries_are_declared_at_every_layer():
    header = open(os.path.join(ROOT, 'include', 'eosvos.h')).read()
    from eosvos_amd import _ffi
    for name in ('eosvos_distance_sq', 'eosvos_adapt_targets'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert name in _ffi.exported_symbols()
    assert 'OnAVOS' in header and 'evaluate.py:231-240' in header
    makefile = open(os.path.join(ROOT, 'e-osvos_amd', 'csrc', 'Makefile')).read()
    assert 'edt_kernels.o' in makefile
