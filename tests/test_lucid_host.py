"""Lucid first-frame synthesis on the host (`eosvos_amd/lucid.py`): the numpy twins against the plain loops of
tests/lucid_ref.py, the parameter checks, `parse_cli`, properties of the rules, the batch rules on the twins, and the wiring
through `evaluate_sequence` with the CPU stand-in of tests/fake_engine.py extended by the two lucid entry points restated
through the twins."""
import copy
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import lucid_ref  # noqa: E402
from fake_engine import FakeDeepLab, FakeEngine  # noqa: E402

from eosvos_amd import _ffi, config, lucid  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402
from eosvos_amd.meta_optim import MetaOptimizer  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- the twins against the plain loops ------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', lucid_ref.SIZES, ids=[f'{h}x{w}' for h, w in lucid_ref.SIZES])
@pytest.mark.parametrize('dilate', [0, 4])
def test_plate_host_equals_the_plain_loops(hw, dilate):
    fr, m = lucid_ref.frame(*hw), lucid_ref.mask(*hw)
    got, want = lucid.plate_host(fr, m, dilate), lucid_ref.plate_loops(fr, m, dilate)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
    hole = lucid.hole_host(m[0] != 0, dilate)
    assert hole.any() and not hole.all() and not np.array_equal(got, fr)


@pytest.mark.parametrize('hw', lucid_ref.SIZES, ids=[f'{h}x{w}' for h, w in lucid_ref.SIZES])
def test_compose_host_equals_the_plain_loops(hw):
    fr, m = lucid_ref.frame(*hw), lucid_ref.mask(*hw)
    plate = lucid.plate_host(fr, m, 4)
    n_mask, centre = lucid.mask_geometry(m)
    cases = lucid_ref.compose_cases(*hw, centre)
    if hw == lucid_ref.SIZES[-1]:                                       # the plain loops take a second per sample at this size
        cases = cases[2:3] + cases[4:]
    prm = [p for _, p in cases]
    im, lb, cn = lucid.compose_host(fr, m, plate, prm)
    im2, lb2, cn2 = lucid_ref.compose_loops(fr, m, plate, prm)
    assert np.array_equal(_bits(im), _bits(im2)) and np.array_equal(lb, lb2) and cn.tolist() == cn2.tolist()
    assert set(np.unique(lb)) == {0.0, 1.0}
    names = [n for n, _ in cases]
    assert 0 < cn[names.index('leaving the frame')] < 0.8 * n_mask       # the case is what its name says


# ---- parameters -----------------------------------------------------------------------------------------------------------
BAD = [{'samples': -1}, {'samples': 1.0}, {'samples': True}, {'dilate': -1}, {'dilate': 17}, {'dilate': 2.0},
       {'rot': -1}, {'rot': 45.5}, {'rot': '3'}, {'bg_rot': -0.1}, {'bg_rot': 46}, {'scale': -0.1}, {'scale': 0.51},
       {'bg_scale': -0.1}, {'bg_scale': 0.6}, {'shift': -0.1}, {'shift': 1.01}, {'bg_shift': -1}, {'bg_shift': 2},
       {'min_keep': 0}, {'min_keep': 1.01}, {'min_keep': float('nan')}, {'rot': float('nan')}, {'lucid': 2}, [2], 'samples=2']


@pytest.mark.parametrize('bad', BAD, ids=[repr(b) for b in BAD])
def test_every_limit_raises_value_error(bad):
    with pytest.raises(ValueError):
        lucid.check(bad)
    with pytest.raises(ValueError):
        lucid.active(bad)


def test_limits_are_inclusive_and_off_is_off():
    assert lucid.DEFAULTS == {'samples': 0, 'dilate': 4, 'rot': 15.0, 'scale': 0.15, 'shift': 0.1, 'bg_rot': 5.0, 'bg_scale': 0.05,
                              'bg_shift': 0.05, 'min_keep': 0.5}
    for ok in ({}, {'samples': 100}, {'dilate': 0}, {'dilate': 16}, {'rot': 0, 'bg_rot': 45}, {'scale': 0.5, 'bg_scale': 0},
               {'shift': 1, 'bg_shift': 0}, {'min_keep': 1}, {'min_keep': 1e-6}):
        assert set(lucid.check(ok)) == set(lucid.DEFAULTS)
    assert not lucid.active(None) and not lucid.active({}) and not lucid.active({'samples': 0}) and not lucid.active(lucid.DEFAULTS)
    assert lucid.active({'samples': 1})


def test_parse_cli_carries_eval_lucid_only_when_asked():
    groups = ('EXTENSIONS', 'POSTPROCESS', 'CLEANUP', 'FILL', 'SNAP', 'MOTION', 'ZOOM', 'LUCID')
    before = copy.deepcopy({g: getattr(config, g) for g in groups + ('BASE',)})
    assert config.LUCID == {'eval_lucid': lucid.DEFAULTS}
    assert 'eval_lucid' not in config.BASE and 'eval_lucid' not in config.parse_cli([])
    assert 'eval_lucid' not in config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS-OnA', 'num_epochs.eval=3', 'eval_zoom.max_zoom=3'])
    cfg = config.parse_cli(['eval_lucid.samples=2', 'eval_lucid.shift=0.2'])
    assert cfg['eval_lucid'] == dict(lucid.DEFAULTS, samples=2, shift=0.2)
    assert all(g not in cfg for g in ('eval_tta', 'eval_crf', 'eval_components', 'eval_holes', 'eval_snap', 'eval_motion', 'eval_zoom'))
    assert {g: getattr(config, g) for g in groups + ('BASE',)} == before                        # nothing leaked
    with pytest.raises(KeyError):
        config.parse_cli(['eval_lucid.lucid=3'])
    for argv in (['eval_lucid.samples=-1'], ['eval_lucid.dilate=17'], ['eval_lucid.samples=2', 'eval_lucid.min_keep=0'],
                 ['eval_lucid.rot=46'], ['eval_lucid.shift=1.5']):
        with pytest.raises(ValueError):
            config.parse_cli(argv)


# ---- properties of the rules ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', lucid_ref.SIZES, ids=[f'{h}x{w}' for h, w in lucid_ref.SIZES])
def test_properties_of_the_rules(hw):
    h, w = hw
    fr, m = lucid_ref.frame(*hw), lucid_ref.mask(*hw)
    n_mask, centre = lucid.mask_geometry(m)
    assert n_mask == int((m != 0).sum())
    # dilate 0, identity matrices, no flip: the frame and its mask, bit for bit
    plate0 = lucid.plate_host(fr, m, 0)
    ident = {'flip': False, 'Bi': lucid.IDENTITY, 'Oi': lucid.IDENTITY}
    im, lb, cn = lucid.compose_host(fr, m, plate0, [ident])
    assert np.array_equal(_bits(im[0]), _bits(fr)) and np.array_equal(lb[0], (m != 0).astype(np.float32)) and cn[0] == n_mask
    assert lucid_ref.sample(h, w, centre)['Oi'] == pytest.approx(lucid.IDENTITY, abs=1e-12)
    # known pixels of the plate carry the frame's bits; the hole is filled with something finite inside the frame's range
    plate = lucid.plate_host(fr, m, 4)
    known = ~lucid.hole_host(m[0] != 0, 4)
    assert np.array_equal(_bits(plate[:, known]), _bits(fr[:, known]))
    assert np.isfinite(plate).all() and plate[:, ~known].min() >= fr.min() and plate[:, ~known].max() <= fr.max()
    assert not np.array_equal(plate[:, ~known], fr[:, ~known])
    # a full mask: nothing is known, the plate is zero
    assert not lucid.plate_host(fr, np.ones_like(m), 4).any()
    # an empty mask: everything is known, the plate is the frame
    assert np.array_equal(_bits(lucid.plate_host(fr, np.zeros_like(m), 4)), _bits(fr))
    # flip is the mirror of the unflipped sample
    for (_, a), (_, b) in zip(lucid_ref.compose_cases(h, w, centre)[1::2], lucid_ref.compose_cases(h, w, centre)[2::2]):
        assert not a['flip'] and b['flip'] and a['Oi'] == b['Oi']
        ia, la, ca = lucid.compose_host(fr, m, plate, [a])
        ib, lb_, cb = lucid.compose_host(fr, m, plate, [b])
        assert np.array_equal(_bits(ib), _bits(ia[..., ::-1])) and np.array_equal(lb_, la[..., ::-1]) and ca[0] == cb[0]
    # the fp64 twin differs from the fp32 one by rounding only
    p64 = lucid.plate_host(fr, m, 4, np.float64)
    assert p64.dtype == np.float64 and 0 < np.abs(p64 - plate).max() < 1e-5


def test_matrices_and_fixed_point():
    m = lucid.forward_matrix(10.0, 7.0, 30.0, 1.25, 3.0, -2.0)
    inv = lucid.invert(m)
    x, y = 4.0, 9.0
    fx, fy = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    assert (inv[0] * fx + inv[1] * fy + inv[2], inv[3] * fx + inv[4] * fy + inv[5]) == pytest.approx((x, y), abs=1e-9)
    assert (m[0] * 10 + m[1] * 7 + m[2], m[3] * 10 + m[4] * 7 + m[5]) == pytest.approx((13.0, 5.0), abs=1e-9)    # c -> c + t
    yq, xq = lucid.fixed_coords(lucid.IDENTITY, 5, 7, False)
    assert np.array_equal(yq, 32 * np.arange(5)[:, None].repeat(7, 1)) and np.array_equal(xq, 32 * np.arange(7)[None].repeat(5, 0))
    assert np.array_equal(lucid.fixed_coords(lucid.IDENTITY, 5, 7, True)[1], xq[:, ::-1])
    tab = lucid.cubic_table()
    assert tab[0].tolist() == [0.0, 1.0, 0.0, 0.0] and np.abs(tab.sum(axis=1) - 1).max() < 1e-6
    assert lucid.levels(33, 65) == [(33, 65), (17, 33), (9, 17), (5, 9), (3, 5), (2, 3), (1, 2), (1, 1)]          # width 2 at height 1
    assert lucid.levels(37, 53) == [(37, 53), (19, 27), (10, 14), (5, 7), (3, 4), (2, 2), (1, 1)]
    assert lucid.accepted(50, 100, 10, 20, 0.5) and not lucid.accepted(49, 100, 10, 20, 0.5) and not lucid.accepted(200, 100, 10, 20, 0.5)


# ---- rules 10-12 on the twins ---------------------------------------------------------------------------------------------
H0, W0 = lucid_ref.SIZES[0]
CORNER = dict(lucid.DEFAULTS, samples=3, shift=0.3)                   # seed 1: tries 4, 3, 2 and no fallback (picked on the twin)
FALLBACK = dict(lucid.DEFAULTS, samples=3, shift=1.0, min_keep=1.0)   # seed 1: sample 0 reaches the identity fallback


def test_batch_host_draws_redraws_and_falls_back():
    fr = lucid_ref.frame(H0, W0)
    tries = []
    for seed in range(10):                                              # a centred object with DEFAULTS: every first draw is accepted
        rec = lucid.batch_host(fr, lucid_ref.centred_mask(H0, W0), dict(lucid.DEFAULTS, samples=4), 4, random.Random(seed))[2]
        tries += [r['tries'] for r in rec]
    assert tries == [1] * 40
    m = lucid_ref.corner_mask(H0, W0)
    n_mask = int(m.sum())
    im, lb, rec = lucid.batch_host(fr, m, CORNER, 3, random.Random(1))
    assert [(r['tries'], r['fallback']) for r in rec] == [(4, False), (3, False), (2, False)]
    assert all(lucid.accepted(r['count'], n_mask, H0, W0, 0.5) for r in rec) and [r['count'] for r in rec] == lb.reshape(3, -1).sum(1).tolist()
    # the order of the draws: 9 per sample, then 4 per redrawn sample in sample order
    rng = random.Random(1)
    first = [lucid.draw_sample(rng, lucid.check(CORNER)) for _ in range(3)]
    assert [r['draw']['bg'] for r in rec] == [d['bg'] for d in first] and [r['flip'] for r in rec] == [d['flip'] for d in first]
    second = [lucid.draw_motion(rng, lucid.check(CORNER)) for _ in range(3)]
    assert rec[2]['draw']['ob'] == second[2] and rec[0]['draw']['ob'] != second[0]
    ref, used = random.Random(1), random.Random(1)
    for _ in range(9 * 3 + 4 * (3 + 2 + 1)):                            # 27 + 12 + 8 + 4 draws in all
        ref.random()
    lucid.batch_host(fr, m, CORNER, 3, used)
    assert used.getstate() == ref.getstate()
    # the fallback: the identity object matrix with the last background draw
    im, lb, rec = lucid.batch_host(fr, m, FALLBACK, 3, random.Random(1))
    assert [(r['tries'], r['fallback']) for r in rec] == [(8, True), (4, False), (2, False)]
    assert rec[0]['Oi'] == lucid.IDENTITY and rec[0]['draw']['ob'] is None and int(lb[0].sum()) == n_mask
    want = m[:, :, ::-1] if rec[0]['flip'] else m
    assert np.array_equal(lb[0], want)
    # layout: plain samples first, no plain call for 0, everything plain for a mask without object or background
    calls = []

    def plain(n):
        calls.append(n)
        return np.repeat(fr[None], n, 0), np.repeat(m[None], n, 0)
    im, lb, rec = lucid.batch_host(fr, m, dict(CORNER, samples=2), 3, random.Random(1), plain=plain)
    assert calls == [1] and len(rec) == 2 and im.shape == (3, 3, H0, W0) and np.array_equal(im[0], fr) and not np.array_equal(im[1], fr)
    assert lucid.batch_host(fr, m, dict(CORNER, samples=7), 3, random.Random(1), plain=None)[0].shape[0] == 3       # cut to the batch
    for blank in (np.zeros_like(m), np.ones_like(m)):
        calls.clear()
        im, lb, rec = lucid.batch_host(fr, blank, CORNER, 3, random.Random(1), plain=plain)
        assert calls == [3] and rec == []


# ---- the stand-in with the two entry points -------------------------------------------------------------------------------
class LucidEngine(FakeEngine):
    """The stand-in with the two lucid calls restated through the numpy twins in fp32; every call is logged."""
    calls = []

    def lucid_plate(self, frame, mask, dilate):
        LucidEngine.calls.append(('lucid_plate', dilate))
        return torch.from_numpy(lucid.plate_host(frame, mask, dilate))

    def lucid_compose(self, frame, mask, plate, params, read_counts=True):
        LucidEngine.calls.append(('lucid_compose', len(params), read_counts))
        im, lb, cn = lucid.compose_host(frame, mask, plate, params)
        return torch.from_numpy(im), torch.from_numpy(lb), (cn.tolist() if read_counts else None)


class LucidDeepLab(FakeDeepLab):
    def _ensure_engine(self, height, width, batch):
        e = self.engine
        if e is None or e.height != height or e.width != width or batch > e.max_batch:
            self.engine = LucidEngine(self.encoder, height, width, max(batch, self.max_batch))
            self._dirty = True
        return super()._ensure_engine(height, width, batch)

    def __call__(self, inputs):
        self.__dict__.setdefault('seen', []).append(inputs.clone())
        return super().__call__(inputs)


def _setup():
    cfg = config.parse_cli([])
    cfg['num_epochs']['eval'] = 3
    cfg['eval_online_adapt'].update(step=3, reset_model_mode='FIRST_STEP', num_epochs=2, min_prop=0.5)
    cfg['data_cfg']['batch_sizes']['train'] = 3
    model = LucidDeepLab('resnet50', num_classes=1, batch_norm=cfg['parent_model']['batch_norm'], max_batch=3)
    model._flat[0], model._flat[-1] = 6.0, -3.0
    mo = MetaOptimizer(model, **cfg['meta_optim_cfg'])
    frames = torch.zeros(5, 3, 40, 48)
    for i in range(5):
        frames[i, :, 10 + i:18 + i, 12 + i:20 + i] = 1.0
    frames += 0.05 * torch.rand(5, 3, 40, 48, generator=torch.Generator().manual_seed(2))
    gt = torch.zeros(1, 40, 48)
    gt[:, 10:18, 12:20] = 1.0
    return cfg, model, mo, mo.state_dict(), frames, gt


def _raise(*a, **k):
    raise AssertionError('a lucid call on the plain path')


def test_off_makes_exactly_todays_calls_and_draws(monkeypatch):
    from eosvos_amd.evaluate import evaluate_sequence
    cfg, model, mo, msd, frames, gt = _setup()
    for cls in (Engine, LucidEngine):
        for name in ('lucid_plate', 'lucid_compose'):
            assert callable(getattr(cls, name))
            monkeypatch.setattr(cls, name, _raise)
    monkeypatch.setattr(lucid, 'LucidAugmenter', _raise)
    outs, states, seen = [], [], []
    for kw in ({}, {'lucid': None}, {'lucid': {'samples': 0}}, {'lucid': dict(lucid.DEFAULTS)}):
        model.seen = []
        outs.append(evaluate_sequence(model, mo, msd, frames, [gt], cfg, **kw))
        states.append(random.getstate())
        seen.append(model.seen)
    for (labels, probs, hist), st, sn in zip(outs[1:], states[1:], seen[1:]):
        assert torch.equal(labels, outs[0][0]) and torch.equal(probs[0], outs[0][1][0]) and hist == outs[0][2]
        assert st == states[0]
        assert len(sn) == len(seen[0]) and all(torch.equal(a, b) for a, b in zip(sn, seen[0]))
    with pytest.raises(AssertionError, match='lucid call'):
        evaluate_sequence(model, mo, msd, frames, [gt], cfg, lucid={'samples': 2})                  # and on means on
    with pytest.raises(ValueError):
        evaluate_sequence(model, mo, msd, frames, [gt], cfg, lucid={'samples': -1})


def test_evaluate_sequence_trains_round_0_on_plain_then_lucid_samples():
    from eosvos_amd.evaluate import evaluate_sequence, finetune_object, object_workers, run_objects_in_flight
    from eosvos_amd.helper_func import set_random_seeds
    cfg, model, mo, msd, frames, gt = _setup()
    L = {'samples': 2, 'shift': 0.2}
    model.seen = []
    plain = evaluate_sequence(model, mo, msd, frames, [gt], cfg)
    plain_seen, n_calls = model.seen, len(model.seen)
    model.seen, LucidEngine.calls = [], []
    labels, probs, hist = evaluate_sequence(model, mo, msd, frames, [gt], cfg, lucid=L)
    assert len(model.seen) == n_calls and len(hist[0][0]) == 3
    assert [c for c in LucidEngine.calls if c[0] == 'lucid_plate'] == [('lucid_plate', 4)]          # once per object
    assert len([c for c in LucidEngine.calls if c[0] == 'lucid_compose' and c[1] == 2]) == 3        # one launch per round-0 batch
    fr, m = frames[0].numpy(), gt.numpy()
    for epoch in (1, 2, 3):                                             # the batches of rule 12, draw for draw
        set_random_seeds(cfg.get('seed', 1) + epoch)
        im, lb, rec = lucid.batch_host(fr, m, L, 3, plain=lambda n: (np.repeat(fr[None], n, 0), np.repeat(m[None], n, 0)))
        got = model.seen[epoch - 1]
        assert got.shape == (3, 3, 40, 48) and np.array_equal(_bits(got.numpy()), _bits(im))
        assert np.array_equal(_bits(got[0].numpy()), _bits(fr)) and not np.array_equal(got[1].numpy(), fr)
    assert n_calls > 3 and all(a.shape == b.shape for a, b in zip(model.seen[3:], plain_seen[3:]))       # the adaptation rounds: as now
    assert all(torch.equal(a[:1], frames[:1]) for a in model.seen[3:])                              # ... on real frames
    assert torch.equal(probs[0][0], plain[1][0][0]) and not torch.equal(probs[0][1:], plain[1][0][1:])
    # samples above the batch size are cut to it: no plain sample, no call of today's path
    model.seen = []
    evaluate_sequence(model, mo, msd, frames, [gt], cfg, lucid={'samples': 9}, augment=_raise_augment)
    assert model.seen[0].shape[0] == 3
    # a mask without object: every batch is today's
    model.seen, LucidEngine.calls = [], []
    evaluate_sequence(model, mo, msd, frames, [torch.zeros_like(gt)], cfg, lucid=L)
    assert LucidEngine.calls == [] and torch.equal(model.seen[0], frames[:1].expand(3, -1, -1, -1))
    # the objects-in-flight path passes it through, with the same result as one object after the other
    gts = [gt, torch.roll(gt, 3, 2)]
    one = [finetune_object(model, mo, msd, frames, g, cfg, lucid=L) for g in gts]
    con = run_objects_in_flight(object_workers(model, mo, cfg['meta_optim_cfg'], 2), msd, frames, gts, cfg, lucid=L)
    for (p2, h2), (p1, h1) in zip(con, one):
        assert h2 == h1 and torch.equal(p2, p1)


def _raise_augment(frame, gt, batch, seed):
    raise AssertionError('today\'s path was called for 0 samples')


# ---- the library ----------------------------------------------------------------------------------------------------------
def test_abi_symbols_exist_in_the_built_library():
    lib = _ffi.load()
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'eosvos.h')).read()
    exported = _ffi.exported_symbols()
    for name, n_args in (('eosvos_lucid_plate', 8), ('eosvos_lucid_compose', 13)):
        assert name in exported and len(getattr(lib, name).argtypes) == n_args and name + '(' in hdr
        decl = hdr[hdr.rindex('int ' + name + '('):]
        assert decl[:decl.index(';')].count(',') + 1 == n_args                                 # the header's argument count
    # null engines are refused on the host, before anything touches a device
    assert lib.eosvos_lucid_plate(None, None, None, 3, 8, 8, 4, None) == 1
    assert b'null' in lib.eosvos_last_error()
    assert lib.eosvos_lucid_compose(None, None, None, None, 3, 8, 8, 1, None, None, None, None, None) == 1
    assert b'null' in lib.eosvos_last_error()
