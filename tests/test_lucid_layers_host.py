"""Lucid synthesis with the other objects as moving layers, on the host (`eosvos_amd/lucid_layers.py`): the numpy twin against
the plain loops of tests/lucid_layers_ref.py, rule L6 on the twin, the order of the draws against a recording generator, the
parameter checks, `parse_cli`, and the wiring through `evaluate_sequence` with the CPU stand-in of tests/fake_engine.py extended by
the lucid entry points restated through the twins."""
import copy
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import lucid_layers_ref as ref  # noqa: E402
import lucid_ref  # noqa: E402
from fake_engine import FakeDeepLab, FakeEngine  # noqa: E402

from eosvos_amd import _ffi, config, lucid, lucid_layers as ll  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402
from eosvos_amd.meta_optim import MetaOptimizer  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- the twin against the plain loops ---------------------------------------------------------------------------------------
TWIN_SIZES = [(1, 1), (7, 5), lucid_ref.SIZES[0]]


@pytest.mark.parametrize('n_layers', [1, 2, 3, 8])
@pytest.mark.parametrize('hw', TWIN_SIZES, ids=[f'{h}x{w}' for h, w in TWIN_SIZES])
def test_compose_host_equals_the_plain_loops(hw, n_layers):
    fr, ids = lucid_ref.frame(*hw), ref.id_map(*hw, n_layers)
    plate = lucid.plate_host(fr, ids != 0, 2)
    prm = ref.samples(*hw, n_layers)
    if hw == TWIN_SIZES[-1]:                                            # the plain loops take a second per sample at this size
        prm = prm[1:]
    im, lb, io, cn = ll.compose_host(fr, ids, plate, prm)
    im2, lb2, io2, cn2 = ref.compose_loops(fr, ids, plate, prm)
    assert im.dtype == np.float32 and np.array_equal(_bits(im), _bits(im2))
    assert np.array_equal(lb, lb2) and np.array_equal(io, io2) and cn.tolist() == cn2.tolist()
    assert cn[:, n_layers:].sum() == 0 and np.array_equal(lb[:, 0], (io == 1).astype(np.float32))
    if hw == TWIN_SIZES[-1]:                                            # the cases are what the docstring says
        assert (cn[:, :n_layers] > 0).any(axis=0).sum() >= min(n_layers, 2)                     # layers that show ...
        assert n_layers == 1 or any(cn[s, k] < (ids == i).sum() // 2 for s, p in enumerate(prm) for k, (i, _) in enumerate(p['layers']))


def test_one_layer_is_todays_compose_on_the_twin():
    hw = lucid_ref.SIZES[0]
    fr, m = lucid_ref.frame(*hw), lucid_ref.mask(*hw)
    plate = lucid.plate_host(fr, m, 4)
    cases = [p for _, p in lucid_ref.compose_cases(*hw, lucid.mask_geometry(m)[1])]
    im, lb, cn = lucid.compose_host(fr, m, plate, cases)
    ids = (m[0] != 0).astype(np.uint8)
    im2, lb2, io, cn2 = ll.compose_host(fr, ids, plate, [{'flip': p['flip'], 'Bi': p['Bi'], 'layers': [(1, p['Oi'])]} for p in cases])
    assert np.array_equal(_bits(im), _bits(im2)) and np.array_equal(lb, lb2) and cn.tolist() == cn2[:, 0].tolist()
    assert np.array_equal(io, lb[:, 0].astype(np.uint8))


def test_depth_order_decides_who_is_seen():
    h, w = 12, 16
    fr = lucid_ref.frame(h, w)
    ids = np.zeros((h, w), dtype=np.uint8)
    ids[2:8, 2:8], ids[2:8, 9:15] = 1, 2
    plate = lucid.plate_host(fr, ids != 0, 1)
    over = lucid.invert((1.0, 0.0, -7.0, 0.0, 1.0, 0.0))             # object 2 moved 7 pixels left: onto the target
    for order, seen in (([(1, lucid.IDENTITY), (2, over)], 2), ([(2, over), (1, lucid.IDENTITY)], 1)):
        im, lb, io, cn = ll.compose_host(fr, ids, plate, [{'flip': False, 'Bi': lucid.IDENTITY, 'layers': order}])
        assert (io[0, 2:8, 2:8] == seen).all() and lb[0, 0, 2:8, 2:8].all() == (seen == 1)
        assert cn[0, :2].tolist() == [0, 36]                                                    # the layer behind is hidden entirely
        assert np.array_equal(_bits(im[0, :, 2:8, 2:8]), _bits(fr[:, 2:8, 9:15] if seen == 2 else fr[:, 2:8, 2:8]))


# ---- the map, its geometry and rule L9 ----------------------------------------------------------------------------------------
def test_layer_map_geometry_and_choice():
    h, w = 9, 11
    t = torch.zeros(1, h, w)
    t[0, 2:5, 2:5] = 1
    a, b, c, d = (torch.zeros(1, h, w) for _ in range(4))
    a[0, 3:7, 4:8] = 1                                                  # partly under the target and under c
    b[0, 3:4, 3:4] = 1                                                  # wholly under the target: no pixel in the map
    c[0, 5:9, 6:10] = 5.0                                               # any non-zero value is the object
    ids = ll.layer_map(t, torch.stack([a, b, c, d]))
    assert ids.dtype == torch.uint8 and ids.shape == (h, w) and ids.is_contiguous()
    want = np.zeros((h, w), dtype=np.uint8)
    want[3:7, 4:8], want[5:9, 6:10], want[2:5, 2:5] = 2, 4, 1           # the target first, else the largest id
    assert np.array_equal(ids.numpy(), want) and np.array_equal(ll.layer_map_host(t, [a, b, c, d]), want)
    assert np.array_equal(ll.layer_map(t[0], None).numpy(), (t[0] != 0).numpy().astype(np.uint8))
    geo = ll.geometry(ids, 5)
    assert [g[0] for g in geo] == [int((want == i).sum()) for i in range(6)] and geo[3] == (0, None) and geo[5] == (0, None)
    assert geo[1] == lucid.mask_geometry(t) and geo[4] == (16, (8.0, 7.0))
    assert ll.choose(geo, 7) == [2, 4] and ll.choose(geo, 1) == [2] and ll.choose(geo, 0) == []
    for cap, kept in ((7, {2: 2, 4: 3}), (1, {2: 2})):
        got, g2 = ll.select(ids, {'others': cap}, 5)
        exp = np.where(want == 1, 1, 0).astype(np.uint8)
        for old, new in kept.items():
            exp[want == old] = new
        assert np.array_equal(got.numpy(), exp) and np.array_equal(ll.select(want, {'others': cap}, 5)[0], exp)
        assert g2 == [geo[0], geo[1]] + [geo[i] for i in kept]


# ---- parameters ---------------------------------------------------------------------------------------------------------------
BAD = [{'others': -1}, {'others': 8}, {'others': 1.0}, {'others': True}, {'others': '2'}, {'front': -0.1}, {'front': 1.01},
       {'front': float('nan')}, {'front': '0.5'}, {'front': True}, {'layers': 2}, [2], 'others=2']


@pytest.mark.parametrize('bad', BAD, ids=[repr(b) for b in BAD])
def test_every_limit_raises_value_error(bad):
    with pytest.raises(ValueError):
        ll.check(bad)
    with pytest.raises(ValueError):
        ll.active(bad)


def test_limits_are_inclusive_and_off_is_off():
    assert ll.DEFAULTS == {'others': 0, 'front': 0.5}
    for ok in ({}, {'others': 7}, {'others': 0}, {'front': 0}, {'front': 1}, {'others': 3, 'front': 0.25}):
        assert set(ll.check(ok)) == set(ll.DEFAULTS)
    assert not ll.active(None) and not ll.active({}) and not ll.active({'others': 0}) and not ll.active(ll.DEFAULTS)
    assert ll.active({'others': 1})
    assert (ll.MAX_LAYERS, ll.MAX_OTHERS, ll.MAX_SAMPLES_PER_LAUNCH) == (8, 7, 8)


def test_parse_cli_carries_eval_lucid_layers_only_when_asked():
    groups = ('EXTENSIONS', 'POSTPROCESS', 'CLEANUP', 'FILL', 'SNAP', 'MOTION', 'ZOOM', 'LUCID', 'ADAPT', 'LAYERS')
    before = copy.deepcopy({g: getattr(config, g) for g in groups + ('BASE',)})
    assert config.LAYERS == {'eval_lucid_layers': ll.DEFAULTS} and config.LUCID == {'eval_lucid': lucid.DEFAULTS}
    assert 'eval_lucid_layers' not in config.BASE and 'eval_lucid_layers' not in config.parse_cli([])
    assert 'eval_lucid_layers' not in config.parse_cli(['eval_lucid.samples=2'])
    cfg = config.parse_cli(['eval_lucid.samples=2', 'eval_lucid_layers.others=3'])
    assert cfg['eval_lucid_layers'] == {'others': 3, 'front': 0.5} and cfg['eval_lucid'] == dict(lucid.DEFAULTS, samples=2)
    cfg = config.parse_cli(['eval_lucid_layers.front=0.25'])             # carried, inactive: no consumer is needed
    assert cfg['eval_lucid_layers'] == {'others': 0, 'front': 0.25} and 'eval_lucid' not in cfg
    assert {g: getattr(config, g) for g in groups + ('BASE',)} == before                        # nothing leaked
    with pytest.raises(KeyError):
        config.parse_cli(['eval_lucid_layers.layers=3'])
    for argv in (['eval_lucid_layers.others=8'], ['eval_lucid_layers.others=-1'], ['eval_lucid_layers.others=1.5'],
                 ['eval_lucid_layers.front=1.5'], ['eval_lucid_layers.front=-1'],
                 ['eval_lucid_layers.others=2'],                         # no consumer: eval_lucid is not there ...
                 ['eval_lucid_layers.others=2', 'eval_lucid.samples=0'], ['eval_lucid_layers.others=2', 'eval_lucid.shift=0.2']):
        with pytest.raises(ValueError):
            config.parse_cli(argv)


# ---- rules L7-L8: the draws -----------------------------------------------------------------------------------------------
class Recording(random.Random):
    """Python's generator with every `random()` logged."""

    def __init__(self, seed):
        super().__init__(seed)
        self.log = []

    def random(self):
        v = super().random()
        self.log.append(v)
        return v


H0, W0 = lucid_ref.SIZES[0]
L2 = {'others': 2, 'front': 0.5}
PLACID = dict(lucid.DEFAULTS, samples=3)                                 # seed 0: every first draw is accepted
REDRAW = dict(lucid.DEFAULTS, samples=3, shift=0.3)                      # seed 5: tries 4, 2, 3 (picked on the twin)
FALLBACK = dict(lucid.DEFAULTS, samples=3, shift=1.0, min_keep=1.0)      # seed 1: tries 6 and 2; sample 1 reaches the fallback with an object drawn in front


def scene():
    """The frame, a target in the corner and two other objects beside it (one overlapping it)."""
    fr = lucid_ref.frame(H0, W0)
    t = lucid_ref.corner_mask(H0, W0)
    a, b = np.zeros_like(t), np.zeros_like(t)
    a[0, 4:16, 8:24] = 1
    b[0, 20:32, 30:48] = 1
    return fr, t, [a, b]


def today(rng, p):
    return lucid.draw_sample(rng, p)


def replay(log, prm, n_others, records):
    """Walks the logged draws in the order of rule L7 and checks them against the records; returns how many it used."""
    p = lucid.check(prm)

    class Feed:
        def __init__(self):
            self.at = 0

        def random(self):
            self.at += 1
            return log[self.at - 1]
    feed = Feed()
    firsts = []
    for r in records:
        d = lucid.draw_sample(feed, p)                                  # today's nine come first, unchanged
        assert (d['flip'], d['bg']) == (r['draw']['flip'], r['draw']['bg']) == (r['flip'], r['draw']['bg'])
        firsts.append(d['ob'])
        others = []
        for _ in range(n_others):                                       # then five per other object
            others.append((lucid.draw_motion(feed, p), feed.random() < L2['front']))
        assert others == r['draw']['others']
    assert feed.at == len(records) * (9 + 5 * n_others)
    for attempt in range(2, lucid.MAX_TRIES + 1):                       # a redraw: the target's four only, in sample order
        for s, r in enumerate(records):
            if r['tries'] >= attempt:
                firsts[s] = lucid.draw_motion(feed, p)
    for s, r in enumerate(records):
        assert r['draw']['ob'] == (None if r['fallback'] else firsts[s])
    return feed.at


@pytest.mark.parametrize('name,prm,seed,tries', [('placid', PLACID, 0, [(1, False)] * 3),
                                                  ('redraw', REDRAW, 5, [(4, False), (2, False), (3, False)]),
                                                  ('fallback', FALLBACK, 1, [(6, False), (8, True), (2, False)])])
def test_batch_host_draws_in_the_order_of_rule_L7(name, prm, seed, tries):
    fr, t, others = scene()
    rng = Recording(seed)
    im, lb, rec = ll.batch_host(fr, t, others, prm, L2, 3, rng)
    assert [(r['tries'], r['fallback']) for r in rec] == tries          # the case is what its name says
    used = replay(rng.log, prm, 2, rec)
    assert used == len(rng.log) == 3 * (9 + 5 * 2) + 4 * sum(n - 1 for n, _ in tries)
    ids = ll.layer_map_host(t, others)
    n_mask = int((ids == 1).sum())
    for s, r in enumerate(rec):
        order = [i for i, _ in r['layers']]
        fronts = [f for _, f in r['draw']['others']]
        if r['fallback']:                                               # the identity, every other object behind
            assert order == [2, 3, 1] and dict(r['layers'])[1] == lucid.IDENTITY and r['count'] is None
            assert int(lb[s].sum()) == n_mask
            assert np.array_equal(lb[s, 0], (ids == 1)[:, ::-1] if r['flip'] else ids == 1)
        else:
            assert order == [i + 2 for i, f in enumerate(fronts) if not f] + [1] + [i + 2 for i, f in enumerate(fronts) if f]
            assert r['count'] == int(lb[s].sum()) and lucid.accepted(r['count'], n_mask, H0, W0, lucid.check(prm)['min_keep'])
    # the same generator state as a second run, and the fp64 twin draws the same
    again = Recording(seed)
    assert ll.batch_host(fr, t, others, prm, L2, 3, again, np.float64)[2] == rec and again.log == rng.log


def test_batch_host_without_layers_is_lucid_batch_host():
    fr, t, others = scene()
    blank = [np.zeros_like(t)]
    under = [t.copy()]                                                  # wholly under the target: no pixel in the id map
    for oth, lp in ((others, None), (others, {'others': 0}), (None, L2), ([], L2), (blank, L2), (under, L2)):
        a, b = Recording(1), Recording(1)
        got = ll.batch_host(fr, t, oth, REDRAW, lp, 3, a)
        want = lucid.batch_host(fr, t, REDRAW, 3, b)
        assert a.log == b.log and got[2] == want[2] and np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
    calls = []

    def plain(n):
        calls.append(n)
        return np.repeat(fr[None], n, 0), np.repeat(t[None], n, 0)
    im, lb, rec = ll.batch_host(fr, t, others, dict(PLACID, samples=2), L2, 3, random.Random(0), plain=plain)
    assert calls == [1] and len(rec) == 2 and np.array_equal(im[0], fr) and all(len(r['layers']) == 3 for r in rec)
    for tgt in (np.zeros_like(t), np.ones_like(t)):                     # rule 12: not synthesised
        calls.clear()
        assert ll.batch_host(fr, tgt, others, PLACID, L2, 3, random.Random(0), plain=plain)[2] == [] and calls == [3]
    one = ll.batch_host(fr, t, others, PLACID, {'others': 1}, 3, random.Random(0))[2]               # at most `others` of them
    assert all(sorted(i for i, _ in r['layers']) == [1, 2] for r in one)


# ---- the stand-in with the three entry points -------------------------------------------------------------------------------
class LayerEngine(FakeEngine):
    """The stand-in with the lucid calls restated through the numpy twins in fp32; every call is logged."""
    calls = []

    def lucid_plate(self, frame, mask, dilate):
        LayerEngine.calls.append(('lucid_plate', dilate, mask.clone()))
        return torch.from_numpy(lucid.plate_host(frame, mask, dilate))

    def lucid_compose(self, frame, mask, plate, params, read_counts=True):
        LayerEngine.calls.append(('lucid_compose', len(params), read_counts))
        im, lb, cn = lucid.compose_host(frame, mask, plate, params)
        return torch.from_numpy(im), torch.from_numpy(lb), (cn.tolist() if read_counts else None)

    def lucid_compose_layers(self, frame, ids, plate, samples, target_id=1, read_counts=True, want_ids=False):
        LayerEngine.calls.append(('lucid_compose_layers', len(samples), read_counts, [len(p['layers']) for p in samples]))
        im, lb, io, cn = ll.compose_host(frame, ids, plate, samples, target_id)
        counts = [cn[s, :len(p['layers'])].tolist() for s, p in enumerate(samples)] if read_counts else None
        return torch.from_numpy(im), torch.from_numpy(lb), counts, (torch.from_numpy(io) if want_ids else None)


class LayerDeepLab(FakeDeepLab):
    def _ensure_engine(self, height, width, batch):
        e = self.engine
        if e is None or e.height != height or e.width != width or batch > e.max_batch:
            self.engine = LayerEngine(self.encoder, height, width, max(batch, self.max_batch))
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
    model = LayerDeepLab('resnet50', num_classes=1, batch_norm=cfg['parent_model']['batch_norm'], max_batch=3)
    model._flat[0], model._flat[-1] = 6.0, -3.0
    mo = MetaOptimizer(model, **cfg['meta_optim_cfg'])
    frames = torch.zeros(5, 3, 40, 48)
    for i in range(5):
        frames[i, :, 10 + i:18 + i, 12 + i:20 + i] = 1.0
        frames[i, :, 24:32, 30 - i:38 - i] = 0.6
    frames += 0.05 * torch.rand(5, 3, 40, 48, generator=torch.Generator().manual_seed(2))
    gt, gt2 = torch.zeros(1, 40, 48), torch.zeros(1, 40, 48)
    gt[:, 10:18, 12:20] = 1.0
    gt2[:, 24:32, 30:38] = 1.0
    return cfg, model, mo, mo.state_dict(), frames, gt, gt2


def _raise(*a, **k):
    raise AssertionError('a layered call on today\'s path')


LUC = {'samples': 2, 'shift': 0.2}


def test_off_makes_exactly_todays_calls_and_batches(monkeypatch):
    from eosvos_amd.evaluate import evaluate_sequence
    cfg, model, mo, msd, frames, gt, gt2 = _setup()
    assert callable(Engine.lucid_compose_layers)
    with monkeypatch.context() as mp:
        for cls in (Engine, LayerEngine):
            mp.setattr(cls, 'lucid_compose_layers', _raise)
        mp.setattr(ll, 'LayeredAugmenter', _raise)
        mp.setattr(ll, 'layer_map', _raise)
        outs, states, seen, calls = [], [], [], []
        for kw in ({}, {'layers': None}, {'layers': {'others': 0}}, {'layers': dict(ll.DEFAULTS)}):
            model.seen, LayerEngine.calls = [], []
            outs.append(evaluate_sequence(model, mo, msd, frames, [gt, gt2], cfg, lucid=LUC, **kw))
            states.append(random.getstate())
            seen.append(model.seen)
            calls.append([c[:2] for c in LayerEngine.calls])
        for (labels, probs, hist), st, sn, cl in zip(outs[1:], states[1:], seen[1:], calls[1:]):
            assert torch.equal(labels, outs[0][0]) and all(torch.equal(a, b) for a, b in zip(probs, outs[0][1])) and hist == outs[0][2]
            assert st == states[0] and cl == calls[0]
            assert len(sn) == len(seen[0]) and all(torch.equal(a, b) for a, b in zip(sn, seen[0]))
        # on with a single object: today's calls, whatever `layers` says
        model.seen, LayerEngine.calls = [], []
        one = evaluate_sequence(model, mo, msd, frames, [gt], cfg, lucid=LUC)
        seen_one, calls_one = model.seen, [c[:2] for c in LayerEngine.calls]
        model.seen, LayerEngine.calls = [], []
        got = evaluate_sequence(model, mo, msd, frames, [gt], cfg, lucid=LUC, layers={'others': 3})
        assert [c[:2] for c in LayerEngine.calls] == calls_one and got[2] == one[2] and torch.equal(got[1][0], one[1][0])
        assert all(torch.equal(a, b) for a, b in zip(model.seen, seen_one))
        with pytest.raises(AssertionError, match='layered call'):
            evaluate_sequence(model, mo, msd, frames, [gt, gt2], cfg, lucid=LUC, layers={'others': 1})      # and on means on
    with pytest.raises(ValueError):
        evaluate_sequence(model, mo, msd, frames, [gt, gt2], cfg, lucid=LUC, layers={'others': 8})
    # without lucid samples the layers have nothing to do: nothing is called
    LayerEngine.calls = []
    evaluate_sequence(model, mo, msd, frames, [gt, gt2], cfg, layers={'others': 1})
    assert LayerEngine.calls == []


def test_evaluate_sequence_composes_two_objects_as_layers():
    from eosvos_amd.evaluate import evaluate_sequence, finetune_object, object_workers, others_at_train_frame, run_objects_in_flight
    from eosvos_amd.helper_func import set_random_seeds
    cfg, model, mo, msd, frames, gt, gt2 = _setup()
    LAY = {'others': 2, 'front': 0.5}
    model.seen, LayerEngine.calls = [], []
    labels, probs, hist = evaluate_sequence(model, mo, msd, frames, [gt, gt2], cfg, lucid=LUC, layers=LAY)
    n_calls = len(model.seen) // 2
    union = ((gt + gt2) != 0).float()
    plates = [c for c in LayerEngine.calls if c[0] == 'lucid_plate']
    assert len(plates) == 2 and all(c[1] == 4 and torch.equal(c[2].reshape(1, 40, 48), union) for c in plates)   # once per object, the union
    assert not [c for c in LayerEngine.calls if c[0] == 'lucid_compose']
    comp = [c for c in LayerEngine.calls if c[0] == 'lucid_compose_layers']
    fr = frames[0].numpy()
    attempts = 0
    for o, (tgt, oth) in enumerate(((gt, gt2), (gt2, gt))):
        for epoch in (1, 2, 3):                                         # the batches of rules 12 / L7, draw for draw
            set_random_seeds(cfg.get('seed', 1) + epoch)
            im, lb, rec = ll.batch_host(fr, tgt.numpy(), [oth.numpy()], LUC, LAY, 3,
                                        plain=lambda n: (np.repeat(fr[None], n, 0), np.repeat(tgt.numpy()[None], n, 0)))
            got = model.seen[o * n_calls + epoch - 1]
            assert got.shape == (3, 3, 40, 48) and np.array_equal(_bits(got.numpy()), _bits(im))
            assert all(len(r['layers']) == 2 for r in rec)
            attempts += max(r['tries'] for r in rec) + any(r['fallback'] for r in rec)
    assert len(comp) == attempts and all(c[3] == [2] * c[1] for c in comp)                      # one call per attempt
    assert others_at_train_frame([gt, gt2], [0, 0], 0).shape == (1, 1, 40, 48) and others_at_train_frame([gt, gt2], [0, 1], 0) is None
    # differs from the single-object synthesis, and the objects-in-flight path gives the same as one object after the other
    plain = evaluate_sequence(model, mo, msd, frames, [gt, gt2], cfg, lucid=LUC)
    assert plain[2][0][0] != hist[0][0]
    gts = [gt, gt2]
    one = [finetune_object(model, mo, msd, frames, g, cfg, lucid=LUC, layers=LAY, lucid_others=others_at_train_frame(gts, [0, 0], o))
           for o, g in enumerate(gts)]
    con = run_objects_in_flight(object_workers(model, mo, cfg['meta_optim_cfg'], 2), msd, frames, gts, cfg, lucid=LUC, layers=LAY)
    for (p2, h2), (p1, h1), h0 in zip(con, one, hist):
        assert h2 == h1 == h0 and torch.equal(p2, p1)


# ---- the library ------------------------------------------------------------------------------------------------------------
def test_abi_symbol_exists_in_the_built_library():
    lib = _ffi.load()
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'eosvos.h')).read()
    name, n_args = 'eosvos_lucid_compose_layers', 17
    assert name in _ffi.exported_symbols() and len(getattr(lib, name).argtypes) == n_args
    decl = hdr[hdr.rindex('int ' + name + '('):]
    assert decl[:decl.index(';')].count(',') + 1 == n_args                                     # the header's argument count
    for rule in ('L1.', 'L2.', 'L3.', 'L4.', 'L5.', 'L6.'):                                     # the rules are stated there in full
        assert rule in hdr and rule in ll.__doc__
    # a null engine is refused on the host, before anything touches a device
    assert lib.eosvos_lucid_compose_layers(None, None, None, None, 3, 8, 8, 1, None, None, None, None, 1, None, None, None, None) == 1
    assert b'null' in lib.eosvos_last_error()
