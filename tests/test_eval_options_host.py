"""The registry of the evaluation's opt-in option groups (`eval_options.py`) and what the evaluation path forwards.

Two halves.  The recorded-call half drives `evaluate_sequence`, `finetune_object`, `run_objects_in_flight` and `evaluate_dataset`
over a matrix of group settings with `finetune_object_steps`, `finetune_object` and `merge_objects` replaced by functions that note
what they were called with, and compares every note with `tests/golden/eval_options_calls.json` -- the notes of the same matrix
on the code as it was before the registry existed (`tools/debug/eval_options_record.py` writes the file from `record_all`).
The registry half checks the table against the modules, `config.py` and `parse_cli`."""
import copy
import importlib
import json
import os

import pytest
import torch

from eosvos_amd import config, evaluate

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval_options_calls.json')

# keyword, config key, the `config` name that holds its neutral values, the keys that switch it on, a command line that sets it
GROUPS = [
    ('tta', 'eval_tta', 'EXTENSIONS', {'flip': True}, ['eval_tta.flip=True', 'eval_tta.scales=[0.75,1.0,1.25]']),
    ('crf', 'eval_crf', 'POSTPROCESS', {'iterations': 2}, ['eval_crf.iterations=5', 'eval_crf.w_appearance=10']),
    ('components', 'eval_components', 'CLEANUP', {'min_area': 3},
     ['eval_components.gate=24', 'eval_components.min_rel_area=0.05', 'eval_components.largest_only=True']),
    ('holes', 'eval_holes', 'FILL', {'max_area': 9}, ['eval_holes.max_area=64', 'eval_holes.prev_overlap=0.5']),
    ('snap', 'eval_snap', 'SNAP', {'step': 8}, ['eval_snap.step=16', 'eval_snap.min_share=0.6']),
    ('motion', 'eval_motion', 'MOTION', {'block': 8}, ['eval_motion.block=8', 'eval_motion.radius=24', 'eval_components.gate=24']),
    ('zoom', 'eval_zoom', 'ZOOM', {'max_zoom': 2}, ['eval_zoom.max_zoom=3', 'eval_zoom.margin=0.5']),
    ('lucid', 'eval_lucid', 'LUCID', {'samples': 1}, ['eval_lucid.samples=2', 'eval_lucid.shift=0.1']),
    ('adapt', 'eval_adapt', 'ADAPT', {'neg_dist': 3}, ['eval_adapt.neg_dist=220', 'eval_adapt.erode=15', 'eval_online_adapt.step=5']),
    ('layers', 'eval_lucid_layers', 'LAYERS', {'others': 1}, ['eval_lucid_layers.others=3', 'eval_lucid.samples=2']),
]
KEYWORDS = [g[0] for g in GROUPS]
OBJECT_STAGE = ('tta', 'zoom', 'lucid', 'adapt', 'layers')
FUNCTIONS = ('finetune_object', 'finetune_object_steps', 'run_objects_in_flight', 'evaluate_sequence', 'evaluate_dataset')


def neutral(kw):
    _, key, name, _, _ = GROUPS[KEYWORDS.index(kw)]
    return copy.deepcopy(getattr(config, name)[key])


def on(kw, **more):
    return {**neutral(kw), **GROUPS[KEYWORDS.index(kw)][3], **more}


def matrix():
    """[(name, groups, data_cfg.normalize, does a second object share the train frame)]"""
    cases = [('none', {}, False, True)]
    for kw in KEYWORDS:
        cases += [(f'{kw}=None', {kw: None}, False, True), (f'{kw} neutral', {kw: neutral(kw)}, False, True),
                  (f'{kw} on', {kw: on(kw)}, False, True)]
    cases.append(('motion + components.gate', {'motion': on('motion'), 'components': on('components', gate=2)}, False, True))
    cases.append(('motion + holes.prev_overlap', {'motion': on('motion'), 'holes': on('holes', prev_overlap=0.5)}, False, True))
    for norm in (False, True):
        cases.append((f'snap, normalize={norm}', {'snap': on('snap')}, norm, True))
        cases.append((f'motion, normalize={norm}', {'motion': on('motion')}, norm, True))
        cases.append((f'snap + motion, normalize={norm}', {'snap': on('snap'), 'motion': on('motion')}, norm, True))
    for shared in (True, False):
        cases.append((f'layers + lucid, shared train frame={shared}', {'layers': on('layers'), 'lucid': on('lucid')}, False, shared))
        cases.append((f'layers neutral + lucid, shared train frame={shared}', {'layers': neutral('layers'), 'lucid': on('lucid')},
                      False, shared))
    cases.append(('holes inactive + crf=None', {'holes': neutral('holes'), 'crf': None}, False, True))
    cases.append(('holes inactive + snap', {'holes': on('holes', max_area=0), 'snap': on('snap')}, True, True))
    cases.append(('all ten', {kw: on(kw) for kw in KEYWORDS}, True, True))
    return cases


# ---- the recorder ---------------------------------------------------------------------------------------------------------
H = W = 8
N = 2


def _note(fn, args, kw):
    e = {'fn': fn, 'positional': len(args), 'keywords': sorted(kw)}
    for k in KEYWORDS:
        if k in kw:
            e[k] = kw[k]
    if fn == 'merge_objects' and len(args) > 3:
        e['crf (positional)'] = args[3]
    if 'keep' in kw:
        e['keep'] = sorted(kw['keep'])
    if 'frame_offset' in kw:
        e['frame_offset'] = list(kw['frame_offset'])
    if 'lucid_others' in kw:
        e['lucid_others'] = None if kw['lucid_others'] is None else list(kw['lucid_others'].shape)
    return e


class _Engine:
    def synchronize(self):
        pass


class _Model:
    device = torch.device('cpu')
    max_batch = 8
    wg_budget = 0

    def __init__(self):
        self.engine = _Engine()

    def set_wg_budget(self, budget):
        pass

    def copy_state_from(self, other):
        pass


class _Dataset:
    """Two sequences of two objects: in 'a' both are annotated on frame 0, in 'b' the second one appears on frame 1."""
    seqs_names = ['a', 'b']
    test_mode = True

    def __init__(self, mean_val=None):
        if mean_val is not None:
            self.mean_val = mean_val

    def sequence_tensors(self, seq, device, with_frame_ids=False):
        return _frames(), _gts(), [0, 0] if seq == 'a' else [0, 1]


def _frames():
    return torch.zeros(N, 3, H, W)


def _gts():
    a, b = torch.zeros(1, H, W), torch.zeros(1, H, W)
    a[0, 1:4, 1:4] = 1
    b[0, 5:7, 4:7] = 1
    return [a, b]


def _workers(n=2):
    ws = [evaluate.ObjectWorker(_Model(), None) for _ in range(n)]
    for w in ws:
        w.wg_budget = 256
    return ws


def record(case, monkeypatch):
    """{driver: [note]} of one case of the matrix."""
    _, groups, normalize, shared = case
    cfg = config.parse_cli([])
    cfg['data_cfg']['normalize'] = normalize
    object_groups = {k: v for k, v in groups.items() if k in OBJECT_STAGE}
    notes = []

    def steps(*a, **k):
        notes.append(_note('finetune_object_steps', a, k))

        def gen():
            return torch.zeros(N, H, W), []
            yield
        return gen()

    def finetune(*a, **k):
        notes.append(_note('finetune_object', a, k))
        return torch.zeros(N, H, W), []

    def merge(*a, **k):
        notes.append(_note('merge_objects', a, k))
        return torch.zeros(N, H, W, dtype=torch.uint8)

    def take():
        out = list(notes)
        del notes[:]
        return out
    out = {}
    with monkeypatch.context() as mp:
        mp.setattr(evaluate, 'merge_objects', merge)
        mp.setattr(evaluate, 'finetune_object', finetune)
        evaluate.evaluate_sequence(_Model(), None, None, _frames(), _gts() if shared else _gts()[:1], cfg, train_frame_id=1, **groups)
        out['evaluate_sequence'] = take()
    with monkeypatch.context() as mp:
        mp.setattr(evaluate, 'merge_objects', merge)
        mp.setattr(evaluate, 'finetune_object_steps', steps)
        others = {'lucid_others': torch.zeros(1, 1, H, W)} if shared and 'layers' in groups else {}
        evaluate.finetune_object(_Model(), None, None, _frames(), _gts()[0], cfg, **object_groups, **others)
        out['finetune_object'] = take()
        evaluate.run_objects_in_flight(_workers(), None, _frames(), _gts(), cfg, train_frame_id=[0, 0] if shared else [0, 1],
                                       **object_groups)
        out['run_objects_in_flight'] = take()
        for in_flight, mean_val in ((1, None), (2, (0.1, 0.2, 0.3))):
            model = _Model()
            model._object_workers = _workers(in_flight)
            evaluate.evaluate_dataset(model, None, None, _Dataset(mean_val), cfg, 'val', objects_in_flight=in_flight, **groups)
            out[f'evaluate_dataset, {in_flight} in flight'] = take()
    return json.loads(json.dumps(out))


def record_all(monkeypatch):
    return {case[0]: record(case, monkeypatch) for case in matrix()}


@pytest.fixture(scope='module')
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_matrix_is_the_recorded_one(recorded):
    assert list(recorded) == [case[0] for case in matrix()]


@pytest.mark.parametrize('case', matrix(), ids=lambda case: case[0])
def test_the_calls_are_the_recorded_ones(case, recorded, monkeypatch):
    got, want = record(case, monkeypatch), recorded[case[0]]
    assert list(got) == list(want)
    for driver in want:
        assert len(got[driver]) == len(want[driver]), driver
        for i, (g, w) in enumerate(zip(got[driver], want[driver])):
            assert g == w, (driver, i)


# ---- the registry ---------------------------------------------------------------------------------------------------------
def test_every_row_names_a_module_with_check_and_active():
    from eosvos_amd import eval_options
    assert [row.keyword for row in eval_options.TABLE] == KEYWORDS and [row.key for row in eval_options.TABLE] == [g[1] for g in GROUPS]
    assert {row.keyword for row in eval_options.TABLE if row.stage == eval_options.OBJECT} == set(OBJECT_STAGE)
    for row in eval_options.TABLE:
        module = importlib.import_module('eosvos_amd.' + row.module)
        assert callable(module.check) and callable(module.active), row.keyword
        assert module.active(row.defaults) is False and module.active(None) is False, row.keyword       # neutral values = off
        assert row.stage in (eval_options.OBJECT, eval_options.MERGE) and row.travels in (eval_options.SET, eval_options.ACTIVE)
        assert row.about and row.example
    assert {row.keyword for row in eval_options.TABLE if row.travels == eval_options.ACTIVE} == {'holes', 'snap', 'motion'}
    assert {row.keyword: row.brings for row in eval_options.TABLE if row.brings} == \
        {'snap': 'frame_offset', 'motion': 'frame_offset', 'layers': 'lucid_others'}


def test_the_defaults_table_and_the_rows_are_one_to_one_and_config_shows_them():
    from eosvos_amd import eval_options
    keys = [row.key for row in eval_options.TABLE]
    assert len(set(keys)) == len(keys) == 10 and sorted(eval_options.DEFAULTS) == sorted(keys)
    assert all(k.startswith('eval_') for k in keys) and len(eval_options.ROWS) == 10
    for _, key, name, _, _ in GROUPS:
        assert getattr(config, name) == {key: eval_options.DEFAULTS[key]}, name
        assert key not in config.BASE
    assert config.EXTENSIONS == {'eval_tta': {'flip': False, 'scales': [1.0]}}                          # a literal, for the values
    assert config.ADAPT == {'eval_adapt': {'neg_dist': 0, 'erode': 0}} and config.LAYERS == {'eval_lucid_layers': {'others': 0, 'front': 0.5}}


def test_from_cfg_carries_what_the_command_line_set():
    from eosvos_amd import eval_options
    assert eval_options.from_cfg(config.parse_cli([])) == {}
    beside = {'motion': ['eval_components.gate=24'], 'adapt': ['eval_online_adapt.step=5'], 'layers': ['eval_lucid.samples=2']}
    for row in eval_options.TABLE:
        cfg = config.parse_cli(row.example.split() + beside.get(row.keyword, []))
        got = eval_options.from_cfg(cfg)
        consumer = {'motion': {'components'}, 'layers': {'lucid'}}.get(row.keyword, set())      # a group of its own, set beside it
        assert set(got) == {row.keyword} | consumer and got[row.keyword] == cfg[row.key] != row.defaults, row.keyword
        assert importlib.import_module('eosvos_amd.' + row.module).active(got[row.keyword]), row.keyword
    for _, key, _, _, example in GROUPS:                                 # the examples of this file's matrix parse too
        assert key in config.parse_cli(example)
    assert eval_options.from_cfg({'eval_tta': None, 'eval_crf': {'iterations': 0}}) == {'crf': {'iterations': 0}}
    assert list(eval_options.from_cfg({row.key: row.defaults for row in reversed(eval_options.TABLE)})) == KEYWORDS


@pytest.mark.parametrize('name', FUNCTIONS)
def test_an_unknown_keyword_is_a_type_error(name):
    fn = getattr(evaluate, name)
    args = [None] * 6
    with pytest.raises(TypeError, match=f"{name}\\(\\) got an unexpected keyword argument 'ttta'"):
        fn(*args, ttta={'flip': True})
    with pytest.raises(TypeError, match='unexpected keyword argument'):
        fn(*args, frame_offset=(0, 0, 0))                                # travels beside a group; not one itself
    if name in ('finetune_object', 'finetune_object_steps', 'run_objects_in_flight'):
        with pytest.raises(TypeError, match=f"{name}\\(\\) got an unexpected keyword argument 'crf'"):
            fn(*args, crf={'iterations': 2})                             # a merge-stage group: these functions do not merge


def test_split_and_travelling():
    from eosvos_amd import eval_options
    groups = {kw: on(kw) for kw in KEYWORDS}
    share, merge_share = eval_options.split('f', dict(groups, zoom=None, crf=None))
    assert sorted(share) == ['adapt', 'layers', 'lucid', 'tta'] and sorted(merge_share) == ['components', 'holes', 'motion', 'snap']
    assert eval_options.travelling({}) == {} and eval_options.travelling({'tta': neutral('tta')}) == {'tta': neutral('tta')}
    assert eval_options.travelling({'layers': neutral('layers')}) == {'layers': neutral('layers'), 'lucid_others': None}
    cfg = config.parse_cli([])
    for kw in ('holes', 'snap', 'motion'):
        assert eval_options.travelling({kw: neutral(kw)}, cfg) == {} and eval_options.travelling({kw: on(kw)}, cfg) == {kw: on(kw)}
        with pytest.raises(ValueError):
            eval_options.travelling({kw: {'bogus': 1}}, cfg)             # `active` validates
    cfg['data_cfg']['normalize'] = True
    from eosvos_amd.data import DAVIS
    assert eval_options.travelling({'snap': on('snap')}, cfg) == {'snap': on('snap'), 'frame_offset': tuple(DAVIS.mean_val)}
    assert eval_options.travelling({'motion': on('motion'), 'holes': on('holes')}, cfg, _Dataset((1, 2, 3))) == \
        {'motion': on('motion'), 'holes': on('holes'), 'frame_offset': (1, 2, 3)}
    assert 'frame_offset' not in eval_options.travelling({'holes': on('holes'), 'crf': on('crf')}, cfg)


BAD = [
    (['eval_tta.scales=[]'], ValueError, 'tta.scales=[]: a non-empty list of scales'),
    (['eval_crf.radius=0'], ValueError, 'crf.radius=0: an integer in [1, 7]'),
    (['eval_components.gate=64'], ValueError, 'components.gate=64: an integer in [0, 63]'),
    (['eval_holes.max_area=-1'], ValueError, 'holes.max_area=-1: an integer in [0, 16777216]'),
    (['eval_snap.step=3'], ValueError, 'snap.step=3: 0 (off) or an integer in [4, 64]'),
    (['eval_motion.block=12'], ValueError, 'motion.block=12: 0 (off), 8 or 16'),
    (['eval_zoom.max_zoom=5'], ValueError, 'zoom.max_zoom=5: 0 (off) or a number in [1, 4]'),
    (['eval_lucid.samples=-1'], ValueError, 'lucid.samples=-1: an integer >= 0 (0 = off)'),
    (['eval_adapt.neg_dist=4096'], ValueError, 'adapt.neg_dist=4096: an integer in [0, 4095]'),
    (['eval_lucid_layers.others=8'], ValueError, 'lucid_layers.others=8: an integer in [0, 7] (0 = off)'),
    (['eval_motion.block=8'], ValueError, 'eval_motion has no consumer: set eval_components.gate or eval_holes.prev_overlap'),
    (['eval_motion.block=8', 'eval_components.min_area=3'], ValueError,
     'eval_motion has no consumer: set eval_components.gate or eval_holes.prev_overlap'),
    (['eval_motion.block=8', 'eval_holes.max_area=9'], ValueError,
     'eval_motion has no consumer: set eval_components.gate or eval_holes.prev_overlap'),
    (['e-OSVOS', 'eval_adapt.neg_dist=220'], ValueError, 'eval_adapt has no consumer: set eval_online_adapt.step'),
    (['eval_lucid_layers.others=2'], ValueError, 'eval_lucid_layers has no consumer: set eval_lucid.samples'),
    (['eval_lucid_layers.others=2', 'eval_lucid.samples=0'], ValueError, 'eval_lucid_layers has no consumer: set eval_lucid.samples'),
    (['eval_tta.bogus=1'], KeyError, "'unknown config key: eval_tta.bogus'"),
]


@pytest.mark.parametrize('argv, error, message', BAD, ids=[' '.join(b[0]) for b in BAD])
def test_parse_cli_raises_what_it_raised(argv, error, message):
    with pytest.raises(error) as caught:
        config.parse_cli(argv)
    assert type(caught.value) is error and str(caught.value) == message


def test_parse_cli_accepts_an_active_group_with_its_consumer_and_an_inactive_one_without():
    assert config.parse_cli(['eval_motion.block=8', 'eval_holes.max_area=9', 'eval_holes.prev_overlap=0.5'])['eval_motion']['block'] == 8
    assert config.parse_cli(['eval_motion.radius=3'])['eval_motion'] == {'block': 0, 'radius': 3, 'bias': 2}
    assert config.parse_cli(['eval_adapt.erode=3'])['eval_adapt'] == {'neg_dist': 0, 'erode': 3}
    assert config.parse_cli(['eval_lucid_layers.front=0.25'])['eval_lucid_layers'] == {'others': 0, 'front': 0.25}
