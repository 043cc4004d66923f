"""Host side of the connected-component clean-up (`eosvos_amd/components.py`): the numpy twin (`label_host`, `filter_host`)
against the flood fill and the per-pixel loops of tests/components_ref.py, bit for bit; what the parameter dictionary accepts;
how the configuration carries it; that the evaluation hands it through; the chunking of `Engine.filter_components`; the C-ABI
symbols.  CPU only: the engine is the stand-in of tests/fake_engine.py, which has no `filter_components` and so takes
`filter_host`."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import components_ref as ref  # noqa: E402
import crf_ref  # noqa: E402
from test_crf_host import LogDeepLab, LogEngine  # noqa: E402

from eosvos_amd import _ffi, components, config, crf  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402
from eosvos_amd.meta_optim import MetaOptimizer  # noqa: E402
from oracle import meta as oracle_meta  # noqa: E402

# 1 x 1, smaller than a tile, one 16 x 64 tile of the kernels exactly, one pixel over it in each direction, several tiles
SIZES = [(1, 1), (5, 7), (16, 64), (17, 65), (33, 130)]


def P(**kw):
    return dict(components.DEFAULTS, **kw)


# ---- the numpy twin against the flood fill ------------------------------------------------------------------------------
@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('h,w', SIZES)
def test_label_host_equals_the_flood_fill(h, w, connectivity):
    pats = ref.patterns(h, w)
    ids = components.label_host(np.stack(list(pats.values())), connectivity)          # one batch: frames never connect
    assert ids.dtype == np.int32 and ids.shape == (len(pats), h, w)
    for k, (name, m) in enumerate(pats.items()):
        np.testing.assert_array_equal(ids[k], ref.label_ref(m, connectivity), err_msg=name)
    count = lambda name: len(np.unique(ids[list(pats).index(name)])) - (1 if (pats[name] == 0).any() else 0)
    if h * w > 1:
        assert count('checkerboard') == (1 if connectivity == 8 else (h * w + 1) // 2)
    if (h, w) == (33, 130):
        assert count('seam_quadrants') == (3 if connectivity == 8 else 4)            # labels 2 and 3 never join label 1
        assert count('serpentine') == count('serpentine_v') == count('spiral') == 1


FILTERS = [P(min_area=3), P(min_rel_area=0.25), P(largest_only=True), P(largest_only=True, connectivity=4),
           P(min_area=2, min_rel_area=0.1, connectivity=4)]


@pytest.mark.parametrize('h,w', [(5, 7), (17, 65)])
def test_filter_host_equals_the_loops_on_the_patterns(h, w):
    maps = np.stack(list(ref.patterns(h, w).values()))
    for params in FILTERS:
        got, removed = components.filter_host(maps, params, return_removed=True)
        want, want_removed = ref.filter_ref(maps, params)
        np.testing.assert_array_equal(got, want, err_msg=str(params))
        np.testing.assert_array_equal(removed, want_removed)
        np.testing.assert_array_equal(removed, (maps != 0).sum(axis=(1, 2)) - (got != 0).sum(axis=(1, 2)))
        assert got.dtype == np.uint8 and bool(((got == maps) | (got == 0)).all())


def test_gate_chain_equals_the_loops_and_means_what_it_says():
    labels, prev, keep = ref.chain(16, 40, 3, 4)
    for params in (P(gate=3), P(gate=3, largest_only=True), P(gate=2, min_area=5), P(gate=3, connectivity=4, min_rel_area=1.0)):
        for pv, kp in ((prev, keep), (None, ()), (prev, ())):
            got, removed = components.filter_host(labels, params, prev=pv, keep=kp, return_removed=True)
            want, want_removed = ref.filter_ref(labels, params, pv, kp)
            np.testing.assert_array_equal(got, want, err_msg=f'{params} {kp}')
            np.testing.assert_array_equal(removed, want_removed)
    for params in (P(gate=3), P(gate=3, largest_only=True)):      # the gate first: the (smaller) object survives, not the distractor
        out = components.filter_host(labels, params, prev=prev, keep=keep)
        for f in (0, 1):
            assert not out[f, :4, -8:].any() and np.array_equal(out[f, :, :-8], labels[f, :, :-8])
        assert not (out[2] == 1).any() and np.array_equal(out[2] == 2, labels[2] == 2)      # object absent, distractor gated away
        np.testing.assert_array_equal(out[4], labels[4])                                    # the keep frame
    out = components.filter_host(labels, P(gate=3), prev=prev, keep=keep)
    np.testing.assert_array_equal(out[3], labels[3])             # nothing of label 1 in frame 2: the gate is inactive, all returns
    np.testing.assert_array_equal(out[5], labels[5])             # the keep frame carried the distractor into the gate
    no_prev = components.filter_host(labels, P(gate=3), keep=keep)
    np.testing.assert_array_equal(no_prev[0], labels[0])         # no R for the first frame: nothing is gated


def test_relative_area_boundary_and_the_largest_only_tie():
    m = np.zeros((1, 8, 40), dtype=np.uint8)
    m[0, 0, 0:32] = 1                                            # Amax = 32
    m[0, 2, 0:8] = 1                                             # A = 8: A * 65536 == q * Amax at min_rel_area = 0.25 exactly
    m[0, 4, 0:7] = 1                                             # A = 7: below
    m[0, 6, 0:32] = 1                                            # a second component of Amax pixels, with the larger id
    for fn in (components.filter_host, lambda *a, **k: ref.filter_ref(*a, **k)[0]):
        out = fn(m, P(min_rel_area=0.25))
        assert out[0, 2, 0:8].all() and not out[0, 4].any() and out[0, 0, :32].all() and out[0, 6, :32].all()
        out = fn(m, P(min_rel_area=0.25 + 2.0 ** -16))           # q one step up: 8 * 65536 < q * 32
        assert not out[0, 2].any() and out[0, 0, :32].all()
        out = fn(m, P(largest_only=True))
        assert out[0, 0, :32].all() and not out[0, 1:].any()     # the tie goes to the smaller id
    assert components.rel_q16(0.25) == 16384 and components.rel_q16(1.0) == 65536 and components.rel_q16(0.0) == 0


# ---- the parameter dictionary -------------------------------------------------------------------------------------------
def test_check_active_and_frames_per_call():
    assert components.DEFAULTS == {'connectivity': 8, 'min_area': 0, 'min_rel_area': 0.0, 'largest_only': False, 'gate': 0}
    assert components.check({}) == components.DEFAULTS and components.check(components.DEFAULTS) == components.DEFAULTS
    assert components.check({'gate': 63, 'min_rel_area': 1})['min_rel_area'] == 1.0
    assert not components.active(None) and not components.active({}) and not components.active(P(connectivity=4))
    for on in ({'min_area': 1}, {'min_rel_area': 0.01}, {'largest_only': True}, {'gate': 1}):
        assert components.active(on)
    assert components.frames_per_call(480, 854) == ((512 << 20) - 256) // (17 * 480 * 854 + 2312)
    assert components.frames_per_call(4095, 4096) == 1 and components.frames_per_call(1, 1) == 65535


@pytest.mark.parametrize('bad', [{'gate': 64}, {'gate': -1}, {'gate': 2.0}, {'gate': True}, {'connectivity': 6},
                                 {'connectivity': '8'}, {'min_rel_area': 1.5}, {'min_rel_area': -0.1},
                                 {'min_rel_area': float('nan')}, {'min_area': -1}, {'min_area': 1.5}, {'largest_only': 1},
                                 {'area': 5}, [8], 8])
def test_invalid_dictionaries_raise_value_error(bad):
    with pytest.raises(ValueError):
        components.check(bad)
    with pytest.raises(ValueError):
        components.active(bad)


def test_twin_rejects_bad_maps():
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((1, 4, 4), np.int32), np.zeros((1, 0, 4), np.uint8),
                np.zeros((1, 4097, 2), np.uint8)):
        with pytest.raises(ValueError):
            components.label_host(bad)
    with pytest.raises(ValueError):
        components.filter_host(np.zeros((1, 4, 4), np.uint8), P(gate=1), prev=np.zeros((4, 5), np.uint8))
    with pytest.raises(ValueError):
        components.label_host(np.zeros((1, 4, 4), np.uint8), connectivity=6)


# ---- configuration ------------------------------------------------------------------------------------------------------
def test_parse_cli_carries_eval_components_only_when_asked():
    base, ext, post = copy.deepcopy(config.BASE), copy.deepcopy(config.EXTENSIONS), copy.deepcopy(config.POSTPROCESS)
    assert config.CLEANUP == {'eval_components': components.DEFAULTS} and not components.active(config.CLEANUP['eval_components'])
    for groups in (config.BASE, config.EXTENSIONS, config.POSTPROCESS, config.parse_cli([])):
        assert 'eval_components' not in groups
    assert 'eval_components' not in config.parse_cli(['with', 'DAVIS-2017', 'eval_crf.iterations=5', 'eval_tta.flip=True'])
    cfg = config.parse_cli(['eval_components.gate=24', 'eval_components.min_rel_area=0.05', 'eval_components.largest_only=True'])
    assert cfg['eval_components'] == P(gate=24, min_rel_area=0.05, largest_only=True)
    assert 'eval_crf' not in cfg and 'eval_tta' not in cfg
    assert config.parse_cli(['eval_components.connectivity=4'])['eval_components'] == P(connectivity=4)      # still off
    assert config.BASE == base and config.EXTENSIONS == ext and config.POSTPROCESS == post
    assert config.CLEANUP == {'eval_components': components.DEFAULTS}                                       # nothing leaked
    with pytest.raises(KeyError):
        config.parse_cli(['eval_components.radius=3'])
    for bad in ('eval_components.gate=64', 'eval_components.connectivity=6', 'eval_components.min_rel_area=1.5',
                'eval_components.min_area=-1', 'eval_components.largest_only=2'):
        with pytest.raises(ValueError):
            config.parse_cli([bad])


# ---- the evaluation loop ------------------------------------------------------------------------------------------------
def _never(*a, **k):
    raise AssertionError('the component filter was called on the plain path')


def test_merge_objects_off_is_today_and_on_filters_after_the_crf(monkeypatch):
    from eosvos_amd.evaluate import merge_objects
    images, probs = crf_ref.scene(24, 32, 2, seed=4, n_frames=5)
    probs[2] = 2.0 * (probs[2] > 0.5)                                # a seeded train frame
    eng = LogEngine('resnet50', 24, 32, 1)
    per_object = [probs[:, o] for o in range(2)]
    today = torch.stack([oracle_meta.merge_labels(probs[f]) for f in range(5)])
    crf_params = dict(crf.DEFAULTS, radius=3, dilation=1, iterations=2)
    refined = merge_objects(eng, per_object, images, crf_params, keep=(2,))
    with monkeypatch.context() as mp:
        mp.setattr(Engine, 'filter_components', _never)
        mp.setattr(components, 'filter', _never)
        mp.setattr(components, 'filter_host', _never)
        for kw in ({'components': None}, {'components': {}}, {'components': P(connectivity=4)}, {'components': P(), 'keep': (2,)}):
            assert torch.equal(merge_objects(eng, per_object, **kw), today)
        assert torch.equal(merge_objects(eng, per_object, images, crf_params, keep=(2,), components=P()), refined)
    params = P(largest_only=True, gate=2)
    on = merge_objects(eng, per_object, keep=(2,), components=params)
    want = components.filter_host(today.numpy(), params, keep=(2,))
    assert on.dtype == torch.uint8 and np.array_equal(on.numpy(), want) and torch.equal(on[2], today[2])
    assert not torch.equal(on, today)
    both = merge_objects(eng, per_object, images, crf_params, keep=(2,), components=params)
    assert np.array_equal(both.numpy(), components.filter_host(refined.numpy(), params, keep=(2,)))       # after the CRF twin
    assert torch.equal(both[2], today[2]) and not torch.equal(both, refined)
    with pytest.raises(ValueError):
        merge_objects(eng, per_object, components={'gate': 64})

    class DeviceEngine(LogEngine):                                   # an engine WITH the entry point is called
        calls = []

        def filter_components(self, labels, prev=None, keep=(), **params):
            DeviceEngine.calls.append((labels.shape[0], prev, tuple(keep), params))
            return torch.from_numpy(components.filter_host(labels, params, prev=prev, keep=keep))
    dev = DeviceEngine('resnet50', 24, 32, 1)
    assert torch.equal(merge_objects(dev, per_object, keep=(2,), components=params), on)
    assert DeviceEngine.calls == [(5, None, (2,), params)]


def test_evaluate_sequence_passes_components_through(monkeypatch):
    from eosvos_amd.evaluate import evaluate_sequence
    cfg = config.parse_cli([])
    cfg['num_epochs']['eval'] = 2
    model = LogDeepLab('resnet50', num_classes=1, batch_norm=cfg['parent_model']['batch_norm'], max_batch=1)
    model._views['backbone.conv1.weight'].view(-1)[0] = 4.0
    mo = MetaOptimizer(model, **cfg['meta_optim_cfg'])
    msd = mo.state_dict()
    images, probs = crf_ref.scene(24, 32, 2, seed=9, n_frames=4)
    gts = [(probs[1, o] > 0.5).float()[None] for o in range(2)]
    plain = evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1)
    with monkeypatch.context() as mp:
        mp.setattr(components, 'filter', _never)
        for kw in ({'components': None}, {'components': P()}):
            off = evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1, **kw)
            assert torch.equal(off[0], plain[0]) and off[2] == plain[2] and all(torch.equal(a, b) for a, b in zip(off[1], plain[1]))
    params = P(largest_only=True)
    on = evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1, components=params)
    assert all(torch.equal(a, b) for a, b in zip(on[1], plain[1])) and on[2] == plain[2]       # the fine-tunes do not see it
    assert np.array_equal(on[0].numpy(), components.filter_host(plain[0].numpy(), params, keep=(1,)))
    assert torch.equal(on[0][1], plain[0][1]) and not torch.equal(on[0], plain[0])
    crf_params = dict(crf.DEFAULTS, radius=2, dilation=2, iterations=3)
    refined = evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1, crf=crf_params)
    both = evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1, crf=crf_params, components=params)
    assert np.array_equal(both[0].numpy(), components.filter_host(refined[0].numpy(), params, keep=(1,)))


def test_evaluate_dataset_cleans_labels_pngs_and_j(tmp_path, monkeypatch):
    from eosvos_amd import data
    from eosvos_amd.evaluate import evaluate_dataset, prediction_paths
    cfg = config.parse_cli(['eval_components.largest_only=True', 'eval_components.gate=3'])
    cfg['num_epochs']['eval'] = 2
    model = LogDeepLab('resnet50', num_classes=1, batch_norm=cfg['parent_model']['batch_norm'], max_batch=2)
    mo = MetaOptimizer(model, **cfg['meta_optim_cfg'])
    ds = data.SyntheticSequences(1, 4, 24, 40, seed=3)
    seq = ds.seqs_names[0]
    plain = evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1)
    with monkeypatch.context() as mp:
        mp.setattr(components, 'filter', _never)
        off = evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1, components=P())
    assert torch.equal(off['labels'][seq], plain['labels'][seq]) and off['J_seq'] == plain['J_seq']
    on = evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1, save_dir=str(tmp_path),
                          components=cfg['eval_components'])
    labels = on['labels'][seq]
    want = components.filter_host(plain['labels'][seq].numpy(), cfg['eval_components'], keep=(0,))
    assert np.array_equal(labels.numpy(), want) and torch.equal(labels[0], plain['labels'][seq][0])
    assert not torch.equal(labels, plain['labels'][seq])
    n_obj = len(ds.sequence_tensors(seq, 'cpu')[1])
    assert on['J_seq'] == [data.sequence_J(labels.numpy(), ds.label_maps(seq), n_obj)]       # J sees the cleaned maps
    from PIL import Image
    preds, _ = prediction_paths(str(tmp_path), cfg['datasets']['val']['name'], cfg['datasets']['val']['split'])
    png = np.asarray(Image.open(os.path.join(preds, seq, ds.frame_names(seq)[2] + '.png')))
    np.testing.assert_array_equal(png, labels[2].numpy())


# ---- chunking -----------------------------------------------------------------------------------------------------------
class _HostLib:
    """`eosvos_filter_components` on host pointers through the twin: lets the chunk loop of `Engine.filter_components` run
    without a device."""
    def __init__(self):
        self.calls = []

    def eosvos_filter_components(self, e, labels, n, h, w, connectivity, min_area, q16, largest_only, gate, prev, keep, out,
                                 removed):
        view = lambda p, *shape: np.ctypeslib.as_array((ctypes.c_uint8 * int(np.prod(shape))).from_address(p.value)).reshape(shape)
        params = P(connectivity=connectivity, min_area=min_area, min_rel_area=q16 / 65536, largest_only=bool(largest_only), gate=gate)
        self.calls.append((n, prev is not None, bytes(keep)))
        res, rem = components.filter_host(view(labels, n, h, w), params, prev=None if prev is None else view(prev, h, w),
                                          keep=[f for f in range(n) if keep[f]], return_removed=True)
        view(out, n, h, w)[:] = res
        if removed is not None:
            for f in range(n):
                removed[f] = int(rem[f])
        return 0


class _HostEngine:
    device = torch.device('cpu')
    h = None
    _check_stream = lambda self: None
    _check_label_maps = Engine._check_label_maps
    filter_components = Engine.filter_components

    def __init__(self):
        self.lib = _HostLib()


def test_chunks_of_two_frames_hand_prev_over(monkeypatch):
    labels, prev, keep = ref.chain(16, 40, 3, 4)
    params = P(gate=3, largest_only=True)
    want, want_removed = components.filter_host(labels, params, prev=prev, keep=keep, return_removed=True)
    for step, calls in ((2, [(2, True, b'\0\0'), (2, True, b'\0\0'), (2, True, b'\1\0')]), (4, [(4, True, b'\0' * 4), (2, True, b'\1\0')]),
                        (6, [(6, True, b'\0\0\0\0\1\0')])):
        monkeypatch.setattr(components, 'frames_per_call', lambda h, w: step)
        eng = _HostEngine()
        out, removed = eng.filter_components(torch.from_numpy(labels), prev=torch.from_numpy(prev), keep=keep, return_removed=True,
                                             **params)
        assert eng.lib.calls == calls
        assert np.array_equal(out.numpy(), want) and np.array_equal(removed, want_removed)
    eng = _HostEngine()                                              # no prev: the first chunk has none, the second gets one
    out = eng.filter_components(torch.from_numpy(labels), keep=keep, **params)
    assert [c[1] for c in eng.lib.calls] == [False] and np.array_equal(out.numpy(), components.filter_host(labels, params, keep=keep))
    monkeypatch.setattr(components, 'frames_per_call', lambda h, w: 2)
    eng = _HostEngine()
    out = eng.filter_components(torch.from_numpy(labels), keep=keep, **params)
    assert [c[1] for c in eng.lib.calls] == [False, True, True]
    assert np.array_equal(out.numpy(), components.filter_host(labels, params, keep=keep))


# ---- C-ABI --------------------------------------------------------------------------------------------------------------
def test_abi_symbols_exist_and_refuse_a_null_engine():
    lib = _ffi.load()
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'eosvos.h')).read()
    for name, n_args in (('eosvos_label_components', 7), ('eosvos_filter_components', 14)):
        assert name in _ffi.exported_symbols() and len(getattr(lib, name).argtypes) == n_args and name + '(' in hdr
    assert lib.eosvos_label_components(None, None, 1, 8, 8, 8, None) == 1
    assert b'label_components' in lib.eosvos_last_error() and b'null' in lib.eosvos_last_error()
    assert lib.eosvos_filter_components(None, None, 1, 8, 8, 8, 0, 0, 0, 0, None, None, None, None) == 1
    assert b'filter_components' in lib.eosvos_last_error() and b'null' in lib.eosvos_last_error()
