"""Host side of the hole filling (`eosvos_amd/holes.py`): the numpy twin (`fill_host`) against the flood fills of
tests/holes_ref.py, bit for bit; what the parameter dictionary accepts; how the configuration carries it; that the evaluation
hands it through; the chunking of `Engine.fill_holes`; the C-ABI symbol.  CPU only: the engine is the stand-in of
tests/fake_engine.py, which has no `fill_holes` and so takes `fill_host`."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import crf_ref  # noqa: E402
import holes_ref as ref  # noqa: E402
from test_crf_host import LogDeepLab, LogEngine  # noqa: E402

from eosvos_amd import _ffi, components, config, holes  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402
from eosvos_amd.meta_optim import MetaOptimizer  # noqa: E402
from oracle import meta as oracle_meta  # noqa: E402

# 1 x 1, smaller than a tile, one 16 x 64 tile of the kernels exactly, one pixel over it in each direction, several tiles
SIZES = [(1, 1), (5, 7), (16, 64), (17, 65), (33, 130), (97, 161)]
ANY = 1 << 24


def P(**kw):
    return dict(holes.DEFAULTS, **kw)


# ---- the numpy twin against the flood fill ------------------------------------------------------------------------------
@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('h,w', SIZES)
def test_fill_host_equals_the_flood_fill_on_every_pattern(h, w, connectivity):
    pats = ref.patterns(h, w)
    maps = np.stack(list(pats.values()))
    for params in (P(connectivity=connectivity, max_area=ANY), P(connectivity=connectivity, max_area=3),
                   P(connectivity=connectivity, max_area=ANY, max_rel_area=0.25)):
        got, filled = holes.fill_host(maps, params, return_filled=True)
        want, want_filled, _ = ref.fill_ref(maps, params)
        assert got.dtype == np.uint8 and filled.dtype == np.int64
        for k, name in enumerate(pats):
            np.testing.assert_array_equal(got[k], want[k], err_msg=f'{name} {params}')
        np.testing.assert_array_equal(filled, want_filled)
        np.testing.assert_array_equal(filled, (got != 0).sum(axis=(1, 2)) - (maps != 0).sum(axis=(1, 2)))
        assert bool(((got == maps) | (maps == 0)).all())             # only background changes
    got, filled = holes.fill_host(maps, P(connectivity=connectivity, max_area=ANY), return_filled=True)
    count = dict(zip(pats, filled))
    assert count['empty'] == 0 and count['full'] == 0
    if 'ring' in count:
        assert count['ring'] > 0 and count['ring_at_border'] == 0 and count['between_two'] == 0 and count['corridor_open'] == 0
        assert count['corner_leak'] == (3 if connectivity == 8 else 0)       # a hole under 8, joined to the outside under 4
        assert count['corridor'] == int((pats['corridor'] == 0).sum())
    if 'nested' in count:
        nested = got[list(pats).index('nested')]
        assert count['nested'] == 1 and nested[5, 5] == 2 and not nested[2, 2:9].any()
    if 'seam_xy' in count:
        assert (count['seam_x'], count['seam_y'], count['seam_xy']) == (4, 8, 16)


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('h,w,p', [(33, 130, 0.1), (33, 130, 0.3), (33, 130, 0.5), (97, 161, 0.3)])
def test_fill_host_equals_the_flood_fill_on_punched_stripes(h, w, p, connectivity):
    labels = np.stack([ref.punched(h, w, p, seed=10 * k + int(p * 10)) for k in range(3)])
    prev = ref.punched(h, w, p, seed=99)
    params = P(connectivity=connectivity, max_area=4, max_rel_area=0.002, prev_overlap=0.5)
    for pv, kp in ((prev, ()), (None, ()), (prev, (1,))):
        got, filled = holes.fill_host(labels, params, prev=pv, keep=kp, return_filled=True)
        want, want_filled, classes = ref.fill_ref(labels, params, prev=pv, keep=kp)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(filled, want_filled)
        assert all(classes[c] > 0 for c in ref.CLASSES), classes     # every outcome of the rules occurs
        if kp:
            np.testing.assert_array_equal(got[1], labels[1])


def test_chain_and_thresholds_on_the_twin():
    labels, prev, keep, real, (sy0, sy1, sx0, sx1) = ref.chain()
    params = P(max_area=16, prev_overlap=0.5)
    for pv, kp in ((prev, keep), (None, keep), (prev, ()), (np.where(prev == 1, 9, prev).astype(np.uint8), ())):
        for par in (params, dict(params, connectivity=4), dict(params, prev_overlap=0.0)):
            got, filled = holes.fill_host(labels, par, prev=pv, keep=kp, return_filled=True)
            want, want_filled, _ = ref.fill_ref(labels, par, prev=pv, keep=kp)
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(filled, want_filled)
    out = holes.fill_host(labels, params, prev=prev, keep=keep)
    for f, (y0, y1, x0, x1) in enumerate(real):
        assert not out[f, y0:y1, x0:x1].any()                        # the real hole stays open
    assert (out[2:4, sy0:sy1, sx0:sx1] == 1).all()                   # the spurious one fills, in frame 3 because R is FILLED
    assert not holes.fill_host(labels[3:4], params, prev=labels[2])[0, sy0:sy1, sx0:sx1].any()
    without_rule = holes.fill_host(labels, dict(params, prev_overlap=0.0), keep=keep)
    assert all(without_rule[f, y0:y1, x0:x1].all() for f, (y0, y1, x0, x1) in enumerate(real) if f)     # naive filling closes it
    # exact thresholds
    m = np.zeros((2, 8, 14), dtype=np.uint8)
    ref._ring(m[0], 1, 1, 5, 7, 1)                                   # hole 2 x 4 = 8
    ref._ring(m[1], 1, 1, 5, 8, 1)                                   # hole 2 x 5 = 10
    m[1, 2, 2] = 1                                                   # ... = 9
    out = holes.fill_host(m, P(max_area=8))
    assert out[0, 2:4, 2:6].all() and not out[1, 3, 2:7].any()
    m = np.zeros((2, 8, 14), dtype=np.uint8)
    ref._ring(m[0], 1, 1, 5, 5, 1)                                   # A = 4, ring of 12
    m[0, 7, 0:4] = 1                                                 # S = 16
    ref._ring(m[1], 1, 1, 4, 8, 1)                                   # A = 5, S = 16
    out = holes.fill_host(m, P(max_area=ANY, max_rel_area=0.25))
    assert out[0, 2:4, 2:4].all() and not out[1, 2, 2:7].any()
    assert not holes.fill_host(m, P(max_area=ANY, max_rel_area=0.25 - 2.0 ** -16))[0, 2:4, 2:4].any()
    prev = np.zeros((8, 14), dtype=np.uint8)
    prev[2, 2:4] = 1                                                 # C = 2 of A = 4
    assert holes.fill_host(m[:1], P(max_area=4, prev_overlap=0.5), prev=prev)[0, 2:4, 2:4].all()
    prev[2, 3], prev[7, 7] = 0, 1                                    # C = 1
    assert not holes.fill_host(m[:1], P(max_area=4, prev_overlap=0.5), prev=prev)[0, 2:4, 2:4].any()
    assert holes.rel_q16(0.25) == 16384 and holes.overlap_q16(0.5) == 32768 and holes.rel_q16(1.0) == 65536


# ---- the parameter dictionary -------------------------------------------------------------------------------------------
def test_check_active_and_frames_per_call():
    assert holes.DEFAULTS == {'connectivity': 8, 'max_area': 0, 'max_rel_area': 1.0, 'prev_overlap': 0.0}
    assert holes.check({}) == holes.DEFAULTS and holes.check(holes.DEFAULTS) == holes.DEFAULTS
    assert holes.check({'max_area': 1 << 24, 'prev_overlap': 1})['prev_overlap'] == 1.0
    for off in (None, {}, P(connectivity=4), P(prev_overlap=0.5), P(max_area=5, max_rel_area=0.0), P(max_rel_area=0.5)):
        assert not holes.active(off)
    assert holes.active({'max_area': 1}) and holes.active(P(max_area=64, max_rel_area=0.01, prev_overlap=0.5))
    assert holes.frames_per_call(480, 854) == ((512 << 20) - 264) // (24 * 480 * 854 + 1288)
    assert holes.frames_per_call(4095, 4096) == 1 and holes.frames_per_call(1, 1) == 65535


@pytest.mark.parametrize('bad', [{'max_area': -1}, {'max_area': (1 << 24) + 1}, {'max_area': 2.0}, {'max_area': True},
                                 {'connectivity': 6}, {'connectivity': '8'}, {'connectivity': True}, {'max_rel_area': 1.5},
                                 {'max_rel_area': -0.1}, {'max_rel_area': float('nan')}, {'max_rel_area': '1'},
                                 {'prev_overlap': 1.5}, {'prev_overlap': -0.1}, {'prev_overlap': float('nan')},
                                 {'prev_overlap': True}, {'min_area': 5}, {'gate': 3}, [8], 8])
def test_invalid_dictionaries_raise_value_error(bad):
    with pytest.raises(ValueError):
        holes.check(bad)
    with pytest.raises(ValueError):
        holes.active(bad)


def test_twin_rejects_bad_maps():
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((1, 4, 4), np.int32), np.zeros((1, 0, 4), np.uint8),
                np.zeros((1, 4097, 2), np.uint8)):
        with pytest.raises(ValueError):
            holes.fill_host(bad, P(max_area=1))
    with pytest.raises(ValueError):
        holes.fill_host(np.zeros((1, 4, 4), np.uint8), P(max_area=1), prev=np.zeros((4, 5), np.uint8))


# ---- configuration ------------------------------------------------------------------------------------------------------
def test_parse_cli_carries_eval_holes_only_when_asked():
    base, ext, post, clean = (copy.deepcopy(g) for g in (config.BASE, config.EXTENSIONS, config.POSTPROCESS, config.CLEANUP))
    assert config.FILL == {'eval_holes': holes.DEFAULTS} and not holes.active(config.FILL['eval_holes'])
    for groups in (config.BASE, config.EXTENSIONS, config.POSTPROCESS, config.CLEANUP, config.parse_cli([])):
        assert 'eval_holes' not in groups
    assert 'eval_holes' not in config.parse_cli(['with', 'DAVIS-2017', 'eval_crf.iterations=5', 'eval_components.gate=3'])
    cfg = config.parse_cli(['eval_holes.max_area=64', 'eval_holes.prev_overlap=0.5'])
    assert cfg['eval_holes'] == P(max_area=64, prev_overlap=0.5)
    assert 'eval_crf' not in cfg and 'eval_tta' not in cfg and 'eval_components' not in cfg
    assert config.parse_cli(['eval_holes.connectivity=4'])['eval_holes'] == P(connectivity=4)          # still off
    assert config.BASE == base and config.EXTENSIONS == ext and config.POSTPROCESS == post and config.CLEANUP == clean
    assert config.FILL == {'eval_holes': holes.DEFAULTS}                                             # nothing leaked
    assert config.CLEANUP == {'eval_components': components.DEFAULTS}
    with pytest.raises(KeyError):
        config.parse_cli(['eval_holes.radius=3'])
    for bad in ('eval_holes.max_area=-1', 'eval_holes.connectivity=6', 'eval_holes.max_rel_area=1.5',
                'eval_holes.prev_overlap=2', 'eval_holes.max_area=1.5'):
        with pytest.raises(ValueError):
            config.parse_cli([bad])


# ---- the evaluation loop ------------------------------------------------------------------------------------------------
def _never(*a, **k):
    raise AssertionError('the hole filler was called on the plain path')


def _punch(probs):
    """Sub-threshold pixels inside the objects: the merge leaves background islands there."""
    probs = probs.clone()
    probs[:, :, 8:10, 8:10] = 0.1
    probs[:, :, 12:14, 20:22] = 0.1
    return probs


def test_merge_objects_off_is_today_and_on_fills_after_the_filter(monkeypatch):
    from eosvos_amd.evaluate import merge_objects
    images, probs = crf_ref.scene(24, 32, 2, seed=4, n_frames=5)
    probs = _punch(probs)
    probs[2] = 2.0 * (probs[2] > 0.5)                                # a seeded train frame
    eng = LogEngine('resnet50', 24, 32, 1)
    per_object = [probs[:, o] for o in range(2)]
    today = torch.stack([oracle_meta.merge_labels(probs[f]) for f in range(5)])
    with monkeypatch.context() as mp:
        mp.setattr(Engine, 'fill_holes', _never)
        mp.setattr(holes, 'fill', _never)
        mp.setattr(holes, 'fill_host', _never)
        for kw in ({'holes': None}, {'holes': {}}, {'holes': P(prev_overlap=0.5)}, {'holes': P(), 'keep': (2,)}):
            assert torch.equal(merge_objects(eng, per_object, **kw), today)
    params = P(max_area=ANY, prev_overlap=0.25)
    on = merge_objects(eng, per_object, keep=(2,), holes=params)
    want = holes.fill_host(today.numpy(), params, keep=(2,))
    assert on.dtype == torch.uint8 and np.array_equal(on.numpy(), want) and torch.equal(on[2], today[2])
    assert not torch.equal(on, today)
    cpar = dict(components.DEFAULTS, min_area=3)
    cleaned = merge_objects(eng, per_object, keep=(2,), components=cpar)
    both = merge_objects(eng, per_object, keep=(2,), components=cpar, holes=params)
    assert np.array_equal(both.numpy(), holes.fill_host(cleaned.numpy(), params, keep=(2,)))       # after the filter
    with pytest.raises(ValueError):
        merge_objects(eng, per_object, holes={'max_area': -1})

    class DeviceEngine(LogEngine):                                   # an engine WITH the entry point is called
        calls = []

        def fill_holes(self, labels, prev=None, keep=(), **params):
            DeviceEngine.calls.append((labels.shape[0], prev, tuple(keep), params))
            return torch.from_numpy(holes.fill_host(labels, params, prev=prev, keep=keep))
    dev = DeviceEngine('resnet50', 24, 32, 1)
    assert torch.equal(merge_objects(dev, per_object, keep=(2,), holes=params), on)
    assert DeviceEngine.calls == [(5, None, (2,), params)]


def test_evaluate_sequence_passes_holes_through(monkeypatch):
    from eosvos_amd import evaluate
    cfg = config.parse_cli([])
    cfg['num_epochs']['eval'] = 2
    model = LogDeepLab('resnet50', num_classes=1, batch_norm=cfg['parent_model']['batch_norm'], max_batch=1)
    model._views['backbone.conv1.weight'].view(-1)[0] = 4.0
    mo = MetaOptimizer(model, **cfg['meta_optim_cfg'])
    msd = mo.state_dict()
    images, probs = crf_ref.scene(24, 32, 2, seed=9, n_frames=4)
    gts = [(probs[1, o] > 0.5).float()[None] for o in range(2)]
    plain = evaluate.evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1)
    seen = []
    merge = evaluate.merge_objects
    with monkeypatch.context() as mp:
        mp.setattr(holes, 'fill', _never)
        mp.setattr(evaluate, 'merge_objects', lambda *a, **k: (seen.append(sorted(k)), merge(*a, **k))[1])
        for kw in ({}, {'holes': None}, {'holes': P()}, {'holes': P(prev_overlap=0.5, connectivity=4)}):
            off = evaluate.evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1, **kw)
            assert torch.equal(off[0], plain[0]) and off[2] == plain[2] and all(torch.equal(a, b) for a, b in zip(off[1], plain[1]))
        assert seen == [[]] * 4                                      # no `holes` keyword, nothing else either: today's call
    params = P(max_area=ANY)
    with monkeypatch.context() as mp:
        mp.setattr(evaluate, 'merge_objects', lambda *a, **k: (seen.append(sorted(k)), merge(*a, **k))[1])
        on = evaluate.evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1, holes=params)
    assert seen[-1] == ['holes', 'keep']
    assert all(torch.equal(a, b) for a, b in zip(on[1], plain[1])) and on[2] == plain[2]       # the fine-tunes do not see it
    assert np.array_equal(on[0].numpy(), holes.fill_host(plain[0].numpy(), params, keep=(1,)))
    assert torch.equal(on[0][1], plain[0][1])
    cpar = dict(components.DEFAULTS, min_area=2)
    cleaned = evaluate.evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1, components=cpar)
    both = evaluate.evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1, components=cpar, holes=params)
    assert np.array_equal(both[0].numpy(), holes.fill_host(cleaned[0].numpy(), params, keep=(1,)))
    assert not torch.equal(both[0], cleaned[0]) or not torch.equal(on[0], plain[0])            # something was filled


def test_evaluate_dataset_fills_labels_pngs_and_j(tmp_path, monkeypatch):
    from eosvos_amd import data
    from eosvos_amd.evaluate import evaluate_dataset, prediction_paths
    cfg = config.parse_cli(['eval_holes.max_area=4096', 'eval_holes.prev_overlap=0.25'])
    cfg['num_epochs']['eval'] = 2
    model = LogDeepLab('resnet50', num_classes=1, batch_norm=cfg['parent_model']['batch_norm'], max_batch=2)
    mo = MetaOptimizer(model, **cfg['meta_optim_cfg'])
    ds = data.SyntheticSequences(1, 4, 24, 40, seed=3)
    seq = ds.seqs_names[0]
    plain = evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1)
    with monkeypatch.context() as mp:
        mp.setattr(holes, 'fill', _never)
        off = evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1, holes=P())
    assert torch.equal(off['labels'][seq], plain['labels'][seq]) and off['J_seq'] == plain['J_seq']
    on = evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1, save_dir=str(tmp_path),
                          holes=cfg['eval_holes'])
    labels = on['labels'][seq]
    want = holes.fill_host(plain['labels'][seq].numpy(), cfg['eval_holes'], keep=(0,))
    assert np.array_equal(labels.numpy(), want) and torch.equal(labels[0], plain['labels'][seq][0])
    n_obj = len(ds.sequence_tensors(seq, 'cpu')[1])
    assert on['J_seq'] == [data.sequence_J(labels.numpy(), ds.label_maps(seq), n_obj)]       # J sees the filled maps
    from PIL import Image
    preds, _ = prediction_paths(str(tmp_path), cfg['datasets']['val']['name'], cfg['datasets']['val']['split'])
    png = np.asarray(Image.open(os.path.join(preds, seq, ds.frame_names(seq)[2] + '.png')))
    np.testing.assert_array_equal(png, labels[2].numpy())


# ---- chunking -----------------------------------------------------------------------------------------------------------
class _HostLib:
    """`eosvos_fill_holes` on host pointers through the twin: lets the chunk loop of `Engine.fill_holes` run without a device."""
    def __init__(self):
        self.calls = []

    def eosvos_fill_holes(self, e, labels, n, h, w, connectivity, max_area, q16, oq16, prev, keep, out, filled):
        view = lambda p, *shape: np.ctypeslib.as_array((ctypes.c_uint8 * int(np.prod(shape))).from_address(p.value)).reshape(shape)
        params = P(connectivity=connectivity, max_area=max_area, max_rel_area=q16 / 65536, prev_overlap=oq16 / 65536)
        self.calls.append((n, prev is not None, bytes(keep)))
        res, cnt = holes.fill_host(view(labels, n, h, w), params, prev=None if prev is None else view(prev, h, w),
                                   keep=[f for f in range(n) if keep[f]], return_filled=True)
        view(out, n, h, w)[:] = res
        if filled is not None:
            for f in range(n):
                filled[f] = int(cnt[f])
        return 0


class _HostEngine:
    device = torch.device('cpu')
    h = None
    _check_stream = lambda self: None
    _check_label_maps = Engine._check_label_maps
    fill_holes = Engine.fill_holes

    def __init__(self):
        self.lib = _HostLib()


def test_chunks_of_two_frames_hand_prev_over(monkeypatch):
    labels, prev, keep, _, _ = ref.chain()
    params = P(max_area=16, prev_overlap=0.5)
    want, want_filled = holes.fill_host(labels, params, prev=prev, keep=keep, return_filled=True)
    for step, calls in ((2, [(2, True, b'\1\0'), (2, True, b'\0\0'), (1, True, b'\0')]), (4, [(4, True, b'\1\0\0\0'), (1, True, b'\0')]),
                        (5, [(5, True, b'\1\0\0\0\0')])):
        monkeypatch.setattr(holes, 'frames_per_call', lambda h, w: step)
        eng = _HostEngine()
        out, filled = eng.fill_holes(torch.from_numpy(labels), prev=torch.from_numpy(prev), keep=keep, return_filled=True, **params)
        assert eng.lib.calls == calls
        assert np.array_equal(out.numpy(), want) and np.array_equal(filled, want_filled)
    monkeypatch.setattr(holes, 'frames_per_call', lambda h, w: 2)
    eng = _HostEngine()                                              # no prev: the first chunk has none, the later ones get one
    out = eng.fill_holes(torch.from_numpy(labels), keep=keep, **params)
    assert [c[1] for c in eng.lib.calls] == [False, True, True]
    assert np.array_equal(out.numpy(), holes.fill_host(labels, params, keep=keep))
    assert int(want_filled.sum()) > 0


# ---- C-ABI --------------------------------------------------------------------------------------------------------------
def test_abi_symbol_exists_and_refuses_a_null_engine():
    lib = _ffi.load()
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'eosvos.h')).read()
    assert 'eosvos_fill_holes' in _ffi.exported_symbols() and len(lib.eosvos_fill_holes.argtypes) == 13
    assert 'eosvos_fill_holes(' in hdr
    assert lib.eosvos_fill_holes(None, None, 1, 8, 8, 8, 4, 65536, 0, None, None, None, None) == 1
    assert b'fill_holes' in lib.eosvos_last_error() and b'null' in lib.eosvos_last_error()
