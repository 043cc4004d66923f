"""Host side of the superpixel snapping (`eosvos_amd/snap.py`): the numpy twin (`superpixels_host`, `snap_host`) against the
plain loops of tests/snap_ref.py, bit for bit; the tie rules on hand-written cases; what the parameter dictionary accepts; how
the configuration carries it; that the evaluation hands it through in the order CRF -> snap -> components -> holes; the chunking
of `Engine.snap_labels`; the C-ABI symbols.  CPU only: the engine is the stand-in of tests/fake_engine.py, which has no
`snap_labels` and so takes `snap_host`."""
import copy
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import crf_ref  # noqa: E402
import snap_ref as ref  # noqa: E402
from test_crf_host import LogDeepLab, LogEngine  # noqa: E402

from eosvos_amd import _ffi, components, config, crf, holes, snap  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402
from eosvos_amd.meta_optim import MetaOptimizer  # noqa: E402
from oracle import meta as oracle_meta  # noqa: E402


def P(**kw):
    return dict(snap.DEFAULTS, **kw)


# ---- the numpy twin against the loops -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loop_case(h, w, S, T, m, n_obj):
    """(rgb, labels, what the loops give with frame 1 kept); computed once, never changed."""
    rgb = ref.noise_rgb(2, h, w, seed=S + T + m)
    lab = ref.blob_labels(2, h, w, n_obj, seed=m)
    return rgb, lab, ref.snap_ref(rgb, lab, n_obj, S, T, m, snap.share_q16(0.5), keep=(1,))


@pytest.mark.parametrize('n_obj', [1, 3])
@pytest.mark.parametrize('m', [1, 10, 64])
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('S', [4, 8])
@pytest.mark.parametrize('h,w', [(1, 1), (5, 7), (37, 53)])
def test_twin_equals_the_loops(h, w, S, T, m, n_obj):
    rgb, lab, (want, want_ids, want_changed, _) = loop_case(h, w, S, T, m, n_obj)
    params = P(step=S, iterations=T, compactness=m)
    got, changed = snap.snap_host(rgb, lab, params, keep=(1,), n_obj=n_obj, return_changed=True)
    ids = snap.superpixels_host(rgb, params)
    assert got.dtype == np.uint8 and ids.dtype == np.int32 and changed.dtype == np.int64
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(changed, want_changed)
    assert (lab > n_obj).any() or (h, w) == (1, 1)                   # labels above n_obj are in the input ...
    np.testing.assert_array_equal(got[lab > n_obj], lab[lab > n_obj])              # ... and pass unchanged
    np.testing.assert_array_equal(got[1], lab[1])                    # the keep frame


def test_a_cluster_that_becomes_empty_keeps_its_centre():
    rgb = ref.binary_rgb(1, 37, 53, seed=0)                          # heavy noise, m = 1: colour alone decides
    lab = ref.blob_labels(1, 37, 53, 3, seed=0)
    want, want_ids, _, empties = ref.snap_ref(rgb, lab, 3, 4, 3, 1, snap.share_q16(0.5))
    assert empties > 0                                               # the n = 0 rule is exercised
    params = P(step=4, iterations=3, compactness=1)
    np.testing.assert_array_equal(snap.superpixels_host(rgb, params), want_ids)
    np.testing.assert_array_equal(snap.snap_host(rgb, lab, params, n_obj=3), want)


# ---- tie rules ----------------------------------------------------------------------------------------------------------
def test_constant_colour_gives_the_nearest_initial_centre_with_ties_to_the_smaller_id():
    # 7 x 10, S = 4: two rows of three cells with centres at y = 2, 6 and x = 2, 6, 9.  y = 4 is as far from 2 as from 6 and
    # x = 4 as far from 2 as from 6: both go to the smaller id.
    rgb = np.full((1, 3, 7, 10), 77, dtype=np.uint8)
    cols = [0, 0, 0, 0, 0, 1, 1, 1, 2, 2]
    want = np.array([[0 + c for c in cols]] * 5 + [[3 + c for c in cols]] * 2, dtype=np.int32)
    for m in (1, 10, 64):
        ids = snap.superpixels_host(rgb, P(step=4, iterations=1, compactness=m))
        np.testing.assert_array_equal(ids[0], want)
        np.testing.assert_array_equal(np.array(ref.superpixels_ref(rgb[0], 4, 1, m)[0]), want)


def test_vote_ties_and_the_exact_threshold():
    # 1 x 8, S = 4, constant colour, one iteration: cluster 0 is x = 0..4 (x = 4 is a tie), cluster 1 is x = 5..7
    rgb = np.full((1, 3, 1, 8), 9, dtype=np.uint8)
    params = P(step=4, iterations=1)
    np.testing.assert_array_equal(snap.superpixels_host(rgb, params)[0, 0], [0, 0, 0, 0, 0, 1, 1, 1])

    def run(labels, n_obj=2, **kw):
        lab = np.array([[labels]], dtype=np.uint8)
        got = snap.snap_host(rgb, lab, dict(params, **kw), n_obj=n_obj)
        q = snap.share_q16(dict(params, **kw)['min_share'])
        np.testing.assert_array_equal(got, ref.snap_ref(rgb, lab, n_obj, 4, 1, 10, q)[0])
        return got[0, 0].tolist()
    # equal counts: the smaller label wins (2 of 4 voters, min_share 0.5 is met exactly); label 200 > n_obj does not vote
    assert run([2, 1, 2, 1, 200, 0, 0, 0]) == [1, 1, 1, 1, 200, 0, 0, 0]
    assert run([0, 2, 2, 0, 200, 2, 1, 0]) == [0, 0, 0, 0, 200, 2, 1, 0]          # 0 is a label like the others; 1 of 3 is no half
    # exactly on the threshold: 3 of 4 voters, q = 49152: 3 * 65536 == 49152 * 4 snaps; one vote less does not
    assert snap.share_q16(0.75) * 4 == 3 * 65536
    assert run([1, 1, 1, 0, 200, 2, 2, 2], min_share=0.75) == [1, 1, 1, 1, 200, 2, 2, 2]
    assert run([1, 1, 2, 0, 200, 2, 2, 2], min_share=0.75) == [1, 1, 2, 0, 200, 2, 2, 2]
    assert run([1, 1, 1, 0, 200, 2, 2, 2], min_share=0.75 + 2.0 ** -16) == [1, 1, 1, 0, 200, 2, 2, 2]
    # a pixel above n_obj would have tipped the vote had it counted
    assert run([1, 1, 2, 2, 2, 0, 0, 0], n_obj=2) == [2, 2, 2, 2, 2, 0, 0, 0]
    assert run([1, 1, 2, 2, 2, 0, 0, 0], n_obj=1) == [1, 1, 2, 2, 2, 0, 0, 0]
    # a cluster without voters is copied
    assert run([7, 7, 7, 7, 7, 1, 0, 1], min_share=0.0) == [7, 7, 7, 7, 7, 1, 1, 1]


def test_min_share_one_changes_nothing_and_zero_always_snaps():
    rgb, lab = ref.noise_rgb(2, 37, 53, seed=5, smooth=True), ref.blob_labels(2, 37, 53, 3, seed=5)
    params = P(step=8, iterations=3)
    got, changed = snap.snap_host(rgb, lab, dict(params, min_share=1.0), n_obj=3, return_changed=True)
    np.testing.assert_array_equal(got, lab)                          # only uniform clusters pass, and they are unchanged
    assert not changed.any()
    got, changed = snap.snap_host(rgb, lab, dict(params, min_share=0.0), n_obj=3, return_changed=True)
    ids = snap.superpixels_host(rgb, params)
    for f in range(2):
        for c in np.unique(ids[f]):
            voters = (ids[f] == c) & (lab[f] <= 3)
            assert len(np.unique(got[f][voters])) <= 1               # every cluster holds one label among its voters
    np.testing.assert_array_equal(changed, (got != lab).sum(axis=(1, 2)))
    assert changed.all()
    kept = snap.snap_host(rgb, lab, dict(params, min_share=0.0), keep=(0,), n_obj=3)
    np.testing.assert_array_equal(kept[0], lab[0])
    np.testing.assert_array_equal(kept[1], got[1])
    np.testing.assert_array_equal(snap.snap_host(rgb, lab, P(), n_obj=3), lab)       # step 0: a copy


@pytest.mark.parametrize('h,w,S', [(37, 53, 8), (97, 161, 16)])
def test_snapping_reduces_the_wrong_pixels_of_a_shifted_prediction(h, w, S):
    rgb, truth, pred = ref.disc_scene(h, w)
    out = snap.snap_host(rgb, pred, P(step=S), n_obj=2)
    before, after = int((pred != truth).sum()), int((out != truth).sum())
    print(f'{h} x {w}, S {S}: {before} -> {after} wrong pixels')
    assert after < before


# ---- parameters ---------------------------------------------------------------------------------------------------------
def test_check_and_active():
    assert snap.check({}) == snap.DEFAULTS and snap.check({'step': 16})['step'] == 16
    assert not snap.active(None) and not snap.active({}) and not snap.active(P()) and not snap.active(P(min_share=0.9))
    assert snap.active(P(step=4)) and snap.active({'step': 64})
    for bad in (None, [], {'radius': 3}, {'step': 3}, {'step': 65}, {'step': -4}, {'step': 16.0}, {'step': True},
                {'iterations': 0}, {'iterations': 21}, {'iterations': 2.5}, {'compactness': 0}, {'compactness': 65},
                {'compactness': '10'}, {'min_share': -0.1}, {'min_share': 1.5}, {'min_share': float('nan')}, {'min_share': '1'},
                {'min_share': True}):
        with pytest.raises(ValueError):
            snap.check(bad)
        if bad is not None:
            with pytest.raises(ValueError):
                snap.active(bad)
    rgb, lab = np.zeros((1, 3, 4, 4), dtype=np.uint8), np.zeros((1, 4, 4), dtype=np.uint8)
    for n_obj in (0, 256, 1.5):
        with pytest.raises(ValueError):
            snap.snap_host(rgb, lab, P(step=4), n_obj=n_obj)
    with pytest.raises(ValueError):
        snap.snap_host(rgb, lab[:, :3], P(step=4))
    with pytest.raises(ValueError):
        snap.snap_host(rgb.astype(np.float32), lab, P(step=4))
    with pytest.raises(ValueError):
        snap.superpixels_host(rgb, P())


def test_frames_per_call_accounts_for_ids_clusters_and_votes(monkeypatch):
    h, w, n_obj = 480, 854, 3
    k = 30 * 54                                                      # S = 16
    assert snap.grid(h, w, 16) == (30, 54)
    assert snap.scratch_bytes(1, n_obj, h, w, 16) == 4 * (h * w + k * (5 + 6) + k * (n_obj + 1)) + 8 + 8
    per_frame = snap.scratch_bytes(1, n_obj, h, w, 16) - 8
    assert snap.frames_per_call(n_obj, h, w, 16) == (snap.SCRATCH_CAP - 8) // per_frame
    assert snap.frames_per_call(n_obj, h, w) == snap.frames_per_call(n_obj, h, w, 4) <= snap.frames_per_call(n_obj, h, w, 16)
    assert snap.frames_per_call(255, 4096, 4096, 4) == 1            # over the cap: the library's to reject
    monkeypatch.setattr(snap, 'SCRATCH_CAP', per_frame + 8)
    assert snap.frames_per_call(n_obj, h, w, 16) == 1
    monkeypatch.setattr(snap, 'SCRATCH_CAP', 3 * per_frame + 8)
    assert snap.frames_per_call(n_obj, h, w, 16) == 3


def test_quantise_equals_the_numpy_expression():
    g = torch.Generator().manual_seed(3)
    rgb8 = torch.randint(0, 256, (2, 3, 9, 11), generator=g, dtype=torch.uint8)
    mean = (104.00699, 116.66877, 122.67892)
    plain = rgb8.float() / 255.0
    shifted = (rgb8.float() - torch.tensor(mean).view(1, 3, 1, 1)) / 255.0
    noisy = torch.rand(2, 3, 9, 11, generator=g) * 1.2 - 0.1         # outside [0, 1] as well: the clamp
    for frames, offset in ((plain, None), (shifted, mean), (noisy, None), (noisy, mean)):
        got = snap.quantise(frames, offset)
        x = frames.numpy() * np.float32(255.0)
        if offset is not None:
            x = x + np.asarray(offset, dtype=np.float32).reshape(1, 3, 1, 1)
        want = np.clip(np.round(x), 0, 255).astype(np.uint8)
        assert got.dtype == torch.uint8 and x.dtype == np.float32
        np.testing.assert_array_equal(got.numpy(), want)
    assert torch.equal(snap.quantise(plain), rgb8) and torch.equal(snap.quantise(shifted, mean), rgb8)       # the round trip


# ---- configuration ------------------------------------------------------------------------------------------------------
def test_parse_cli_carries_eval_snap_only_when_asked():
    groups = (config.BASE, config.EXTENSIONS, config.POSTPROCESS, config.CLEANUP, config.FILL)
    before = [copy.deepcopy(g) for g in groups]
    assert config.SNAP == {'eval_snap': snap.DEFAULTS} and not snap.active(config.SNAP['eval_snap'])
    for g in groups + (config.parse_cli([]),):
        assert 'eval_snap' not in g
    assert 'eval_snap' not in config.parse_cli(['with', 'DAVIS-2017', 'eval_crf.iterations=5', 'eval_holes.max_area=3'])
    cfg = config.parse_cli(['eval_snap.step=16', 'eval_snap.min_share=0.6'])
    assert cfg['eval_snap'] == P(step=16, min_share=0.6) and snap.active(cfg['eval_snap'])
    assert all(k not in cfg for k in ('eval_crf', 'eval_tta', 'eval_components', 'eval_holes'))
    assert config.parse_cli(['eval_snap.compactness=20'])['eval_snap'] == P(compactness=20)             # still off
    assert [copy.deepcopy(g) for g in groups] == before and config.SNAP == {'eval_snap': snap.DEFAULTS}  # nothing leaked
    with pytest.raises(KeyError):
        config.parse_cli(['eval_snap.radius=3'])
    for bad in ('eval_snap.step=3', 'eval_snap.step=65', 'eval_snap.iterations=0', 'eval_snap.compactness=65',
                'eval_snap.min_share=1.5', 'eval_snap.step=16.5'):
        with pytest.raises(ValueError):
            config.parse_cli([bad])


# ---- the evaluation -----------------------------------------------------------------------------------------------------
def _never(*a, **k):
    raise AssertionError('the snapping stage was called on the plain path')


class CountingEngine(LogEngine):
    """The stand-in with the four stage entry points, each the host twin, logging the order of the calls."""
    calls = []

    def crf_labels(self, images, probs, return_q=False, **params):
        CountingEngine.calls.append('crf')
        return crf.refine_host(images, probs, params, dtype=torch.float32)[0]

    def snap_labels(self, rgb, labels, n_obj=255, keep=(), **params):
        CountingEngine.calls.append('snap')
        return torch.from_numpy(snap.snap_host(rgb, labels, params, keep=keep, n_obj=n_obj))

    def superpixels(self, rgb, **params):
        CountingEngine.calls.append('superpixels')
        return torch.from_numpy(snap.superpixels_host(rgb, params))

    def filter_components(self, labels, prev=None, keep=(), **params):
        CountingEngine.calls.append('components')
        return torch.from_numpy(components.filter_host(labels, params, prev=prev, keep=keep))

    def fill_holes(self, labels, prev=None, keep=(), **params):
        CountingEngine.calls.append('holes')
        return torch.from_numpy(holes.fill_host(labels, params, prev=prev, keep=keep))


def test_merge_objects_off_is_today_and_on_runs_between_the_crf_and_the_filter(monkeypatch):
    from eosvos_amd.evaluate import merge_objects
    images, probs = crf_ref.scene(24, 32, 2, seed=4, n_frames=5)
    probs[2] = 2.0 * (probs[2] > 0.5)                                # a seeded train frame
    per_object = [probs[:, o] for o in range(2)]
    today = torch.stack([oracle_meta.merge_labels(probs[f]) for f in range(5)])
    eng = CountingEngine('resnet50', 24, 32, 1)
    CountingEngine.calls = []
    with monkeypatch.context() as mp:
        mp.setattr(snap, 'snap', _never)
        mp.setattr(snap, 'snap_host', _never)
        mp.setattr(snap, 'quantise', _never)
        for kw in ({'snap': None}, {'snap': {}}, {'snap': P(min_share=0.9)}, {'snap': P(), 'keep': (2,)},
                   {'snap': P(), 'frames': images}):
            assert torch.equal(merge_objects(eng, per_object, **kw), today)
    assert CountingEngine.calls == []                                # none of the new calls, nor any other stage
    sp = P(step=4, iterations=3, min_share=0.0)
    rgb = snap.quantise(images)
    on = merge_objects(eng, per_object, images, keep=(2,), snap=sp)
    assert CountingEngine.calls == ['snap']
    want = snap.snap_host(rgb, today, sp, keep=(2,), n_obj=2)
    assert on.dtype == torch.uint8 and np.array_equal(on.numpy(), want) and torch.equal(on[2], today[2])
    assert not torch.equal(on, today)
    # all four stages: CRF -> snap -> components -> holes, composed from the host twins
    cp = dict(crf.DEFAULTS, radius=1, dilation=1, iterations=1)
    fp = dict(components.DEFAULTS, min_area=3)
    hp = dict(holes.DEFAULTS, max_area=1 << 24)
    sc = P(step=4, iterations=3, min_share=0.8)
    CountingEngine.calls = []
    chain = merge_objects(eng, per_object, images, cp, keep=(2,), components=fp, holes=hp, snap=sc)
    assert CountingEngine.calls == ['crf', 'snap', 'components', 'holes']
    refined = merge_objects(LogEngine('resnet50', 24, 32, 1), per_object, images, cp, keep=(2,)).numpy()
    snapped = snap.snap_host(rgb, refined, sc, keep=(2,), n_obj=2)
    cleaned = components.filter_host(snapped, fp, keep=(2,))
    filled = holes.fill_host(cleaned, hp, keep=(2,))
    np.testing.assert_array_equal(chain.numpy(), filled)
    assert not np.array_equal(snapped, refined) and not np.array_equal(cleaned, snapped) and not np.array_equal(filled, cleaned)
    swapped = snap.snap_host(rgb, components.filter_host(refined, fp, keep=(2,)), sc, keep=(2,), n_obj=2)
    assert not np.array_equal(swapped, cleaned)                      # the filter before the snapping gives other maps
    # an engine without the entry points takes the twins and gives the same maps
    plain_engine = merge_objects(LogEngine('resnet50', 24, 32, 1), per_object, images, cp, keep=(2,), components=fp, holes=hp, snap=sc)
    assert torch.equal(plain_engine, chain)
    # the offset of a normalised data set reaches the quantiser
    mean = (104.00699, 116.66877, 122.67892)
    shifted = images - torch.tensor(mean).view(1, 3, 1, 1) / 255.0
    assert torch.equal(merge_objects(eng, per_object, shifted, keep=(2,), snap=sp, frame_offset=mean), on)
    for frames in (None, images[:4], images[:, :, :20]):
        with pytest.raises(ValueError, match='snap needs the frames'):
            merge_objects(eng, per_object, frames, snap=sp)
    with pytest.raises(ValueError):
        merge_objects(eng, per_object, images, snap={'step': 3})


def test_evaluate_sequence_passes_snap_through(monkeypatch):
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
        mp.setattr(snap, 'snap', _never)
        mp.setattr(evaluate, 'merge_objects', lambda *a, **k: (seen.append(sorted(k)), merge(*a, **k))[1])
        for kw in ({}, {'snap': None}, {'snap': P()}, {'snap': P(iterations=2, min_share=0.1)}):
            off = evaluate.evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1, **kw)
            assert torch.equal(off[0], plain[0]) and off[2] == plain[2] and all(torch.equal(a, b) for a, b in zip(off[1], plain[1]))
        assert seen == [[]] * 4                                      # no `snap` keyword, nothing else either: today's call
    sp = P(step=4, min_share=0.0)
    with monkeypatch.context() as mp:
        mp.setattr(evaluate, 'merge_objects', lambda *a, **k: (seen.append(sorted(k)), merge(*a, **k))[1])
        on = evaluate.evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1, snap=sp)
        assert seen[-1] == ['keep', 'snap']
        norm = copy.deepcopy(cfg)
        norm['data_cfg']['normalize'] = True
        evaluate.evaluate_sequence(model, mo, msd, images, gts, norm, train_frame_id=1, snap=sp)
        assert seen[-1] == ['frame_offset', 'keep', 'snap']
    assert all(torch.equal(a, b) for a, b in zip(on[1], plain[1])) and on[2] == plain[2]       # the fine-tunes do not see it
    want = snap.snap_host(snap.quantise(images), plain[0], sp, keep=(1,), n_obj=2)
    assert np.array_equal(on[0].numpy(), want) and torch.equal(on[0][1], plain[0][1]) and not torch.equal(on[0], plain[0])


def test_evaluate_dataset_snaps_labels_and_j(monkeypatch):
    from eosvos_amd import data
    from eosvos_amd.evaluate import evaluate_dataset
    cfg = config.parse_cli(['eval_snap.step=4', 'eval_snap.min_share=0.0'])
    cfg['num_epochs']['eval'] = 2
    model = LogDeepLab('resnet50', num_classes=1, batch_norm=cfg['parent_model']['batch_norm'], max_batch=2)
    mo = MetaOptimizer(model, **cfg['meta_optim_cfg'])
    ds = data.SyntheticSequences(1, 4, 24, 40, seed=3)
    seq = ds.seqs_names[0]
    plain = evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1)
    with monkeypatch.context() as mp:
        mp.setattr(snap, 'snap', _never)
        off = evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1, snap=P())
    assert torch.equal(off['labels'][seq], plain['labels'][seq]) and off['J_seq'] == plain['J_seq']
    on = evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1, snap=cfg['eval_snap'])
    labels = on['labels'][seq]
    frames, gts = ds.sequence_tensors(seq, 'cpu')[:2]
    want = snap.snap_host(snap.quantise(frames), plain['labels'][seq], cfg['eval_snap'], keep=(0,), n_obj=len(gts))
    assert np.array_equal(labels.numpy(), want) and torch.equal(labels[0], plain['labels'][seq][0])
    assert on['J_seq'] == [data.sequence_J(labels.numpy(), ds.label_maps(seq), len(gts))]       # J sees the snapped maps


# ---- chunking -----------------------------------------------------------------------------------------------------------
class _HostLib:
    """`eosvos_snap_labels` / `eosvos_superpixels` on host pointers through the twin: lets the chunk loops of the `Engine`
    methods run without a device."""
    def __init__(self):
        self.calls = []

    @staticmethod
    def _view(p, dtype, *shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return np.frombuffer((ctypes.c_uint8 * n).from_address(p.value), dtype=dtype).reshape(shape)

    def eosvos_snap_labels(self, e, rgb, labels, n, h, w, n_obj, step, iterations, compactness, q16, keep, out, changed):
        params = P(step=step, iterations=iterations, compactness=compactness, min_share=q16 / 65536)
        self.calls.append((n, bytes(keep), changed is not None))
        res, cnt = snap.snap_host(self._view(rgb, np.uint8, n, 3, h, w), self._view(labels, np.uint8, n, h, w), params,
                                  keep=[f for f in range(n) if keep[f]], n_obj=n_obj, return_changed=True)
        self._view(out, np.uint8, n, h, w)[:] = res
        if changed is not None:
            for f in range(n):
                changed[f] = int(cnt[f])
        return 0

    def eosvos_superpixels(self, e, rgb, n, h, w, step, iterations, compactness, ids):
        self.calls.append((n,))
        self._view(ids, np.int32, n, h, w)[:] = snap.superpixels_host(self._view(rgb, np.uint8, n, 3, h, w),
                                                                       P(step=step, iterations=iterations, compactness=compactness))
        return 0


class _HostEngine:
    device = torch.device('cpu')
    h = None
    _check_stream = lambda self: None
    _check_rgb = Engine._check_rgb
    snap_labels = Engine.snap_labels
    superpixels = Engine.superpixels

    def __init__(self):
        self.lib = _HostLib()


def test_engine_methods_chunk_under_the_scratch_cap(monkeypatch):
    rgb, lab = ref.noise_rgb(5, 20, 33, seed=2, smooth=True), ref.blob_labels(5, 20, 33, 2, seed=2)
    params = P(step=8, iterations=2, min_share=0.3)
    want, want_changed = snap.snap_host(rgb, lab, params, keep=(0, 3), n_obj=2, return_changed=True)
    want_ids = snap.superpixels_host(rgb, params)
    per_frame = snap.scratch_bytes(1, 2, 20, 33, 8) - 8
    for frames, calls in ((1, [(1, b'\1', True), (1, b'\0', True), (1, b'\0', True), (1, b'\1', True), (1, b'\0', True)]),
                          (2, [(2, b'\1\0', True), (2, b'\0\1', True), (1, b'\0', True)]), (9, [(5, b'\1\0\0\1\0', True)])):
        monkeypatch.setattr(snap, 'SCRATCH_CAP', frames * per_frame + 8)
        eng = _HostEngine()
        out, changed = eng.snap_labels(torch.from_numpy(rgb), torch.from_numpy(lab), n_obj=2, keep=(0, 3), return_changed=True, **params)
        assert eng.lib.calls == calls
        assert np.array_equal(out.numpy(), want) and np.array_equal(changed, want_changed)
    eng = _HostEngine()                                              # the cap is still that of 9 frames, with n_obj = 2 votes
    assert torch.equal(eng.snap_labels(torch.from_numpy(rgb), torch.from_numpy(lab), n_obj=2, **params),
                       torch.from_numpy(snap.snap_host(rgb, lab, params, n_obj=2)))
    assert eng.lib.calls == [(5, b'\0' * 5, False)]
    monkeypatch.setattr(snap, 'SCRATCH_CAP', 2 * (snap.scratch_bytes(1, 0, 20, 33, 8) - 8) + 8)
    eng = _HostEngine()
    ids = eng.superpixels(torch.from_numpy(rgb), step=8, iterations=2)
    assert eng.lib.calls == [(2,), (2,), (1,)] and ids.dtype == torch.int32 and np.array_equal(ids.numpy(), want_ids)
    off = eng.snap_labels(torch.from_numpy(rgb), torch.from_numpy(lab), n_obj=2, step=0)
    assert torch.equal(off, torch.from_numpy(lab)) and len(eng.lib.calls) == 3                     # step 0: a copy, no call
    for bad in (dict(step=3), dict(iterations=0), dict(compactness=65), dict(min_share=2.0), dict(n_obj=256), dict(n_obj=0)):
        with pytest.raises(ValueError):
            eng.snap_labels(torch.from_numpy(rgb), torch.from_numpy(lab), **dict(dict(step=8), **bad))
    with pytest.raises(ValueError):
        eng.superpixels(torch.from_numpy(rgb), step=0)
    with pytest.raises(ValueError):
        eng.snap_labels(torch.from_numpy(rgb).float(), torch.from_numpy(lab), step=8)
    with pytest.raises(ValueError):
        eng.snap_labels(torch.from_numpy(rgb), torch.from_numpy(lab[:, :10]), step=8)


# ---- C-ABI --------------------------------------------------------------------------------------------------------------
def test_abi_symbols_exist_and_refuse_a_null_engine():
    lib = _ffi.load()
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'eosvos.h')).read()
    exported = _ffi.exported_symbols()
    assert 'eosvos_superpixels' in exported and len(lib.eosvos_superpixels.argtypes) == 9
    assert 'eosvos_snap_labels' in exported and len(lib.eosvos_snap_labels.argtypes) == 14
    assert 'eosvos_superpixels(' in hdr and 'eosvos_snap_labels(' in hdr
    assert lib.eosvos_superpixels(None, None, 1, 8, 8, 8, 1, 10, None) == 1
    assert b'superpixels' in lib.eosvos_last_error() and b'null' in lib.eosvos_last_error()
    assert lib.eosvos_snap_labels(None, None, None, 1, 8, 8, 1, 8, 1, 10, 32768, None, None, None) == 1
    assert b'snap_labels' in lib.eosvos_last_error() and b'null' in lib.eosvos_last_error()
