"""Host side of the object-centred zoom pass (`eosvos_amd/zoom.py`): the numpy twin of the box rule against the plain loops of
tests/zoom_ref.py, what `check` rejects, how the configuration carries `eval_zoom`, that "off" makes exactly today's calls,
that the evaluation loop hands `zoom` to every inference call, and the ABI.  CPU only: the engine is the stand-in of
tests/fake_engine.py, extended here with the four zoom entry points restated through `zoom.py`'s host functions."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import zoom_ref  # noqa: E402
from fake_engine import FakeDeepLab, FakeEngine  # noqa: E402

from eosvos_amd import _ffi, config, zoom  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402
from eosvos_amd.meta_optim import MetaOptimizer  # noqa: E402

CASES = zoom_ref.cases()


# ---- the box rule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,p0,prm', CASES, ids=[c[0] for c in CASES])
def test_boxes_host_equals_the_plain_loops(name, p0, prm):
    want = zoom_ref.box_ref(p0, prm)
    got = zoom.boxes_host(p0[None], prm)
    assert got.dtype == np.int32 and got.shape == (1, 5)
    assert tuple(int(v) for v in got[0]) == want
    assert np.array_equal(zoom.boxes_host(torch.from_numpy(p0)[None, None], prm), got)       # (N, 1, H, W) tensors too
    valid, y0, x0, bh, bw = want
    H, W = p0.shape
    assert 0 <= y0 and y0 + bh <= H and 0 <= x0 and x0 + bw <= W
    if not valid:
        assert want == (0, 0, 0, H, W)


def test_the_cases_are_what_their_names_say():
    by_name = {c[0]: c for c in CASES}
    assert zoom_ref.box_ref(*by_name['anchor'][1:]) == zoom_ref.ANCHOR == (1, 29, 49, 32, 54)
    for H, W in zoom_ref.SIZES:
        t = f'{H}x{W}'
        box = lambda n: zoom_ref.box_ref(*by_name[f'{t} {n}'][1:])                                   # noqa: E731
        assert box('pixel at the origin')[:3] == (1, 0, 0) and box('pixel at the far corner')[0] == 1
        far = box('pixel at the far corner')
        assert (far[1] + far[3], far[2] + far[4]) == (H, W)
        assert box('blob on the top border')[1] == 0 and box('blob on the left border')[2] == 0
        b = box('blob on the bottom border')
        assert b[0] == 1 and b[1] + b[3] == H
        b = box('blob on the right border')
        assert b[0] == 1 and b[2] + b[4] == W
        assert box('wanted width exceeds W') == (1, 0, 0, H, W) and box('wanted width exceeds W, too large')[0] == 0
        assert box('min_pixels - 1')[0] == 0 and box('exactly min_pixels')[0] == 1
        b = box('at the min_zoom boundary')
        assert b[0] == 1 and b[3] == H // 2 and box('past the min_zoom boundary')[0] == 0
        assert zoom_ref.active_term(*by_name[f'{t} max_zoom floor active'][1:])[0] == ['floor']
        assert zoom_ref.active_term(*by_name[f'{t} aspect term active'][1:])[0] == ['aspect']
        assert box('max_zoom floor active')[0] == 1 and box('aspect term active')[0] == 1
        assert box('two distant blobs')[0] == 0 and box('empty')[0] == 0
        assert box('exactly at the threshold')[0] == 1                                       # 25 pixels at 0.5, the rest just below


def test_boxes_host_takes_several_frames_and_rejects_other_input():
    p0 = np.stack([zoom_ref.frame(33, 70, (10, 15, 20, 27)), zoom_ref.frame(33, 70), zoom_ref.frame(33, 70, (0, 32, 0, 69))])
    got = zoom.boxes_host(p0, zoom_ref.BASE)
    assert np.array_equal(got, zoom_ref.boxes_ref(p0, zoom_ref.BASE)) and got[:, 0].tolist() == [1, 0, 0]
    with pytest.raises(ValueError):
        zoom.boxes_host(p0.astype(np.float64), zoom_ref.BASE)
    with pytest.raises(ValueError):
        zoom.boxes_host(p0[0], zoom_ref.BASE)
    with pytest.raises(ValueError):
        zoom.boxes_host(p0, dict(zoom_ref.BASE, max_zoom=0))


# ---- check / active -----------------------------------------------------------------------------------------------------
BAD = [{'max_zoom': 0.5}, {'max_zoom': 4.5}, {'max_zoom': -1}, {'max_zoom': True}, {'max_zoom': '3'}, {'max_zoom': float('nan')},
       {'max_zoom': 3, 'min_zoom': 0.9}, {'max_zoom': 3, 'min_zoom': 3.5}, {'max_zoom': 1}, {'max_zoom': 3, 'min_zoom': None},
       {'threshold': 0}, {'threshold': 1}, {'threshold': -0.1}, {'threshold': float('nan')},
       {'min_pixels': 0}, {'min_pixels': 1.5}, {'min_pixels': True},
       {'margin': -0.1}, {'margin': 4.1}, {'margin': float('inf')},
       {'margin_px': -1}, {'margin_px': 257}, {'margin_px': 2.0},
       {'weight': 0}, {'weight': 1.01}, {'weight': float('nan')},
       {'feather': -1}, {'feather': 65}, {'feather': 1.0},
       {'zoom': 3}, [3], 'max_zoom=3']


@pytest.mark.parametrize('bad', BAD, ids=[repr(b) for b in BAD])
def test_every_limit_raises_value_error(bad):
    with pytest.raises(ValueError):
        zoom.check(bad)
    with pytest.raises(ValueError):
        zoom.active(bad)


def test_limits_are_inclusive_where_the_table_says_so_and_off_is_off():
    assert zoom.DEFAULTS == {'max_zoom': 0, 'min_zoom': 1.5, 'threshold': 0.5, 'min_pixels': 16, 'margin': 0.5, 'margin_px': 8,
                             'weight': 0.5, 'feather': 8}
    for ok in ({'max_zoom': 1, 'min_zoom': 1}, {'max_zoom': 4, 'min_zoom': 4}, {'max_zoom': 3, 'margin': 0, 'margin_px': 0},
               {'max_zoom': 3, 'margin': 4, 'margin_px': 256}, {'max_zoom': 3, 'weight': 1, 'feather': 0},
               {'max_zoom': 3, 'feather': 64, 'min_pixels': 1}, {}):
        assert set(zoom.check(ok)) == set(zoom.DEFAULTS)
    assert not zoom.active(None) and not zoom.active({}) and not zoom.active({'max_zoom': 0}) and not zoom.active(zoom.DEFAULTS)
    assert zoom.active({'max_zoom': 3}) and zoom.active({'max_zoom': 1, 'min_zoom': 1})
    assert zoom.q16(1.5) == 98304 and zoom.q16(3) == 196608 and zoom.q16(0.5) == 32768


def test_parse_cli_carries_eval_zoom_only_when_asked():
    groups = ('EXTENSIONS', 'POSTPROCESS', 'CLEANUP', 'FILL', 'SNAP', 'MOTION', 'ZOOM')
    before = copy.deepcopy({g: getattr(config, g) for g in groups + ('BASE',)})
    assert config.ZOOM == {'eval_zoom': zoom.DEFAULTS}
    assert 'eval_zoom' not in config.BASE and 'eval_zoom' not in config.parse_cli([])
    assert 'eval_zoom' not in config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS-OnA', 'num_epochs.eval=3', 'eval_tta.flip=True'])
    cfg = config.parse_cli(['eval_zoom.max_zoom=3', 'eval_zoom.margin=0.25'])
    assert cfg['eval_zoom'] == dict(zoom.DEFAULTS, max_zoom=3, margin=0.25)
    assert all(g not in cfg for g in ('eval_tta', 'eval_crf', 'eval_components', 'eval_holes', 'eval_snap', 'eval_motion'))
    assert {g: getattr(config, g) for g in groups + ('BASE',)} == before                        # nothing leaked
    assert config.EXTENSIONS == {'eval_tta': {'flip': False, 'scales': [1.0]}}
    with pytest.raises(KeyError):
        config.parse_cli(['eval_zoom.zoom=3'])
    for argv in (['eval_zoom.max_zoom=5'], ['eval_zoom.max_zoom=1.5', 'eval_zoom.min_zoom=2'], ['eval_zoom.max_zoom=3', 'eval_zoom.weight=0'],
                 ['eval_zoom.max_zoom=3', 'eval_zoom.feather=65'], ['eval_zoom.threshold=1']):
        with pytest.raises(ValueError):
            config.parse_cli(argv)


# ---- the stand-in with the four entry points ------------------------------------------------------------------------------
class ZoomEngine(FakeEngine):
    """The stand-in with `infer_view` and the four zoom calls restated through `zoom.py`'s host functions in fp32; every
    call is logged."""
    calls = []

    def infer(self, images):
        ZoomEngine.calls.append(('infer', images.shape[0]))
        self._logits = self._net(images)                            # what `debug_tensor('logits')` of the plain path reads
        return super().infer(images)

    def infer_view(self, images, mirror=False):
        ZoomEngine.calls.append(('infer_view', bool(mirror), images.shape[0], (float(self.theta[0]), float(self.theta[-1]))))
        self._logits = self._net(torch.flip(images, [3]) if mirror else images)

    def zoom_boxes(self, probs, params):
        ZoomEngine.calls.append(('zoom_boxes', probs.shape[0]))
        return torch.from_numpy(zoom.boxes_host(probs, params))

    def zoom_crop(self, frames, boxes, out=None):
        ZoomEngine.calls.append(('zoom_crop', frames.shape[0]))
        view = zoom.crop_host(frames, boxes, torch.float32)
        return view if out is None else out.copy_(view)

    def zoom_accumulate(self, boxes, pz, view_weight, mirror=False, first=False):
        ZoomEngine.calls.append(('zoom_accumulate', bool(mirror), bool(first), view_weight))
        part = view_weight * zoom.put_back_host([(self._logits, mirror)], boxes, torch.float32)
        for f, (valid, y0, x0, bh, bw) in enumerate(zoom._boxes_list(boxes)):
            if valid:
                sl = (f, 0, slice(y0, y0 + bh), slice(x0, x0 + bw))
                pz[sl] = part[sl] if first else pz[sl] + part[sl]
        return pz

    def zoom_blend(self, boxes, pz, probs, weight, feather):
        ZoomEngine.calls.append(('zoom_blend', probs.shape[0]))
        return probs.copy_(zoom.blend_host(probs, torch.nan_to_num(pz), boxes, weight, feather, torch.float32))


class ZoomDeepLab(FakeDeepLab):
    def _ensure_engine(self, height, width, batch):
        e = self.engine
        if e is None or e.height != height or e.width != width or batch > e.max_batch:
            self.engine = ZoomEngine(self.encoder, height, width, max(batch, self.max_batch))
            self._dirty = True
        return super()._ensure_engine(height, width, batch)


def _setup(max_batch=3):
    cfg = config.parse_cli([])
    cfg['num_epochs']['eval'] = 3
    cfg['eval_online_adapt'].update(step=3, reset_model_mode='FIRST_STEP', num_epochs=2, min_prop=0.5)
    cfg['data_cfg']['batch_sizes']['train'] = 3
    model = ZoomDeepLab('resnet50', num_classes=1, batch_norm=cfg['parent_model']['batch_norm'], max_batch=max_batch)
    model._flat[0], model._flat[-1] = 6.0, -3.0                      # logits = 6 * mean_c(frame) - 3: a blob of 1s is foreground
    mo = MetaOptimizer(model, **cfg['meta_optim_cfg'])
    frames = torch.zeros(8, 3, 40, 48)
    for i in range(8):
        frames[i, :, 10 + i:18 + i, 12 + i:20 + i] = 1.0
    frames += 0.05 * torch.rand(8, 3, 40, 48, generator=torch.Generator().manual_seed(2))
    gt = torch.zeros(1, 40, 48)
    gt[:, 10:18, 12:20] = 1.0
    return cfg, model, mo, mo.state_dict(), frames, gt


Z = {'max_zoom': 3, 'min_zoom': 1.5, 'margin': 0.5, 'margin_px': 2, 'min_pixels': 4, 'weight': 0.5, 'feather': 3}


def _raise(*a, **k):
    raise AssertionError('a zoom call on the plain path')


def test_off_makes_exactly_todays_calls(monkeypatch):
    from eosvos_amd.evaluate import evaluate_sequence
    from eosvos_amd.helper_func import run_frames
    cfg, model, mo, msd, frames, gt = _setup()
    gts = gt.expand(2, 1, 40, 48)
    for cls in (Engine, ZoomEngine):
        for name in ('zoom_boxes', 'zoom_crop', 'zoom_accumulate', 'zoom_blend'):
            assert callable(getattr(cls, name))
            monkeypatch.setattr(cls, name, _raise)
    runs, logs = [], []
    for kw in ({}, {'zoom': None}, {'zoom': {'max_zoom': 0}}, {'zoom': dict(zoom.DEFAULTS)}):
        ZoomEngine.calls = []
        runs.append(run_frames(model, frames[:2], gts, **kw))
        logs.append(ZoomEngine.calls)
    assert logs[0] == [('infer', 1), ('infer', 1)] and all(l == logs[0] for l in logs)
    for losses, accs, probs in runs[1:]:
        assert torch.equal(probs, runs[0][2]) and torch.equal(losses, runs[0][0]) and torch.equal(accs, runs[0][1])
    outs, logs = [], []
    for kw in ({}, {'zoom': None}, {'zoom': {'max_zoom': 0}}):
        ZoomEngine.calls = []
        outs.append(evaluate_sequence(model, mo, msd, frames, [gt], cfg, **kw))
        logs.append(ZoomEngine.calls)
    assert logs[0] and {c[0] for c in logs[0]} == {'infer'} and all(l == logs[0] for l in logs)
    for labels, probs, hist in outs[1:]:
        assert torch.equal(labels, outs[0][0]) and torch.equal(probs[0], outs[0][1][0]) and hist == outs[0][2]
    with pytest.raises(AssertionError, match='zoom call'):
        run_frames(model, frames[:1], zoom=Z)                                                   # and on means on
    with pytest.raises(ValueError):
        run_frames(model, frames[:1], zoom={'max_zoom': 5})


def test_run_frames_with_zoom_is_the_composed_pipeline():
    from eosvos_amd.helper_func import run_frames
    cfg, model, mo, msd, frames, gt = _setup()
    gts = gt.expand(2, 1, 40, 48)
    plain = run_frames(model, frames[:2], gts)
    eng = model.engine
    for tta, mirrors in ((None, [False]), ({'flip': True, 'scales': [1.0]}, [False, True])):
        ZoomEngine.calls = []
        kw = {} if tta is None else {'tta': tta}
        if tta is not None:
            eng.tta_accumulate = lambda acc, weight, mirror=False, first=False, e=eng: acc.copy_(        # identity-size views
                weight * torch.sigmoid(torch.flip(e._logits, [3]) if mirror else e._logits) + (0 if first else acc))
        losses, accs, probs = run_frames(model, frames[:2], gts, zoom=Z, **kw)
        per_frame = [c[0] for c in ZoomEngine.calls if c[0].startswith('zoom') or c[0] == 'infer_view'][-(3 + 2 * len(mirrors)):]
        assert per_frame == ['zoom_boxes', 'zoom_crop'] + ['infer_view', 'zoom_accumulate'] * len(mirrors) + ['zoom_blend']
        acc_calls = [c for c in ZoomEngine.calls if c[0] == 'zoom_accumulate']
        assert [c[1:] for c in acc_calls[:len(mirrors)]] == [(m, k == 0, 1.0 / len(mirrors)) for k, m in enumerate(mirrors)]
        score = lambda view, mirror: eng._net(torch.flip(view, [3]) if mirror else view)             # noqa: E731
        for i in range(2):
            want, boxes = zoom.refine_host(frames[i:i + 1], plain[2][i:i + 1], Z, score, flip=len(mirrors) == 2, dtype=torch.float32)
            assert boxes[0, 0] == 1 and boxes[0, 3] < 40                                            # a real, magnifying box
            assert float((probs[i:i + 1] - want).abs().max()) < 1e-6
        assert float((probs - plain[2]).abs().max()) > 1e-4                                         # the second look changed something
        assert losses.shape == (2,) and bool(torch.isfinite(losses).all()) and accs.shape == (2,)


def test_evaluate_sequence_hands_zoom_to_every_inference_batch():
    from eosvos_amd.evaluate import (evaluate_sequence, finetune_object, object_workers, online_adapt_schedule,
                                     run_objects_in_flight)
    cfg, model, mo, msd, frames, gt = _setup()
    ZoomEngine.calls = []
    plain = evaluate_sequence(model, mo, msd, frames, [gt], cfg)
    n_infer = [c[1] for c in ZoomEngine.calls if c[0] == 'infer']
    ZoomEngine.calls = []
    labels, probs, hist = evaluate_sequence(model, mo, msd, frames, [gt], cfg, zoom=Z)
    calls = ZoomEngine.calls
    rounds = online_adapt_schedule(8, 0, 3, 3)
    batches = [min(3, r['eval_max'] - f) for r in rounds for f in range(r['eval_min'], r['eval_max'], 3)]
    assert [c[1] for c in calls if c[0] == 'infer'] == batches == n_infer                   # the first pass stays today's call
    for name in ('zoom_boxes', 'zoom_crop', 'zoom_blend'):
        assert [c[1] for c in calls if c[0] == name] == batches
    iv = [c for c in calls if c[0] == 'infer_view']
    assert [c[1:3] for c in iv] == [(False, b) for b in batches]
    assert (6.0, -3.0) not in {c[3] for c in iv} and len({c[3] for c in iv}) > 1               # the rounds' fine-tuned weights
    assert hist[0][0] == plain[2][0][0] and probs[0].shape == plain[1][0].shape                 # round 0 trains before any inference
    assert not torch.equal(probs[0][1:4], plain[1][0][1:4])
    # the objects-in-flight path passes it through, with the same result as one object after the other
    gts = [gt, torch.roll(gt, 3, 2)]
    one = [finetune_object(model, mo, msd, frames, g, cfg, zoom=Z) for g in gts]
    workers = object_workers(model, mo, cfg['meta_optim_cfg'], 2)
    con = run_objects_in_flight(workers, msd, frames, gts, cfg, zoom=Z)
    for (p2, h2), (p1, h1) in zip(con, one):
        assert h2 == h1 and torch.equal(p2, p1)


# ---- the library --------------------------------------------------------------------------------------------------------
def test_abi_symbols_exist_in_the_built_library():
    lib = _ffi.load()
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'eosvos.h')).read()
    exported = _ffi.exported_symbols()
    for name, n_args in (('eosvos_zoom_boxes', 12), ('eosvos_zoom_crop', 8), ('eosvos_zoom_accumulate', 7), ('eosvos_zoom_blend', 9)):
        assert name in exported and len(getattr(lib, name).argtypes) == n_args and name + '(' in hdr
        decl = hdr[hdr.rindex('int ' + name + '('):]
        assert decl[:decl.index(';')].count(',') + 1 == n_args                                 # the header's argument count
    # null engines are refused on the host, before anything touches a device
    assert lib.eosvos_zoom_boxes(None, None, 1, 8, 8, 0.5, 1, 0, 0, 65536, 65536, None) == 1
    assert b'null' in lib.eosvos_last_error()
    assert lib.eosvos_zoom_crop(None, None, None, 1, 3, 8, 8, None) == 1
    assert lib.eosvos_zoom_accumulate(None, None, 1, 0, 1.0, 1, None) == 1
    assert lib.eosvos_zoom_blend(None, None, 1, 8, 8, 0.5, 0, None, None) == 1
    assert b'null' in lib.eosvos_last_error()
