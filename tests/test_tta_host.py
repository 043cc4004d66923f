"""Host side of test-time augmentation (`eosvos_amd/tta.py`): which views a `tta` dictionary means, what is rejected, how the
configuration carries it, and that the evaluation loop hands it to every inference call.  CPU only: the engine is the
stand-in of tests/fake_engine.py, extended here with the three view entry points."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from fake_engine import FakeDeepLab, FakeEngine  # noqa: E402

from eosvos_amd import _ffi, config, tta  # noqa: E402
from eosvos_amd.meta_optim import MetaOptimizer  # noqa: E402


class ViewEngine(FakeEngine):
    """The stand-in with `infer_view` / `tta_accumulate` / `resize_frames` restated in torch; every call is logged."""
    calls = []

    def infer(self, images):
        ViewEngine.calls.append(('infer', self.height, self.width, images.shape[0]))
        return super().infer(images)

    def infer_view(self, images, mirror=False):
        assert tuple(images.shape[2:]) == (self.height, self.width)
        ViewEngine.calls.append(('infer_view', self.height, self.width, bool(mirror), images.shape[0], float(self.theta[0]),
                                 float(self.theta[-1])))
        self._logits = self._net(torch.flip(images, [3]) if mirror else images)

    def tta_accumulate(self, acc, weight, mirror=False, first=False):
        u = torch.flip(self._logits, [3]) if mirror else self._logits
        p = weight * torch.sigmoid(F.interpolate(u, acc.shape[2:], mode='bilinear', align_corners=False))
        ViewEngine.calls.append(('tta_accumulate', self.height, self.width, bool(mirror), bool(first), weight))
        acc.copy_(p if first else acc + p)
        return acc

    def resize_frames(self, frames, height, width):
        ViewEngine.calls.append(('resize_frames', tuple(frames.shape[2:]), (height, width)))
        return F.interpolate(frames, (height, width), mode='bilinear', align_corners=False)


class ViewDeepLab(FakeDeepLab):
    def _ensure_engine(self, height, width, batch):
        e = self.engine
        if e is None or e.height != height or e.width != width or batch > e.max_batch:
            self.engine = ViewEngine(self.encoder, height, width, max(batch, self.max_batch))
            self._dirty = True
        return super()._ensure_engine(height, width, batch)

    def _build_view_engine(self, height, width, batch):
        return ViewEngine(self.encoder, height, width, batch)


# ---- the views of a dictionary ------------------------------------------------------------------------------------------
def test_view_enumeration_sizes_and_weights():
    v = tta.views({'flip': True, 'scales': [0.75, 1.0, 1.25]}, 96, 160)
    assert [(h, w, m) for h, w, m, _ in v] == [(72, 120, False), (72, 120, True), (96, 160, False), (96, 160, True),
                                                (120, 200, False), (120, 200, True)]
    assert all(wt == 1.0 / 6 for *_, wt in v) and abs(sum(wt for *_, wt in v) - 1.0) < 1e-12
    assert [(h, w) for h, w, _, _ in tta.views({'flip': False, 'scales': [0.75]}, 97, 163)] == [(73, 122)]      # round()
    assert tta.views({'flip': False, 'scales': [1.0]}, 480, 854) == [(480, 854, False, 1.0)]
    assert tta.views({'flip': True}, 480, 854) == [(480, 854, False, 0.5), (480, 854, True, 0.5)]               # scales default
    assert tta.views({'scales': [0.5, 2]}, 64, 64) == [(32, 32, False, 0.5), (128, 128, False, 0.5)]
    assert not tta.active(None) and not tta.active({'flip': False, 'scales': [1.0]}) and not tta.active({})
    assert tta.active({'flip': True, 'scales': [1.0]}) and tta.active({'flip': False, 'scales': [1.0, 1.0]})
    assert tta.active({'flip': False, 'scales': [0.75]})


@pytest.mark.parametrize('bad', [{'flip': True, 'scales': []}, {'flip': False, 'scales': [1.0, 0]}, {'scales': [-0.5]},
                                 {'scales': [float('nan')]}, {'scales': [float('inf')]}, {'scales': 1.0}, {'scales': ['1.0']},
                                 {'flip': 1, 'scales': [1.0]}, {'flip': True, 'scale': [1.0]}, [1.0], {'scales': [True]}])
def test_invalid_dictionaries_raise_value_error(bad):
    with pytest.raises(ValueError):
        tta.check(bad)
    with pytest.raises(ValueError):
        tta.active(bad)


def test_a_view_below_the_smallest_engine_frame_raises():
    assert tta.MIN_FRAME == 32
    tta.views({'scales': [0.5]}, 64, 64)
    with pytest.raises(ValueError, match='at least 32 x 32'):
        tta.views({'scales': [0.49]}, 64, 64)
    with pytest.raises(ValueError):
        tta.views({'flip': True, 'scales': [1.0, 0.25]}, 96, 160)
    model = ViewDeepLab('resnet50', num_classes=1, batch_norm=config.BASE['parent_model']['batch_norm'], max_batch=1)
    from eosvos_amd.helper_func import run_frames
    with pytest.raises(ValueError):
        run_frames(model, torch.rand(1, 3, 40, 48), tta={'scales': [0.75]})
    with pytest.raises(ValueError):
        run_frames(model, torch.rand(1, 3, 40, 48), tta={'scales': []})


# ---- configuration ------------------------------------------------------------------------------------------------------
def test_parse_cli_carries_eval_tta_only_when_asked():
    import copy
    base = copy.deepcopy(config.BASE)
    assert config.EXTENSIONS == {'eval_tta': {'flip': False, 'scales': [1.0]}}
    assert 'eval_tta' not in config.BASE and 'eval_tta' not in config.parse_cli([])
    assert 'eval_tta' not in config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS-OnA', 'num_epochs.eval=3'])
    cfg = config.parse_cli(['eval_tta.flip=True'])
    assert cfg['eval_tta'] == {'flip': True, 'scales': [1.0]}
    cfg = config.parse_cli(['with', 'DAVIS-2017', 'eval_tta.flip=True', 'eval_tta.scales=[0.75,1.0,1.25]'])
    assert cfg['eval_tta'] == {'flip': True, 'scales': [0.75, 1.0, 1.25]}
    assert config.parse_cli(['eval_tta.scales=[0.5, 1]'])['eval_tta'] == {'flip': False, 'scales': [0.5, 1]}
    assert config.BASE == base and config.EXTENSIONS == {'eval_tta': {'flip': False, 'scales': [1.0]}}       # nothing leaked
    with pytest.raises(KeyError):
        config.parse_cli(['eval_tta.rotate=True'])
    with pytest.raises(ValueError):
        config.parse_cli(['eval_tta.scales=[]'])
    with pytest.raises(ValueError):
        config.parse_cli(['eval_tta.scales=[1.0,-1]'])


# ---- the evaluation loop ------------------------------------------------------------------------------------------------
def _setup(max_batch=3):
    cfg = config.parse_cli([])
    cfg['num_epochs']['eval'] = 3
    cfg['eval_online_adapt'].update(step=3, reset_model_mode='FIRST_STEP', num_epochs=2, min_prop=0.5)
    cfg['data_cfg']['batch_sizes']['train'] = 3
    model = ViewDeepLab('resnet50', num_classes=1, batch_norm=cfg['parent_model']['batch_norm'], max_batch=max_batch)
    model._views['backbone.conv1.weight'].view(-1)[0] = 0.3
    mo = MetaOptimizer(model, **cfg['meta_optim_cfg'])
    g = torch.Generator().manual_seed(2)
    frames = torch.rand(8, 3, 40, 48, generator=g)
    gt = (torch.rand(1, 40, 48, generator=g) > 0.5).float()
    return cfg, model, mo, mo.state_dict(), frames, gt


def test_evaluate_sequence_hands_tta_to_every_inference_call_of_every_round():
    from eosvos_amd.evaluate import evaluate_sequence, online_adapt_schedule
    cfg, model, mo, msd, frames, gt = _setup()
    T = {'flip': True, 'scales': [1.0, 1.25]}
    ViewEngine.calls = []
    labels, probs, hist = evaluate_sequence(model, mo, msd, frames, [gt], cfg, tta=T)
    calls, ViewEngine.calls = ViewEngine.calls, []
    rounds = online_adapt_schedule(8, 0, 3, 3)
    assert len(rounds) == 3                                         # frames 1..3, 4..6, 7: three rounds, each with inference
    batches = [min(3, r['eval_max'] - f) for r in rounds for f in range(r['eval_min'], r['eval_max'], 3)]
    assert not [c for c in calls if c[0] == 'infer']                # no single-view call is left
    iv = [c for c in calls if c[0] == 'infer_view']
    want = [(h, w, m, b) for b in batches for (h, w, m) in ((40, 48, False), (40, 48, True), (50, 60, False), (50, 60, True))]
    assert [c[1:5] for c in iv] == want
    # every view ran on the weights of its round: three distinct fine-tuned states, the same for all four views of a call
    thetas = [c[5:] for c in iv]
    assert all(len(set(thetas[i:i + 4])) == 1 for i in range(0, len(thetas), 4))
    assert len(set(thetas)) == len(rounds) and (0.3, 0.0) not in thetas
    acc = [c for c in calls if c[0] == 'tta_accumulate']
    assert [c[4] for c in acc] == [True, False, False, False] * len(batches) and all(c[5] == 0.25 for c in acc)
    assert [c for c in calls if c[0] == 'resize_frames'] == [('resize_frames', (40, 48), (50, 60))] * len(batches)
    # the stand-in's network is pointwise: mirrored views change nothing, the 1.25 view only resamples -> close to one view
    plain = evaluate_sequence(model, mo, msd, frames, [gt], cfg)
    assert hist[0][0] == plain[2][0][0]                             # round 0 trains before any inference: the same
    assert probs[0].shape == plain[1][0].shape and float((probs[0][1:4] - plain[1][0][1:4]).abs().max()) < 0.1
    assert [c[0] for c in ViewEngine.calls if c[0] != 'infer'] == []            # tta=None: today's calls only
    ViewEngine.calls = []
    neutral = evaluate_sequence(model, mo, msd, frames, [gt], cfg, tta={'flip': False, 'scales': [1.0]})
    assert {c[0] for c in ViewEngine.calls} == {'infer'}
    assert torch.equal(neutral[1][0], plain[1][0]) and torch.equal(neutral[0], plain[0])
    model.close_parked_engines()
    assert model.__dict__['_view_engines'] == {}


def test_objects_in_flight_and_run_frames_pass_tta_through():
    from eosvos_amd.evaluate import finetune_object, object_workers, run_objects_in_flight
    from eosvos_amd.helper_func import run_frames
    cfg, model, mo, msd, frames, gt = _setup()
    T = {'flip': False, 'scales': [1.0, 0.8]}
    gts = [gt, 1.0 - gt]
    one = [finetune_object(model, mo, msd, frames, g, cfg, tta=T) for g in gts]
    workers = object_workers(model, mo, cfg['meta_optim_cfg'], 2)
    con = run_objects_in_flight(workers, msd, frames, gts, cfg, tta=T)
    for (p2, h2), (p1, h1) in zip(con, one):
        assert h2 == h1 and torch.equal(p2, p1)
    ViewEngine.calls = []
    losses, accs, probs = run_frames(model, frames[:2], gts[0].expand(2, 1, 40, 48), tta=T)
    assert [c[:4] for c in ViewEngine.calls if c[0] == 'infer_view'] == [('infer_view', 40, 48, False),
                                                                        ('infer_view', 32, 38, False)] * 2
    assert probs.shape == (2, 1, 40, 48) and losses.shape == (2,) and bool(torch.isfinite(losses).all())


# ---- the library --------------------------------------------------------------------------------------------------------
def test_abi_symbols_exist_in_the_built_library():
    lib = _ffi.load()
    for name in ('eosvos_infer_view', 'eosvos_tta_accumulate', 'eosvos_resize_frames'):
        assert name in _ffi.exported_symbols() and getattr(lib, name).argtypes is not None
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'eosvos.h')).read()
    for name in ('eosvos_infer_view(', 'eosvos_tta_accumulate(', 'eosvos_resize_frames('):
        assert name in header
    # null engines are refused on the host, before anything touches a device
    assert lib.eosvos_infer_view(None, None, 1, 0) == 1
    assert lib.eosvos_tta_accumulate(None, 1, 1, 1, 0, 1.0, 1, None, 1, 1) == 1
    assert lib.eosvos_resize_frames(None, None, 1, 3, 8, 8, 8, 8, None) == 1
    assert b'null' in lib.eosvos_last_error()
