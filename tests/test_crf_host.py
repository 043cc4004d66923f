"""Host side of the local dense-CRF refinement (`eosvos_amd/crf.py`): the torch twin `refine_host` against the per-pixel loop
restatement of tests/crf_ref.py, what the parameter dictionary accepts, how the configuration carries it, and that the
evaluation's merge hands it through.  CPU only: the engine is the stand-in of tests/fake_engine.py, which has no
`crf_labels` and so takes `refine_host`."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import crf_ref  # noqa: E402
from fake_engine import FakeDeepLab, FakeEngine  # noqa: E402

from eosvos_amd import _ffi, config, crf  # noqa: E402
from eosvos_amd.meta_optim import MetaOptimizer  # noqa: E402
from oracle import meta as oracle_meta  # noqa: E402


def P(**kw):
    return dict(crf.DEFAULTS, **kw)


# ---- the torch twin against the loops -----------------------------------------------------------------------------------
# 9 x 11: the reach r * d = 10 / 2 / 6 goes outside the frame everywhere / near the border; 2 x 2 with d = 2: no neighbour at all
@pytest.mark.parametrize('h,w,n_obj,r,d,T', [(9, 11, 2, 5, 2, 5), (9, 11, 3, 2, 1, 2), (9, 11, 1, 2, 3, 1), (2, 2, 1, 2, 2, 3),
                                             (2, 2, 2, 1, 1, 2)])
def test_refine_host_equals_the_per_pixel_loops(h, w, n_obj, r, d, T):
    images, probs = crf_ref.scene(h, w, n_obj, seed=3 + h + n_obj)
    probs[0, 0, 0, 0], probs[0, -1, -1, -1] = 2.0, -0.25            # outside [0, 1]: clamped
    params = P(iterations=T, radius=r, dilation=d)
    labels, q = crf.refine_host(images, probs, params)
    want_labels, want_q = crf_ref.refine_loops(images[0].numpy(), probs[0].numpy(), params)
    assert q.dtype == torch.float64 and q.shape == (1, n_obj + 1, h, w) and labels.dtype == torch.uint8
    # both sides are fp64 and differ in the order of at most 120 additions of positive terms and in the softmax's form
    assert float(np.abs(q[0].numpy() - want_q).max()) <= 1e-13
    np.testing.assert_array_equal(labels[0].numpy(), want_labels)
    np.testing.assert_allclose(q.sum(dim=1).numpy(), 1.0, atol=1e-14)
    if (h, w, d) == (2, 2, 2):                                       # no neighbour: Q^T = Q^0
        assert float((q - crf.refine_host(images, probs, P(iterations=0))[1]).abs().max()) <= 1e-15


def test_refinement_changes_the_labels_and_follows_the_image():
    images, probs = crf_ref.scene(48, 64, 2, seed=11)
    plain = torch.stack([oracle_meta.merge_labels(probs[0])])
    refined, _ = crf.refine_host(images, probs, P(radius=3, dilation=2))
    assert float((refined != plain).float().mean()) > 0.01
    yy, xx = torch.meshgrid(torch.arange(48.0), torch.arange(64.0), indexing='ij')
    truth = torch.zeros(48, 64, dtype=torch.uint8)
    for o in range(2):
        truth[torch.sqrt((yy - (0.3 + 0.4 * o) * 48) ** 2 + (xx - (0.3 + 0.4 * o) * 64) ** 2) < 0.22 * 48] = o + 1
    assert float((refined[0] == truth).float().mean()) > float((plain[0] == truth).float().mean())


def test_zero_iterations_is_merge_labels():
    g = torch.Generator().manual_seed(5)
    for n_obj in (1, 3):
        probs = torch.rand(2, n_obj, 13, 17, generator=g)
        probs[0, :, 0, :4] = 0.5                                     # the threshold itself, tied between the objects
        probs[0, 0, 1, :4] = 0.5
        probs[0, :, 2, :4] = 2.0                                     # the seeded train frame, tied
        probs[0, -1, 3, :4] = 2.0
        probs[1, :, 4, :] = probs[1, 0, 4, :].clone()                      # exact ties between objects, both sides of 0.5
        probs[1, :, 5, :4] = 0.49999997
        images = torch.rand(2, 3, 13, 17, generator=g)
        labels, q = crf.refine_host(images, probs, P(iterations=0))
        want = torch.stack([oracle_meta.merge_labels(probs[f]) for f in range(2)])
        assert torch.equal(labels, want)
        assert q.shape == (2, n_obj + 1, 13, 17)
        labels32, _ = crf.refine_host(images, probs, P(iterations=0), dtype=torch.float32)
        assert torch.equal(labels32, want)
        for f in range(2):
            np.testing.assert_array_equal(crf_ref.refine_loops(images[f], probs[f], P(iterations=0))[0], want[f].numpy())


# ---- the parameter dictionary -------------------------------------------------------------------------------------------
def test_check_and_active():
    assert crf.DEFAULTS == {'iterations': 5, 'radius': 5, 'dilation': 2, 'w_appearance': 10.0, 'w_smooth': 3.0,
                            'theta_alpha': 8.0, 'theta_beta': 0.05, 'theta_gamma': 3.0}
    assert crf.check({}) == crf.DEFAULTS and crf.check(crf.DEFAULTS) == crf.DEFAULTS
    assert crf.check({'iterations': 2, 'w_smooth': 0})['w_smooth'] == 0.0
    assert crf.check({'radius': 4, 'dilation': 4})['radius'] == 4 and crf.check({'radius': 7, 'dilation': 2})
    assert not crf.active(None) and not crf.active({'iterations': 0}) and not crf.active(P(iterations=0))
    assert crf.active({}) and crf.active(crf.DEFAULTS) and crf.active({'iterations': 1})
    assert crf.frames_per_call(3, 480, 854) == (512 << 20) // (3 * 4 * 480 * 854 * 4) and crf.frames_per_call(255, 2000, 2000) == 1


@pytest.mark.parametrize('bad', [{'iterations': -1}, {'iterations': 21}, {'iterations': 2.0}, {'iterations': True},
                                 {'radius': 0}, {'radius': 8}, {'dilation': 0}, {'dilation': 5}, {'radius': 6, 'dilation': 3},
                                 {'w_appearance': -1.0}, {'w_smooth': float('nan')}, {'w_smooth': float('inf')},
                                 {'theta_alpha': 0}, {'theta_beta': -0.05}, {'theta_gamma': float('inf')},
                                 {'theta_beta': float('nan')}, {'theta_beta': '0.05'}, {'iters': 5}, [5], 5])
def test_invalid_dictionaries_raise_value_error(bad):
    with pytest.raises(ValueError):
        crf.check(bad)
    with pytest.raises(ValueError):
        crf.active(bad)


def test_refine_host_rejects_bad_tensors():
    img, pr = torch.rand(2, 3, 8, 8), torch.rand(2, 2, 8, 8)
    for a, b in ((img[:1], pr), (img[:, :2], pr), (img, pr[:, :, :7]), (img[0], pr[0]), (img, torch.rand(2, 0, 8, 8)),
                 (img, torch.rand(2, 256, 8, 8))):
        with pytest.raises(ValueError):
            crf.refine_host(a, b, crf.DEFAULTS)


# ---- configuration ------------------------------------------------------------------------------------------------------
def test_parse_cli_carries_eval_crf_only_when_asked():
    base, ext = copy.deepcopy(config.BASE), copy.deepcopy(config.EXTENSIONS)
    neutral = dict(crf.DEFAULTS, iterations=0)
    assert config.POSTPROCESS == {'eval_crf': neutral} and not crf.active(config.POSTPROCESS['eval_crf'])
    assert 'eval_crf' not in config.BASE and 'eval_crf' not in config.EXTENSIONS and 'eval_crf' not in config.parse_cli([])
    assert 'eval_crf' not in config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS-OnA', 'num_epochs.eval=3', 'eval_tta.flip=True'])
    cfg = config.parse_cli(['eval_crf.iterations=5'])
    assert cfg['eval_crf'] == crf.DEFAULTS and 'eval_tta' not in cfg
    cfg = config.parse_cli(['with', 'DAVIS-2017', 'eval_crf.iterations=3', 'eval_crf.w_appearance=4', 'eval_crf.theta_beta=0.1'])
    assert cfg['eval_crf'] == dict(crf.DEFAULTS, iterations=3, w_appearance=4, theta_beta=0.1)
    assert config.parse_cli(['eval_crf.radius=3'])['eval_crf'] == dict(neutral, radius=3)      # still off: 0 iterations
    assert config.BASE == base and config.EXTENSIONS == ext and config.POSTPROCESS == {'eval_crf': neutral}   # nothing leaked
    with pytest.raises(KeyError):
        config.parse_cli(['eval_crf.sigma=3'])
    for bad in ('eval_crf.iterations=21', 'eval_crf.radius=0', 'eval_crf.w_smooth=-1', 'eval_crf.theta_beta=0'):
        with pytest.raises(ValueError):
            config.parse_cli([bad])
    with pytest.raises(ValueError):
        config.parse_cli(['eval_crf.radius=7', 'eval_crf.dilation=3'])


# ---- the evaluation loop ------------------------------------------------------------------------------------------------
class LogEngine(FakeEngine):
    """The stand-in, logging its merges; its probabilities follow the frame's brightness under a deterministic pseudo-noise, so
    that a merge has something to refine."""
    merges = []

    def infer(self, images):
        return torch.sigmoid(8.0 * (images.float().mean(dim=1, keepdim=True) - 0.4) + 2.0 * torch.sin(1000.0 * images[:, 1:2].float()))

    def merge_labels(self, probs):
        LogEngine.merges.append(probs.clone())
        return super().merge_labels(probs)


class LogDeepLab(FakeDeepLab):
    def _ensure_engine(self, height, width, batch):
        e = self.engine
        if e is None or e.height != height or e.width != width or batch > e.max_batch:
            self.engine = LogEngine(self.encoder, height, width, max(batch, self.max_batch))
            self._dirty = True
        return super()._ensure_engine(height, width, batch)


def test_merge_objects_off_is_today_and_on_keeps_the_listed_frames():
    from eosvos_amd.evaluate import merge_objects
    images, probs = crf_ref.scene(24, 32, 2, seed=4, n_frames=5)
    probs[2] = 2.0 * (probs[2] > 0.5)                                # a seeded train frame
    eng = LogEngine('resnet50', 24, 32, 1)
    per_object = [probs[:, o] for o in range(2)]
    today = torch.stack([oracle_meta.merge_labels(probs[f]) for f in range(5)])
    LogEngine.merges = []
    for kw in ({}, {'crf': None}, {'frames': images, 'crf': P(iterations=0), 'keep': (2,)}, {'frames': images}):
        out = merge_objects(eng, per_object, **kw)
        assert out.dtype == torch.uint8 and torch.equal(out, today)
    assert len(LogEngine.merges) == 4 * 5                            # off: one merge_labels call per frame, as before
    LogEngine.merges = []
    params = P(radius=3, dilation=1, iterations=2)
    on = merge_objects(eng, per_object, images, params, keep=(2,))
    want, _ = crf.refine_host(images, probs, params, dtype=torch.float32)
    assert len(LogEngine.merges) == 1 and torch.equal(LogEngine.merges[0], probs[2])
    assert torch.equal(on[2], today[2])
    for f in (0, 1, 3, 4):
        assert torch.equal(on[f], want[f]) and not torch.equal(on[f], today[f])
    assert torch.equal(merge_objects(eng, per_object, images, params)[2], want[2])             # nothing kept
    with pytest.raises(ValueError):
        merge_objects(eng, per_object, None, params)
    with pytest.raises(ValueError):
        merge_objects(eng, per_object, images, {'iterations': 99})

    class DeviceEngine(LogEngine):                                   # an engine WITH the entry point is called, in chunks
        calls = []

        def crf_labels(self, images, probs, return_q=False, **params):
            DeviceEngine.calls.append((images.shape[0], params))
            return crf.refine_host(images, probs, params, dtype=torch.float32)[0]
    dev = DeviceEngine('resnet50', 24, 32, 1)
    assert torch.equal(merge_objects(dev, per_object, images, params, keep=(2,)), on)
    assert DeviceEngine.calls == [(4, params)]


def test_evaluate_sequence_passes_crf_through():
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
    for kw in ({'crf': None}, {'crf': P(iterations=0)}):
        off = evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1, **kw)
        assert torch.equal(off[0], plain[0]) and off[2] == plain[2] and all(torch.equal(a, b) for a, b in zip(off[1], plain[1]))
    params = P(radius=2, dilation=2, iterations=3)
    on = evaluate_sequence(model, mo, msd, images, gts, cfg, train_frame_id=1, crf=params)
    assert all(torch.equal(a, b) for a, b in zip(on[1], plain[1])) and on[2] == plain[2]       # the fine-tunes do not see it
    want, _ = crf.refine_host(images, torch.stack(on[1], dim=1), params, dtype=torch.float32)
    assert torch.equal(on[0][1], plain[0][1])                        # the train frame: the seeded ground truth
    for f in (0, 2, 3):
        assert torch.equal(on[0][f], want[f])
    assert not torch.equal(on[0], plain[0])


def test_evaluate_dataset_refines_labels_pngs_and_j(tmp_path):
    from eosvos_amd import data
    from eosvos_amd.evaluate import evaluate_dataset
    cfg = config.parse_cli(['eval_crf.iterations=2', 'eval_crf.radius=2'])
    cfg['num_epochs']['eval'] = 2
    model = LogDeepLab('resnet50', num_classes=1, batch_norm=cfg['parent_model']['batch_norm'], max_batch=2)
    mo = MetaOptimizer(model, **cfg['meta_optim_cfg'])
    ds = data.SyntheticSequences(1, 4, 24, 40, seed=3)
    seq = ds.seqs_names[0]
    plain = evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1)
    off = evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1, crf=P(iterations=0))
    assert torch.equal(off['labels'][seq], plain['labels'][seq]) and off['J_seq'] == plain['J_seq']
    captured = []
    import eosvos_amd.evaluate as ev
    real = ev.merge_objects

    def spy(engine, probs_all, *a, **k):
        captured.append((probs_all, a, k))
        return real(engine, probs_all, *a, **k)
    ev.merge_objects = spy
    try:
        on = evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1, save_dir=str(tmp_path),
                              crf=cfg['eval_crf'])
    finally:
        ev.merge_objects = real
    (probs_all, a, k), = captured
    assert k['crf'] == cfg['eval_crf'] and k['keep'] == (0,) and k['frames'].shape == (4, 3, 24, 40)
    frames = ds.sequence_tensors(seq, 'cpu')[0]
    want, _ = crf.refine_host(frames, torch.stack(list(probs_all), dim=1), cfg['eval_crf'], dtype=torch.float32)
    labels = on['labels'][seq]
    assert torch.equal(labels[0], plain['labels'][seq][0]) and torch.equal(labels[1:], want[1:])
    assert not torch.equal(labels, plain['labels'][seq])
    assert on['J_seq'] == [data.sequence_J(labels.numpy(), ds.label_maps(seq), len(probs_all))]       # J sees the refined maps
    from PIL import Image
    from eosvos_amd.evaluate import prediction_paths
    preds, _ = prediction_paths(str(tmp_path), cfg['datasets']['val']['name'], cfg['datasets']['val']['split'])
    png = np.asarray(Image.open(os.path.join(preds, seq, ds.frame_names(seq)[2] + '.png')))
    np.testing.assert_array_equal(png, labels[2].numpy())


def test_abi_symbol_exists_and_refuses_a_null_engine():
    lib = _ffi.load()
    assert 'eosvos_crf_labels' in _ffi.exported_symbols() and len(lib.eosvos_crf_labels.argtypes) == 17
    assert 'eosvos_crf_labels(' in open(os.path.join(os.path.dirname(HERE), 'include', 'eosvos.h')).read()
    assert lib.eosvos_crf_labels(None, None, None, 1, 1, 8, 8, 5, 5, 2, 10.0, 3.0, 8.0, 0.05, 3.0, None, None) == 1
    assert b'null' in lib.eosvos_last_error()
