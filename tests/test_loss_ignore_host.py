"""Host-side checks of the void label (`ignore`) of the losses (no GPU): the fp64 restatements the device kernels are held to
(tests/loss_ignore_ref.py) against the reference fixture and against hand-computed values, `compute_loss` passing the
keyword through, the `[lo, hi]` form of `eval_online_adapt.min_prop`, and the refusal of labels a target could take."""
import os
import re

import numpy as np
import pytest
import torch

import loss_ignore_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'lovasz_ignore.npz'))


@pytest.mark.parametrize('tag,per_image', [('per_image', True), ('flat', False)])
def test_restatement_reproduces_the_reference_fixture(fixture, tag, per_image):
    g = fixture
    x, t, ign = g['logits'], g['labels'], float(g['ignore'])
    assert (t[1] == ign).all() and not (t[2] == ign).any() and 0 < (t[0] == ign).sum() < t[0].size      # the case is what it says
    loss, grad = R.lovasz_hinge(x, t, ign, per_image)
    ref_loss, ref_grad = float(g[f'{tag}_loss']), g[f'{tag}_dlogits'].astype(np.float64)
    # the stored distances were measured against this very restatement; fp32 storage of the reference's values adds 2^-24
    assert abs(loss - ref_loss) <= float(g[f'{tag}_ref_vs_f64_loss']) + 1e-7 * abs(ref_loss)
    assert np.abs(grad - ref_grad).max() <= (float(g[f'{tag}_ref_vs_f64_grad']) + 1e-7) * np.abs(grad).max()
    assert not grad[t == ign].any() and not ref_grad[t == ign].any()


@pytest.mark.parametrize('kind', R.KINDS)
def test_void_pixels_are_the_pixels_left_out(kind):
    """Each masked formula on (x, t) equals the unmasked one on the valid pixels alone -- except class-balanced BCE, whose
    trailing divisions keep the full size (the OSVOS convention) -- and non-finite logits at void pixels change nothing."""
    rng = np.random.RandomState(3)
    n = 300
    x = (3 * rng.randn(n)).astype(np.float32)
    t = (rng.rand(n) < 0.4).astype(np.float32)
    void = rng.rand(n) < 0.3
    t[void] = 255
    loss, grad = R.one_set(kind, x, t, 255)
    sub_loss, sub_grad = R.one_set(kind, x[~void], t[~void])
    scale = (~void).sum() / n if kind == 'class_balanced_cross_entropy' else 1.0
    assert loss == pytest.approx(sub_loss * scale, rel=1e-12)
    np.testing.assert_allclose(grad[~void], sub_grad * scale, rtol=1e-12)
    assert not grad[void].any()
    xb = x.copy()
    xb[void] = np.where(rng.rand(int(void.sum())) < 0.5, np.nan, np.inf)
    loss_b, grad_b = R.one_set(kind, xb, t, 255)
    assert loss_b == loss and np.array_equal(grad_b, grad)
    assert R.one_set(kind, x, np.full(n, 255, np.float32), 255) == (0.0, pytest.approx(np.zeros(n)))      # empty V


def test_class_balanced_by_hand():
    # V = {0, 1, 2}: one positive, two negatives; n = 4.  L = (2 * bce(x0, 1) + 1 * (bce(x1, 0) + bce(x2, 0))) / (3 * 4)
    x = np.array([0.3, -1.0, 2.0, 5.0], dtype=np.float32)
    t = np.array([1, 0, 0, 255], dtype=np.float32)
    sp = lambda v: np.log1p(np.exp(np.float64(v)))                  # bce(x, 0) = softplus(x), bce(x, 1) = softplus(-x)
    want = (2 * sp(-np.float32(0.3)) + sp(np.float32(-1.0)) + sp(np.float32(2.0))) / 12
    assert R.class_balanced_bce(x, t, 255)[0] == pytest.approx(want, rel=1e-12)


def test_per_image_mean_counts_the_all_void_image(fixture):
    x, t = fixture['logits'], fixture['labels']
    per = [R.lovasz_flat(x[b], t[b], 255)[0] for b in range(3)]
    assert per[1] == 0.0 and R.lovasz_hinge(x, t, 255, True)[0] == pytest.approx(sum(per) / 3, rel=1e-15)


# ---- compute_loss and the online-adaptation band, on a stand-in engine ---------------------------------------------------
class StubEngine:
    """Records how the host code calls the engine; `infer` returns the probabilities it was given."""
    max_batch = 3

    def __init__(self, probs=None):
        self.probs, self.calls = probs, []

    def loss(self, kind, masks, ignore=None):
        self.calls.append(('loss', kind, masks.clone(), ignore))
        return torch.tensor([0.5 / len([c for c in self.calls if c[0] == 'loss'])])      # falls: no early stop surprises

    def loss_of(self, kind, logits, masks, ignore=None):
        self.calls.append(('loss_of', kind, masks.clone(), ignore))
        return torch.tensor([1.0])

    def propagation_targets(self, probs, lo, hi, ignore, counts=True):
        self.calls.append(('propagation_targets', lo, hi, ignore, probs.clone()))
        out = torch.where(probs >= hi, torch.ones_like(probs), torch.where(probs < lo, torch.zeros_like(probs),
                                                                        torch.full_like(probs, ignore)))
        return out, [int((f >= hi).sum()) for f in probs]

    def infer(self, frames):
        i = int(frames[0, 0, 0, 0])                                                   # frames carry their index
        return self.probs[i:i + frames.shape[0]].clone()

    def snapshot(self):
        pass

    def restore(self):
        pass


class StubModel:
    _dirty = False

    def __init__(self, engine):
        self.engine = engine

    def __call__(self, x):
        out = torch.zeros(x.shape[0], 1, *x.shape[2:])
        out._eosvos_engine = self.engine
        return [out]

    def train_without_dropout(self):
        pass

    def zero_grad(self):
        pass

    def eval(self):
        pass


class StubMetaOptim:
    class meta_model:
        @staticmethod
        def detach_param_groups():
            pass

    def load_state_dict(self, sd):
        pass

    def reset(self):
        pass

    def eval(self):
        pass

    def set_train_loss(self, loss):
        pass

    def step(self, loss):
        pass


def test_compute_loss_passes_ignore_through():
    from eosvos_amd.helper_func import compute_loss
    eng = StubEngine()
    logits = torch.zeros(2, 1, 4, 4)
    logits._eosvos_engine = eng
    gts = torch.zeros(2, 1, 4, 4)
    for kind in R.KINDS:
        eng.calls.clear()
        compute_loss(kind, logits, gts)
        compute_loss(kind, logits, gts, {'ignore': 255})
        compute_loss(kind, logits, gts, {'ignore': 255, 'batch_average': False})
        assert [(c[0], c[1], c[3]) for c in eng.calls] == [('loss', kind, None), ('loss', kind, 255)] + [('loss_of', kind, 255)] * 2
    eng.calls.clear()
    compute_loss('lovasz_hinge', logits, gts, {'ignore': -1.0, 'per_image': False})
    assert eng.calls[0][1] == 'lovasz_hinge_flat' and eng.calls[0][3] == -1.0


def run_online_adapt(min_prop, positives=True):
    from eosvos_amd import evaluate
    H, W, n = 4, 6, 7                                            # step 3, batch 3: round 1 propagates frames 3 and 2
    probs = torch.full((n, 1, H, W), 0.1)
    if positives:
        probs[2, 0, 0, :3] = torch.tensor([0.3, 0.7, 0.5])       # exact lo and hi: 0.3 is void (not < lo), 0.7 is positive
        probs[2, 0, 1, :] = 0.9
        probs[2, 0, 2, :] = 0.6
    probs[3] = 0.4                                               # no pixel >= 0.7 (band), none >= 0.5 either: skipped in both
    eng = StubEngine(probs)
    frames = torch.arange(n, dtype=torch.float32).view(n, 1, 1, 1).expand(n, 3, H, W).contiguous()
    gt = torch.zeros(1, H, W)
    gt[0, :2, :2] = 1
    cfg = {'eval_online_adapt': {'step': 3, 'reset_model_mode': 'FIRST_STEP', 'num_epochs': 2, 'min_prop': min_prop},
           'data_cfg': {'batch_sizes': {'train': 3}}, 'num_epochs': {'eval': 2}, 'loss_func': 'dice', 'seed': 1}
    masks, hist = evaluate.finetune_object(StubModel(eng), StubMetaOptim(), {}, frames, gt, cfg)
    return eng, masks, hist, probs


def test_scalar_min_prop_is_untouched():
    eng, masks, hist, probs = run_online_adapt(0.5)
    assert not [c for c in eng.calls if c[0] == 'propagation_targets']
    losses = [c for c in eng.calls if c[0] == 'loss']
    assert losses and all(c[3] is None for c in losses)
    for c in losses:
        assert set(np.unique(c[2].numpy())) <= {0.0, 1.0}        # hard targets, as before
    assert any(c[2].shape[0] > 1 for c in losses)                # a propagated frame did join a batch


def test_min_prop_band_builds_void_targets_once_per_round():
    from eosvos_amd import evaluate
    eng, masks, hist, probs = run_online_adapt([0.3, 0.7])
    prop = [c for c in eng.calls if c[0] == 'propagation_targets']
    assert len(prop) == len(hist) - 1                            # one call per adaptation round
    assert all(c[1:4] == (0.3, 0.7, evaluate.PROPAGATION_IGNORE) for c in prop)
    losses = [c for c in eng.calls if c[0] == 'loss']
    n0 = len(hist[0])
    assert all(c[3] is None for c in losses[:n0])                # round 0: the ground truth, never void
    assert all(c[3] == evaluate.PROPAGATION_IGNORE for c in losses[n0:])
    for c in losses[n0:]:
        m = c[2]
        assert set(np.unique(m[0].numpy())) <= {0.0, 1.0}        # the train frame's ground truth
        for f in m[1:]:
            assert (f == 1).any()                                # frames without a positive are skipped
    seen = torch.cat([c[2][1:].reshape(-1) for c in losses[n0:]])
    assert (seen == evaluate.PROPAGATION_IGNORE).any()
    # frame 2 joins round 1 (frame 3 has no positive): p = 0.3 -> void, 0.7 -> 1, 0.5 -> void, 0.1 -> 0
    assert prop[0][4].shape[0] == 2                              # both propagated frames went through the one call
    first = losses[n0][2]
    assert first.shape[0] == 2 and first[1, 0, 0, :4].tolist() == [255.0, 1.0, 255.0, 0.0]


def test_a_round_without_a_surviving_frame_takes_the_plain_loss():
    """No propagated frame has a positive pixel: the batch is the train frame alone, no target is void, no void label is passed."""
    eng, masks, hist, probs = run_online_adapt([0.3, 0.7], positives=False)
    assert len([c for c in eng.calls if c[0] == 'propagation_targets']) == len(hist) - 1
    losses = [c for c in eng.calls if c[0] == 'loss']
    assert len(losses) > len(hist[0]) and all(c[3] is None for c in losses)
    assert all(c[2].shape[0] == 1 for c in losses[len(hist[0]):])


@pytest.mark.parametrize('bad', [[0.7, 0.3], [0.5, 0.5], [0.5], [0.2, 0.5, 0.7], [-0.1, 0.5], [0.5, 1.5], ['a', 0.5], [True, 0.5]])
def test_malformed_band_raises_at_the_top(bad):
    from eosvos_amd import evaluate
    with pytest.raises(ValueError):
        evaluate.min_prop_band(bad)
    eng = StubEngine(torch.zeros(5, 1, 4, 6))
    cfg = {'eval_online_adapt': {'step': 2, 'reset_model_mode': 'FIRST_STEP', 'num_epochs': 2, 'min_prop': bad},
           'data_cfg': {'batch_sizes': {'train': 3}}, 'num_epochs': {'eval': 2}}
    gen = evaluate.finetune_object_steps(StubModel(eng), StubMetaOptim(), {}, torch.zeros(5, 3, 4, 6), torch.zeros(1, 4, 6), cfg)
    with pytest.raises(ValueError):
        next(gen)
    assert not eng.calls                                         # before any engine work


def test_min_prop_band_accepts_what_the_issue_allows():
    from eosvos_amd import evaluate
    assert evaluate.min_prop_band(0.5) is None and evaluate.min_prop_band(1) is None
    assert evaluate.min_prop_band([0.3, 0.7]) == (0.3, 0.7) and evaluate.min_prop_band((0, 1)) == (0.0, 1.0)


@pytest.mark.parametrize('bad', [0.5, 0.0, 1.0, float('nan'), float('inf'), float('-inf')])
def test_bad_ignore_values_raise(bad):
    from eosvos_amd.engine import check_ignore
    with pytest.raises(ValueError):
        check_ignore(bad)
    assert check_ignore(255) == 255.0 and check_ignore(-1) == -1.0


def test_entries_are_declared_at_every_layer():
    header = open(os.path.join(ROOT, 'include', 'eosvos.h')).read()
    from eosvos_amd import _ffi
    for name in ('eosvos_loss_ignore', 'eosvos_loss_tensors_ignore', 'eosvos_set_loss_ignore', 'eosvos_propagation_targets'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert name in _ffi.exported_symbols()
    assert 'loss_lovasz.py:78-126' in header
