"""DAVIS-2017 J and F measures (`data.boundary_counts_host`, `data.sequence_measures`, `evaluate_dataset`'s J / F keys).

The counts are checked against an independent restatement of the `davis` package's F measure written here with
scipy.ndimage (meshgrid disk, border 0); the statistics against hand-computed values.  CPU only: the engine of the
`evaluate_dataset` test is the stand-in of tests/fake_engine.py, which has no `davis_counts` (host counts).
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fake_engine import FakeDeepLab  # noqa: E402

from eosvos_amd import config as config_mod  # noqa: E402
from eosvos_amd import data  # noqa: E402
from eosvos_amd import evaluate as product_eval  # noqa: E402
from eosvos_amd.meta_optim import MetaOptimizer  # noqa: E402


def _bmap_ref(s):
    """seg2bmap, written out pixel by pixel."""
    h, w = s.shape
    b = np.zeros((h, w), dtype=bool)
    at = lambda y, x: bool(s[y, x]) if y < h and x < w else False
    for y in range(h):
        for x in range(w):
            v, e, d, se = at(y, x), at(y, x + 1), at(y + 1, x), at(y + 1, x + 1)
            if y == h - 1 and x == w - 1:
                b[y, x] = False
            elif y == h - 1:
                b[y, x] = v != e
            elif x == w - 1:
                b[y, x] = v != d
            else:
                b[y, x] = (v != e) or (v != d) or (v != se)
    return b


def _counts_ref(pred, gt, n_obj, bound_th=0.008):
    n, h, w = pred.shape
    r = bound_th if bound_th >= 1 else int(math.ceil(bound_th * math.sqrt(h * h + w * w)))
    yy, xx = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing='ij')
    disk = yy ** 2 + xx ** 2 <= r ** 2
    dil = lambda b: ndimage.binary_dilation(b, structure=disk, border_value=0) if b.any() else b
    out = np.zeros((n, n_obj, 6), dtype=np.int64)
    for f in range(n):
        for o in range(1, n_obj + 1):
            p, g = pred[f] == o, gt[f] == o
            bp, bg = _bmap_ref(p), _bmap_ref(g)
            out[f, o - 1] = [(p & g).sum(), (p | g).sum(), bp.sum(), bg.sum(), (bp & dil(bg)).sum(), (bg & dil(bp)).sum()]
    return out


def _blobs(rng, n, h, w, n_obj, n_blobs=3):
    lab = np.zeros((n, h, w), dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w]
    for f in range(n):
        for _ in range(n_blobs * n_obj):
            o = int(rng.integers(1, n_obj + 1))
            cy, cx = rng.uniform(0, h), rng.uniform(0, w)
            ry, rx = rng.uniform(1, max(2, h / 3)), rng.uniform(1, max(2, w / 3))
            lab[f][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = o
    return lab


CASES = {
    'blobs': lambda rng: (_blobs(rng, 3, 37, 53, 3), _blobs(rng, 3, 37, 53, 3), 3, 0.008),
    'blobs_r5': lambda rng: (_blobs(rng, 2, 40, 70, 2), _blobs(rng, 2, 40, 70, 2), 2, 5),
    'noise': lambda rng: (rng.integers(0, 4, (2, 23, 31)).astype(np.uint8), rng.integers(0, 4, (2, 23, 31)).astype(np.uint8), 3, 3),
    'h1': lambda rng: (rng.integers(0, 3, (3, 1, 40)).astype(np.uint8), rng.integers(0, 3, (3, 1, 40)).astype(np.uint8), 2, 2),
    'w1': lambda rng: (rng.integers(0, 3, (3, 40, 1)).astype(np.uint8), rng.integers(0, 3, (3, 40, 1)).astype(np.uint8), 2, 2),
    'h1w1': lambda rng: (np.array([[[1]], [[0]], [[1]]], np.uint8), np.array([[[1]], [[1]], [[0]]], np.uint8), 1, 1),
    'labels_above_n_obj': lambda rng: (rng.integers(0, 7, (2, 20, 30)).astype(np.uint8), rng.integers(0, 7, (2, 20, 30)).astype(np.uint8), 3, 2),
    'radius_above_height': lambda rng: (_blobs(rng, 2, 6, 50, 2), _blobs(rng, 2, 6, 50, 2), 2, 9),
    'radius_63': lambda rng: (_blobs(rng, 1, 40, 65, 2), _blobs(rng, 1, 40, 65, 2), 2, 63),
    'r0': lambda rng: (_blobs(rng, 2, 20, 30, 2), _blobs(rng, 2, 20, 30, 2), 2, 0.0),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_boundary_counts_host_matches_scipy_restatement(case):
    pred, gt, n_obj, th = CASES[case](np.random.default_rng(sorted(CASES).index(case)))
    got = data.boundary_counts_host(pred, gt, n_obj, th)
    assert got.dtype == np.int64 and got.shape == (pred.shape[0], n_obj, 6)
    np.testing.assert_array_equal(got, _counts_ref(pred, gt, n_obj, th))


def _edge_frames():
    """Objects touching the last row / column, 1-pixel objects, empty pred or GT or both."""
    h, w = 16, 21
    pred = np.zeros((5, h, w), np.uint8)
    gt = np.zeros((5, h, w), np.uint8)
    pred[0, 10:, 15:] = 1; gt[0, 9:, 14:] = 1                 # object 1 in the bottom-right corner
    pred[0, 3, 4] = 2; gt[0, 3, 6] = 2                         # 1-pixel objects, 2 px apart
    pred[1, -1, :] = 1; gt[1, :, -1] = 1                        # last row vs last column
    pred[1, 0, -1] = 2; gt[1, -1, 0] = 2                        # 1-pixel objects at the far corners
    gt[2, 4:9, 4:9] = 1                                         # empty pred, non-empty GT
    pred[3, 4:9, 4:9] = 2                                       # non-empty pred, empty GT
    pred[4, 5, 5] = 3; gt[4, 5, 5] = 3                          # frame 4: objects 1 and 2 empty in both
    return pred, gt


def test_boundary_counts_host_edge_cases():
    pred, gt = _edge_frames()
    got = data.boundary_counts_host(pred, gt, 3, 2)
    np.testing.assert_array_equal(got, _counts_ref(pred, gt, 3, 2))
    assert got[2, 0, 2] == 0 and got[2, 0, 3] > 0              # n_fg = 0, n_gt > 0
    assert got[3, 1, 2] > 0 and got[3, 1, 3] == 0              # n_fg > 0, n_gt = 0
    assert (got[4, :2] == 0).all()                               # both empty
    assert tuple(got[4, 2]) == (1, 1, 4, 4, 4, 4)               # a lone pixel: itself and its left / upper neighbours


def test_f_special_cases_and_j_definition():
    c = np.zeros((1, 4, 6), np.int64)
    c[0, 0] = (0, 25, 0, 16, 0, 0)      # empty pred: P, R = 1, 0 -> F 0
    c[0, 1] = (0, 25, 16, 0, 0, 0)      # empty GT: P, R = 0, 1 -> F 0
    c[0, 2] = (0, 0, 0, 0, 0, 0)        # both empty: F 1, J 1
    c[0, 3] = (3, 4, 10, 20, 5, 8)      # P = 0.5, R = 0.4
    m = data.measures_from_counts(c)
    assert m['F']['mean'] == [0.0, 0.0, 1.0, 2 * 0.5 * 0.4 / 0.9]
    assert m['J']['mean'] == [0.0, 0.0, 1.0, 0.75]
    c[0, 3] = (1, 4, 10, 20, 0, 0)      # P + R = 0 -> F 0
    assert data.measures_from_counts(c)['F']['mean'][3] == 0.0


def _stats_by_hand(x):
    x = [float(v) for v in x]
    n = len(x)
    # round(linspace(1, n, 5) + 1e-10) - 1: the 1e-10 rounds the halves (1.5, 2.5, 3.5) up
    bounds = {1: [0, 0, 0, 0, 0], 2: [0, 0, 1, 1, 1], 3: [0, 1, 1, 2, 2], 4: [0, 1, 2, 2, 3], 5: [0, 1, 2, 3, 4],
              6: [0, 1, 3, 4, 5]}[n]
    b0, b3 = x[bounds[0]:bounds[1] + 1], x[bounds[3]:bounds[4] + 1]
    return sum(x) / n, sum(v > 0.5 for v in x) / n, sum(b0) / len(b0) - sum(b3) / len(b3)


@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 6])
def test_statistics_by_hand(n):
    x = [0.9, 0.2, 0.75, 0.5, 0.6, 0.1][:n]
    mean, recall, decay = data.davis_statistics(x)
    em, er, ed = _stats_by_hand(x)
    assert mean == pytest.approx(em, abs=1e-15) and recall == er and decay == pytest.approx(ed, abs=1e-15)


def test_statistics_uint8_wrap_n300():
    """n = 300: ids = round(linspace(1, 300, 5) + 1e-10) - 1 = 0, 75, 150, 224, 299, cast to uint8 -> 299 wraps to 43.
    Bin 0 = X[0:76]; bin 3 = X[224:44] is empty, so the published code's decay is NaN."""
    x = np.linspace(0.0, 1.0, 300)
    mean, recall, decay = data.davis_statistics(x)
    assert mean == float(np.mean(x)) and recall == float(np.mean(x > 0.5))
    assert math.isnan(decay)
    # n = 259: ids 0, 64, 129, 193, 258 -> 258 wraps to 2, bin 3 = X[193:3] empty as well; n = 256: ids ... 255, and the
    # bin end 255 + 1 wraps to 0 in uint8 arithmetic
    assert math.isnan(data.davis_statistics(np.ones(259))[2])
    assert math.isnan(data.davis_statistics(np.ones(256))[2])
    # n = 200 (no wrap): bins X[0:51] and X[149:200]
    y = np.arange(200) / 200.0
    assert data.davis_statistics(y)[2] == float(np.mean(y[0:51])) - float(np.mean(y[149:200]))
    assert data.davis_statistics([])[0] != data.davis_statistics([])[0]          # NaN, as np.mean of nothing


def test_sequence_measures_j_equals_sequence_j():
    rng = np.random.default_rng(5)
    pred, gt = _blobs(rng, 7, 30, 44, 3), _blobs(rng, 7, 30, 44, 3)
    pred[3] = 0                                                   # a frame with nothing predicted
    m = data.sequence_measures(pred, gt, 3)
    assert set(m) == {'J', 'F'} and all(len(m[k][s]) == 3 for k in 'JF' for s in ('mean', 'recall', 'decay'))
    for o in range(1, 4):
        assert m['J']['mean'][o - 1] == data.sequence_J((pred == o).astype(np.uint8), (gt == o).astype(np.uint8), 1)
    assert float(np.mean(m['J']['mean'])) == data.sequence_J(pred, gt, 3)
    counts = data.boundary_counts_host(pred, gt, 3)[1:6]
    assert m == data.measures_from_counts(counts)


def test_bound_pix():
    assert data.davis_bound_pix(0.008, 480, 854) == 8
    assert data.davis_bound_pix(0.008, 720, 1280) == 12
    assert data.davis_bound_pix(5, 480, 854) == 5
    with pytest.raises(ValueError):
        data.davis_bound_pix(1.5, 480, 854)


# evaluate_dataset on SyntheticSequences (2 objects, 6 frames, 24 x 40) with the stand-in engine; J_seq / mean_J as the
# parent commit returned them for this configuration
J_SEQ_AT_PARENT = [0.040625, 0.040625]


def _evaluate(tmp_path, test_mode=False):
    cfg = config_mod.parse_cli([])
    cfg['num_epochs']['eval'] = 2
    cfg['eval_online_adapt'].update(step=3, reset_model_mode='FIRST_STEP', num_epochs=1, min_prop=0.5)
    cfg['data_cfg']['batch_sizes']['train'] = 2
    torch.manual_seed(0)
    model = FakeDeepLab('resnet50', num_classes=1, batch_norm=cfg['parent_model']['batch_norm'], max_batch=2)
    model._views['backbone.conv1.weight'].view(-1)[0] = 0.3
    mo = MetaOptimizer(model, **cfg['meta_optim_cfg'])
    ds = data.SyntheticSequences(2, 6, 24, 40, seed=3)
    if test_mode:
        ds.test_mode = True
    res = product_eval.evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1)
    return res, ds


def test_evaluate_dataset_reports_j_and_f(tmp_path):
    res, ds = _evaluate(tmp_path)
    keys = ('J_obj', 'J_recall_seq', 'J_decay_seq', 'F_seq', 'F_recall_seq', 'F_decay_seq')
    assert all(len(res[k]) == 4 for k in keys)                  # 2 sequences x 2 objects
    j_expected = [data.sequence_J(res['labels'][s].numpy(), ds.label_maps(s), 2) for s in ds.seqs_names]
    assert res['J_seq'] == j_expected and res['mean_J'] == float(np.mean(j_expected))
    assert res['J_seq'] == J_SEQ_AT_PARENT
    ref = {k: [] for k in keys}
    for s in ds.seqs_names:
        m = data.sequence_measures(res['labels'][s].numpy(), ds.label_maps(s), 2)
        for k, (mm, st) in zip(keys, [(a, b) for a in 'JF' for b in ('mean', 'recall', 'decay')]):
            ref[k].extend(m[mm][st])
    for k in keys:
        assert res[k] == ref[k], k
    assert res['mean_F'] == float(np.mean(ref['F_seq']))
    assert res['mean_JF'] == (float(np.mean(ref['J_obj'])) + res['mean_F']) / 2


def test_evaluate_dataset_test_mode_reports_zeros(tmp_path):
    res, ds = _evaluate(tmp_path, test_mode=True)
    for k in ('J_obj', 'J_recall_seq', 'J_decay_seq', 'F_seq', 'F_recall_seq', 'F_decay_seq'):
        assert res[k] == [0.0, 0.0]                              # one zero per sequence, evaluate.py:345-347
    assert res['mean_F'] == 0.0 and res['mean_JF'] == 0.0 and res['J_seq'] == [0.0, 0.0]
