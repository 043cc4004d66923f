"""DAVIS J / F counts on the MI355X (`eosvos_davis_counts`, `Engine.davis_counts`) against the host twin
`data.boundary_counts_host`, count for count, and `evaluate_dataset`'s J / F statistics against the host path."""
import ctypes

import numpy as np
import pytest
import torch

from eosvos_amd import _ffi, data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from eosvos_amd.engine import Engine
    e = Engine('resnet50', 64, 96, max_batch=1, device='cuda:0')
    yield e
    e.close()


def _blobs(rng, n, h, w, n_obj, n_blobs=3, max_label=None):
    """Elliptic blobs of ids 1..n_obj (or up to max_label: ids above n_obj belong to no object), plus speckle."""
    top = max_label or n_obj
    lab = np.zeros((n, h, w), dtype=np.uint8)
    yy, xx = np.ogrid[:h, :w]
    for f in range(n):
        for _ in range(n_blobs * top):
            o = int(rng.integers(1, top + 1))
            cy, cx = rng.uniform(-5, h + 5), rng.uniform(-5, w + 5)
            ry, rx = rng.uniform(0.5, max(2, h / 4)), rng.uniform(0.5, max(2, w / 4))
            lab[f][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = o
        speck = rng.random((h, w)) < 0.002
        lab[f][speck] = rng.integers(0, top + 1, int(speck.sum()))
    return lab


def _device_counts(eng, pred, gt, n_obj, bound_th=0.008):
    """The C entry point with the host output pre-filled with garbage (every count must be written)."""
    n, h, w = pred.shape
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    out = np.full((n, n_obj, 6), 0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    _ffi.check(eng.lib.eosvos_davis_counts(eng.h, ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(g.data_ptr()), n, h, w, n_obj,
                                           data.davis_bound_pix(bound_th, h, w),
                                           out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    return out


SIZES = [  # (frames, H, W, n_obj, bound_th, max_label)
    (3, 480, 854, 3, 0.008, None),        # r = 8
    (2, 720, 1280, 2, 0.008, None),       # r = 12
    (3, 97, 161, 4, 0.008, 6),            # r = 2, labels above n_obj
    (2, 40, 63, 2, 3, None),
    (2, 40, 64, 2, 3, None),
    (2, 40, 65, 2, 63, None),             # the largest radius
    (2, 33, 129, 3, 5, None),
    (2, 1, 200, 2, 2, None),
    (2, 50, 1, 2, 2, None),
    (1, 30, 4096, 2, 9, None),            # the widest frame
    (2, 17, 23, 2, 0.0, None),            # r = 0
]


@pytest.mark.parametrize('n,h,w,n_obj,th,max_label', SIZES)
def test_davis_counts_bit_identical_to_host(eng, n, h, w, n_obj, th, max_label):
    rng = np.random.default_rng(h * 7919 + w)
    pred, gt = _blobs(rng, n, h, w, n_obj, max_label=max_label), _blobs(rng, n, h, w, n_obj, max_label=max_label)
    pred[0, : h // 2] = 0                                          # empty predictions on part of a frame
    np.testing.assert_array_equal(_device_counts(eng, pred, gt, n_obj, th), data.boundary_counts_host(pred, gt, n_obj, th))


def test_davis_counts_every_object_count(eng):
    rng = np.random.default_rng(11)
    pred, gt = _blobs(rng, 2, 61, 130, 10), _blobs(rng, 2, 61, 130, 10)
    for n_obj in range(1, 11):
        np.testing.assert_array_equal(_device_counts(eng, pred, gt, n_obj), data.boundary_counts_host(pred, gt, n_obj))


def test_davis_counts_80_frame_sequence(eng):
    """A whole 480p sequence through `Engine.davis_counts` (one object shifted a little per frame, as in a video)."""
    rng = np.random.default_rng(3)
    base_p, base_g = _blobs(rng, 1, 480, 854, 3)[0], _blobs(rng, 1, 480, 854, 3)[0]
    pred = np.stack([np.roll(base_p, 3 * f, axis=1) for f in range(80)])
    gt = np.stack([np.roll(base_g, 2 * f, axis=0) for f in range(80)])
    got = eng.davis_counts(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), 3)
    assert got.shape == (80, 3, 6) and got.dtype == np.int64
    np.testing.assert_array_equal(got, data.boundary_counts_host(pred, gt, 3))
    m_dev = data.sequence_measures(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), 3, engine=eng)
    assert m_dev == data.measures_from_counts(got[1:79])


def test_davis_counts_rejects_bad_arguments(eng):
    p = torch.zeros(2, 32, 48, dtype=torch.uint8, device='cuda:0')
    with pytest.raises(_ffi.EosvosError, match='radius'):
        eng.davis_counts(p, p, 2, bound_th=70)
    lib, h = eng.lib, eng.h
    out = np.zeros(2 * 255 * 6 + 6, dtype=np.int64)
    optr = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    ptr = ctypes.c_void_p(p.data_ptr())
    assert lib.eosvos_davis_counts(h, ptr, ptr, 2, 32, 48, 0, 1, optr) != 0            # n_obj < 1
    assert lib.eosvos_davis_counts(h, ptr, ptr, 2, 32, 48, 256, 1, optr) != 0          # n_obj > 255
    assert lib.eosvos_davis_counts(h, ptr, ptr, 1, 1, 4097, 1, 1, optr) != 0           # wider than 64 x 64
    assert lib.eosvos_davis_counts(h, ptr, ptr, 2, 32, 48, 1, -1, optr) != 0           # negative radius
    assert lib.eosvos_davis_counts(h, None, ptr, 2, 32, 48, 1, 1, optr) != 0
    assert lib.eosvos_davis_counts(h, ptr, ptr, 2, 32, 48, 1, 1, None) != 0
    assert not out.any()                                                               # nothing was written
    with pytest.raises(ValueError):
        eng.davis_counts(p.float(), p.float(), 2)
    # the engine still works after the rejections
    np.testing.assert_array_equal(eng.davis_counts(p, p, 2), data.boundary_counts_host(p.cpu().numpy(), p.cpu().numpy(), 2))


def test_evaluate_dataset_jf_on_the_device_matches_host():
    """evaluate_dataset at 480x854: the J / F statistics computed from the device counts equal the host path on the returned
    label maps, and J_seq is still `sequence_J` of those maps."""
    from eosvos_amd import config
    from eosvos_amd import evaluate as ev
    from eosvos_amd import synthetic
    from eosvos_amd.helper_func import init_parent_model
    from eosvos_amd.meta_optim import MetaOptimizer
    cfg = config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS', 'num_epochs.eval=3'])
    model, _ = init_parent_model(**dict(cfg['parent_model']))
    model.to('cuda:0')
    model.max_batch = 3
    model.load_state_dict(synthetic.synthetic_state(cfg['parent_model']['encoder']))
    torch.manual_seed(1)
    mo = MetaOptimizer(model, **cfg['meta_optim_cfg'])
    ds = data.SyntheticSequences(2, 6, 480, 854, seed=3)
    res = ev.evaluate_dataset(model, mo, mo.state_dict(), ds, cfg, 'val', objects_in_flight=1)
    keys = ('J_obj', 'J_recall_seq', 'J_decay_seq', 'F_seq', 'F_recall_seq', 'F_decay_seq')
    ref = {k: [] for k in keys}
    j_seq = []
    for s in ds.seqs_names:
        labels, gt = res['labels'][s].numpy(), ds.label_maps(s)
        j_seq.append(data.sequence_J(labels, gt, 2))
        m = data.sequence_measures(labels, gt, 2)                     # host counts
        for k, (mm, st) in zip(keys, [(a, b) for a in 'JF' for b in ('mean', 'recall', 'decay')]):
            ref[k].extend(m[mm][st])
    assert res['J_seq'] == j_seq and res['mean_J'] == float(np.mean(j_seq))
    for k in keys:
        assert res[k] == ref[k], k
    assert res['mean_F'] == float(np.mean(ref['F_seq']))
    assert res['mean_JF'] == (float(np.mean(ref['J_obj'])) + res['mean_F']) / 2
    if model.engine is not None:
        model.engine.close()
