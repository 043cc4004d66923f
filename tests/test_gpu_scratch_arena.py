"""The one scratch arena of the evaluation-stage entry points on the MI355X (csrc/engine.cpp `scratch_for`, the layouts of
csrc/scratch_layout.h): every stage through two engines in opposite orders -- the arena grows at different calls on the two --
and, on one of them, with every byte of the arena set to 0xFF between calls.  A stage that read a region it did not write or
clear itself, or whose regions overlapped, would differ between the engines, from its own repeat, or from its numpy twin.
Needs an MI355X: pytest -m gpu.  Everything is compared exactly (the fp32 results by their bits)."""
import numpy as np
import pytest
import torch

import adapt_ref
import crf_ref
import snap_ref
import zoom_ref
from eosvos_amd import adapt, components, data, holes, motion, snap, zoom
from eosvos_amd.engine import Engine
from test_gpu_adapt import fill_scratch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_OBJ = 3
FILTER = dict(connectivity=8, min_area=6, gate=3)
HOLES = dict(connectivity=8, max_area=60, prev_overlap=0.5)
SNAP = dict(step=8, iterations=3, compactness=10, min_share=0.5)
MOTION = dict(block=8, radius=4, bias=2)
ADAPT = dict(neg_dist=40, erode=3)
KEEP = (2,)


def raw(a):
    """A result as numpy arrays that compare exactly: tensors from the device, fp32 as its bits."""
    if isinstance(a, (tuple, list)):
        return [raw(v) for v in a]
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    if isinstance(a, list):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a.dtype == b.dtype and np.array_equal(a, b)


@pytest.fixture(scope='module')
def inputs():
    """5 frames of 37 x 53 with 3 objects and 3 frames of 97 x 161, all from seeds; `mv`: the twin's vectors of the small frames."""
    lab = snap_ref.blob_labels(5, 37, 53, N_OBJ, seed=3, above=False)
    rgb = snap_ref.noise_rgb(5, 37, 53, seed=5, smooth=True)
    images, probs = crf_ref.scene(97, 161, N_OBJ, seed=11, n_frames=3)
    p, a = adapt_ref.three_frames(97, 161)
    z = np.stack([zoom_ref.frame(97, 161, (40, 49, 70, 81)), zoom_ref.frame(97, 161), zoom_ref.frame(97, 161, (0, 8, 150, 160))])
    return dict(lab=lab, gt=snap_ref.blob_labels(5, 37, 53, N_OBJ, seed=4, above=False), rgb=rgb, images=images, probs=probs,
                p=p, a=a, z=z, mv=motion.vectors_host(rgb, MOTION))


def calls(eng, x):
    """[(name, the call)] in engine A's order, every input on the device."""
    d = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(DEV) for k, v in x.items()}
    davis = lambda: eng.davis_counts(d['lab'], d['gt'], N_OBJ)
    crf = lambda: eng.crf_labels(d['images'], d['probs'], iterations=2, return_q=True)
    return [
        ('davis_counts', davis),
        ('crf_labels', crf),
        ('filter_components', lambda: eng.filter_components(d['lab'], keep=KEEP, return_removed=True, **FILTER)),
        ('snap_labels', lambda: eng.snap_labels(d['rgb'], d['lab'], n_obj=N_OBJ, keep=KEEP, return_changed=True, **SNAP)),
        ('fill_holes', lambda: eng.fill_holes(d['lab'], keep=KEEP, return_filled=True, **HOLES)),
        ('block_motion', lambda: eng.block_motion(d['rgb'], **MOTION)),
        ('warp_labels', lambda: eng.warp_labels(d['lab'], d['mv'], MOTION['block'])),
        ('adapt_targets', lambda: eng.adapt_targets(d['p'], d['a'], 0.3, 0.7, ADAPT, adapt_ref.IGN)),
        ('zoom_boxes', lambda: eng.zoom_boxes(d['z'], zoom_ref.BASE)),
        ('davis_counts again', davis),
        ('crf_labels again', crf),
    ]


def test_every_stage_shares_one_arena(inputs):
    x = inputs
    a, b = (Engine('resnet50', 96, 160, max_batch=1, device=DEV) for _ in range(2))
    try:
        got_a, got_b = {}, {}
        for name, call in calls(a, x):
            got_a[name] = raw(call())
            fill_scratch(a)                                            # the next call finds 0xFF in every byte of the arena
        for name, call in reversed(calls(b, x)):
            got_b[name] = raw(call())
    finally:
        a.close()
        b.close()
    for name in got_a:
        assert same(got_a[name], got_b[name]), name
    for name in ('davis_counts', 'crf_labels'):
        assert same(got_a[name + ' again'], got_a[name]) and same(got_b[name + ' again'], got_b[name]), name
    twins = {
        'davis_counts': data.boundary_counts_host(x['lab'], x['gt'], N_OBJ),
        'filter_components': components.filter_host(x['lab'], FILTER, keep=KEEP, return_removed=True),
        'snap_labels': snap.snap_host(x['rgb'], x['lab'], SNAP, keep=KEEP, n_obj=N_OBJ, return_changed=True),
        'fill_holes': holes.fill_host(x['lab'], HOLES, keep=KEEP, return_filled=True),
        'block_motion': x['mv'],
        'warp_labels': motion.warp_host(x['lab'], x['mv'], MOTION['block']),
        'adapt_targets': adapt.targets_host(x['p'], x['a'], 0.3, 0.7, ADAPT, adapt_ref.IGN),
        'zoom_boxes': zoom.boxes_host(x['z'], zoom_ref.BASE),
    }
    removed, changed, filled = got_a['filter_components'][1], got_a['snap_labels'][1], got_a['fill_holes'][1]
    assert [v[0] for v in twins['zoom_boxes']] == [1, 0, 1]
    assert removed.sum() > 0 and changed.sum() > 0 and filled.sum() > 0 and removed[2] == changed[2] == filled[2] == 0
    for name, want in twins.items():
        got = got_a[name]
        if name == 'adapt_targets':                                    # the counts come back as a list of ints
            got, want = [got[0], np.asarray(got[1], dtype=np.int64)], (want[0], want[1].astype(np.int64))
        assert same(got, raw(want)), name
