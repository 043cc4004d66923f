"""SLIC superpixels and the superpixel snapping on the MI355X (`eosvos_superpixels`, `eosvos_snap_labels`,
csrc/slic_kernels.hip) against the numpy twin of `eosvos_amd/snap.py`.  Integer arithmetic on both sides: the ids, the snapped
maps and the counts of changed pixels are compared bit for bit, nothing is left out.  Needs an MI355X: pytest -m gpu.

The kernels' tile is 64 wide and 16 high, so the sizes are: 1 x 1, 7 x 5 (inside a tile and, with S 16 or 64, inside a cell),
37 x 53 and 97 x 161 (odd: no multiple of the tile or of S), 64 x 128 (exact multiples of both).  A tile's slice of the vote
table is kept in LDS up to 2048 words: n_obj 1 and 3 stay below that, 255 is above it in every tile of more than 8 clusters, and
n_obj 15 at S 4 has both kinds of tile in one launch (133 * 16 > 2048 in the interior, fewer clusters at the frame's border)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import snap_ref as ref  # noqa: E402

from eosvos_amd import _ffi, components, holes, snap  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = [(1, 1), (7, 5), (37, 53), (97, 161), (64, 128)]


def P(**kw):
    return dict(snap.DEFAULTS, **kw)


@pytest.fixture(scope='module')
def eng():
    e = Engine('resnet50', 96, 160, max_batch=1, device=DEV)        # lends its stream and scratch; frames are of any size
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def frames_case(h, w):
    """Three frames of different content: uniform noise, a gradient with noise, 0 / 255 noise; computed once, never changed."""
    return np.concatenate([ref.noise_rgb(1, h, w, seed=h + w), ref.noise_rgb(1, h, w, seed=h, smooth=True), ref.binary_rgb(1, h, w, seed=w)])


@functools.lru_cache(maxsize=None)
def labels_case(h, w, n_obj):
    return ref.blob_labels(3, h, w, n_obj, seed=n_obj)


@functools.lru_cache(maxsize=None)
def twin_ids(h, w, S, T, m):
    return snap.superpixels_host(frames_case(h, w), P(step=S, iterations=T, compactness=m))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_as_twin(eng, rgb, lab, params, n_obj, keep=(), ids=None, msg=''):
    """ids, snapped maps and changed counts of the device against the twin; returns the twin's (ids, maps, changed)."""
    want_ids = snap.superpixels_host(rgb, params) if ids is None else ids
    want, want_changed = snap.snap_host(rgb, lab, params, keep=keep, n_obj=n_obj, return_changed=True, ids=want_ids)
    x, l = dev(rgb), dev(lab)
    sp = {k: params[k] for k in ('step', 'iterations', 'compactness')}
    got_ids = eng.superpixels(x, **sp)
    got, changed = eng.snap_labels(x, l, n_obj=n_obj, keep=keep, return_changed=True, **params)
    assert got_ids.dtype == torch.int32 and got.dtype == torch.uint8
    np.testing.assert_array_equal(got_ids.cpu().numpy(), want_ids, err_msg=f'ids {msg}')
    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'maps {msg}')
    np.testing.assert_array_equal(changed, want_changed, err_msg=f'changed {msg}')
    np.testing.assert_array_equal(changed, (want != lab).sum(axis=(1, 2)))            # the count of differing pixels
    return want_ids, want, want_changed


# ---- sizes and parameters -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [4, 16, 64])
@pytest.mark.parametrize('h,w', SIZES)
def test_ids_and_maps_equal_the_twin(eng, h, w, S):
    rgb, lab = frames_case(h, w), labels_case(h, w, 3)
    for T in (1, 5):
        for m in (1, 10, 64):
            same_as_twin(eng, rgb, lab, P(step=S, iterations=T, compactness=m), 3, ids=twin_ids(h, w, S, T, m), msg=f'T {T} m {m}')


def test_two_frames_at_480_x_854(eng):
    rgb = np.concatenate([ref.noise_rgb(1, 480, 854, seed=1, smooth=True), ref.disc_scene(480, 854)[0]])
    lab = np.concatenate([ref.blob_labels(1, 480, 854, 2, seed=8), ref.disc_scene(480, 854)[2]])
    _, want, changed = same_as_twin(eng, rgb, lab, P(step=16, iterations=5, compactness=10), 2)
    assert changed.all()


def test_frames_of_one_call_do_not_leak_into_each_other(eng):
    rgb, lab = frames_case(97, 161), labels_case(97, 161, 3)
    params = P(step=16, iterations=5, min_share=0.3)
    x, l = dev(rgb), dev(lab)
    ids = eng.superpixels(x, step=16, iterations=5)
    out = eng.snap_labels(x, l, n_obj=3, **params)
    for f in range(3):
        assert torch.equal(eng.superpixels(x[f:f + 1], step=16, iterations=5)[0], ids[f]), f
        assert torch.equal(eng.snap_labels(x[f:f + 1], l[f:f + 1], n_obj=3, **params)[0], out[f]), f
    assert not torch.equal(ids[0], ids[1]) and not torch.equal(ids[1], ids[2])         # the contents do differ
    np.testing.assert_array_equal(out.cpu().numpy(), snap.snap_host(rgb, lab, params, n_obj=3))


def test_the_largest_distances_fit_32_bits(eng):
    h, w = 130, 200
    yy, xx = np.mgrid[0:h, 0:w]
    board = ((((yy // 64) + (xx // 64)) % 2) * 255).astype(np.uint8)
    corner = np.zeros((h, w), dtype=np.uint8)
    corner[:40, :50] = 255                                           # one saturated corner on black
    rgb = np.stack([np.stack([board] * 3), np.stack([corner] * 3), np.stack([board, 255 - board, board])])
    lab = ref.blob_labels(3, h, w, 3, seed=7)
    for T in (1, 5):
        ids, _, _ = same_as_twin(eng, rgb, lab, P(step=64, iterations=T, compactness=64), 3, msg=f'T {T}')
    # the twin's 64-bit D of a far candidate of another colour is beyond 2^29 here: the 32-bit bound is under load
    assert 3 * 255 ** 2 * 64 ** 2 + 64 ** 2 * 2 * 191 ** 2 < 2 ** 32


# ---- n_obj, keep, changed -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_obj,S', [(1, 4), (3, 16), (15, 4), (255, 4), (255, 16), (255, 64)])
def test_objects_keep_and_changed(eng, n_obj, S):
    h, w = 97, 161
    rgb, lab = frames_case(h, w), labels_case(h, w, n_obj)
    params = P(step=S, iterations=3, min_share=0.4 if n_obj < 255 else 0.0)      # no label of 256 holds 0.4 of a large cluster
    ids = twin_ids(h, w, S, 3, 10)
    _, want, changed = same_as_twin(eng, rgb, lab, params, n_obj, ids=ids)
    assert changed.any()
    _, kept, kept_changed = same_as_twin(eng, rgb, lab, params, n_obj, keep=(1,), ids=ids)
    assert kept_changed[1] == 0 and np.array_equal(kept[1], lab[1]) and np.array_equal(kept[[0, 2]], want[[0, 2]])
    same_as_twin(eng, rgb, lab, params, n_obj, keep=(0, 1, 2), ids=ids)
    quiet = eng.snap_labels(dev(rgb), dev(lab), n_obj=n_obj, keep=(1,), **params)     # changed_out null: nothing waits
    np.testing.assert_array_equal(quiet.cpu().numpy(), kept)
    if n_obj < 255:
        assert (lab > n_obj).any() and np.array_equal(want[lab > n_obj], lab[lab > n_obj])


def test_min_share_extremes(eng):
    rgb, lab = frames_case(37, 53), labels_case(37, 53, 3)
    for share in (0.0, 0.5, 1.0):
        _, want, changed = same_as_twin(eng, rgb, lab, P(step=8, iterations=3, min_share=share), 3)
        assert changed.any() == (share < 1.0)


# ---- scratch ------------------------------------------------------------------------------------------------------------
def test_scratch_is_reused_and_a_repeat_gives_the_same_bits(eng):
    big, big_lab = frames_case(97, 161), labels_case(97, 161, 3)
    small, small_lab = frames_case(37, 53), labels_case(37, 53, 3)
    pb, ps = P(step=4, iterations=5), P(step=16, iterations=2, compactness=64)
    xb, lb, xs, ls = dev(big), dev(big_lab), dev(small), dev(small_lab)
    a1 = eng.snap_labels(xb, lb, n_obj=3, **pb)                      # the larger call first
    b1 = eng.snap_labels(xs, ls, n_obj=3, **ps)                      # back to back on the same scratch
    i1 = eng.superpixels(xs, step=16, iterations=2, compactness=64)
    c1 = eng.filter_components(lb, largest_only=True)                # the filter and the hole filler share that scratch
    a2 = eng.snap_labels(xb, lb, n_obj=3, **pb)
    h1 = eng.fill_holes(ls, max_area=1 << 24)
    b2 = eng.snap_labels(xs, ls, n_obj=3, **ps)
    i2 = eng.superpixels(xs, step=16, iterations=2, compactness=64)
    assert torch.equal(a1, a2) and torch.equal(b1, b2) and torch.equal(i1, i2)
    np.testing.assert_array_equal(a1.cpu().numpy(), snap.snap_host(big, big_lab, pb, n_obj=3))
    np.testing.assert_array_equal(b1.cpu().numpy(), snap.snap_host(small, small_lab, ps, n_obj=3))
    np.testing.assert_array_equal(i1.cpu().numpy(), snap.superpixels_host(small, ps))
    np.testing.assert_array_equal(c1.cpu().numpy(), components.filter_host(big_lab, dict(components.DEFAULTS, largest_only=True)))
    np.testing.assert_array_equal(h1.cpu().numpy(), holes.fill_host(small_lab, dict(holes.DEFAULTS, max_area=1 << 24)))


def test_chunks_of_one_frame_equal_the_unchunked_call(eng, monkeypatch):
    rgb, lab = frames_case(97, 161), labels_case(97, 161, 3)
    params = P(step=16, iterations=3)
    x, l = dev(rgb), dev(lab)
    whole, whole_changed = eng.snap_labels(x, l, n_obj=3, keep=(2,), return_changed=True, **params)
    whole_ids = eng.superpixels(x, step=16, iterations=3)
    assert snap.frames_per_call(3, 97, 161, 16) >= 3
    monkeypatch.setattr(snap, 'SCRATCH_CAP', snap.scratch_bytes(1, 3, 97, 161, 16) + 64)
    assert snap.frames_per_call(3, 97, 161, 16) == 1 and snap.frames_per_call(0, 97, 161, 16) == 1
    calls = []
    real = eng.lib.eosvos_snap_labels
    monkeypatch.setattr(eng, 'lib', type('Lib', (), {'__getattr__': lambda s, k: getattr(_ffi.load(), k),
                                                     'eosvos_snap_labels': lambda s, *a: (calls.append(a[3]), real(*a))[1]})())
    parts, parts_changed = eng.snap_labels(x, l, n_obj=3, keep=(2,), return_changed=True, **params)
    assert calls == [1, 1, 1]                                        # one frame per call
    assert torch.equal(parts, whole) and np.array_equal(parts_changed, whole_changed)
    assert torch.equal(eng.superpixels(x, step=16, iterations=3), whole_ids)


# ---- rejections ---------------------------------------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def test_limits_are_refused_without_a_launch(eng):
    rgb, lab = frames_case(37, 53), labels_case(37, 53, 3)
    x, l = dev(rgb), dev(lab)
    out = torch.full((3, 37, 53), 77, dtype=torch.uint8, device=DEV)
    ids = torch.full((3, 37, 53), -5, dtype=torch.int32, device=DEV)
    lib, h = eng.lib, eng.h

    def snp(e=h, r=x, lb=l, n=3, H=37, W=53, n_obj=3, S=8, T=3, m=10, q=32768, o=out):
        return lib.eosvos_snap_labels(e, _ptr(r), _ptr(lb), n, H, W, n_obj, S, T, m, q, None, _ptr(o), None)

    def sup(e=h, r=x, n=3, H=37, W=53, S=8, T=3, m=10, o=ids):
        return lib.eosvos_superpixels(e, _ptr(r), n, H, W, S, T, m, _ptr(o))
    # arguments only: they are refused before anything is read, so the buffers need not have the size that is named
    common = (dict(S=3), dict(S=65), dict(S=0), dict(T=0), dict(T=21), dict(m=0), dict(m=65), dict(H=4097, W=1), dict(H=1, W=4097),
              dict(H=0), dict(W=0), dict(n=-1), dict(n=65536), dict(e=None), dict(r=None), dict(o=None))
    for kw in common + (dict(n_obj=256), dict(n_obj=0), dict(q=-1), dict(q=65537), dict(lb=None),
                        dict(H=4096, W=4096, S=4, n_obj=255)):
        assert snp(**kw) != 0, kw
        assert lib.eosvos_last_error().decode().startswith('snap_labels'), kw
    assert 'cap' in lib.eosvos_last_error().decode()                 # the last one: a single frame over 512 MB is rejected
    for kw in common + (dict(n=65535, H=4096, W=4096, S=4),):
        assert sup(**kw) != 0, kw
        assert lib.eosvos_last_error().decode().startswith('superpixels'), kw
    assert 'cap' in lib.eosvos_last_error().decode()
    eng.synchronize()
    assert bool((out == 77).all()) and bool((ids == -5).all())       # nothing was written
    with pytest.raises(_ffi.EosvosError, match='snap_labels'):
        _ffi.check(snp(S=3))
    assert snp() == 0 and sup() == 0                                 # valid calls right after succeed
    eng.synchronize()
    params = P(step=8, iterations=3)
    np.testing.assert_array_equal(out.cpu().numpy(), snap.snap_host(rgb, lab, params, n_obj=3))
    np.testing.assert_array_equal(ids.cpu().numpy(), snap.superpixels_host(rgb, params))
    for bad in (dict(step=3), dict(iterations=0), dict(compactness=65), dict(n_obj=256), dict(min_share=1.5)):
        with pytest.raises(ValueError):
            eng.snap_labels(x, l, **dict(dict(step=8), **bad))
    with pytest.raises(ValueError):
        eng.snap_labels(x.cpu(), l, step=8)
    with pytest.raises(ValueError):
        eng.snap_labels(x, l.int(), step=8)
    with pytest.raises(ValueError):
        eng.snap_labels(x, l[:, :, :50], step=8)
    with pytest.raises(ValueError):
        eng.superpixels(x.float(), step=8)


# ---- the evaluation -----------------------------------------------------------------------------------------------------
def test_merge_objects_chain_on_the_engine_equals_the_host_twins(eng):
    from eosvos_amd.evaluate import merge_objects
    h, w, n = 97, 161, 4
    rgb, truth, pred = ref.disc_scene(h, w, seed=2)
    g = torch.Generator().manual_seed(5)
    frames = torch.from_numpy(np.repeat(rgb, n, axis=0)).float() / 255.0
    frames = torch.roll(frames, shifts=3, dims=3)                    # the frame is not where the prediction is
    probs = torch.stack([torch.from_numpy(pred[0] == o + 1).float() * 0.8 + 0.1 for o in range(2)])[None].repeat(n, 1, 1, 1)
    probs = (probs + 0.35 * (torch.rand(probs.shape, generator=g) - 0.5)).clamp(0, 1)          # speckle around the threshold
    frames, probs = frames.to(DEV), probs.to(DEV)
    per_object = [probs[:, o].contiguous() for o in range(2)]
    today = merge_objects(eng, per_object)
    sp = P(step=8, iterations=5, min_share=0.6)
    cp = dict(components.DEFAULTS, min_area=4, largest_only=True)
    hp = dict(holes.DEFAULTS, max_area=64)
    got = merge_objects(eng, per_object, frames, crf=None, keep=(1,), snap=sp, components=cp, holes=hp)
    snapped = snap.snap_host(snap.quantise(frames.cpu()), today.cpu().numpy(), sp, keep=(1,), n_obj=2)
    cleaned = components.filter_host(snapped, cp, keep=(1,))
    want = holes.fill_host(cleaned, hp, keep=(1,))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert torch.equal(got[1], today[1]) and not np.array_equal(snapped, today.cpu().numpy())
    assert torch.equal(snap.quantise(frames).cpu(), snap.quantise(frames.cpu()))               # the quantiser agrees across devices
    only = merge_objects(eng, per_object, frames, keep=(1,), snap=sp)
    np.testing.assert_array_equal(only.cpu().numpy(), snapped)
    assert torch.equal(merge_objects(eng, per_object, frames, snap=P()), today)                # off: today's maps
    with pytest.raises(ValueError, match='snap needs the frames'):
        merge_objects(eng, per_object, snap=sp)


def test_nothing_else_moves():
    from eosvos_amd import synthetic
    e = Engine('resnet50', 96, 160, max_batch=1, device=DEV)
    try:
        e.load_model_state(synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50'))
        frames, _ = synthetic.synthetic_frames(1, 96, 160, seed=3)
        frames = frames.to(DEV)
        before = e.infer(frames).clone()
        probs = torch.cat([before[0], 1.0 - before[0]]).contiguous()
        merged = e.merge_labels(probs).clone()
        fp = e.plan_fingerprint()
        rgb = snap.quantise(frames)
        ids = e.superpixels(rgb, step=16)
        out = e.snap_labels(rgb, merged[None], n_obj=2, step=16)
        np.testing.assert_array_equal(ids.cpu().numpy(), snap.superpixels_host(rgb, P(step=16)))
        np.testing.assert_array_equal(out.cpu().numpy(), snap.snap_host(rgb, merged[None], P(step=16), n_obj=2))
        assert torch.equal(e.infer(frames), before) and torch.equal(e.merge_labels(probs), merged)
        assert e.plan_fingerprint() == fp                            # no matrix kernel: the conv plans did not move
    finally:
        e.close()
