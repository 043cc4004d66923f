"""Block motion and the warp of label maps on the MI355X (`eosvos_block_motion`, `eosvos_warp_labels`,
csrc/motion_kernels.hip) against the numpy twin of `eosvos_amd/motion.py`.  Integer arithmetic on both sides: vectors and maps
are compared bit for bit, nothing is left out.  Needs an MI355X: pytest -m gpu.

The search kernel's tile is 32 rows x 64 columns of pixels.  The sizes: the four of the host test (inside one partial block, one
exact block, odd sizes with blocks cut by both borders, partial 16-blocks with the largest bias), 48 x 128 (two tiles side by
side, the moving-object scenario's size and radius), 64 x 96 at block 16 and radius 32 (the largest window: 96 rows x 132
bytes, and every item pass of a wave), 33 x 200 (wide and low: four tile seams, a window higher than the frame, a last block
row of one pixel row) and 130 x 70 (five tile rows, 16-blocks cut by both borders)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import motion_ref as ref  # noqa: E402

from eosvos_amd import _ffi, components, holes, motion  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = ref.SHAPES + [(48, 128, 8, 24, 2), (64, 96, 16, 32, 0), (33, 200, 8, 32, 3), (130, 70, 16, 7, 255)]


def P(**kw):
    return dict(motion.DEFAULTS, **kw)


@pytest.fixture(scope='module')
def eng():
    e = Engine('resnet50', 96, 160, max_batch=1, device=DEV)        # lends its stream and scratch; frames are of any size
    yield e
    e.close()


def planted(R):
    return (min(2, R), -min(3, R))


@functools.lru_cache(maxsize=None)
def case(kind, h, w, R):
    return ref.frames_case(kind, h, w, shift=planted(R))


@functools.lru_cache(maxsize=None)
def twin(kind, h, w, B, R, bias):
    """The twin's vectors of a case; computed once, never changed."""
    mv = motion.vectors_host(case(kind, h, w, R), P(block=B, radius=R, bias=bias))
    mv.setflags(write=False)
    return mv


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- vectors and warp ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ref.KINDS)
@pytest.mark.parametrize('h,w,B,R,bias', SHAPES)
def test_vectors_and_warp_equal_the_twin(eng, h, w, B, R, bias, kind):
    rgb = case(kind, h, w, R)
    want = twin(kind, h, w, B, R, bias)
    x = dev(rgb)
    kw = dict(block=B, radius=R, bias=bias)
    got = eng.block_motion(x, **kw)
    assert got.dtype == torch.int8 and tuple(got.shape) == (3,) + motion.grid(h, w, B) + (2,)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    # one call on frames 0..2 == a call on 0..1 and a call on 2 with frame 1 handed over
    head, tail = eng.block_motion(x[:2], **kw), eng.block_motion(x[2:], prev_rgb=x[1], **kw)
    assert torch.equal(torch.cat([head, tail]), got)
    assert torch.equal(eng.block_motion(x, **kw), got)               # a repeat gives the same bytes
    if kind == 'flat':
        assert not bool(got.any())
    if kind == 'shift' and bias == 0:
        inside = ref.interior_blocks(h, w, B, planted(R))
        assert (want[1:][:, inside] == np.array(planted(R))).all()   # every interior block returns the planted vector
    lab = ref.blob_labels(3, h, w, 3, seed=R)
    warped = eng.warp_labels(dev(lab), got, B)
    assert warped.dtype == torch.uint8
    np.testing.assert_array_equal(warped.cpu().numpy(), motion.warp_host(lab, want, B))


def test_one_frame_and_chunks_of_one_frame(eng, monkeypatch):
    h, w, B, R, bias = 37, 53, 8, 5, 0
    x = dev(case('noise', h, w, R))
    kw = dict(block=B, radius=R, bias=bias)
    whole = eng.block_motion(x, **kw)
    assert not bool(eng.block_motion(x[:1], **kw).any())            # a single frame without a predecessor: zeros
    monkeypatch.setattr(motion, 'frames_per_call', lambda *a: 1)
    assert torch.equal(eng.block_motion(x, **kw), whole)            # the engine hands the last frame of a chunk over


# ---- the evaluation -----------------------------------------------------------------------------------------------------
def probs_of(lab, n_obj=1):
    lab = torch.from_numpy(lab).to(DEV)
    return [((lab == o + 1).float() * 0.8 + 0.1).contiguous() for o in range(n_obj)]


def composed(rgb, lab, cp, hp, mp, keep):
    """Rule 8 of `motion.py` from the host twins, frame by frame."""
    mv = motion.vectors_host(rgb, mp)
    out = lab
    for stage, params in ((components.filter_host, cp), (holes.fill_host, hp)):
        if params is None:
            continue
        src, out, prev = out, np.empty_like(out), None
        for f in range(src.shape[0]):
            out[f] = stage(src[f:f + 1], params, prev=prev, keep=(0,) if f in keep else ())[0]
            if f + 1 < src.shape[0]:
                prev = motion.warp_host(out[f:f + 1], mv[f + 1:f + 2], mp['block'])[0]
    return out


def test_the_chain_with_motion_on_the_moving_object(eng):
    from eosvos_amd.evaluate import merge_objects
    rgb, lab, obj, blob = ref.moving_object(0)
    frames = (torch.from_numpy(rgb).float() / 255.0).to(DEV)
    cp = dict(components.DEFAULTS, gate=2)
    hp = dict(holes.DEFAULTS, max_area=16, prev_overlap=0.5)
    mp = P(block=8, radius=24, bias=2)
    plain = merge_objects(eng, probs_of(lab), frames, keep=(0,), components=cp).cpu().numpy()
    assert [int((plain[f] == 1)[obj[f]].sum()) for f in range(4)] == [144, 0, 144, 0]
    assert [int((plain[f] == 1)[blob[f]].sum()) for f in range(4)] == [0, 0, 16, 16]
    moved = merge_objects(eng, probs_of(lab), frames, keep=(0,), components=cp, motion=mp).cpu().numpy()
    assert [int((moved[f] == 1)[obj[f]].sum()) for f in range(4)] == [144, 144, 144, 144]
    assert not (moved == 1)[blob].any()
    np.testing.assert_array_equal(moved, composed(rgb, lab, cp, None, mp, keep=(0,)))
    both = merge_objects(eng, probs_of(lab), frames, keep=(0,), components=cp, holes=hp, motion=mp).cpu().numpy()
    np.testing.assert_array_equal(both, composed(rgb, lab, cp, hp, mp, keep=(0,)))


def test_the_chain_with_motion_on_random_blobs_and_on_static_frames(eng):
    from eosvos_amd.evaluate import merge_objects
    h, w, n = 37, 53, 5
    lab = ref.blob_labels(n, h, w, 3, seed=4)
    cp = dict(components.DEFAULTS, gate=2, min_area=2)
    hp = dict(holes.DEFAULTS, max_area=40, prev_overlap=0.5)
    mp = P(block=8, radius=5)
    rgb = ref.frames_case('shift', h, w, n=n, shift=(2, -3))
    frames = (torch.from_numpy(rgb).float() / 255.0).to(DEV)
    got = merge_objects(eng, probs_of(lab, 3), frames, keep=(1,), components=cp, holes=hp, motion=mp)
    np.testing.assert_array_equal(got.cpu().numpy(), composed(rgb, lab, cp, hp, mp, keep=(1,)))
    off = merge_objects(eng, probs_of(lab, 3), frames, keep=(1,), components=cp, holes=hp)
    assert not torch.equal(got, off)
    still = frames[:1].repeat(n, 1, 1, 1)
    assert torch.equal(merge_objects(eng, probs_of(lab, 3), still, keep=(1,), components=cp, holes=hp, motion=mp),
                       merge_objects(eng, probs_of(lab, 3), still, keep=(1,), components=cp, holes=hp))


# ---- rejections ---------------------------------------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def test_bad_arguments_are_refused_without_a_launch(eng):
    h, w = 37, 53
    rgb = case('noise', h, w, 5)
    x = dev(rgb)
    lab = dev(ref.blob_labels(3, h, w, 3))
    by, bx = motion.grid(h, w, 8)
    mv = torch.full((3, by, bx, 2), 77, dtype=torch.int8, device=DEV)
    out = torch.full((3, h, w), 77, dtype=torch.uint8, device=DEV)
    lib, e = eng.lib, eng.h

    def mot(e=e, r=x, p=None, n=3, H=h, W=w, B=8, R=5, bias=0, o=mv):
        return lib.eosvos_block_motion(e, _ptr(r), _ptr(p), n, H, W, B, R, bias, _ptr(o))

    def wrp(e=e, lb=lab, v=mv, n=3, H=h, W=w, B=8, o=out):
        return lib.eosvos_warp_labels(e, _ptr(lb), _ptr(v), n, H, W, B, _ptr(o))
    # arguments only: they are refused before anything is read, so the buffers need not have the size that is named
    for kw in (dict(B=12), dict(B=0), dict(B=4), dict(R=0), dict(R=33), dict(bias=-1), dict(bias=256), dict(H=4097, W=1),
               dict(H=1, W=4097), dict(H=0), dict(W=0), dict(n=-1), dict(n=65535), dict(e=None), dict(r=None), dict(o=None),
               dict(n=200, H=4096, W=4096)):
        assert mot(**kw) != 0, kw
        assert lib.eosvos_last_error().decode().startswith('block_motion'), kw
    assert 'cap' in lib.eosvos_last_error().decode()                 # the last one: 201 planes of 16 MB exceed 512 MB
    for kw in (dict(B=12), dict(B=0), dict(H=4097, W=1), dict(H=0), dict(W=0), dict(n=-1), dict(n=65536), dict(e=None), dict(lb=None),
               dict(v=None), dict(o=None)):
        assert wrp(**kw) != 0, kw
        assert lib.eosvos_last_error().decode().startswith('warp_labels'), kw
    eng.synchronize()
    assert bool((mv == 77).all()) and bool((out == 77).all())        # nothing was written
    with pytest.raises(_ffi.EosvosError, match='block_motion'):
        _ffi.check(mot(B=12))
    assert mot() == 0                                                # valid calls right after succeed
    eng.synchronize()
    want = motion.vectors_host(rgb, P(block=8, radius=5, bias=0))
    np.testing.assert_array_equal(mv.cpu().numpy(), want)
    assert wrp() == 0
    eng.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), motion.warp_host(lab.cpu().numpy(), want, 8))
    # the Python side: wrong dtype, device or shape, a block that is none, a radius of 0, an mv of the wrong size
    for bad in (dict(block=12), dict(block=0), dict(radius=0), dict(radius=33), dict(bias=256)):
        with pytest.raises(ValueError):
            eng.block_motion(x, **dict(dict(block=8), **bad))
    for bad_rgb in (x.float(), x.cpu(), x[:, :2], x[0]):
        with pytest.raises(ValueError):
            eng.block_motion(bad_rgb, block=8)
    for bad_prev in (x[0].float(), x[0].cpu(), x[0, :, :30], x[:1]):
        with pytest.raises(ValueError):
            eng.block_motion(x, block=8, prev_rgb=bad_prev)
    for bad_mv in (mv[:2], mv[:, :by - 1], mv[:, :, :bx - 1], mv.int(), mv.cpu(), mv[..., :1]):
        with pytest.raises(ValueError):
            eng.warp_labels(lab, bad_mv, 8)
    with pytest.raises(ValueError):
        eng.warp_labels(lab, mv, 16)                                 # the vectors of another block size
    with pytest.raises(ValueError):
        eng.warp_labels(lab, mv, 12)
    with pytest.raises(ValueError):
        eng.warp_labels(lab.int(), mv, 8)
