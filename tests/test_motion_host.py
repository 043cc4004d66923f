"""Host side of the motion compensation (`eosvos_amd/motion.py`): the numpy twin against the plain loops of
tests/motion_ref.py, what the parameter dictionary accepts, how the configuration carries it, and what the evaluation's merge
does with it.  CPU only: the engine is the stand-in of tests/fake_engine.py, which has none of the entry points and so takes the
twins."""
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
from fake_engine import FakeEngine  # noqa: E402

from eosvos_amd import _ffi, components, config, holes, motion  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402


def P(**kw):
    return dict(motion.DEFAULTS, **kw)


def planted(R):
    return (min(2, R), -min(3, R))


@functools.lru_cache(maxsize=None)
def case(kind, h, w, R):
    return ref.frames_case(kind, h, w, shift=planted(R))


# ---- the twin against the loops -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ref.KINDS)
@pytest.mark.parametrize('h,w,B,R,bias', ref.SHAPES)
def test_twin_equals_the_loops(h, w, B, R, bias, kind):
    rgb = case(kind, h, w, R)
    params = P(block=B, radius=R, bias=bias)
    mv = motion.vectors_host(rgb, params)
    assert mv.dtype == np.int8 and mv.shape == (3,) + motion.grid(h, w, B) + (2,)
    np.testing.assert_array_equal(mv, ref.vectors_loops(rgb, B, R, bias))
    assert not mv[0].any()                                           # no frame before the first: zeros
    with_prev = motion.vectors_host(rgb[1:], params, prev_rgb=rgb[0])
    np.testing.assert_array_equal(with_prev, mv[1:])                 # the chunked call: frame 0 hands itself over
    np.testing.assert_array_equal(with_prev, ref.vectors_loops(rgb[1:], B, R, bias, prev_rgb=rgb[0]))
    if kind == 'flat':
        assert not mv.any()
    if kind == 'shift':
        # frame f at (y, x) is frame f - 1 at (y + sy, x + sx): the planted vector costs bias * n, every other non-zero
        # candidate bias * n plus a sum of absolute differences of noise, (0, 0) that sum alone.  So the planted vector wins
        # exactly where bias * n is below the sum at rest, and with the largest bias (255 >= every difference) rest wins.
        s = planted(R)
        inside = ref.interior_blocks(h, w, B, s)
        y = motion.luma_host(rgb).astype(np.int64)
        for f in (1, 2):
            rest = np.add.reduceat(np.add.reduceat(np.abs(y[f] - y[f - 1]), np.arange(0, h, B), axis=0), np.arange(0, w, B), axis=1)
            n = np.add.reduceat(np.add.reduceat(np.ones((h, w), dtype=np.int64), np.arange(0, h, B), axis=0), np.arange(0, w, B), axis=1)
            moved = inside & (bias * n < rest)
            assert (mv[f][moved] == np.array(s)).all()
            assert bias or moved.sum() == inside.sum()               # without a bias every interior block returns it
            assert not mv[f][bias * n > rest].any()
    lab = ref.blob_labels(3, h, w, 3, seed=R)
    warped = motion.warp_host(lab, mv, B)
    assert warped.dtype == np.uint8
    np.testing.assert_array_equal(warped, ref.warp_loops(lab, mv, B))


def test_luma_and_the_order_of_equal_costs():
    rgb = np.zeros((1, 3, 2, 3), dtype=np.uint8)
    rgb[0, :, 0, 0], rgb[0, :, 0, 1], rgb[0, :, 0, 2] = (255, 255, 255), (255, 0, 0), (1, 2, 3)
    rgb[0, :, 1, 0], rgb[0, :, 1, 1] = (0, 255, 0), (0, 0, 255)
    np.testing.assert_array_equal(motion.luma_host(rgb)[0], [[255, 77, 2], [149, 29, 0]])
    # a flat pair of frames and no bias: every candidate costs 0; the shortest wins, (0, 0)
    flat = np.full((2, 3, 16, 16), 7, dtype=np.uint8)
    assert not motion.vectors_host(flat, P(block=8, radius=3, bias=0)).any()
    # equal costs at equal length: the current frame is constant, the previous one too but for a dark middle block
    cur = np.full((3, 8, 24), 100, dtype=np.uint8)
    prev = np.full((3, 8, 24), 100, dtype=np.uint8)
    prev[:, :, 8:16] = 0                                             # the middle block of the previous frame is dark
    mv = motion.vectors_host(cur[None], P(block=8, radius=8, bias=0), prev_rgb=prev)[0]
    # left and right block rest at cost 0; the middle block reaches cost 0 at dx = -8 and dx = +8 alike: dx = -8 is smaller
    np.testing.assert_array_equal(mv[0], [[0, 0], [0, -8], [0, 0]])
    np.testing.assert_array_equal(mv, ref.vectors_loops(cur[None], 8, 8, 0, prev_rgb=prev)[0])


def test_warp_clamps_vectors_from_elsewhere_and_refuses_wrong_sizes():
    lab = ref.blob_labels(1, 9, 10, 2)
    mv = np.zeros((1, 2, 2, 2), dtype=np.int8)
    mv[0, 0, 0], mv[0, 1, 1] = (-20, 3), (100, 100)
    out = motion.warp_host(lab, mv, 8)
    np.testing.assert_array_equal(out[0, :8, :8], np.repeat(lab[0, :1, 3:10], 8, axis=0)[:, list(range(7)) + [6]])
    assert (out[0, 8:, 8:] == lab[0, 8, 9]).all()
    for bad in (mv[:, :1], mv[0], np.zeros((1, 2, 2, 3), dtype=np.int8)):
        with pytest.raises(ValueError):
            motion.warp_host(lab, bad, 8)
    with pytest.raises(ValueError):
        motion.warp_host(lab, mv, 12)
    with pytest.raises(ValueError):
        motion.warp_host(lab, mv.astype(np.int32), 8)
    with pytest.raises(ValueError):
        motion.vectors_host(np.zeros((1, 3, 8, 8), dtype=np.float32), P(block=8))
    with pytest.raises(ValueError):
        motion.vectors_host(np.zeros((1, 3, 8, 8), dtype=np.uint8), P(block=8), prev_rgb=np.zeros((3, 8, 9), dtype=np.uint8))
    with pytest.raises(ValueError):
        motion.vectors_host(np.zeros((1, 3, 8, 8), dtype=np.uint8), P())


# ---- parameters and the command line ------------------------------------------------------------------------------------
def test_check_active_and_frames_per_call():
    assert motion.DEFAULTS == {'block': 0, 'radius': 16, 'bias': 2}
    assert motion.check({}) == motion.DEFAULTS and not motion.active(None) and not motion.active({}) and not motion.active(P())
    assert motion.active({'block': 8}) and motion.active(P(block=16, radius=32, bias=255)) and motion.active(P(block=8, radius=1, bias=0))
    for bad in ({'block': 12}, {'block': 4}, {'block': True}, {'block': 8.0}, {'radius': 33}, {'radius': 0}, {'bias': 256},
                {'bias': -1}, {'radius': 2.5}, {'step': 8}, [8]):
        with pytest.raises(ValueError):
            motion.check(bad)
        with pytest.raises(ValueError):
            motion.active(bad)
    # one luma plane per frame, rows padded to four bytes, and one plane for the frame before the first
    assert motion.plane_bytes(480, 854) == 480 * 856
    assert motion.frames_per_call(480, 854) == (512 << 20) // (480 * 856) - 1
    assert motion.frames_per_call(4096, 4096) == 31 and motion.frames_per_call(1, 1) == 65534


def test_parse_cli_carries_eval_motion_only_when_asked():
    assert 'eval_motion' not in config.parse_cli([]) and config.MOTION == {'eval_motion': motion.DEFAULTS}
    assert 'eval_motion' not in config.parse_cli(['eval_components.gate=2', 'eval_snap.step=16'])
    cfg = config.parse_cli(['eval_motion.block=8', 'eval_components.gate=2'])
    assert cfg['eval_motion'] == P(block=8) and cfg['eval_components']['gate'] == 2
    cfg = config.parse_cli(['eval_motion.block=16', 'eval_motion.radius=24', 'eval_holes.max_area=64', 'eval_holes.prev_overlap=0.5'])
    assert cfg['eval_motion'] == P(block=16, radius=24)
    assert config.parse_cli(['eval_motion.radius=8'])['eval_motion'] == P(radius=8)                      # still off: no consumer needed
    for bad in ('eval_motion.block=12', 'eval_motion.radius=33', 'eval_motion.bias=256'):
        with pytest.raises(ValueError):
            config.parse_cli([bad, 'eval_components.gate=2'])
    with pytest.raises(KeyError):
        config.parse_cli(['eval_motion.step=3'])
    for argv in (['eval_motion.block=8'], ['eval_motion.block=8', 'eval_components.min_area=4'],
                 ['eval_motion.block=8', 'eval_holes.max_area=64'], ['eval_motion.block=8', 'eval_holes.prev_overlap=0.5']):
        with pytest.raises(ValueError, match='no consumer'):
            config.parse_cli(argv)


# ---- the evaluation -----------------------------------------------------------------------------------------------------
def probs_of(lab, n_obj=1):
    """Per-object probabilities whose merge is `lab`."""
    lab = torch.from_numpy(lab)
    return [(lab == o + 1).float() * 0.8 + 0.1 for o in range(n_obj)]


def engine_for(h, w):
    return FakeEngine('resnet50', h, w, 1)


def composed(rgb, lab, cp, hp, mp, keep):
    """The chain's rule 8 from the host twins, frame by frame."""
    mv = motion.vectors_host(rgb, mp)
    out = lab
    for on, stage, params in ((cp is not None and cp['gate'] > 0, components.filter_host, cp),
                              (hp is not None and hp['prev_overlap'] > 0, holes.fill_host, hp)):
        if params is None:
            continue
        if not on:
            out = stage(out, params, keep=keep)
            continue
        src, out, prev = out, np.empty_like(out), None
        for f in range(src.shape[0]):
            out[f] = stage(src[f:f + 1], params, prev=prev, keep=(0,) if f in keep else ())[0]
            if f + 1 < src.shape[0]:
                prev = motion.warp_host(out[f:f + 1], mv[f + 1:f + 2], mp['block'])[0]
    return out


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_a_fast_object_survives_and_the_look_alike_goes(seed):
    from eosvos_amd.evaluate import merge_objects
    rgb, lab, obj, blob = ref.moving_object(seed)
    frames = torch.from_numpy(rgb).float() / 255.0
    eng = engine_for(48, 128)
    cp = dict(components.DEFAULTS, gate=2)
    mp = P(block=8, radius=24, bias=2)
    plain = merge_objects(eng, probs_of(lab), frames, keep=(0,), components=cp).numpy()
    assert [int((plain[f] == 1)[obj[f]].sum()) for f in range(4)] == [144, 0, 144, 0]       # removed on every second frame
    assert [int((plain[f] == 1)[blob[f]].sum()) for f in range(4)] == [0, 0, 16, 16]        # and the look-alike stays
    moved = merge_objects(eng, probs_of(lab), frames, keep=(0,), components=cp, motion=mp).numpy()
    assert [int((moved[f] == 1)[obj[f]].sum()) for f in range(4)] == [144, 144, 144, 144]
    assert not (moved == 1)[blob].any() and np.array_equal(moved == 1, obj)
    np.testing.assert_array_equal(moved, composed(rgb, lab, cp, None, mp, keep=(0,)))


def test_identical_frames_give_the_output_without_motion_and_both_stages_follow():
    from eosvos_amd.evaluate import merge_objects
    h, w, n = 37, 53, 5
    lab = ref.blob_labels(n, h, w, 3, seed=4)
    still = torch.from_numpy(np.repeat(ref.frames_case('noise', h, w, n=1), n, axis=0)).float() / 255.0
    eng = engine_for(h, w)
    cp = dict(components.DEFAULTS, gate=2, min_area=2)
    hp = dict(holes.DEFAULTS, max_area=40, prev_overlap=0.5)
    mp = P(block=8, radius=5)
    off = merge_objects(eng, probs_of(lab, 3), still, keep=(1,), components=cp, holes=hp)
    on = merge_objects(eng, probs_of(lab, 3), still, keep=(1,), components=cp, holes=hp, motion=mp)
    assert torch.equal(on, off) and not np.array_equal(off.numpy(), lab)
    assert torch.equal(merge_objects(eng, probs_of(lab, 3), still, keep=(1,), components=cp, holes=hp, motion=P()), off)
    # moving frames: both temporal stages against the composition of the twins; a stage whose rule is off stays batched
    rgb = ref.frames_case('shift', h, w, n=n, shift=(2, -3))
    frames = torch.from_numpy(rgb).float() / 255.0
    for c, hcfg in ((cp, hp), (cp, dict(hp, prev_overlap=0.0)), (dict(cp, gate=0), hp), (None, hp), (cp, None)):
        kw = {k: v for k, v in (('components', c), ('holes', hcfg)) if v is not None}
        got = merge_objects(eng, probs_of(lab, 3), frames, keep=(1,), motion=mp, **kw)
        np.testing.assert_array_equal(got.numpy(), composed(rgb, lab, c, hcfg, mp, keep=(1,)))
    assert not torch.equal(merge_objects(eng, probs_of(lab, 3), frames, keep=(1,), components=cp, holes=hp, motion=mp),
                           merge_objects(eng, probs_of(lab, 3), frames, keep=(1,), components=cp, holes=hp))


def test_motion_needs_the_frames_and_a_consumer():
    from eosvos_amd.evaluate import merge_objects
    lab = ref.blob_labels(2, 16, 16, 1)
    frames = torch.zeros(2, 3, 16, 16)
    eng = engine_for(16, 16)
    mp = P(block=8)
    gate = dict(components.DEFAULTS, gate=2)
    for kw in ({}, {'components': dict(components.DEFAULTS, min_area=3)}, {'holes': dict(holes.DEFAULTS, max_area=9)},
               {'holes': dict(holes.DEFAULTS, prev_overlap=0.5)}):
        with pytest.raises(ValueError, match='no consumer'):
            merge_objects(eng, probs_of(lab), frames, motion=mp, **kw)
    for bad in (None, frames[:1], frames[:, :, :8]):
        with pytest.raises(ValueError, match='motion needs the frames'):
            merge_objects(eng, probs_of(lab), bad, components=gate, motion=mp)
    with pytest.raises(ValueError):
        merge_objects(eng, probs_of(lab), frames, components=gate, motion={'block': 12})
    merge_objects(eng, probs_of(lab), frames, components=gate, motion=mp)


def test_evaluate_sequence_passes_motion_only_when_it_is_on(monkeypatch):
    from eosvos_amd import evaluate
    seen = []
    monkeypatch.setattr(evaluate, 'finetune_object', lambda model, mo, msd, frames, gt, *a, **k: (torch.zeros(frames.shape[0], 8, 8), []))
    monkeypatch.setattr(evaluate, 'merge_objects', lambda *a, **k: seen.append(sorted(k)) or torch.zeros(2, 8, 8, dtype=torch.uint8))

    class Model:
        engine = None
    frames, gts = torch.zeros(2, 3, 8, 8), [torch.zeros(1, 8, 8)]
    cfg = config.parse_cli([])
    gate = dict(components.DEFAULTS, gate=2)
    for kw in ({}, {'motion': None}, {'motion': P()}, {'motion': P(radius=3)}):
        evaluate.evaluate_sequence(Model(), None, None, frames, gts, cfg, **kw)
    assert seen == [[]] * 4                                          # off: today's call, no new keyword
    evaluate.evaluate_sequence(Model(), None, None, frames, gts, cfg, components=gate, motion=P(block=8))
    assert seen[-1] == ['components', 'keep', 'motion']
    cfg['data_cfg']['normalize'] = True
    evaluate.evaluate_sequence(Model(), None, None, frames, gts, cfg, components=gate, motion=P(block=8), snap={'step': 8})
    assert seen[-1] == ['components', 'frame_offset', 'keep', 'motion', 'snap']


# ---- chunking and the C-ABI ---------------------------------------------------------------------------------------------
class _HostLib:
    """`eosvos_block_motion` / `eosvos_warp_labels` on host pointers through the twin: lets the chunk loop of the `Engine`
    method run without a device."""
    def __init__(self):
        self.calls = []

    @staticmethod
    def _view(p, dtype, *shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return np.frombuffer((ctypes.c_uint8 * n).from_address(p.value), dtype=dtype).reshape(shape)

    def eosvos_block_motion(self, e, rgb, prev_rgb, n, h, w, block, radius, bias, mv):
        self.calls.append((n, prev_rgb is not None))
        prev = None if prev_rgb is None else self._view(prev_rgb, np.uint8, 3, h, w)
        self._view(mv, np.int8, n, *motion.grid(h, w, block), 2)[:] = \
            motion.vectors_host(self._view(rgb, np.uint8, n, 3, h, w), P(block=block, radius=radius, bias=bias), prev_rgb=prev)
        return 0

    def eosvos_warp_labels(self, e, labels, mv, n, h, w, block, out):
        self.calls.append((n,))
        self._view(out, np.uint8, n, h, w)[:] = motion.warp_host(self._view(labels, np.uint8, n, h, w),
                                                                  self._view(mv, np.int8, n, *motion.grid(h, w, block), 2), block)
        return 0


class _HostEngine:
    device = torch.device('cpu')
    h = None
    _check_stream = lambda self: None
    _check_rgb = Engine._check_rgb
    _check_label_maps = Engine._check_label_maps
    block_motion = Engine.block_motion
    warp_labels = Engine.warp_labels

    def __init__(self):
        self.lib = _HostLib()


def test_engine_methods_chunk_and_hand_the_last_frame_over(monkeypatch):
    h, w = 20, 33
    rgb = ref.frames_case('shift', h, w, n=5, shift=(1, -2))
    params = P(block=8, radius=3, bias=1)
    want = motion.vectors_host(rgb, params)
    for frames, calls in ((1, [(1, False)] + [(1, True)] * 4), (2, [(2, False), (2, True), (1, True)]), (9, [(5, False)])):
        monkeypatch.setattr(motion, 'SCRATCH_CAP', (frames + 1) * motion.plane_bytes(h, w))
        eng = _HostEngine()
        mv = eng.block_motion(torch.from_numpy(rgb), **params)
        assert eng.lib.calls == calls and mv.dtype == torch.int8 and np.array_equal(mv.numpy(), want)
    eng = _HostEngine()
    tail = eng.block_motion(torch.from_numpy(rgb[1:]), prev_rgb=torch.from_numpy(rgb[0]), **params)
    assert eng.lib.calls == [(4, True)] and np.array_equal(tail.numpy(), want[1:])
    lab = ref.blob_labels(5, h, w, 2)
    out = eng.warp_labels(torch.from_numpy(lab), tail.new_tensor(want), 8)
    assert eng.lib.calls[-1] == (5,) and np.array_equal(out.numpy(), motion.warp_host(lab, want, 8))
    n_calls = len(eng.lib.calls)
    for bad in (dict(block=0), dict(block=12), dict(radius=0), dict(bias=256)):
        with pytest.raises(ValueError):
            eng.block_motion(torch.from_numpy(rgb), **dict(params, **bad))
    with pytest.raises(ValueError):
        eng.block_motion(torch.from_numpy(rgb).float(), **params)
    with pytest.raises(ValueError):
        eng.block_motion(torch.from_numpy(rgb), prev_rgb=torch.from_numpy(rgb[0, :, :10]), **params)
    with pytest.raises(ValueError):
        eng.warp_labels(torch.from_numpy(lab), torch.from_numpy(want[:4]), 8)
    with pytest.raises(ValueError):
        eng.warp_labels(torch.from_numpy(lab), torch.from_numpy(want), 16)
    assert len(eng.lib.calls) == n_calls                             # refused before any call


def test_abi_symbols_exist_and_refuse_a_null_engine():
    lib = _ffi.load()
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'eosvos.h')).read()
    exported = _ffi.exported_symbols()
    assert 'eosvos_block_motion' in exported and len(lib.eosvos_block_motion.argtypes) == 10
    assert 'eosvos_warp_labels' in exported and len(lib.eosvos_warp_labels.argtypes) == 8
    assert 'eosvos_block_motion(' in hdr and 'eosvos_warp_labels(' in hdr
    assert lib.eosvos_block_motion(None, None, None, 1, 8, 8, 8, 1, 0, None) == 1
    assert b'block_motion' in lib.eosvos_last_error() and b'null' in lib.eosvos_last_error()
    assert lib.eosvos_warp_labels(None, None, None, 1, 8, 8, 8, None) == 1
    assert b'warp_labels' in lib.eosvos_last_error() and b'null' in lib.eosvos_last_error()
