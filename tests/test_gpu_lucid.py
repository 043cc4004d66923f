"""Lucid first-frame synthesis on the MI355X (`eosvos_amd/lucid.py`): the plate and the composed images against fp64, labels
and counts against the numpy twin bit for bit, the batch rules draw for draw, and `evaluate_sequence` with `lucid=`.  Needs an
MI355X: pytest -m gpu.

Tolerances are not fixed numbers (the yardstick of tests/test_gpu_zoom.py): the numpy twin evaluates the rules in fp32 and in
fp64; the kernel may differ from the fp64 value by twice what the fp32 twin does, and every case prints both (`pytest -s`)."""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import lucid_ref  # noqa: E402
from test_gpu_zoom import BN_CFG, MO_CFG, _fp32_error, _meta_state  # noqa: E402,F401

from eosvos_amd import _ffi, lucid, synthetic  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SMALL = (96, 160)
SIZES = lucid_ref.SIZES
SENTINEL = 7.0
IDS = [f'{h}x{w}' for h, w in SIZES]

_ENGINE = []


def _engine():
    """One engine for the whole module: the lucid calls are not tied to its frame size."""
    if not _ENGINE:
        _ENGINE.append(Engine('resnet50', *SMALL, max_batch=1, device=DEV))
    return _ENGINE[0]


@pytest.fixture(scope='module', autouse=True)
def _close_engine():
    yield
    for e in _ENGINE:
        e.close()
    _ENGINE.clear()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _inputs(hw):
    fr, m = lucid_ref.frame(*hw), lucid_ref.mask(*hw)
    return fr, m, torch.from_numpy(fr).to(DEV), torch.from_numpy(m).to(DEV)


def _err(expr):
    """`_fp32_error` of tests/test_gpu_zoom.py for a numpy expression of the dtype."""
    return _fp32_error(lambda dt: torch.from_numpy(np.asarray(expr(np.float64 if dt == torch.float64 else np.float32))))


# ---- 1. the plate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dilate', [0, 4, 16])
@pytest.mark.parametrize('hw', SIZES, ids=IDS)
def test_plate_against_fp64(hw, dilate):
    fr, m, frd, md = _inputs(hw)
    got = _engine().lucid_plate(frd, md, dilate).cpu()
    r64, err32 = _err(lambda dt: lucid.plate_host(fr, m, dilate, dt))
    err = float((got.double() - r64).abs().max())
    same = torch.equal(_bits(got), _bits(torch.from_numpy(lucid.plate_host(fr, m, dilate))))
    print(f'lucid_plate {hw[0]}x{hw[1]} dilate={dilate}: numpy fp32 error {err32:.3e}, kernel error {err:.3e}, allowed {2 * err32:.3e}; '
          f'the fp32 twin\'s bits: {same}')
    assert err32 > 0
    assert err <= 2 * err32
    known = torch.from_numpy(~lucid.hole_host(m[0] != 0, dilate))
    assert bool(known.any()) and not bool(known.all())
    assert torch.equal(_bits(got)[:, known], _bits(torch.from_numpy(fr))[:, known])             # known pixels: the frame's bits
    assert bool(torch.isfinite(got).all())


def test_plate_of_a_full_and_of_an_empty_mask():
    fr, m, frd, md = _inputs(SIZES[0])
    assert not bool(_engine().lucid_plate(frd, torch.ones_like(md), 4).any())                       # nothing known: all zero
    assert torch.equal(_bits(_engine().lucid_plate(frd, torch.zeros_like(md), 4)), _bits(frd))


# ---- 2. the composition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', SIZES, ids=IDS)
def test_compose_against_the_twin_and_fp64(hw):
    fr, m, frd, md = _inputs(hw)
    eng = _engine()
    plate = eng.lucid_plate(frd, md, 4)
    n_mask, centre = lucid.mask_geometry(m)
    cases = lucid_ref.compose_cases(*hw, centre)
    prm = [p for _, p in cases]
    images, labels, counts = eng.lucid_compose(frd, md, plate, prm)
    want = lucid.compose_host(fr, m, plate, prm)
    assert counts == want[2].tolist() and torch.equal(_bits(labels), _bits(torch.from_numpy(want[1])))
    assert 0 < counts[-1] < 0.8 * n_mask and counts[0] == n_mask                                 # leaving the frame; identity
    p32, p64 = lucid.plate_host(fr, m, 4), lucid.plate_host(fr, m, 4, np.float64)
    for i, (name, p) in enumerate(cases):
        r64, err32 = _err(lambda dt: lucid.compose_host(fr, m, p64 if dt == np.float64 else p32, [p], dt)[0])
        err = float((images[i:i + 1].cpu().double() - r64).abs().max())
        same = torch.equal(_bits(images[i]), _bits(torch.from_numpy(want[0][i])))
        print(f'lucid_compose {hw[0]}x{hw[1]} {name}: numpy fp32 error {err32:.3e}, kernel error {err:.3e}, allowed {2 * err32:.3e}; '
              f'the fp32 twin\'s bits: {same}')
        assert err32 > 0
        assert err <= 2 * err32
    # one sample per launch gives the same bits as the batch's launch, and the call without the host read too
    one = eng.lucid_compose(frd, md, plate, prm[3:4], read_counts=False)
    assert one[2] is None and torch.equal(_bits(one[0]), _bits(images[3:4])) and torch.equal(_bits(one[1]), _bits(labels[3:4]))
    # dilate 0, identity, no flip: the frame and its mask, bit for bit
    ident = {'flip': False, 'Bi': lucid.IDENTITY, 'Oi': lucid.IDENTITY}
    im, lb, cn = eng.lucid_compose(frd, md, eng.lucid_plate(frd, md, 0), [ident])
    assert torch.equal(_bits(im[0]), _bits(frd)) and torch.equal(lb[0], (md != 0).float()) and cn == [n_mask]


# ---- 3. NaN-filled buffers ------------------------------------------------------------------------------------------------
def device_digests(eng):
    """{size: digests of the plate, the images and the labels, and the counts} of the three test sizes, from the device."""
    out = {}
    for hw in SIZES:
        fr, m, frd, md = _inputs(hw)
        plate = eng.lucid_plate(frd, md, 4)
        prm = [p for _, p in lucid_ref.compose_cases(*hw, lucid.mask_geometry(m)[1])]
        images, labels, counts = eng.lucid_compose(frd, md, plate, prm)
        out[f'{hw[0]}x{hw[1]}'] = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (plate, images, labels)] + [counts]
    return out


CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from eosvos_amd.engine import Engine
import test_gpu_lucid as T
eng = Engine('resnet50', 96, 160, max_batch=1, device='cuda:0')
out = T.device_digests(eng)
eng.close()
print(json.dumps(out))
'''


def test_nan_filled_buffers_give_the_same_bits():
    """The same calls in a process whose engine buffers (the pyramid and the count record included) start out as NaN words, and
    in one that gets the allocator's pages as they come: a kernel that reads scratch nothing wrote would differ."""
    want = device_digests(_engine())
    for fill in (None, '7fc00000'):
        env = dict(os.environ, EOSVOS_MODE_GUARD='0')
        env.pop('EOSVOS_DEBUG_FILL', None)
        if fill:
            env['EOSVOS_DEBUG_FILL'] = fill
        p = subprocess.run([sys.executable, '-c', CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
        assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        assert json.loads(lines[-1]) == want, fill


# ---- 4. rules 10-11: the batch, draw for draw -----------------------------------------------------------------------------
H0, W0 = SIZES[0]
BATCH_CASES = [
    # name, mask, parameters, seed, (tries, fallback) per sample as the twin gave them on the CPU
    ('centred object, DEFAULTS', lucid_ref.centred_mask, dict(lucid.DEFAULTS, samples=4), 0, [(1, False)] * 4),
    ('corner object, redraws', lucid_ref.corner_mask, dict(lucid.DEFAULTS, samples=3, shift=0.3), 1,
     [(4, False), (3, False), (2, False)]),
    ('identity fallback', lucid_ref.corner_mask, dict(lucid.DEFAULTS, samples=3, shift=1.0, min_keep=1.0), 1,
     [(8, True), (4, False), (2, False)]),
]


@pytest.mark.parametrize('name,mask_of,prm,seed,tries', BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
def test_batch_equals_the_twin_draw_for_draw(name, mask_of, prm, seed, tries):
    fr, m = lucid_ref.frame(H0, W0), mask_of(H0, W0)
    k = prm['samples']
    him, hlb, hrec = lucid.batch_host(fr, m, prm, k, random.Random(seed))
    assert [(r['tries'], r['fallback']) for r in hrec] == tries                                 # the case is what its name says
    rng = random.Random(seed)
    aug = lucid.LucidAugmenter(_engine(), torch.from_numpy(fr).to(DEV), torch.from_numpy(m).to(DEV), prm, rng=rng)
    images, labels, rec = aug.batch(k)
    assert rec == hrec                                                  # parameters, draws, tries, counts, fallbacks
    assert torch.equal(_bits(labels), _bits(torch.from_numpy(hlb)))
    after = random.Random(seed)
    lucid.batch_host(fr, m, prm, k, after)
    assert rng.getstate() == after.getstate()
    h64 = lucid.batch_host(fr, m, prm, k, random.Random(seed), np.float64)[0]
    err32, err = float(np.abs(him - h64).max()), float((images.cpu().double() - torch.from_numpy(h64)).abs().max())
    print(f'lucid batch, {name}: numpy fp32 error {err32:.3e}, kernel error {err:.3e}, allowed {2 * err32:.3e}')
    assert err32 > 0
    assert err <= 2 * err32


# ---- 5. end to end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model_and_optim():
    from eosvos_amd.helper_func import init_parent_model
    from eosvos_amd.meta_optim import MetaOptimizer
    model, _ = init_parent_model(architecture='DeepLabV3Plus', encoder='resnet50', train_encoder=True,
                                 decoder_norm_layer='BatchNorm2d', replace_batch_with_group_norms=False, batch_norm=BN_CFG,
                                 roi_pool_output_sizes=None, eval_augment_rpn_proposals_mode=None, box_nms_thresh=None,
                                 maskrcnn_loss=None)
    sd, msd = _meta_state()
    model.load_state_dict(sd)
    mo = MetaOptimizer(model, **MO_CFG)
    yield model, mo, msd
    model.close_engines()


def test_evaluate_sequence_on_and_off(model_and_optim, monkeypatch):
    from eosvos_amd import config
    from eosvos_amd.evaluate import _repeat_batch, device_augment, evaluate_sequence
    from eosvos_amd.helper_func import set_random_seeds
    model, mo, msd = model_and_optim
    mo.load_state_dict(msd)
    mo.reset()
    cfg = config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS-OnA', 'num_epochs.eval=3', 'eval_online_adapt.num_epochs=1',
                            'eval_online_adapt.step=2'])
    bsz = cfg['data_cfg']['batch_sizes']['train']
    frames, gt = synthetic.synthetic_frames(1, *SMALL, seed=3)
    seq = torch.cat([torch.roll(frames, shifts=4 * i, dims=3) for i in range(4)]).to(DEV)
    seen = []
    call = type(model).__call__

    def recording(self, inputs):
        seen.append(inputs.clone())
        return call(self, inputs)
    monkeypatch.setattr(type(model), '__call__', recording)
    with monkeypatch.context() as mp:
        def no_lucid(*a, **k):
            raise AssertionError('a lucid call on the plain path')
        for name in ('lucid_plate', 'lucid_compose'):
            mp.setattr(Engine, name, no_lucid)
        outs = [evaluate_sequence(model, mo, msd, seq, [gt[0]], cfg, **kw) for kw in ({}, {'lucid': None}, {'lucid': {'samples': 0}})]
    for labels, probs, hist in outs[1:]:
        assert torch.equal(labels, outs[0][0]) and hist == outs[0][2]
        assert torch.equal(_bits(probs[0]), _bits(outs[0][1][0]))
    n_off = len(seen) // 3
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(seen[n_off:2 * n_off], seen[:n_off]))
    del seen[:]
    L = {'samples': 2}
    labels, probs, hist = evaluate_sequence(model, mo, msd, seq, [gt[0]], cfg, lucid=L)
    assert len(seen) == n_off and len(hist[0][0]) == 3 and bool(torch.isfinite(probs[0]).all())
    g = gt[0].to(DEV).float().view(1, 1, *SMALL)
    assert torch.equal(probs[0][0], 2 * g[0, 0])                      # the train frame of the result is the seeded ground truth
    # the batches the model saw in round 0: [plain ..., lucid ...] of rule 12, replayed with the same draws
    got = [t.clone() for t in seen[:3]]
    augment = device_augment(model) if cfg['data_cfg'].get('random_train_transform') else _repeat_batch
    k = min(2, bsz)
    eng = model._ensure_engine(*SMALL, bsz)
    aug = lucid.LucidAugmenter(eng, seq[0].contiguous(), g[0].contiguous(), L)
    fr, m = seq[0].cpu().numpy(), g[0].cpu().numpy()
    aug_labels = {}
    for epoch in (1, 2, 3):
        seed = cfg.get('seed', 1) + epoch
        set_random_seeds(seed)
        parts = [augment(seq[:1], g, bsz - k, seed)[0]] if bsz - k else []
        lucid_images, lucid_labels, _ = aug.batch(k)
        aug_labels[epoch - 1] = lucid_labels
        want = torch.cat(parts + [lucid_images])
        assert got[epoch - 1].shape == (bsz, 3, *SMALL) and torch.equal(_bits(got[epoch - 1]), _bits(want))
        plain = (lambda n: augment(seq[:1], g, n, seed)) if bsz - k else None
        twin = {}
        for dt in (np.float32, np.float64):                             # ... and the twin, from the same draws
            set_random_seeds(seed)
            twin[dt] = lucid.batch_host(fr, m, L, bsz, dtype=dt, plain=plain)
        assert len(twin[np.float32][2]) == k
        assert torch.equal(_bits(aug_labels[epoch - 1]), _bits(torch.from_numpy(twin[np.float32][1][bsz - k:])))
        r64 = torch.from_numpy(twin[np.float64][0][bsz - k:])
        err32 = float((torch.from_numpy(twin[np.float32][0][bsz - k:]).double() - r64).abs().max())
        err = float((got[epoch - 1][bsz - k:].cpu().double() - r64).abs().max())
        print(f'evaluate_sequence, lucid samples of epoch {epoch}: numpy fp32 error {err32:.3e}, kernel error {err:.3e}, allowed '
              f'{2 * err32:.3e}')
        assert err32 > 0
        assert err <= 2 * err32
        assert not torch.equal(got[epoch - 1][bsz - 1], seq[0])
    mo.reset()


# ---- 6. bad arguments -----------------------------------------------------------------------------------------------------
def test_bad_arguments_return_errors_without_launching():
    eng = _engine()
    lib, h = eng.lib, eng.h
    H, W = SIZES[0]
    fr, m, frd, md = _inputs((H, W))
    plate = torch.full((3, H, W), SENTINEL, device=DEV)
    images = torch.full((1, 3, H, W), SENTINEL, device=DEV)
    labels = torch.full((1, 1, H, W), SENTINEL, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                        # noqa: E731
    flips = (ctypes.c_int32 * 17)()
    mats = (ctypes.c_double * (12 * 17))(*(list(lucid.IDENTITY) * 34))
    nan = (ctypes.c_double * 12)(*([float('nan')] + [0.0] * 11))
    counts = (ctypes.c_int32 * 17)(*([77] * 17))
    pl = lambda **k: lib.eosvos_lucid_plate(*[k.get(n, d) for n, d in (                              # noqa: E731
        ('e', h), ('frame', P(frd)), ('mask', P(md)), ('C', 3), ('H', H), ('W', W), ('dilate', 4), ('plate', P(plate)))])
    co = lambda **k: lib.eosvos_lucid_compose(*[k.get(n, d) for n, d in (                            # noqa: E731
        ('e', h), ('frame', P(frd)), ('mask', P(md)), ('plate', P(frd)), ('C', 3), ('H', H), ('W', W), ('n', 1), ('flips', flips),
        ('mats', mats), ('images', P(images)), ('labels', P(labels)), ('counts', counts))])
    bad = [
        lambda: pl(e=None), lambda: pl(frame=None), lambda: pl(mask=None), lambda: pl(plate=None), lambda: pl(C=0), lambda: pl(C=65),
        lambda: pl(H=0), lambda: pl(W=0), lambda: pl(H=4097), lambda: pl(W=4097), lambda: pl(dilate=-1), lambda: pl(dilate=17),
        lambda: co(e=None), lambda: co(frame=None), lambda: co(mask=None), lambda: co(plate=None), lambda: co(flips=None),
        lambda: co(mats=None), lambda: co(images=None), lambda: co(labels=None), lambda: co(C=0), lambda: co(H=0), lambda: co(W=0),
        lambda: co(H=4097), lambda: co(W=4097), lambda: co(n=0), lambda: co(n=17), lambda: co(mats=nan),
    ]
    for i, call in enumerate(bad):
        assert call() == 1, i
        assert lib.eosvos_last_error().decode(), i
    torch.cuda.synchronize()
    assert bool((plate == SENTINEL).all()) and bool((images == SENTINEL).all()) and bool((labels == SENTINEL).all())
    assert list(counts) == [77] * 17                                    # nothing was written
    with pytest.raises(_ffi.EosvosError):
        _ffi.check(co(n=0))
    ident = {'flip': False, 'Bi': lucid.IDENTITY, 'Oi': lucid.IDENTITY}
    for call in (lambda: eng.lucid_plate(frd, md, 17), lambda: eng.lucid_plate(frd.cpu(), md, 4), lambda: eng.lucid_plate(frd, md[:, 1:], 4),
                 lambda: eng.lucid_plate(frd, md, 2.0), lambda: eng.lucid_compose(frd, md, frd, []),
                 lambda: eng.lucid_compose(frd, md, frd, [ident] * 17), lambda: eng.lucid_compose(frd, md, frd[:, 1:].contiguous(), [ident]),
                 lambda: eng.lucid_compose(frd.double(), md, frd, [ident])):
        with pytest.raises(ValueError):
            call()
