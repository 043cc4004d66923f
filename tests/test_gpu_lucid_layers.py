"""Lucid synthesis with the other objects as moving layers on the MI355X (`eosvos_amd/lucid_layers.py`): labels, visible ids and
counts against the numpy twin bit for bit, the images against fp64, rule L6 against `Engine.lucid_compose`, occlusion, stale
buffers, bad arguments, the batch rules draw for draw, and `evaluate_sequence` with `layers=`.  Needs an MI355X: pytest -m gpu.

Tolerances are not fixed numbers (the yardstick of tests/test_gpu_lucid.py): the numpy twin evaluates the rules in fp32 and in
fp64; the kernel may differ from the fp64 twin by twice what the fp32 twin does, and every case prints both (`pytest -s`)."""
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

import lucid_layers_ref as ref  # noqa: E402
import lucid_ref  # noqa: E402
from test_gpu_zoom import BN_CFG, MO_CFG, _meta_state  # noqa: E402
from test_lucid_layers_host import FALLBACK, L2, PLACID, REDRAW, scene  # noqa: E402

from eosvos_amd import _ffi, lucid, lucid_layers as ll, synthetic  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SMALL = (96, 160)
SIZES = lucid_ref.SIZES + [(5, 300), (1, 1)]          # the host suite's sizes, a row across the 256-thread block, one pixel
IDS = [f'{h}x{w}' for h, w in SIZES]
LAYERS = [1, 2, 3, 8]
CAP = ll.MAX_SAMPLES_PER_LAUNCH
SAMPLES = [1, 3, CAP, CAP + 1]                         # the per-launch cap and the chunk seam behind it
SENTINEL = 7.0

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


def _case(hw, n_layers, n_samples):
    """(frame, id map, samples): the ids 1 .. n_layers in rotating depth orders, both flip values, layers that overlap each
    other and leave the frame."""
    fr, ids = lucid_ref.frame(*hw), ref.id_map(*hw, n_layers)
    up = list(range(1, n_layers + 1))
    prm = []
    for s in range(n_samples):
        order = up[s % n_layers:] + up[:s % n_layers]
        prm.append(ref.sample(*hw, order[::-1] if s & 2 else order, flip=bool(s & 1), shift=s))
    return fr, ids, prm


def _check_against_the_twin(hw, n_layers, n_samples):
    fr, ids, prm = _case(hw, n_layers, n_samples)
    eng = _engine()
    frd, idsd = torch.from_numpy(fr).to(DEV), torch.from_numpy(ids).to(DEV)
    plate = eng.lucid_plate(frd, (idsd != 0).float()[None], 2)
    images, labels, counts = ll.compose_chunked(eng, frd, idsd, plate, prm)
    ids_out = torch.cat([eng.lucid_compose_layers(frd, idsd, plate, prm[i:i + CAP], want_ids=True)[3] for i in range(0, len(prm), CAP)])
    p32, p64 = lucid.plate_host(fr, ids != 0, 2), lucid.plate_host(fr, ids != 0, 2, np.float64)
    w32 = ll.compose_host(fr, ids, p32, prm)
    w64 = ll.compose_host(fr, ids, p64, prm, dtype=np.float64)
    assert images.shape == (n_samples, 3, *hw) and labels.shape == (n_samples, 1, *hw) and ids_out.shape == (n_samples, *hw)
    assert counts == [w32[3][s, :n_layers].tolist() for s in range(n_samples)]
    assert torch.equal(_bits(labels), _bits(torch.from_numpy(w32[1]))) and torch.equal(ids_out.cpu(), torch.from_numpy(w32[2]))
    err32 = float(np.abs(w32[0].astype(np.float64) - w64[0]).max())
    err = float((images.cpu().double() - torch.from_numpy(w64[0])).abs().max())
    same = torch.equal(_bits(images), _bits(torch.from_numpy(w32[0])))
    print(f'lucid_compose_layers {hw[0]}x{hw[1]} layers={n_layers} samples={n_samples}: numpy fp32 error {err32:.3e}, kernel error '
          f'{err:.3e}, allowed {2 * err32:.3e}; the fp32 twin\'s bits: {same}')
    assert err <= 2 * err32
    return err32


# ---- 1. the device against the twin -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_layers', LAYERS)
@pytest.mark.parametrize('hw', SIZES, ids=IDS)
def test_compose_layers_against_the_twin_and_fp64(hw, n_layers):
    n_samples = SAMPLES[(SIZES.index(hw) + LAYERS.index(n_layers)) % len(SAMPLES)]              # every count at every size or depth
    err32 = _check_against_the_twin(hw, n_layers, n_samples)
    assert err32 > 0 or hw == (1, 1)                                    # one pixel of an all-hole plate: nothing to round


@pytest.mark.parametrize('n_samples', SAMPLES)
@pytest.mark.parametrize('n_layers', LAYERS)
def test_every_sample_count_at_every_depth(n_layers, n_samples):
    assert _check_against_the_twin(SIZES[0], n_layers, n_samples) > 0


# ---- 2. rule L6: one layer is today's compose -------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', lucid_ref.SIZES, ids=IDS[:3])
def test_one_layer_is_todays_compose(hw):
    fr, m = lucid_ref.frame(*hw), lucid_ref.mask(*hw)
    eng = _engine()
    frd, md = torch.from_numpy(fr).to(DEV), torch.from_numpy(m).to(DEV)
    plate = eng.lucid_plate(frd, md, 4)
    cases = [p for _, p in lucid_ref.compose_cases(*hw, lucid.mask_geometry(m)[1])]
    images, labels, counts = eng.lucid_compose(frd, md, plate, cases)
    idsd = (md[0] != 0).to(torch.uint8).contiguous()
    got = eng.lucid_compose_layers(frd, idsd, plate, [{'flip': p['flip'], 'Bi': p['Bi'], 'layers': [(1, p['Oi'])]} for p in cases],
                                   want_ids=True)
    assert torch.equal(_bits(got[0]), _bits(images)) and torch.equal(_bits(got[1]), _bits(labels)) and [c[0] for c in got[2]] == counts
    assert torch.equal(got[3], labels[:, 0].to(torch.uint8))


# ---- 3. occlusion -----------------------------------------------------------------------------------------------------------
def test_an_object_in_front_hides_the_target_and_one_behind_does_not():
    hw = lucid_ref.SIZES[2]
    h, w = hw
    fr = lucid_ref.frame(*hw)
    ids = np.zeros(hw, dtype=np.uint8)
    ids[30:60, 40:90], ids[20:70, 100:140] = 1, 2
    eng = _engine()
    frd, idsd = torch.from_numpy(fr).to(DEV), torch.from_numpy(ids).to(DEV)
    plate = eng.lucid_plate(frd, (idsd != 0).float()[None], 4)
    c1, c2 = ll.geometry(ids, 2)[1][1], ll.geometry(ids, 2)[2][1]
    oi = ref.motion(h, w, c1, 4.0, 1.05, 0.03, -0.02)
    over = ref.motion(h, w, c2, -6.0, 1.1, 0.02, -50.5 / w)             # object 2 moved half-way over the target
    bi = ref.motion(h, w, (w / 2.0, h / 2.0), 2.0, 1.02, 0.01, 0.02)
    front = {'flip': False, 'Bi': bi, 'layers': [(1, oi), (2, over)]}
    behind = {'flip': False, 'Bi': bi, 'layers': [(2, over), (1, oi)]}
    images, labels, counts, ids_out = eng.lucid_compose_layers(frd, idsd, plate, [front, behind], want_ids=True)
    t_mask, o_mask = (idsd == 1).float()[None].contiguous(), (idsd == 2).float()[None].contiguous()
    alone = eng.lucid_compose(frd, t_mask, plate, [{'flip': False, 'Bi': bi, 'Oi': oi}])         # the target on its own
    other = eng.lucid_compose(frd, o_mask, plate, [{'flip': False, 'Bi': bi, 'Oi': over}])       # the other object on its own
    yo, xo = lucid.fixed_coords(over, h, w, False)
    a_other = torch.from_numpy(ll.coverage(ids == 2, yo, xo)).to(DEV)
    assert torch.equal(other[1][0, 0], (a_other >= 512).float())                                # the twin's A is the device's
    # in front: the target's visible count drops, labels are 0 where the other layer's A >= 512, the image is that layer's
    # bicubic sample where its A == 1024
    assert 0 < counts[0][0] < alone[2][0] - 100 and counts[0][1] == other[2][0]
    assert not bool(labels[0, 0][a_other >= 512].any()) and bool((ids_out[0][a_other >= 512] == 2).all())
    assert torch.equal(labels[0, 0], alone[1][0, 0] * (a_other < 512).float())
    full = a_other == 1024
    assert int(full.sum()) > 100 and torch.equal(_bits(images[0][:, full]), _bits(other[0][0][:, full]))
    # behind: the labels of the single-object compose for the same Oi, bit for bit, and its count
    assert torch.equal(_bits(labels[1]), _bits(alone[1][0])) and counts[1][1] == alone[2][0] and counts[1][0] < other[2][0]
    full_t = torch.from_numpy(ll.coverage(ids == 1, *lucid.fixed_coords(oi, h, w, False))).to(DEV) == 1024
    assert torch.equal(_bits(images[1][:, full_t]), _bits(alone[0][0][:, full_t]))


# ---- 4. stale buffers ---------------------------------------------------------------------------------------------------------
def _raw(eng, frd, idsd, plate, prm, images, labels, ids_out, counts, target_id=1):
    n = len(prm)
    flips = (ctypes.c_int32 * n)(*[int(p['flip']) for p in prm])
    n_layers = (ctypes.c_int32 * n)(*[len(p['layers']) for p in prm])
    layer_ids = (ctypes.c_uint8 * (8 * n))()
    mats = (ctypes.c_double * (54 * n))()
    for s, p in enumerate(prm):
        for k, row in enumerate([p['Bi']] + [oi for _, oi in p['layers']]):
            mats[s * 54 + k * 6:s * 54 + k * 6 + 6] = row
        for k, (i, _) in enumerate(p['layers']):
            layer_ids[s * 8 + k] = i
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    return eng.lib.eosvos_lucid_compose_layers(eng.h, P(frd), P(idsd), P(plate), 3, *frd.shape[1:], n, flips, n_layers, layer_ids, mats,
                                               target_id, P(images), P(labels), P(ids_out), counts)


def test_stale_outputs_and_the_call_without_the_host_read():
    hw = SIZES[0]
    fr, ids, prm = _case(hw, 3, 3)
    eng = _engine()
    frd, idsd = torch.from_numpy(fr).to(DEV), torch.from_numpy(ids).to(DEV)
    plate = eng.lucid_plate(frd, (idsd != 0).float()[None], 2)
    want = eng.lucid_compose_layers(frd, idsd, plate, prm, want_ids=True)
    quiet = eng.lucid_compose_layers(frd, idsd, plate, prm, read_counts=False, want_ids=True)   # nothing waits
    assert quiet[2] is None and all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(quiet[::3] + quiet[1:2], want[::3] + want[1:2]))
    for byte in (0xFF, None):                                           # 0xFF bytes, then NaN words
        bufs = [torch.empty(3, 3, *hw, device=DEV), torch.empty(3, 1, *hw, device=DEV), torch.empty(3, *hw, dtype=torch.uint8, device=DEV)]
        for b in bufs:
            if byte is None and b.dtype == torch.float32:
                b.fill_(float('nan'))
            else:
                b.view(torch.uint8).fill_(0xFF)
        counts = (ctypes.c_int32 * 24)(*([-1] * 24))
        assert _raw(eng, frd, idsd, plate, prm, *bufs, counts) == 0
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(bufs, (want[0], want[1], want[3])))
        assert [list(counts[s * 8:s * 8 + 3]) for s in range(3)] == want[2] and all(counts[s * 8 + k] == 0 for s in range(3) for k in range(3, 8))
        bufs[2] = None                                                  # ids_out is optional
        assert _raw(eng, frd, idsd, plate, prm, bufs[0].zero_(), bufs[1].zero_(), None, None) == 0
        assert torch.equal(_bits(bufs[0]), _bits(want[0])) and torch.equal(_bits(bufs[1]), _bits(want[1]))


def device_digests(eng):
    """{case: digests of the images, the labels and the visible ids, and the counts} from the device."""
    out = {}
    for hw, n_layers, n_samples in ((SIZES[0], 3, 3), (SIZES[1], 8, CAP)):
        fr, ids, prm = _case(hw, n_layers, n_samples)
        frd, idsd = torch.from_numpy(fr).to(DEV), torch.from_numpy(ids).to(DEV)
        plate = eng.lucid_plate(frd, (idsd != 0).float()[None], 2)      # leaves the pyramid's floats in the scratch
        res = eng.lucid_compose_layers(frd, idsd, plate, prm, want_ids=True)
        out[f'{hw[0]}x{hw[1]}'] = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (res[0], res[1], res[3])] + [res[2]]
    return out


CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from eosvos_amd.engine import Engine
import test_gpu_lucid_layers as T
eng = Engine('resnet50', 96, 160, max_batch=1, device='cuda:0')
out = T.device_digests(eng)
eng.close()
print(json.dumps(out))
'''


def test_stale_scratch_gives_the_same_bits():
    """The same calls in processes whose engine buffers (the count record included) start out as 0xFF bytes and as NaN words: a
    kernel that reads scratch nothing wrote, or adds to counts nothing zeroed, would differ."""
    want = device_digests(_engine())
    for fill in ('ffffffff', '7fc00000'):
        env = dict(os.environ, EOSVOS_MODE_GUARD='0', EOSVOS_DEBUG_FILL=fill)
        p = subprocess.run([sys.executable, '-c', CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
        assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        assert json.loads(lines[-1]) == want, fill


# ---- 5. bad arguments ---------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_errors_without_launching():
    eng = _engine()
    lib, h = eng.lib, eng.h
    H, W = SIZES[0]
    fr, ids, _ = _case((H, W), 2, 1)
    frd, idsd = torch.from_numpy(fr).to(DEV), torch.from_numpy(ids).to(DEV)
    images = torch.full((1, 3, H, W), SENTINEL, device=DEV)
    labels = torch.full((1, 1, H, W), SENTINEL, device=DEV)
    ids_out = torch.full((1, H, W), 7, dtype=torch.uint8, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                        # noqa: E731
    n_max = CAP + 1
    flips = (ctypes.c_int32 * n_max)()
    two = (ctypes.c_int32 * n_max)(*([2] * n_max))
    lids = (ctypes.c_uint8 * (8 * n_max))(*([1, 2, 3, 4, 5, 6, 7, 8] * n_max))
    mats = (ctypes.c_double * (54 * n_max))(*(list(lucid.IDENTITY) * (9 * n_max)))
    counts = (ctypes.c_int32 * (8 * n_max))(*([77] * (8 * n_max)))
    layers = lambda v: (ctypes.c_int32 * n_max)(*([v] * n_max))        # noqa: E731
    zero_id = (ctypes.c_uint8 * 8)(1, 0, 3, 4, 5, 6, 7, 8)
    twice = (ctypes.c_uint8 * 8)(4, 4, 3, 1, 5, 6, 7, 8)
    twice_late = (ctypes.c_uint8 * 8)(1, 2, 3, 4, 5, 6, 7, 1)

    def bad_matrix(at, v):
        m = (ctypes.c_double * 54)(*(list(lucid.IDENTITY) * 9))
        m[at] = v
        return m
    co = lambda **k: lib.eosvos_lucid_compose_layers(*[k.get(n, d) for n, d in (                    # noqa: E731
        ('e', h), ('frame', P(frd)), ('ids', P(idsd)), ('plate', P(frd)), ('C', 3), ('H', H), ('W', W), ('n', 1), ('flips', flips),
        ('layers', two), ('lids', lids), ('mats', mats), ('target', 1), ('images', P(images)), ('labels', P(labels)),
        ('ids_out', P(ids_out)), ('counts', counts))])
    bad = [
        lambda: co(e=None), lambda: co(frame=None), lambda: co(ids=None), lambda: co(plate=None), lambda: co(flips=None),
        lambda: co(layers=None), lambda: co(lids=None), lambda: co(mats=None), lambda: co(images=None), lambda: co(labels=None),
        lambda: co(C=0), lambda: co(C=65), lambda: co(H=0), lambda: co(W=0), lambda: co(H=4097), lambda: co(W=4097),
        lambda: co(n=0), lambda: co(n=CAP + 1), lambda: co(n=-1), lambda: co(layers=layers(0)), lambda: co(layers=layers(9)),
        lambda: co(layers=layers(-1)), lambda: co(lids=zero_id), lambda: co(lids=twice), lambda: co(lids=twice_late, layers=layers(8)),
        lambda: co(target=0), lambda: co(target=256), lambda: co(target=-1),
        lambda: co(mats=bad_matrix(0, float('nan'))), lambda: co(mats=bad_matrix(8, float('inf'))),
        lambda: co(mats=bad_matrix(17, float('-inf'))),
    ]
    for i, call in enumerate(bad):
        assert call() == 1, i
        assert lib.eosvos_last_error().decode(), i
    torch.cuda.synchronize()
    assert bool((images == SENTINEL).all()) and bool((labels == SENTINEL).all()) and bool((ids_out == 7).all())
    assert list(counts) == [77] * (8 * n_max)                           # nothing was written
    many_i, many_l = torch.empty(CAP, 3, H, W, device=DEV), torch.empty(CAP, 1, H, W, device=DEV)
    assert co(n=CAP, images=P(many_i), labels=P(many_l), ids_out=None, counts=None) == 0       # the cap and both nullable pointers
    assert co(lids=twice_late) == 0                                     # only the layers a sample has are looked at
    assert co(mats=bad_matrix(18, float('nan'))) == 0                   # ... and only their matrices
    with pytest.raises(_ffi.EosvosError):
        _ffi.check(co(n=0))
    ident = {'flip': False, 'Bi': lucid.IDENTITY, 'layers': [(1, lucid.IDENTITY)]}
    for call in (lambda: eng.lucid_compose_layers(frd, idsd, frd, []), lambda: eng.lucid_compose_layers(frd, idsd, frd, [ident] * (CAP + 1)),
                 lambda: eng.lucid_compose_layers(frd, idsd.float(), frd, [ident]), lambda: eng.lucid_compose_layers(frd, idsd[1:], frd, [ident]),
                 lambda: eng.lucid_compose_layers(frd, idsd.cpu(), frd, [ident]), lambda: eng.lucid_compose_layers(frd, idsd, frd, [ident], target_id=0),
                 lambda: eng.lucid_compose_layers(frd, idsd, frd, [dict(ident, layers=[])]),
                 lambda: eng.lucid_compose_layers(frd, idsd, frd, [dict(ident, layers=[(i, lucid.IDENTITY) for i in range(1, 10)])]),
                 lambda: eng.lucid_compose_layers(frd, idsd, frd, [dict(ident, layers=[(0, lucid.IDENTITY)])]),
                 lambda: eng.lucid_compose_layers(frd, idsd, frd[:, 1:].contiguous(), [ident])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_ffi.EosvosError):                               # a repeated id is the library's to refuse
        eng.lucid_compose_layers(frd, idsd, frd, [dict(ident, layers=[(2, lucid.IDENTITY), (2, lucid.IDENTITY)])])


# ---- 6. rules L7-L8: the batch, draw for draw ---------------------------------------------------------------------------------
BATCH_CASES = [('placid', PLACID, 0, [(1, False)] * 3), ('redraw', REDRAW, 5, [(4, False), (2, False), (3, False)]),
               ('fallback', FALLBACK, 1, [(6, False), (8, True), (2, False)])]


@pytest.mark.parametrize('name,prm,seed,tries', BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
def test_batch_equals_the_twin_draw_for_draw(name, prm, seed, tries):
    fr, t, others = scene()
    him, hlb, hrec = ll.batch_host(fr, t, others, prm, L2, 3, random.Random(seed))
    assert [(r['tries'], r['fallback']) for r in hrec] == tries          # the case is what its name says
    rng = random.Random(seed)
    aug = ll.LayeredAugmenter(_engine(), torch.from_numpy(fr).to(DEV), torch.from_numpy(t).to(DEV),
                              torch.from_numpy(np.stack(others)).to(DEV), prm, L2, rng=rng)
    assert aug.has_object and aug.has_layers and torch.equal(aug.ids.cpu(), torch.from_numpy(ll.layer_map_host(t, others)))
    images, labels, rec = aug.batch(3)
    assert rec == hrec                                                  # parameters, draws, tries, counts, fallbacks
    assert torch.equal(_bits(labels), _bits(torch.from_numpy(hlb)))
    after = random.Random(seed)
    ll.batch_host(fr, t, others, prm, L2, 3, after)
    assert rng.getstate() == after.getstate()
    h64 = ll.batch_host(fr, t, others, prm, L2, 3, random.Random(seed), np.float64)[0]
    err32, err = float(np.abs(him - h64).max()), float((images.cpu().double() - torch.from_numpy(h64)).abs().max())
    print(f'layered batch, {name}: numpy fp32 error {err32:.3e}, kernel error {err:.3e}, allowed {2 * err32:.3e}')
    assert err32 > 0
    assert err <= 2 * err32


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------
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
    from eosvos_amd.evaluate import evaluate_sequence
    model, mo, msd = model_and_optim
    mo.load_state_dict(msd)
    mo.reset()
    cfg = config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS-OnA', 'num_epochs.eval=3', 'eval_online_adapt.num_epochs=1',
                            'eval_online_adapt.step=2'])
    frames, gt = synthetic.synthetic_frames(1, *SMALL, seed=3)
    seq = torch.cat([torch.roll(frames, shifts=4 * i, dims=3) for i in range(4)]).to(DEV)
    g1 = gt[0].float().view(1, *SMALL)
    g2 = torch.zeros_like(g1)
    g2[:, 10:40, 100:150] = 1.0
    g2 = g2 * (g1 == 0)                                                 # a second object beside the first
    assert 0 < int(g1.sum()) and 0 < int(g2.sum())
    L = {'samples': 2}
    with monkeypatch.context() as mp:
        def no_layers(*a, **k):
            raise AssertionError('a layered call on today\'s path')
        mp.setattr(Engine, 'lucid_compose_layers', no_layers)
        outs = [evaluate_sequence(model, mo, msd, seq, [g1, g2], cfg, lucid=L, **kw)
                for kw in ({}, {'layers': None}, {'layers': {'others': 0}})]
    for labels, probs, hist in outs[1:]:                                # off: the run without the keyword, bit for bit
        assert torch.equal(labels, outs[0][0]) and hist == outs[0][2]
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(probs, outs[0][1]))
    labels, probs, hist = evaluate_sequence(model, mo, msd, seq, [g1, g2], cfg, lucid=L, layers={'others': 1})
    for o in range(2):
        assert len(hist[o][0]) == 3 and hist[o][0] != outs[0][2][o][0]                          # round 0 saw other samples
        assert len(hist[o]) == len(outs[0][2][o]) > 1 and all(len(r) for r in hist[o][1:])        # the later stages ran
        assert bool(torch.isfinite(probs[o]).all()) and torch.equal(probs[o][0], 2 * (g1, g2)[o][0].to(DEV))
    assert labels.shape == outs[0][0].shape
    mo.reset()
