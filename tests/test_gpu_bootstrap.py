"""The bootstrapped (hard-pixel) cross-entropy on the MI355X: EOSVOS_LOSS_BOOTSTRAPPED_BCE through eosvos_loss[_ignore],
eosvos_loss_tensors[_ignore], eosvos_set_loss_bootstrap and the fused entry points, against the numpy twin
`eosvos_amd.bootstrap.loss_host` (itself held to the plain loops of tests/bootstrap_ref.py by tests/test_bootstrap_host.py).
pytest -m gpu.

Bounds: the project's BCE bounds (test_gpu_parity.py / test_gpu_loss_ignore.py: the same expressions, a mean of k <= n terms):
loss within 2e-6 * max(1, |loss|) of the fp64 twin, dL/dlogits within 1e-4 of max |dL/dlogits| + 1e-10.  The selection itself
is exact: the gradient is exactly +0 wherever the twin's weight is 0 and at every void pixel, and (all cases here keep
|z| <= 8, where no kept pixel's fp32 gradient can vanish) non-zero wherever the twin's weight is not.  Every check prints its
measured margin (MARGIN lines, pytest -s) before it asserts.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from eosvos_amd import bootstrap, synthetic
from loss_common import dev, dlogits_of, dlogits_raw, masked_frames, poke_logits, void_mask

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (96, 160)
DEV = 'cuda:0'
IGN = 255.0
NAME = 'bootstrapped_cross_entropy'
LOSS_TOL, DLOGITS_TOL = 2e-6, 1e-4
PATTERNS = ('none', 'all', 'random30', 'block', 'last_valid')            # test_gpu_loss_ignore.py's
FRACTIONS = (1 / 65536, 0.1, 0.25, 1.0)
GRID_CAP = 256                                                          # BOOTSTRAP_BLOCKS (csrc/kernels.h), 256 threads each


@pytest.fixture(scope='module')
def weights():
    return synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50')


@pytest.fixture(scope='module')
def eng(weights):
    """96 x 160, batch 3, after one batch-3 forward: `debug_tensor('dlogits')` then shows all 3 x 96 x 160 elements."""
    from eosvos_amd.engine import Engine
    e = Engine('resnet50', *SMALL, max_batch=3, device=DEV)
    e.load_model_state(*weights)
    x, _ = synthetic.synthetic_frames(3, *SMALL, seed=3)
    e.forward(x.to(DEV), want_logits=False)
    yield e
    e.close()


def make_case(n, pattern, seed):
    rng = np.random.RandomState(seed)
    x = np.clip(3.0 * rng.randn(n), -8, 8).astype(np.float32)
    t = (rng.rand(n) < 0.3).astype(np.float32)
    void = void_mask(n, pattern, rng)
    t[void] = IGN
    return x, t, void


def check(tag, loss, grad, x, t, fraction, ign, sets=1):
    """The device's loss / gradient of logits x, targets t (`sets` sets) against the fp64 twin: prints, then asserts."""
    x, t = np.asarray(x).reshape(sets, -1), np.asarray(t).reshape(sets, -1)
    ref_loss, ref_grad, w, ks = bootstrap.loss_host(x, t, fraction, ignore=ign)
    grad, ref_grad, w = np.asarray(grad).reshape(-1), ref_grad.reshape(-1), w.reshape(-1)
    gmax = float(np.abs(ref_grad).max())
    dl, dg = abs(loss - float(ref_loss)), float(np.abs(grad - ref_grad).max())
    print(f'MARGIN {tag}: k {ks} loss {loss:.9g} vs {float(ref_loss):.12g} diff {dl:.2e} (allowed {LOSS_TOL * max(1.0, abs(ref_loss)):.2e}); '
          f'dlogits diff {dg:.2e} (allowed {DLOGITS_TOL * gmax + 1e-10:.2e}); kept {int((grad != 0).sum())} twin {int((w != 0).sum())}')
    assert np.isfinite(loss) and np.isfinite(grad).all(), tag
    off = w == 0                                             # dropped and void pixels
    assert not grad[off].any() and not np.signbit(grad[off]).any(), f'{tag}: the gradient of a dropped or void pixel is not +0'
    assert np.array_equal(grad != 0, w != 0), f'{tag}: the kept pixels differ from the twin\'s'
    assert dl <= LOSS_TOL * max(1.0, abs(float(ref_loss))), tag
    assert dg <= DLOGITS_TOL * gmax + 1e-10, tag
    return ks


# ---- one set against the twin --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('fraction', FRACTIONS)
@pytest.mark.parametrize('n', [1, 2, 255, 257, 769, 4097])
def test_one_set_vs_twin(eng, n, fraction, pattern):
    x, t, void = make_case(n, pattern, seed=n + 7 * PATTERNS.index(pattern))
    ign = None if pattern == 'none' else IGN
    loss = float(eng.loss_of(NAME, dev(x), dev(t), ignore=ign, fraction=fraction))
    ks = check(f'n={n} f={fraction:.6f} {pattern}', loss, dlogits_of(eng, n), x, t, fraction, ign)
    assert ks == [bootstrap.k_of(int((~void).sum()), fraction)]
    if pattern == 'all':
        assert loss == 0.0


# ---- the selection's hard cases ------------------------------------------------------------------------------------------
def hard_case(name):
    """(logits, targets): targets 0 make the key the logit itself."""
    rng = np.random.RandomState(11)
    n = 769
    t = np.zeros(n, dtype=np.float32)
    if name == 'all_equal':
        x = np.full(n, 0.75, dtype=np.float32)
    elif name == 'ties_across_a_block_seam':                 # 100 above, 121 tied over elements 200 .. 320: k = 192, r = 92 < T
        x = -1.0 - rng.rand(n).astype(np.float32)
        x[400:500] = 2.0 + rng.rand(100).astype(np.float32)
        x[200:321] = 1.0
    elif name == 'last_10_bits':                             # 1 + i 2^-23: equal in the top 22 bits
        n = 1024
        x = (np.float32(1) + rng.permutation(n).astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
        t = np.zeros(n, dtype=np.float32)
    elif name == 'middle_11_bits':                           # 1 + j 2^-13: equal in the top 11 bits and in the last 10
        n = 2048
        x = (np.float32(1) + rng.permutation(n).astype(np.float32) * np.float32(2.0 ** -13)).astype(np.float32)
        t = np.zeros(n, dtype=np.float32)
    elif name == 'around_zero':
        vals = np.array([-1.0, -1e-30, -1e-45, -0.0, 0.0, 1e-45, 1e-30, 1.0], dtype=np.float32)
        x = vals[rng.randint(0, len(vals), n)]
        t = (rng.rand(n) < 0.5).astype(np.float32)
    else:
        raise KeyError(name)
    return x, t


@pytest.mark.parametrize('fraction', [0.1, 0.25])
@pytest.mark.parametrize('name', ['all_equal', 'ties_across_a_block_seam', 'last_10_bits', 'middle_11_bits', 'around_zero'])
def test_hard_cases_of_the_selection(eng, name, fraction):
    x, t = hard_case(name)
    n = x.size
    loss = float(eng.loss_of(NAME, dev(x), dev(t), fraction=fraction))
    grad = dlogits_of(eng, n)
    ks = check(f'{name} f={fraction}', loss, grad, x, t, fraction, None)
    if name == 'all_equal':                                  # T = n: every weight k / n, the loss the single BCE value
        bce = max(0.75, 0.0) + np.log1p(np.exp(-0.75))
        assert abs(loss - bce) <= LOSS_TOL * max(1.0, bce)
        assert (grad != 0).all() and len(set(grad.view(np.uint32).tolist())) == 1
    if name == 'ties_across_a_block_seam' and fraction == 0.25:
        assert ks == [192] and len(set(grad[200:321].view(np.uint32).tolist())) == 1 and (grad[200:321] != 0).all()


def test_a_nan_logit_on_a_valid_pixel_makes_the_loss_nan(eng):
    x, t, _ = make_case(4097, 'random30', seed=5)
    i = int(np.flatnonzero(t != IGN)[100])
    x[i] = np.nan
    assert np.isnan(float(eng.loss_of(NAME, dev(x), dev(t), ignore=IGN, fraction=0.25)))
    assert np.isnan(float(eng.loss_of(NAME, dev(x), dev(np.where(t == IGN, 0, t).astype(np.float32)), fraction=0.25)))


def test_non_finite_logits_at_void_pixels_never_reach_the_loss(eng):
    n = 4097
    x, t, void = make_case(n, 'random30', seed=5)
    clean = x.copy()
    clean[void] = 0.0
    bad = x.copy()
    bad[void] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[np.arange(int(void.sum())) % 3]
    a = eng.loss_of(NAME, dev(clean), dev(t), ignore=IGN, fraction=0.25).cpu().numpy()
    ga = dlogits_of(eng, n).copy()
    b = eng.loss_of(NAME, dev(bad), dev(t), ignore=IGN, fraction=0.25).cpu().numpy()
    gb = dlogits_of(eng, n)
    assert np.isfinite(b).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (a, b)
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
    check('void NaN / inf', float(b[0]), gb, clean, t, 0.25, IGN)


# ---- a second trip of the grid -------------------------------------------------------------------------------------------
BIG = (296, 296)                                        # batch 3: the engine's scratch holds BIG_N elements
BIG_N = GRID_CAP * 256 + 257                            # the smallest set whose grid-stride loops run twice, with a ragged tail


def test_second_trip_of_the_grid(weights):
    from eosvos_amd.engine import Engine
    e = Engine('resnet50', *BIG, max_batch=3, device=DEV)
    try:
        x, t, void = make_case(BIG_N, 'random30', seed=53)
        loss = float(e.loss_of(NAME, dev(x), dev(t), ignore=IGN, fraction=0.25))
        check(f'n={BIG_N} random30', loss, dlogits_raw(e, BIG_N), x, t, 0.25, IGN)
    finally:
        e.close()


# ---- batch 3 through eosvos_loss / eosvos_loss_ignore --------------------------------------------------------------------
def test_batch3_k_per_image(eng):
    """Image 0 30 % void, image 1 all void, image 2 without void: k per image, the mean over all 3 images."""
    P = SMALL[0] * SMALL[1]
    x, t, void = make_case(3 * P, 'random30', seed=17)
    t, void = t.reshape(3, P), void.reshape(3, P)
    t[1], void[1] = IGN, True
    t[2] = np.where(void[2], 0.0, t[2])
    void[2] = False
    poke_logits(eng, dev(x))
    loss = float(eng.loss(NAME, dev(t).view(3, 1, *SMALL), ignore=IGN, fraction=0.25))
    ks = check('batch 3', loss, dlogits_of(eng, 3 * P), x, t, 0.25, IGN, sets=3)
    assert ks == [bootstrap.k_of(int((~void[0]).sum()), 0.25), 0, bootstrap.k_of(P, 0.25)] and ks[0] != ks[2]


def test_without_a_void_pixel_the_bits_are_those_of_the_plain_call(eng):
    n = 3 * SMALL[0] * SMALL[1]
    x, t, _ = make_case(n, 'none', seed=41)
    xd, td = dev(x), dev(t)
    eng.set_loss_bootstrap(0.25)
    for m in (4097, n):
        a = eng.loss_of(NAME, xd[:m], td[:m]).cpu().numpy().view(np.uint32)
        ga = dlogits_of(eng, m).view(np.uint32).copy()
        b = eng.loss_of(NAME, xd[:m], td[:m], ignore=IGN).cpu().numpy().view(np.uint32)
        gb = dlogits_of(eng, m).view(np.uint32)
        assert np.array_equal(a, b) and np.array_equal(ga, gb), m
    poke_logits(eng, xd)
    masks = td.view(3, 1, *SMALL)
    a = eng.loss(NAME, masks)
    ga = dlogits_of(eng, n).view(np.uint32).copy()
    b = eng.loss(NAME, masks, ignore=-1.0)
    gb = dlogits_of(eng, n).view(np.uint32)
    assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)) and np.array_equal(ga, gb)
    check('batch 3 plain', float(a), dlogits_of(eng, n), x, t, 0.25, None, sets=3)


# ---- reproducibility -----------------------------------------------------------------------------------------------------
def repro_case():
    return make_case(3 * SMALL[0] * SMALL[1] - 3, 'random30', seed=33)


def repro_digest(e, n, loss):
    return [int(loss.cpu().numpy().view(np.uint32)[0]), hashlib.sha256(dlogits_raw(e, n).tobytes()).hexdigest()]


CHILD = r'''
import json, sys
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from eosvos_amd.engine import Engine
import test_gpu_bootstrap as T
eng = Engine('resnet50', 96, 160, max_batch=3, device='cuda:0')
x, t, _ = T.repro_case()
loss = eng.loss_of(T.NAME, torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda(), ignore=T.IGN)
print(json.dumps(T.repro_digest(eng, x.size, loss)))
eng.close()
'''


def test_two_evaluations_are_bit_identical_also_from_dirty_or_nan_filled_scratch(eng):
    x, t, _ = repro_case()
    xd, td = dev(x), dev(t)
    eng.set_loss_bootstrap(0.25)
    got = []
    for between in (None, 'dice', 'lovasz_hinge'):
        if between:
            eng.loss_of(between, xd, td, ignore=IGN)                   # another kind through the gradient buffer in between
        got.append(repro_digest(eng, x.size, eng.loss_of(NAME, xd, td, ignore=IGN)))
    assert got[0] == got[1] == got[2], got
    env = dict(os.environ, EOSVOS_MODE_GUARD='0', EOSVOS_DEBUG_FILL='7fc00000')      # every engine buffer starts out as NaN words
    p = subprocess.run([sys.executable, '-c', CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [l for l in p.stdout.splitlines() if l.startswith('[')]
    assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert json.loads(lines[-1]) == got[0]


# ---- the setter ----------------------------------------------------------------------------------------------------------
def kept(e, xd, td, n, **kw):
    e.loss_of(NAME, xd, td, **kw)
    return int((dlogits_raw(e, n) != 0).sum())


def test_the_setter(eng, weights):
    from eosvos_amd.engine import Engine
    n = 4000                                                 # distinct keys: the number of kept pixels is k
    rng = np.random.RandomState(2)
    x = np.clip(rng.permutation(n).astype(np.float32) * np.float32(1e-3) - 2.0, -8, 8).astype(np.float32)
    t = np.zeros(n, dtype=np.float32)
    xd, td = dev(x), dev(t)
    eng.set_loss_bootstrap(0.1)
    assert kept(eng, xd, td, n) == bootstrap.k_of(n, 0.1) == 400
    for bad in (0.0, -0.25, 1.5, float('nan'), float('inf')):
        assert eng.lib.eosvos_set_loss_bootstrap(eng.h, ctypes.c_float(bad)) != 0
        assert b'fraction' in eng.lib.eosvos_last_error()
        with pytest.raises(ValueError):
            eng.set_loss_bootstrap(bad)
        with pytest.raises(ValueError):
            eng.loss_of(NAME, xd, td, fraction=bad)
    assert kept(eng, xd, td, n) == 400                      # still usable, the fraction unchanged
    other = Engine('resnet50', *SMALL, max_batch=3, device=DEV)
    try:
        assert kept(other, xd, td, n) == bootstrap.k_of(n, 0.25) == 1000      # a new engine evaluates at 0.25
        other.load_model_state(*weights)
        other.alias_state(eng)
        assert kept(other, xd, td, n) == 1000               # ... also while it aliases the state of an engine set to 0.1
        assert kept(eng, xd, td, n) == 400
        other.unalias_state()
    finally:
        other.close()
    assert kept(eng, xd, td, n, fraction=0.5) == 2000       # the keyword, the suffix and the setter all change k at once
    assert kept(eng, xd, td, n) == 2000
    e2 = eng.loss_of(NAME + '_1', xd, td)
    assert kept(eng, xd, td, n) == 40 and np.isfinite(float(e2))
    eng.set_loss_bootstrap(0.25)
    assert eng.lib.eosvos_set_loss(eng.h, 7) != 0 and b'unknown loss kind' in eng.lib.eosvos_last_error()


# ---- integration ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ign', [None, IGN])
def test_fused_step_equals_the_separate_calls(eng, weights, ign):
    """set_loss('bootstrapped_cross_entropy_25', ignore=v) + finetune_step == forward -> loss -> backward_step, bit for bit."""
    xd, yd, ym = masked_frames(4, SMALL, 0.3)
    masks = yd if ign is None else ym
    eng.load_model_state(*weights)
    eng.set_loss_bootstrap(0.5)                              # the suffix below must win over what the engine held
    eng.set_loss(NAME + '_25', ignore=ign)
    try:
        fused = [eng.finetune_step(xd, masks) for _ in range(2)]
        p_fused = eng.get_params().clone()
    finally:
        eng.set_loss('cross_entropy')
    eng.load_model_state(*weights)
    sep = []
    for _ in range(2):
        eng.forward(xd, want_logits=False)
        sep.append(float(eng.loss(NAME, masks, ignore=ign, fraction=0.25)))
        eng.backward_step()
    p_sep = eng.get_params()
    eng.load_model_state(*weights)
    assert np.array_equal(np.float32(fused).view(np.uint32), np.float32(sep).view(np.uint32)), (fused, sep)
    assert torch.equal(p_fused, p_sep)
    logits = eng.forward(xd).cpu().numpy()                   # the first step's loss is the twin's on the first logits
    ref, _, _, ks = bootstrap.loss_host(logits.reshape(3, -1), masks.cpu().numpy().reshape(3, -1), 0.25, ignore=ign)
    print(f'MARGIN fused step ignore={ign}: losses {fused}; twin on the first logits {float(ref):.9g}, k {ks}')
    assert abs(fused[0] - float(ref)) <= LOSS_TOL * max(1.0, abs(float(ref)))


def test_meta_grad_and_the_matrix_mode_guard_run_under_the_kind(eng, weights):
    xd, yd, ym = masked_frames(8, SMALL, 0.3)
    eng.load_model_state(*weights)
    eng.set_loss(NAME, ignore=IGN, fraction=0.25)
    try:
        eng.meta_task_begin()
        eng.finetune_step(xd, ym, accumulate=True)
        flat = torch.zeros(eng.n_lr + eng.n_param, device=DEV)
        ml = eng.meta_grad(xd, ym, flat)
        logits = eng.debug_tensor('logits').cpu().numpy()
        ref, _, _, ks = bootstrap.loss_host(logits.reshape(3, -1), ym.cpu().numpy().reshape(3, -1), 0.25, ignore=IGN)
        print(f'MARGIN meta_grad: {ml} vs {float(ref)} k {ks}')
        assert abs(ml - float(ref)) <= LOSS_TOL * max(1.0, abs(float(ref)))
        assert bool(torch.isfinite(flat).all()) and float(flat.abs().max()) > 0
        eng.load_model_state(*weights)
        eng.set_loss(NAME, fraction=0.25)
        mode = eng.verify_matrix_mode(xd, yd)
        print(f'MARGIN verify_matrix_mode under {NAME}: {mode} {getattr(eng, "last_step_check", None)}')
        assert mode == 'f16x3'
    finally:
        eng.set_loss('cross_entropy')
        eng.load_model_state(*weights)


def test_compute_loss_keyword_equals_suffix(eng, weights):
    from eosvos_amd.helper_func import compute_loss
    xd, yd, _ = masked_frames(12, SMALL, 0.3)
    eng.load_model_state(*weights)
    out = eng.forward(xd)
    out._eosvos_engine = eng
    n = out.numel()
    a = compute_loss(NAME, out, yd, {'fraction': 0.1})
    ga = dlogits_of(eng, n).view(np.uint32).copy()
    eng.set_loss_bootstrap(0.25)
    b = compute_loss(NAME + '_10', out, yd)
    gb = dlogits_of(eng, n).view(np.uint32)
    assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)) and np.array_equal(ga, gb)
    check('compute_loss', float(a), dlogits_of(eng, n), out.cpu().numpy(), yd.cpu().numpy(), 0.1, None, sets=3)
    per = compute_loss(NAME + '_10', out, yd, {'batch_average': False})
    ref = [float(bootstrap.loss_host(out[i].cpu().numpy().reshape(-1), yd[i].cpu().numpy().reshape(-1), 0.1)[0]) for i in range(3)]
    assert per.shape == (3,) and np.abs(per.cpu().numpy() - ref).max() <= LOSS_TOL * max(1.0, max(ref))
    with pytest.raises(ValueError):
        compute_loss(NAME + '_10', out, yd, {'fraction': 0.25})
