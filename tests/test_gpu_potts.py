"""The image-aware pairwise loss `potts` on the MI355X: EOSVOS_LOSS_POTTS through eosvos_potts_loss (caller tensors with their
frames, any frame shape), eosvos_loss[_ignore], eosvos_loss_sum, eosvos_set_loss_potts and the fused step, against the numpy
twin `eosvos_amd.potts.loss_host` (itself held to per-pixel loops by tests/test_potts_host.py).  pytest -m gpu.

Floats: per case err32 is the largest difference between the twin in float32 and in float64 (the loss; elementwise the
gradient), and the device may differ from the float64 twin by 4 x err32 -- tests/test_gpu_crf.py's factor, for its reason: up to
(2r + 1)^2 - 1 contracted products per pixel, summed in another order, with the hardware exp.  Every check prints the measured
error beside the allowance (PARITY lines, pytest -s) before it asserts, and asserts err32 > 0.  Everything else is compared
bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import potts_ref as ref
from eosvos_amd import loss_sum, potts, synthetic
from loss_common import _debug_pointer, dev, dlogits_of, masked_frames, poke_logits

pytestmark = pytest.mark.gpu

FRAME = (112, 176)
DEV = 'cuda:0'
IGN = 255.0
# (images, H, W, r, d): 9 x 35 has one tile seam each way (tiles of 8 x 32); 19 x 70 batch 2 has interior tiles, a Z per image
# and the image stride; at 5 x 40 the window (13 rows) is taller than the frame; the last two have the largest halos (14, 16)
CASES = [(1, 9, 35, 3, 2), (2, 19, 70, 3, 2), (1, 5, 40, 3, 2), (1, 24, 40, 7, 2), (1, 24, 40, 4, 4)]


@pytest.fixture(scope='module')
def weights():
    return synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50')


@pytest.fixture(scope='module')
def eng(weights):
    from eosvos_amd.engine import Engine
    e = Engine('resnet50', *FRAME, max_batch=3, device=DEV)
    e.load_model_state(*weights)
    yield e
    e.close()


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if hasattr(t, 'detach') else np.ascontiguousarray(t, dtype=np.float32)
    return a.reshape(-1).view(np.uint32)


_TWINS = {}


def twins(key, z, img, r, d):
    """(the float64 twin, the float32 twin) of a case at the default sigmas, computed once."""
    if key not in _TWINS:
        _TWINS[key] = (potts.loss_host(z, img, r, d), potts.loss_host(z, img, r, d, dtype=np.float32))
    return _TWINS[key]


def check(tag, loss, grad, key, z, img, r, d, where=None):
    """Device loss / gradient against the float64 twin within 4 x err32: prints the figures, then asserts."""
    (l64, g64), (l32, g32) = twins(key, z, img, r, d)
    grad = np.asarray(grad, dtype=np.float64).reshape(g64.shape)
    err_l = abs(float(l32) - float(l64))
    err_g = float(np.abs(g32.astype(np.float64) - g64).max())
    dl = abs(float(loss) - float(l64))
    dg = float(np.abs(grad - g64)[where].max()) if where is not None else float(np.abs(grad - g64).max())
    print(f'PARITY {tag}: loss {float(loss):.9g} vs {float(l64):.12g} diff {dl:.3e} allowed {4 * err_l:.3e} (err32 {err_l:.3e}); '
          f'dlogits diff {dg:.3e} allowed {4 * err_g:.3e} (err32 {err_g:.3e}, max |g64| {float(np.abs(g64).max()):.3e})')
    assert err_l > 0 and err_g > 0, tag
    assert np.isfinite(float(loss)) and np.isfinite(grad).all(), tag
    assert dl <= 4 * err_l, tag
    assert dg <= 4 * err_g, tag


def fill_scratch_with_nan(e):
    """Every word of the engine's scratch arena (where the partials and scales live) becomes a NaN."""
    ptr, words = _debug_pointer(e, b'ccl_scratch')
    assert ptr.value and words > 0
    nan = torch.full((words,), float('nan'), device=DEV)
    e.synchronize()
    torch.cuda.synchronize()
    assert ctypes.CDLL('libamdhip64.so').hipMemcpy(ptr, ctypes.c_void_p(nan.data_ptr()), ctypes.c_size_t(words * 4), 3) == 0


# ---- caller tensors against the twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('images,H,W,r,d', CASES)
def test_potts_loss_vs_twin(eng, images, H, W, r, d):
    z, img = ref.case(images, H, W, seed=H + W + r)
    zd, xd = dev(z), dev(img)
    loss, grad = eng.potts_loss(zd, xd, window=r, dilation=d)
    check(f'potts_loss B={images} {H}x{W} r={r} d={d}', float(loss), grad.cpu().numpy(), (images, H, W, r, d), z, img, r, d)
    loss2, grad2 = eng.potts_loss(zd, xd, window=r, dilation=d)                 # run to run
    assert np.array_equal(bits(loss), bits(loss2)) and np.array_equal(bits(grad), bits(grad2))
    fill_scratch_with_nan(eng)                                                  # nothing depends on what the scratch held
    loss3, grad3 = eng.potts_loss(zd, xd, window=r, dilation=d)
    assert np.array_equal(bits(loss), bits(loss3)) and np.array_equal(bits(grad), bits(grad3))
    only = torch.full((1,), float('nan'), device=DEV)                           # dlogits_out may be null
    assert eng.lib.eosvos_potts_loss(eng.h, ctypes.c_void_p(zd.data_ptr()), ctypes.c_void_p(xd.data_ptr()), images, H, W, r, d,
                                     ctypes.c_float(0.0), ctypes.c_float(0.0), ctypes.c_void_p(only.data_ptr()), None) == 0
    eng.synchronize()
    assert np.array_equal(bits(only), bits(loss))


def test_one_image_the_sigmas_and_the_closed_cases(eng):
    z, img = ref.case(2, 19, 70, seed=7)
    la, ga = eng.potts_loss(dev(z[1]), dev(img[1]))                              # (H, W) and (3, H, W); the defaults 3, 2, 6, 0.1
    lb, gb = eng.potts_loss(dev(z[1:]), dev(img[1:]), window=3, dilation=2, sigma_xy=6.0, sigma_rgb=0.1)
    assert ga.shape == (19, 70) and np.array_equal(bits(la), bits(lb)) and np.array_equal(bits(ga), bits(gb))
    lc, _ = eng.potts_loss(dev(z[1]), dev(img[1]), sigma_rgb=0.3)
    assert not np.array_equal(bits(la), bits(lc))
    lo, go = eng.potts_loss(dev(z[1]), dev(img[1] + np.float32(0.25)))           # an offset of the frame: differences only
    assert abs(float(lo) - float(la)) <= 1e-4 * float(la)
    l1, g1 = eng.potts_loss(torch.full((1, 1), 0.7, device=DEV), torch.full((3, 1, 1), 0.4, device=DEV))
    assert float(l1) == 0.0 and float(g1) == 0.0                                 # a one-pixel image: Z = 0
    for v in (40.0, -40.0):                                                      # p is 0 or 1 everywhere
        ls, gs = eng.potts_loss(torch.full((19, 70), v, device=DEV), dev(img[0]))
        assert abs(float(ls)) <= 1e-12 and float(gs.abs().max()) <= 1e-12
    bad = z[1].copy()
    bad[3, 5] = np.nan
    ln, _ = eng.potts_loss(dev(bad), dev(img[1]))
    assert np.isnan(float(ln))


# ---- on the engine ---------------------------------------------------------------------------------------------------------
def frame_case(e, seed=5):
    """Batch 3 at the engine's frame size: a real forward of the frames, then the case's logits poked in as its result."""
    z, img = ref.case(3, *FRAME, seed=seed)
    zd, xd = dev(z), dev(img)
    e.forward(xd, want_logits=False)
    poke_logits(e, zd)
    _, y = synthetic.synthetic_frames(3, *FRAME, seed=3)
    return z, img, zd, xd, y.to(DEV)


def test_the_engine_equals_potts_loss_bit_for_bit_and_reads_no_target(eng):
    z, img, zd, xd, masks = frame_case(eng)
    n = z.size
    want_l, want_g = eng.potts_loss(zd, xd, window=2, dilation=1)               # the planar route to the frame
    check('potts_loss at the frame size, r=2 d=1', float(want_l), want_g.cpu().numpy(), 'frame', z, img, 2, 1)
    l0 = eng.loss('potts_2x1', masks)                                            # the engine's padded NHWC copy
    g0 = dlogits_of(eng, n)
    assert np.array_equal(bits(l0), bits(want_l)) and np.array_equal(bits(g0), bits(want_g))
    lk = eng.loss('potts', masks, window=2)                                      # the keyword; the dilation stays the engine's
    assert np.array_equal(bits(lk), bits(l0)) and np.array_equal(bits(dlogits_of(eng, n)), bits(g0))
    # a void label, half the mask void: the same bits, and the void pixels have the twin's gradient, not 0
    half = masks.clone()
    half[:, :, :, FRAME[1] // 2:] = IGN
    lv = eng.loss('potts_2x1', half, ignore=IGN)
    gv = dlogits_of(eng, n)
    assert np.array_equal(bits(lv), bits(l0)) and np.array_equal(bits(gv), bits(g0))
    void = (half.cpu().numpy() == IGN).reshape(3, *FRAME)
    check('the gradient at void pixels', float(lv), gv, 'frame', z, img, 2, 1, where=void)
    g64 = twins('frame', z, img, 2, 1)[0][1]
    assert float(np.abs(gv.reshape(3, *FRAME)[void]).max()) > 0.5 * float(np.abs(g64[void]).max()) > 0
    # the other parameters through the setter
    eng.set_loss_potts(sigma_rgb=0.3)
    ls = eng.loss('potts', masks)
    ws, _ = eng.potts_loss(zd, xd, window=2, dilation=1, sigma_rgb=0.3)
    assert np.array_equal(bits(ls), bits(ws)) and not np.array_equal(bits(ls), bits(l0))
    eng.set_loss_potts(0, 0, 0, 0)                                               # back to the defaults: 3, 2, 6, 0.1
    ld = eng.loss('potts', masks)
    wd, gd = eng.potts_loss(zd, xd)
    assert np.array_equal(bits(ld), bits(wd)) and np.array_equal(bits(dlogits_of(eng, n)), bits(gd))
    fill_scratch_with_nan(eng)
    ld2 = eng.loss('potts', masks)
    assert np.array_equal(bits(ld2), bits(ld)) and np.array_equal(bits(dlogits_of(eng, n)), bits(gd))


def test_a_sum_with_the_kind_is_the_combine_of_its_terms(eng):
    z, img, zd, xd, masks = frame_case(eng)
    n = z.size
    eng.set_loss_potts(0, 0, 0, 0)
    ls = eng.loss('cross_entropy+0.1*potts', masks)
    gs = dlogits_of(eng, n)
    terms = eng.last_loss_terms()
    lc = eng.loss('cross_entropy', masks)
    gc = dlogits_of(eng, n)
    lp = eng.loss('potts', masks)
    gp = dlogits_of(eng, n)
    assert np.array_equal(bits(np.float32(terms)), np.concatenate([bits(lc), bits(lp)]))
    w = loss_sum.parse('cross_entropy+0.1*potts')[1][0]
    wl, wg = loss_sum.combine_host([float(lc), float(lp)], [gc, gp], [1.0, w])
    assert np.array_equal(bits(ls), bits(np.float32([wl]))) and np.array_equal(bits(gs), bits(wg))
    with pytest.raises(ValueError):
        eng.loss('potts_2+0.5*potts_3', masks)
    # the per-frame metric of run_frames, which holds the frame: the terms' own values under the sum's rule
    lf = eng.loss_of_framed('cross_entropy+0.1*potts', zd[:1], masks[:1], xd[:1])
    c1, p1 = eng.loss_of('cross_entropy', zd[:1], masks[:1]), eng.potts_loss(zd[:1], xd[:1])[0]
    assert np.array_equal(bits(lf), bits(np.float32([loss_sum.combine_host([float(c1), float(p1)], None, [1.0, w])[0]])))
    assert np.array_equal(bits(eng.loss_of_framed('dice', zd[:1], masks[:1], xd[:1])), bits(eng.loss_of('dice', zd[:1], masks[:1])))


def test_cross_entropy_keeps_the_bits_of_an_engine_that_never_saw_the_kind(eng, weights):
    """The unchanged kinds through their existing entry points, on a fresh engine that never evaluates `potts`, against this
    engine between two `potts` calls; the fresh engine also shows that a loss call before any forward fails."""
    from eosvos_amd.engine import Engine
    z, img, zd, xd, masks = frame_case(eng)
    n = z.size
    p1 = eng.loss('potts', masks)
    ce, gce = eng.loss('cross_entropy', masks), dlogits_of(eng, n)
    dice, gdice = eng.loss('dice', masks), dlogits_of(eng, n)
    p2 = eng.loss('potts', masks)
    assert np.array_equal(bits(p1), bits(p2))
    fresh = Engine('resnet50', *FRAME, max_batch=3, device=DEV)
    try:
        fresh.load_model_state(*weights)
        for name in ('potts', 'cross_entropy+0.1*potts'):
            with pytest.raises(RuntimeError, match='forward'):                   # no forward yet: no frames to read
                fresh.loss(name, masks)
        with pytest.raises(RuntimeError):
            fresh.backward_step()                                                # ... and it left no gradient
        frame_case(fresh)
        cb, gcb = fresh.loss_bce(masks), dlogits_of(fresh, n)                    # eosvos_loss_bce
        cf, gcf = fresh.loss('cross_entropy', masks), dlogits_of(fresh, n)       # eosvos_loss
        df, gdf = fresh.loss('dice', masks), dlogits_of(fresh, n)
    finally:
        fresh.close()
    for a, b in ((cb, gcb), (cf, gcf)):
        assert np.array_equal(bits(ce), bits(a)) and np.array_equal(bits(gce), bits(b))
    assert np.array_equal(bits(dice), bits(df)) and np.array_equal(bits(gdice), bits(gdf))


def test_one_finetune_step_under_the_sum(eng, weights):
    xd, yd, ym = masked_frames(4, FRAME, 0.3)
    eng.load_model_state(*weights)
    eng.set_loss_potts(0, 0, 0, 0)
    before = eng.get_params().clone()
    eng.set_loss('cross_entropy+0.1*potts', ignore=IGN)
    try:
        loss = eng.finetune_step(xd, ym)
        terms = eng.last_loss_terms()
        after = eng.get_params().clone()
    finally:
        eng.set_loss('cross_entropy')
        eng.load_model_state(*weights)
    print(f'PARITY finetune_step under cross_entropy+0.1*potts: loss {loss}, terms {terms}')
    assert np.isfinite(loss) and len(terms) == 2 and 0 < terms[1] < 1
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)


@pytest.mark.parametrize('frozen', [False, True])
def test_fused_steps_equal_the_separate_calls_and_meta_grad_runs(eng, weights, frozen):
    """set_loss(sum with potts, ignore=v) + finetune_step == forward -> loss -> backward_step, bit for bit, also with the frozen
    encoder (whose forward still leaves the frames); meta_grad runs under the sum."""
    from eosvos_amd import topology
    xd, yd, ym = masked_frames(6, FRAME, 0.3)
    name = 'cross_entropy+0.1*potts_2x1'
    eng.load_model_state(*weights)
    eng.set_trainable_from(topology.trainable_from('resnet50', False) if frozen else 0)
    eng.set_loss(name, ignore=IGN)
    try:
        fused = [eng.finetune_step(xd, ym) for _ in range(2)]
        p_fused = eng.get_params().clone()
        eng.load_model_state(*weights)
        sep = []
        for _ in range(2):
            eng.forward(xd, want_logits=False)
            sep.append(float(eng.loss(name, ym, ignore=IGN)))
            eng.backward_step()
        p_sep = eng.get_params().clone()
        ml, terms, flat = 0.0, [0.0, 0.0], torch.ones(1, device=DEV)
        if not frozen:
            eng.load_model_state(*weights)
            eng.meta_task_begin()
            eng.finetune_step(xd, ym, accumulate=True)
            flat = torch.zeros(eng.n_lr + eng.n_param, device=DEV)
            ml = eng.meta_grad(xd, ym, flat)
            terms = eng.last_loss_terms()
    finally:
        eng.set_loss('cross_entropy')
        eng.set_loss_potts(0, 0, 0, 0)
        eng.set_trainable_from(0)
        eng.load_model_state(*weights)
    assert np.array_equal(bits(np.float32(fused)), bits(np.float32(sep))), (fused, sep)
    assert torch.equal(p_fused, p_sep) and fused[1] != fused[0]
    assert np.isfinite(ml) and len(terms) == 2 and bool(torch.isfinite(flat).all()) and float(flat.abs().max()) > 0


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched_and_the_engine_usable(eng):
    z, img, zd, xd, masks = frame_case(eng)
    H, W, B = 9, 11, 2
    zs, xs = torch.zeros(B, H, W, device=DEV), torch.rand(B, 3, H, W, device=DEV)
    loss = torch.full((1,), 7.5, device=DEV)
    grad = torch.full((B, H, W), 7.5, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f = ctypes.c_float
    L = eng.lib.eosvos_potts_loss
    ok = (eng.h, p(zs), p(xs), B, H, W, 3, 2, f(6.0), f(0.1), p(loss), p(grad))
    changes = [{0: None}, {1: None}, {2: None}, {10: None}, {3: 0}, {3: 65536}, {4: 0}, {4: 4097}, {5: 0}, {5: 4097},
               {6: -1}, {6: 8}, {7: -1}, {7: 5}, {6: 5, 7: 4}, {6: 6, 7: 3},    # (5 * 4 and 6 * 3 are more than 16)
               {8: f(-1.0)}, {8: f(float('nan'))}, {8: f(float('inf'))}, {9: f(-0.1)}, {9: f(float('nan'))}, {9: f(float('inf'))}]
    for change in changes:
        assert L(*[change.get(i, v) for i, v in enumerate(ok)]) != 0 and eng.lib.eosvos_last_error(), change
    S = eng.lib.eosvos_set_loss_potts
    for args in ((8, 0, 0.0, 0.0), (-1, 0, 0.0, 0.0), (0, 5, 0.0, 0.0), (0, -1, 0.0, 0.0), (5, 4, 0.0, 0.0), (6, 3, 0.0, 0.0),
                 (0, 0, -1.0, 0.0), (0, 0, float('nan'), 0.0), (0, 0, 0.0, float('inf')), (0, 0, 0.0, -0.1)):
        assert S(eng.h, args[0], args[1], f(args[2]), f(args[3])) != 0 and eng.lib.eosvos_last_error(), args
    for kw in ({'window': 8}, {'window': -1}, {'window': 2.5}, {'dilation': 5}, {'window': 5, 'dilation': 4}, {'sigma_xy': -1.0},
               {'sigma_rgb': float('nan')}, {'sigma_rgb': float('inf')}):
        with pytest.raises(ValueError):
            eng.set_loss_potts(**kw)
        with pytest.raises(ValueError):
            eng.potts_loss(zs, xs, **kw)
    with pytest.raises(ValueError):
        eng.loss('potts', masks, window=8)
    with pytest.raises(ValueError):
        eng.loss('potts', masks, radius=4)
    eng.synchronize()
    assert (loss == 7.5).all() and (grad == 7.5).all()
    # kinds 7 and 11 are still unknown
    for kind in (7, 11):
        assert eng.lib.eosvos_set_loss(eng.h, kind) != 0 and b'unknown loss kind' in eng.lib.eosvos_last_error()
        assert eng.lib.eosvos_loss(eng.h, kind, p(masks), 3, None) != 0 and b'unknown loss kind' in eng.lib.eosvos_last_error()
    # no frames travel with caller tensors through these entry points
    for name in ('potts', 'potts_2x1', 'cross_entropy+0.1*potts'):
        with pytest.raises(RuntimeError, match='potts_loss'):
            eng.loss_of(name, zd[0], masks[0])
        with pytest.raises(RuntimeError, match='potts_loss'):
            eng.loss_grad_of(name, zd[0], masks[0])
    # still usable, with the settings it had
    eng.set_loss_potts(0, 0, 0, 0)
    assert L(*ok) == 0
    eng.synchronize()
    assert float(loss) == 0.25 and bool(torch.isfinite(grad).all())              # z = 0: every pair costs 1/4 of its kernel
    la = eng.loss('potts', masks)
    wa, _ = eng.potts_loss(zd, xd)
    assert np.array_equal(bits(la), bits(wa))
