"""The topology-aware centreline loss `cldice` on the MI355X: EOSVOS_LOSS_CLDICE through eosvos_soft_skeleton and
eosvos_cldice_loss (caller tensors, any frame shape), eosvos_loss[_ignore], eosvos_loss_sum[_tensors], eosvos_set_loss_cldice
and the fused steps, against the numpy twins of `eosvos_amd.cldice` (themselves held to per-pixel loops and to torch autograd of
the published implementation by tests/test_cldice_host.py).  pytest -m gpu.

The selection chain is exact: `soft_skeleton` of a plane must equal the float32 twin bit for bit.  Floats: per case err32 is the
largest difference between the twin in float32 and in float64 (the loss; elementwise the gradient), and the device may differ
from the float64 twin by 4 x err32 (tests/test_gpu_potts.py's rule: the device sums in another order and in fp64, and its
exp rounds differently from numpy's), with a floor of 8 ulp (fp32) of the loss, and of max |g64| for the gradient
(tests/test_gpu_surface.py's margin).  Every check prints the measured error beside the allowance (PARITY lines, pytest -s)
before it asserts, and asserts err32 > 0.  Everything else is compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import cldice_ref as ref
from eosvos_amd import cldice, loss_sum, synthetic, topology
from loss_common import _debug_pointer, dev, dlogits_of, masked_frames, poke_logits

pytestmark = pytest.mark.gpu

FRAME = (112, 176)
DEV = 'cuda:0'
IGN = ref.IGN
VOIDS = ['none', 'ring', 'speckle']


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


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def fill_scratch_with_nan(e):
    """Every word of the engine's scratch arena (where the caller-tensor entries keep their planes) becomes a NaN."""
    ptr, words = _debug_pointer(e, b'ccl_scratch')
    assert ptr.value and words > 0
    nan = torch.full((words,), float('nan'), device=DEV)
    e.synchronize()
    torch.cuda.synchronize()
    assert ctypes.CDLL('libamdhip64.so').hipMemcpy(ptr, ctypes.c_void_p(nan.data_ptr()), ctypes.c_size_t(words * 4), 3) == 0


_INPUTS, _TWINS = {}, {}


def inputs(images, H, W, void):
    """(logits, targets, the void label or None) of a case, computed once."""
    key = (images, H, W, void)
    if key not in _INPUTS:
        z, y = ref.case(images, H, W, seed=H + W)
        if void == 'ring':
            z, y, _ = ref.void_ring(z, y)
        elif void == 'speckle':
            y = ref.speckle(y, seed=H)
        _INPUTS[key] = (z, y, None if void == 'none' else IGN)
    return _INPUTS[key]


def twins(key, z, y, depth, ign):
    """(the float64 twin, the float32 twin) of a case, computed once."""
    if key not in _TWINS:
        _TWINS[key] = (cldice.loss_host(z, y, depth, ign), cldice.loss_host(z, y, depth, ign, dtype=np.float32))
    return _TWINS[key]


def check(tag, loss, grad, key, z, y, depth, ign):
    """Device loss / gradient against the float64 twin within max(4 x err32, 8 ulp32): prints the figures, then asserts."""
    (l64, g64), (l32, g32) = twins(key, z, y, depth, ign)
    grad = np.asarray(grad, dtype=np.float64).reshape(g64.shape)
    gmax = float(np.abs(g64).max())
    err_l = abs(float(l32) - float(l64))
    err_g = float(np.abs(g32.astype(np.float64) - g64).max())
    tol_l, tol_g = max(4 * err_l, 8 * ulp32(float(l64))), max(4 * err_g, 8 * ulp32(gmax))
    dl, dg = abs(float(loss) - float(l64)), float(np.abs(grad - g64).max())
    print(f'PARITY {tag}: loss {float(loss):.9g} vs {float(l64):.12g} diff {dl:.3e} allowed {tol_l:.3e} (err32 {err_l:.3e}, '
          f'ratio {dl / tol_l:.3f}); dlogits diff {dg:.3e} allowed {tol_g:.3e} (err32 {err_g:.3e}, max |g64| {gmax:.3e}, '
          f'ratio {dg / tol_g:.3f})')
    assert err_l > 0 and err_g > 0, tag
    assert np.isfinite(float(loss)) and np.isfinite(grad).all(), tag
    assert dl <= tol_l, tag
    assert dg <= tol_g, tag
    if ign is not None:                                                           # exactly +0 at void pixels
        void = (y == np.float32(ign)).reshape(-1)
        assert void.any() and not bits(np.float32(grad.reshape(-1)[void])).any(), tag


# ---- caller tensors against the twins ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('void', VOIDS)
@pytest.mark.parametrize('images,H,W,depth', ref.CASES)
def test_soft_skeleton_equals_the_float32_twin_bit_for_bit(eng, images, H, W, depth, void):
    z, y, ign = inputs(images, H, W, void)
    valid = np.ones(y.shape, dtype=bool) if ign is None else y != np.float32(ign)
    p = np.where(valid, cldice.sigmoid_host(np.where(valid, z, 0).astype(np.float32), np.float32)[0], np.float32(0.5))
    masks = None if ign is None else dev(y)
    for name, maps in (('p', p.astype(np.float32)), ('y', y)):
        want = cldice.skeleton_host(maps, depth, ignore=ign, masks=None if ign is None else y)
        got = eng.soft_skeleton(dev(maps), depth, ignore=ign, masks=masks)
        assert got.shape == maps.shape and np.array_equal(bits(got), bits(want)), (name, void)
    if ign is not None:                                                           # the maps themselves carry the void label
        got = eng.soft_skeleton(dev(y), depth, ignore=ign)
        assert np.array_equal(bits(got), bits(cldice.skeleton_host(y, depth, ignore=ign)))
    one = eng.soft_skeleton(dev(y[0]), depth, ignore=ign)                         # (H, W)
    assert one.shape == y.shape[1:] and np.array_equal(bits(one), bits(cldice.skeleton_host(y[0], depth, ignore=ign)))


@pytest.mark.parametrize('void', VOIDS)
@pytest.mark.parametrize('images,H,W,depth', ref.CASES)
def test_cldice_loss_vs_twin(eng, images, H, W, depth, void):
    z, y, ign = inputs(images, H, W, void)
    zd, yd = dev(z), dev(y)
    loss, grad = eng.cldice_loss(zd, yd, depth=depth, ignore=ign)
    check(f'cldice_loss B={images} {H}x{W} k={depth} void={void}', float(loss), grad.cpu().numpy(), (images, H, W, depth, void),
          z, y, depth, ign)
    loss2, grad2 = eng.cldice_loss(zd, yd, depth=depth, ignore=ign)                # run to run
    assert np.array_equal(bits(loss), bits(loss2)) and np.array_equal(bits(grad), bits(grad2))
    fill_scratch_with_nan(eng)                                                    # nothing is read that this call did not write
    loss3, grad3 = eng.cldice_loss(zd, yd, depth=depth, ignore=ign)
    assert np.array_equal(bits(loss), bits(loss3)) and np.array_equal(bits(grad), bits(grad3))
    skel = eng.soft_skeleton(yd, depth, ignore=ign)
    fill_scratch_with_nan(eng)
    assert np.array_equal(bits(skel), bits(eng.soft_skeleton(yd, depth, ignore=ign)))
    only = torch.full((1,), float('nan'), device=DEV)                             # dlogits_out may be null
    v = None if ign is None else ctypes.byref(ctypes.c_float(ign))
    assert eng.lib.eosvos_cldice_loss(eng.h, ctypes.c_void_p(zd.data_ptr()), ctypes.c_void_p(yd.data_ptr()), *z.shape, depth, v,
                                      ctypes.c_void_p(only.data_ptr()), None) == 0
    eng.synchronize()
    assert np.array_equal(bits(only), bits(loss))


def test_the_closed_cases(eng):
    z, y, _ = inputs(2, 19, 37, 'none')
    zd = dev(z)
    for target in (np.zeros_like(y), np.ones_like(y)):                            # an empty and a full target: finite
        l, g = eng.cldice_loss(zd, dev(target), depth=3)
        assert np.isfinite(float(l)) and bool(torch.isfinite(g).all()) and 0 <= float(l) <= 1
    l, g = eng.cldice_loss(zd, torch.full(z.shape, IGN, device=DEV), depth=3, ignore=IGN)
    assert float(l) == 0.0 and not bits(g).any()                                  # no valid pixel: 0 and +0
    for v in (40.0, -40.0):
        l, g = eng.cldice_loss(torch.full(z.shape, v, device=DEV), dev(y), depth=3)
        assert np.isfinite(float(l)) and bool(torch.isfinite(g).all())
    bad = z.copy()
    bad[0, 3, 5] = np.nan
    assert np.isnan(float(eng.cldice_loss(dev(bad), dev(y), depth=3)[0]))
    void = y.copy()
    void[0, 3, 5] = IGN                                                           # a void pixel's logit never reaches the result
    l, g = eng.cldice_loss(dev(bad), dev(void), depth=3, ignore=IGN)
    assert np.isfinite(float(l)) and bool(torch.isfinite(g).all()) and float(g[0, 3, 5]) == 0.0
    la, ga = eng.cldice_loss(zd[1], dev(y[1]))                                    # (H, W), this shape's default depth: 1
    lb, gb = eng.cldice_loss(zd[1:], dev(y[1:]), depth=cldice.default_depth(19, 37))
    assert ga.shape == (19, 37) and np.array_equal(bits(la), bits(lb)) and np.array_equal(bits(ga), bits(gb))


# ---- on the engine -------------------------------------------------------------------------------------------------------------
def frame_case(e, void=False):
    """Batch 3 at the engine's frame size: a real forward, then lattice logits poked in as its result; the case's targets."""
    z, y = ref.case(3, *FRAME, seed=5)
    if void:
        y = ref.speckle(y, seed=9)
    x, _ = synthetic.synthetic_frames(3, *FRAME, seed=3)
    e.forward(x.to(DEV), want_logits=False)
    zd = dev(z)
    poke_logits(e, zd)
    return z, y, zd, dev(y).reshape(3, 1, *FRAME)


@pytest.mark.parametrize('void', [False, True])
def test_the_engine_equals_cldice_loss_bit_for_bit(eng, void):
    z, y, zd, masks = frame_case(eng, void)
    ign = IGN if void else None
    n = z.size
    want_l, want_g = eng.cldice_loss(zd, dev(y), depth=3, ignore=ign)
    check(f'cldice_loss at the frame size, k=3 void={void}', float(want_l), want_g.cpu().numpy(), ('frame', void), z, y, 3, ign)
    eng.set_loss_cldice(7)                                                        # the suffix below must win over what the engine held
    l0 = eng.loss('cldice_3', masks, ignore=ign)
    g0 = dlogits_of(eng, n)
    assert np.array_equal(bits(l0), bits(want_l)) and np.array_equal(bits(g0), bits(want_g))
    lk = eng.loss('cldice', masks, ignore=ign, depth=3)                           # the keyword
    assert np.array_equal(bits(lk), bits(l0)) and np.array_equal(bits(dlogits_of(eng, n)), bits(g0))
    # two evaluations are bit-identical, also with other kinds that need the frame's shape in between
    eng.loss('boundary_f', masks, ignore=ign)
    eng.loss('surface', masks, ignore=ign)
    l1 = eng.loss('cldice', masks, ignore=ign)
    assert np.array_equal(bits(l1), bits(l0)) and np.array_equal(bits(dlogits_of(eng, n)), bits(g0))
    # a depth change takes effect (a deeper one needs a larger scratch), and 0 returns to the default (1 at this frame size)
    l16 = eng.loss('cldice_16', masks, ignore=ign)
    w16, g16 = eng.cldice_loss(zd, dev(y), depth=16, ignore=ign)
    assert np.array_equal(bits(l16), bits(w16)) and np.array_equal(bits(dlogits_of(eng, n)), bits(g16))
    assert not np.array_equal(bits(l16), bits(l0))
    eng.set_loss_cldice(0)
    ld = eng.loss('cldice', masks, ignore=ign)
    wd, gd = eng.cldice_loss(zd, dev(y), ignore=ign)
    w1, _ = eng.cldice_loss(zd, dev(y), depth=cldice.default_depth(*FRAME), ignore=ign)
    assert np.array_equal(bits(ld), bits(wd)) and np.array_equal(bits(dlogits_of(eng, n)), bits(gd))
    assert np.array_equal(bits(wd), bits(w1)) and not np.array_equal(bits(ld), bits(l0))
    # one image through the caller-tensor entries, which take the engine's H * W elements only
    one = eng.loss_of('cldice_3', zd[0], masks[0], ignore=ign)
    o1, og = eng.cldice_loss(zd[0], dev(y[0]), depth=3, ignore=ign)
    assert np.array_equal(bits(one), bits(o1))
    lg, gg = eng.loss_grad_of('cldice_3', zd[0], masks[0], ignore=ign)
    assert np.array_equal(bits(lg), bits(o1)) and np.array_equal(bits(gg), bits(og))
    with pytest.raises(RuntimeError, match='cldice_loss'):
        eng.loss_of('cldice_3', zd[0, :50], masks[0, 0, :50])
    eng.set_loss_cldice(0)


def test_a_sum_with_the_kind_is_the_combine_of_its_terms(eng):
    z, y, zd, masks = frame_case(eng)
    n = z.size
    name = 'dice+0.5*cldice_3'
    ls = eng.loss(name, masks)
    gs = dlogits_of(eng, n)
    terms = eng.last_loss_terms()
    ld = eng.loss('dice', masks)
    gd = dlogits_of(eng, n)
    lc = eng.loss('cldice_3', masks)
    gc = dlogits_of(eng, n)
    assert np.array_equal(bits(np.float32(terms)), np.concatenate([bits(ld), bits(lc)]))
    wl, wg = loss_sum.combine_host([float(ld), float(lc)], [gd, gc], [1.0, 0.5])
    assert np.array_equal(bits(ls), bits(np.float32([wl]))) and np.array_equal(bits(gs), bits(wg))
    # on caller tensors: one image of the engine's frame
    l1, g1 = eng.loss_grad_of(name, zd[0], masks[0])
    terms1 = eng.last_loss_terms()
    d1, dg1 = eng.loss_grad_of('dice', zd[0], masks[0])
    c1, cg1 = eng.cldice_loss(zd[0], dev(y[0]), depth=3)
    wl, wg = loss_sum.combine_host([float(d1), float(c1)], [dg1.cpu().numpy(), cg1.cpu().numpy()], [1.0, 0.5])
    assert np.array_equal(bits(l1), bits(np.float32([wl]))) and np.array_equal(bits(g1), bits(wg))
    assert np.array_equal(bits(np.float32(terms1)), np.concatenate([bits(d1), bits(c1)]))
    assert np.array_equal(bits(eng.loss_of(name, zd[0], masks[0])), bits(l1))
    with pytest.raises(ValueError):
        eng.loss('cldice_2+0.5*cldice_3', masks)
    with pytest.raises(ValueError):
        eng.loss('dice+cldice_3', masks, depth=4)
    with pytest.raises(ValueError):
        eng.loss('dice', masks, depth=4)
    eng.set_loss_cldice(0)


@pytest.mark.parametrize('frozen', [False, True])
def test_fused_steps_equal_the_separate_calls(eng, weights, frozen):
    """set_loss(sum with cldice, ignore=v) + finetune_step == forward -> loss -> backward_step, bit for bit, also with the
    frozen encoder; meta_grad's loss is the unfused loss on the logits it left, bit for bit."""
    xd, yd, ym = masked_frames(6, FRAME, 0.1)
    name = 'dice+0.5*cldice_3'
    eng.load_model_state(*weights)
    eng.set_trainable_from(topology.trainable_from('resnet50', False) if frozen else 0)
    eng.set_loss(name, ignore=IGN)
    try:
        fused = [eng.finetune_step(xd, ym) for _ in range(2)]
        terms = eng.last_loss_terms()
        p_fused = eng.get_params().clone()
        eng.load_model_state(*weights)
        sep = []
        for _ in range(2):
            eng.forward(xd, want_logits=False)
            sep.append(float(eng.loss(name, ym, ignore=IGN)))
            eng.backward_step()
        p_sep = eng.get_params().clone()
        ml, again, flat = 0.0, 0.0, torch.ones(1, device=DEV)
        if not frozen:
            eng.load_model_state(*weights)
            eng.meta_task_begin()
            eng.finetune_step(xd, ym, accumulate=True)
            flat = torch.zeros(eng.n_lr + eng.n_param, device=DEV)
            ml = eng.meta_grad(xd, ym, flat)
            again = float(eng.loss(name, ym, ignore=IGN))                         # on the logits meta_grad's forward left
    finally:
        eng.set_loss('cross_entropy')
        eng.set_loss_cldice(0)
        eng.set_trainable_from(0)
        eng.load_model_state(*weights)
    print(f'PARITY fused steps under {name} frozen={frozen}: losses {fused}, terms {terms}, meta_grad {ml}')
    assert np.array_equal(bits(np.float32(fused)), bits(np.float32(sep))), (fused, sep)
    assert torch.equal(p_fused, p_sep) and fused[1] != fused[0]
    assert len(terms) == 2 and 0 < terms[1] < 1
    assert np.array_equal(bits(np.float32([ml])), bits(np.float32([again])))
    assert np.isfinite(ml) and bool(torch.isfinite(flat).all()) and float(flat.abs().max()) > 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched_and_the_engine_usable(eng):
    z, y, zd, masks = frame_case(eng)
    H, W, B = 9, 11, 2
    zs, ys = torch.zeros(B, H, W, device=DEV), torch.zeros(B, H, W, device=DEV)
    loss = torch.full((1,), 7.5, device=DEV)
    grad = torch.full((B, H, W), 7.5, device=DEV)
    out = torch.full((B, H, W), 7.5, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    inside, nan = ctypes.byref(ctypes.c_float(0.5)), ctypes.byref(ctypes.c_float(float('nan')))
    L, S = eng.lib.eosvos_cldice_loss, eng.lib.eosvos_soft_skeleton
    ok = (eng.h, p(zs), p(ys), B, H, W, 3, None, p(loss), p(grad))
    for change in ({0: None}, {1: None}, {2: None}, {8: None}, {3: 0}, {3: 65536}, {4: 0}, {4: 4097}, {5: 0}, {5: 4097},
                   {6: -1}, {6: 17}, {7: inside}, {7: nan}):
        assert L(*[change.get(i, v) for i, v in enumerate(ok)]) != 0 and eng.lib.eosvos_last_error(), change
    ok_s = (eng.h, p(zs), None, B, H, W, 3, None, p(out))
    for change in ({0: None}, {1: None}, {8: None}, {3: 0}, {4: 4097}, {5: 4097}, {6: -1}, {6: 17}, {7: inside}):
        assert S(*[change.get(i, v) for i, v in enumerate(ok_s)]) != 0 and eng.lib.eosvos_last_error(), change
    for depth in (17, -1):
        assert eng.lib.eosvos_set_loss_cldice(eng.h, depth) != 0 and eng.lib.eosvos_last_error()
    for bad in (17, -1, 2.5, True):
        with pytest.raises(ValueError):
            eng.set_loss_cldice(bad)
        with pytest.raises(ValueError):
            eng.cldice_loss(zs, ys, depth=bad)
        with pytest.raises(ValueError):
            eng.soft_skeleton(ys, bad)
        with pytest.raises(ValueError):
            eng.loss('cldice', masks, depth=bad)
    with pytest.raises(ValueError):
        eng.cldice_loss(zs, ys, ignore=0.5)
    with pytest.raises(ValueError):
        eng.loss('cldice', masks, radius=4)
    with pytest.raises(NotImplementedError):
        eng.set_loss('cldice_17')
    eng.synchronize()
    assert (loss == 7.5).all() and (grad == 7.5).all() and (out == 7.5).all()
    # kinds 7, 11 and 14 are still unknown
    for kind in (7, 11, 14):
        assert eng.lib.eosvos_set_loss(eng.h, kind) != 0 and b'unknown loss kind' in eng.lib.eosvos_last_error()
        assert eng.lib.eosvos_loss(eng.h, kind, p(masks), 3, None) != 0 and b'unknown loss kind' in eng.lib.eosvos_last_error()
    # still usable, with the settings it had
    assert L(*ok) == 0 and S(*ok_s) == 0
    eng.synchronize()
    assert np.isfinite(float(loss)) and bool(torch.isfinite(grad).all()) and not bits(out).any()      # S of an empty map is 0
    la = eng.loss('cldice', masks)
    wa, _ = eng.cldice_loss(zd, dev(y))
    assert np.array_equal(bits(la), bits(wa))
    assert np.isfinite(float(eng.loss('cross_entropy', masks)))
