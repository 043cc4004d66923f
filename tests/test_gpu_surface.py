"""The distance-weighted surface loss on the MI355X: EOSVOS_LOSS_SURFACE through eosvos_surface_weights / eosvos_surface_loss
(any frame shape), eosvos_loss[_ignore], eosvos_loss_tensors[_ignore], eosvos_loss_sum*, eosvos_set_loss_surface and the fused
entry points, against the numpy twins of `eosvos_amd.surface` (themselves held to the all-pairs definition by
tests/test_surface_host.py).  pytest -m gpu.

Integers (rule 1) and the weights (rule 2) are compared bit for bit: c with `surface.distance_host`, w with the numpy float32
expression of rule 2.

Floats, the project's rule for its float stages: device against the fp64 twin, absolute for the loss and elementwise for the
gradient, at most twice the fp32 twin's own largest error on the same input (the device may order its sums and evaluate the
sigmoid differently from numpy), with a floor of 8 ulp (fp32) of max |g64| for the gradient and of the loss for the loss, for
inputs on which the fp32 twin happens to be nearly exact.  Every check prints its ratio to the bound (PARITY lines, pytest -s;
collected in profiles/surface_parity.txt) before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import surface_ref as ref
from eosvos_amd import loss_sum, surface, synthetic, topology
from loss_common import dlogits_dev, masked_frames, poke_logits

pytestmark = pytest.mark.gpu

FRAME = (112, 176)
DEV = 'cuda:0'
IGN = ref.IGN
N = 'surface'
# (H, W, images): they straddle the 16-row chunks of the column pass, the 64-lane waves and the 256-pixel strides of the row pass
SHAPES = [(1, 1, 1), (5, 7, 1), (33, 65, 2), (17, 130, 3), (97, 161, 3)]
# ... rows wider than one 256-pixel stride of the row pass and one 256-column workgroup of the column pass
WIDE_SHAPES = [(3, 300, 1), (18, 515, 2)]
CAPS = [1, 8, 255, 4095]
# ... and for the float launches: images that are whole float4 (the 16-byte path; the shapes above take single words), images
# of more than 256 x 256 words / float4, where a workgroup of the partial sums strides over its image more than once, and more
# images than the 256 threads of the final reduction
FLOAT_SHAPES = SHAPES + [(8, 68, 3), (515, 130, 1), (1028, 256, 1), (5, 7, 300)]
KINDS = ('blob', 'checkerboard', 'corner')


@pytest.fixture(scope='module')
def weights():
    return synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50')


@pytest.fixture(scope='module')
def eng(weights):
    from eosvos_amd.engine import Engine
    e = Engine('resnet50', *FRAME, max_batch=3, device=DEV)
    e.load_model_state(*weights)
    x, _ = synthetic.synthetic_frames(3, *FRAME, seed=3)
    e.forward(x.to(DEV), want_logits=False)
    yield e
    e.close()


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if hasattr(t, 'detach') else np.ascontiguousarray(t)
    return a.view(np.uint32)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ---- inputs and references, computed once --------------------------------------------------------------------------------
_TARGETS, _DIST, _TWINS = {}, {}, {}


def targets(H, W, images, void, kinds=KINDS):
    key = (H, W, images, void, kinds)
    if key not in _TARGETS:
        _TARGETS[key] = np.stack([ref.target(kinds[i % len(kinds)], H, W, void) for i in range(images)])
    return _TARGETS[key]


def logits_for(y, seed):
    rng = np.random.RandomState(seed)
    sign = np.where(y >= 0.5, 1.0, -1.0)
    return (2 * rng.randn(*y.shape) + 3 * sign * rng.rand(*y.shape)).astype(np.float32)


def distance_ref(key, y, cap, ign):
    if key not in _DIST:
        _DIST[key] = surface.distance_host(y, cap, ign)
    return _DIST[key]


def twins(key, z, y, cap, ign):
    if key not in _TWINS:
        _TWINS[key] = (surface.loss_host(z, y, cap, ign), surface.loss_host(z, y, cap, ign, dtype=np.float32))
    return _TWINS[key]


def weights_rule(c, cap):
    """Rule 2 as the numpy float32 expression."""
    lf = np.float32(cap)
    return np.where(c > cap * cap, lf, np.sqrt(c.astype(np.float32))) / lf


def weights_raw(e, y, cap, ign, want_c=True, want_w=True):
    """eosvos_surface_weights into outputs pre-filled with all-ones bits (c) and NaN (w)."""
    yd = torch.from_numpy(y).to(DEV)
    images, H, W = y.shape
    c = torch.full(y.shape, -1, dtype=torch.int32, device=DEV)
    w = torch.full(y.shape, float('nan'), dtype=torch.float32, device=DEV)
    v = None if ign is None else ctypes.byref(ctypes.c_float(ign))
    rc = e.lib.eosvos_surface_weights(e.h, ctypes.c_void_p(yd.data_ptr()), images, H, W, cap, v,
                                      ctypes.c_void_p(c.data_ptr()) if want_c else None,
                                      ctypes.c_void_p(w.data_ptr()) if want_w else None)
    assert rc == 0, e.lib.eosvos_last_error()
    e.synchronize()
    return c.cpu().numpy(), w.cpu().numpy()


def check(tag, loss, grad, key, z, y, cap, ign):
    """Device loss / gradient against the fp64 twin under the module's bound: prints the ratios, then asserts."""
    (l64, g64), (l32, g32) = twins(key, z, y, cap, ign)
    l64, g64 = float(l64), g64.reshape(-1)
    grad = np.asarray(grad, dtype=np.float64).reshape(-1)
    gmax = float(np.abs(g64).max())
    tol_g = max(2 * float(np.abs(g32.reshape(-1).astype(np.float64) - g64).max()), 8 * ulp32(gmax) if gmax > 0 else 0.0)
    tol_l = max(2 * abs(float(l32) - l64), 8 * ulp32(l64) if l64 > 0 else 0.0)
    dg, dl = float(np.abs(grad - g64).max()), abs(loss - l64)
    print(f'PARITY {tag}: loss {loss:.9g} vs {l64:.12g} diff {dl:.2e} bound {tol_l:.2e} ratio {dl / tol_l if tol_l else 0:.3f}; '
          f'dlogits diff {dg:.2e} bound {tol_g:.2e} ratio {dg / tol_g if tol_g else 0:.3f} (max |g64| {gmax:.2e})')
    assert np.isfinite(loss) and np.isfinite(grad).all(), tag
    assert dl <= tol_l, tag
    assert dg <= tol_g, tag


def void_bits_are_plus_zero(grad, y):
    return not bits(np.asarray(grad, dtype=np.float32).reshape(-1)[(y == IGN).reshape(-1)]).any()


# ---- rules 1 and 2, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('void', [False, True])
@pytest.mark.parametrize('cap', CAPS)
@pytest.mark.parametrize('H,W,images', SHAPES + WIDE_SHAPES)
def test_distances_and_weights_bit_for_bit(eng, H, W, images, cap, void):
    y = targets(H, W, images, void)
    ign = IGN if void else None
    want = distance_ref(('generic', H, W, images, cap, void), y, cap, ign)
    c, w = weights_raw(eng, y, cap, ign)
    assert np.array_equal(c, want)
    assert np.array_equal(bits(w), bits(weights_rule(want, cap)))
    c2, w2 = weights_raw(eng, y, cap, ign)                  # run to run
    assert np.array_equal(c, c2) and np.array_equal(bits(w), bits(w2))


@pytest.mark.parametrize('void', [False, True])
@pytest.mark.parametrize('kind', ['empty', 'full', 'all_void', 'corner', 'void_band', 'checkerboard'])
def test_degenerate_targets_bit_for_bit(eng, kind, void):
    for H, W, images in ((33, 65, 2), (97, 161, 3)):
        y = targets(H, W, images, void, (kind,))
        ign = IGN if ref.uses_void(kind, void) else None
        for cap in CAPS:
            want = distance_ref((kind, H, W, images, cap, void), y, cap, ign)
            c, w = weights_raw(eng, y, cap, ign)
            assert np.array_equal(c, want), (kind, H, W, cap)
            assert np.array_equal(bits(w), bits(weights_rule(want, cap))), (kind, H, W, cap)
    if kind in ('empty', 'full') and not void:
        assert (c == cap * cap + 1).all() and (w == 1).all()
    if kind == 'all_void':
        assert not c.any() and not bits(w).any()


def test_either_output_alone_and_the_engine_method(eng):
    y = targets(33, 65, 2, True)
    c, w = weights_raw(eng, y, 8, IGN)
    c1, w1 = weights_raw(eng, y, 8, IGN, want_w=False)
    assert np.array_equal(c1, c) and np.isnan(w1).all()     # the output that was not asked for is untouched
    c2, w2 = weights_raw(eng, y, 8, IGN, want_c=False)
    assert (c2 == -1).all() and np.array_equal(bits(w2), bits(w))
    cm, wm = eng.surface_weights(torch.from_numpy(y).to(DEV), cap=8, ignore=IGN)
    assert cm.dtype == torch.int32 and np.array_equal(cm.cpu().numpy(), c) and np.array_equal(bits(wm), bits(w))
    cd, _ = eng.surface_weights(torch.from_numpy(y[0]).to(DEV), ignore=IGN)      # (H, W); the shape's default cap
    assert surface.default_cap(33, 65) == 8 and np.array_equal(cd.cpu().numpy(), c[0])


# ---- the loss and the gradient against the twin ----------------------------------------------------------------------------
def run(e, z, y, cap, ign):
    loss, grad = e.surface_loss(torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV), cap=cap, ignore=ign)
    return loss, grad


@pytest.mark.parametrize('void', [False, True])
@pytest.mark.parametrize('cap', [1, 8, 4095])
@pytest.mark.parametrize('H,W,images', FLOAT_SHAPES)
def test_loss_and_gradient_vs_twin(eng, H, W, images, cap, void):
    y = targets(H, W, images, void)
    ign = IGN if void else None
    z = logits_for(y, H * W + images)
    loss, grad = run(eng, z, y, cap, ign)
    check(f'surface B={images} {H}x{W} cap={cap} void={void}', float(loss), grad.cpu().numpy(), ('generic', H, W, images, cap, void), z, y,
          cap, ign)
    if void:
        assert void_bits_are_plus_zero(grad.cpu().numpy(), y)
    loss2, grad2 = run(eng, z, y, cap, ign)                 # run to run, another input through the scratch in between
    assert np.array_equal(bits(loss), bits(loss2)) and np.array_equal(bits(grad), bits(grad2))


def test_void_pixels_non_finite_logits_and_an_all_void_batch(eng):
    y = targets(33, 65, 2, True)
    z = logits_for(y, 9)
    la, ga = run(eng, z, y, 8, IGN)
    bad = z.copy()
    void = y == IGN
    bad[void] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[np.arange(int(void.sum())) % 3]
    lb, gb = run(eng, bad, y, 8, IGN)
    assert np.array_equal(bits(la), bits(lb)) and np.array_equal(bits(ga), bits(gb)) and bool(torch.isfinite(gb).all())
    assert void_bits_are_plus_zero(gb.cpu().numpy(), y)
    lp, gp = run(eng, z, np.where(void, 0, y).astype(np.float32), 8, -1.0)       # a label no pixel carries: the plain call's bits
    lq, gq = run(eng, z, np.where(void, 0, y).astype(np.float32), 8, None)
    assert np.array_equal(bits(lp), bits(lq)) and np.array_equal(bits(gp), bits(gq))
    allv = np.full_like(y, IGN)
    lv, gv = run(eng, bad, allv, 8, IGN)
    assert float(lv) == 0.0 and not bits(lv).any() and not bits(gv).any()
    mixed = np.stack([y[0], allv[0]])                       # an all-void image adds 0 to the mean and gets gradient +0
    lm, gm = run(eng, z, mixed, 8, IGN)
    check('one all-void image of two', float(lm), gm.cpu().numpy(), 'mixed', z, mixed, 8, IGN)
    assert not bits(gm[1]).any()
    loss_only = torch.full((1,), float('nan'), device=DEV)  # dlogits_out may be null
    v = ctypes.byref(ctypes.c_float(IGN))
    zd, yd = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    assert eng.lib.eosvos_surface_loss(eng.h, ctypes.c_void_p(zd.data_ptr()), ctypes.c_void_p(yd.data_ptr()), 2, 33, 65, 8, v,
                                       ctypes.c_void_p(loss_only.data_ptr()), None) == 0
    eng.synchronize()
    assert np.array_equal(bits(loss_only), bits(la))


def test_an_empty_target_is_the_mean_foreground_probability(eng):
    y = np.zeros((2, 33, 65), dtype=np.float32)
    z = logits_for(y + 1, 4)
    loss, grad = run(eng, z, y, 255, None)
    check('empty target', float(loss), grad.cpu().numpy(), 'empty', z, y, 255, None)
    p = 1 / (1 + np.exp(-z.astype(np.float64)))
    assert abs(float(loss) - p.mean()) <= 8 * ulp32(p.mean())


# ---- bad arguments at the ABI ------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_outputs_untouched(eng):
    H, W, B = 9, 11, 2
    z = torch.zeros(B, H, W, device=DEV)
    y = torch.zeros(B, H, W, device=DEV)
    loss = torch.full((1,), 7.5, device=DEV)
    grad = torch.full((B, H, W), 7.5, device=DEV)
    c = torch.full((B, H, W), 77, dtype=torch.int32, device=DEV)
    w = torch.full((B, H, W), 7.5, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f = lambda x: ctypes.byref(ctypes.c_float(x))
    L, Wt = eng.lib.eosvos_surface_loss, eng.lib.eosvos_surface_weights
    bad_loss = [(None, p(z), p(y), B, H, W, 3, None, p(loss), p(grad)), (eng.h, None, p(y), B, H, W, 3, None, p(loss), p(grad)),
                (eng.h, p(z), None, B, H, W, 3, None, p(loss), p(grad)), (eng.h, p(z), p(y), B, H, W, 3, None, None, p(grad)),
                (eng.h, p(z), p(y), B, H, W, -1, None, p(loss), p(grad)), (eng.h, p(z), p(y), B, H, W, 4096, None, p(loss), p(grad)),
                (eng.h, p(z), p(y), 0, H, W, 3, None, p(loss), p(grad)), (eng.h, p(z), p(y), B, 0, W, 3, None, p(loss), p(grad)),
                (eng.h, p(z), p(y), B, H, 4097, 3, None, p(loss), p(grad)), (eng.h, p(z), p(y), B, 4097, W, 3, None, p(loss), p(grad)),
                (eng.h, p(z), p(y), B, H, W, 3, f(0.5), p(loss), p(grad)), (eng.h, p(z), p(y), B, H, W, 3, f(float('nan')), p(loss), p(grad)),
                (eng.h, p(z), p(y), B, H, W, 3, f(float('inf')), p(loss), p(grad))]
    for args in bad_loss:
        assert L(*args) != 0 and eng.lib.eosvos_last_error(), args
    bad_w = [(None, p(y), B, H, W, 3, None, p(c), p(w)), (eng.h, None, B, H, W, 3, None, p(c), p(w)),
             (eng.h, p(y), B, H, W, 3, None, None, None), (eng.h, p(y), B, H, W, -1, None, p(c), p(w)),
             (eng.h, p(y), B, H, W, 4096, None, p(c), p(w)), (eng.h, p(y), 0, H, W, 3, None, p(c), p(w)),
             (eng.h, p(y), B, 0, W, 3, None, p(c), p(w)), (eng.h, p(y), B, H, 4097, 3, None, p(c), p(w)),
             (eng.h, p(y), B, H, W, 3, f(1.0), p(c), p(w))]
    for args in bad_w:
        assert Wt(*args) != 0 and eng.lib.eosvos_last_error(), args
    for cap in (-1, 4096):
        assert eng.lib.eosvos_set_loss_surface(eng.h, cap) != 0 and b'cap' in eng.lib.eosvos_last_error()
        with pytest.raises(ValueError):
            eng.set_loss_surface(cap)
    assert eng.lib.eosvos_set_loss_surface(None, 3) != 0
    eng.synchronize()
    assert (loss == 7.5).all() and (grad == 7.5).all() and (c == 77).all() and (w == 7.5).all()
    assert eng.lib.eosvos_set_loss(eng.h, 7) != 0 and b'unknown loss kind' in eng.lib.eosvos_last_error()      # kind 7 stays unknown
    assert eng.lib.eosvos_set_loss(eng.h, 11) != 0
    assert L(eng.h, p(z), p(y), B, H, W, 3, None, p(loss), p(grad)) == 0          # still usable
    eng.synchronize()
    assert float(loss) == 0.5 and bool(torch.isfinite(grad).all())               # z = 0, empty target: the mean of p = 1/2


# ---- through the engine ----------------------------------------------------------------------------------------------------
def frame_case(e, void):
    """Batch 3 at the engine's frame size, poked in as the logits of the last forward."""
    y = targets(*FRAME, 3, void)
    z = logits_for(y, 5)
    zd = torch.from_numpy(z).to(DEV)
    x, _ = synthetic.synthetic_frames(3, *FRAME, seed=3)
    e.forward(x.to(DEV), want_logits=False)                 # a batch-3 forward for the loss calls to follow
    poke_logits(e, zd)
    return z, y, zd, torch.from_numpy(y).to(DEV)


@pytest.mark.parametrize('void', [False, True])
def test_the_loss_entries_on_poked_logits(eng, void):
    from eosvos_amd.helper_func import compute_loss
    z, y, zd, yd = frame_case(eng, void)
    ign = IGN if void else None
    n = z.size
    masks = yd.view(3, 1, *FRAME)
    assert surface.default_cap(*FRAME) == 28
    eng.set_loss_surface(0)
    kw = {} if ign is None else {'ignore': ign}
    l0, g0 = eng.loss(N, masks, **kw), dlogits_dev(eng, n)
    check(f'engine loss, default cap, void={void}', float(l0), g0.cpu().numpy(), ('frame', 28, void), z, y, 28, ign)
    if void:
        assert void_bits_are_plus_zero(g0.cpu().numpy(), y)
    ref0 = eng.surface_loss(zd, yd, ignore=ign)             # the stand-alone entry, this shape's default: the same launches
    assert np.array_equal(bits(l0), bits(ref0[0])) and np.array_equal(bits(g0), bits(ref0[1].reshape(-1)))
    # the suffix, the keyword and the setter agree
    l8, g8 = eng.loss(N + '_8', masks, **kw), dlogits_dev(eng, n)
    check(f'engine loss, surface_8, void={void}', float(l8), g8.cpu().numpy(), ('frame', 8, void), z, y, 8, ign)
    eng.set_loss_surface(0)
    l8k, g8k = eng.loss(N, masks, cap=8, **kw), dlogits_dev(eng, n)
    l8s, g8s = eng.loss(N, masks, **kw), dlogits_dev(eng, n)                     # the cap stays the engine's
    for a, b in ((l8k, g8k), (l8s, g8s)):
        assert np.array_equal(bits(l8), bits(a)) and np.array_equal(bits(g8), bits(b))
    assert not np.array_equal(bits(g0), bits(g8))
    with pytest.raises(ValueError):
        eng.loss(N + '_8', masks, cap=4)
    # one image through the tensor entries, and per sample through compute_loss
    one64 = surface.loss_host(z[1], y[1], 8, ign)
    a = eng.loss_of(N + '_8', zd[1], yd[1], **kw)
    b, gb = eng.loss_grad_of(N, zd[1], yd[1], cap=8, **kw)
    assert np.array_equal(bits(a), bits(b))
    check(f'loss_grad_of one image, void={void}', float(b), gb.cpu().numpy(), ('frame one', 8, void), z[1], y[1], 8, ign)
    assert abs(float(a) - float(one64[0])) <= max(8 * ulp32(float(one64[0])), 2 * abs(float(surface.loss_host(z[1], y[1], 8, ign, np.float32)[0]) - float(one64[0])))
    for m in (FRAME[0] * FRAME[1] - 1, 2 * FRAME[0] * FRAME[1], 1):
        with pytest.raises(RuntimeError, match='H \\* W'):
            eng.loss_of(N, zd.reshape(-1)[:m], yd.reshape(-1)[:m])
    out = zd.view(3, 1, *FRAME)
    out._eosvos_engine = eng
    eng.set_loss_surface(0)
    lk = {'cap': 8} if ign is None else {'cap': 8, 'ignore': ign}
    cl = compute_loss(N, out, masks, lk)
    assert np.array_equal(bits(cl.reshape(1)), bits(l8)) and np.array_equal(bits(dlogits_dev(eng, n)), bits(g8))
    per = compute_loss(N + '_8', out, masks, dict(lk, batch_average=False, cap=None))
    want = [float(surface.loss_host(z[i], y[i], 8, ign)[0]) for i in range(3)]
    w32 = [float(surface.loss_host(z[i], y[i], 8, ign, np.float32)[0]) for i in range(3)]
    print(f'PARITY compute_loss per sample void={void}: {per.cpu().numpy()} vs {want}')
    assert per.shape == (3,)
    for i in range(3):
        assert abs(float(per[i]) - want[i]) <= max(8 * ulp32(want[i]), 2 * abs(w32[i] - want[i]))
    with pytest.raises(ValueError):
        compute_loss('dice', out, masks, {'cap': 8})
    eng.set_loss_surface(0)


def test_a_sum_with_the_kind_is_the_combine_of_its_terms(eng):
    z, y, zd, yd = frame_case(eng, True)
    n = z.size
    masks = yd.view(3, 1, *FRAME)
    name = 'dice+0.5*surface_8'
    ls, gs = eng.loss(name, masks, ignore=IGN), dlogits_dev(eng, n)
    terms = eng.last_loss_terms()
    ld, gd = eng.loss('dice', masks, ignore=IGN), dlogits_dev(eng, n)
    lf, gf = eng.loss(N + '_8', masks, ignore=IGN), dlogits_dev(eng, n)
    assert np.array_equal(np.float32(terms).view(np.uint32), np.concatenate([bits(ld), bits(lf)]))
    wl, wg = loss_sum.combine_host([float(ld), float(lf)], [gd.cpu().numpy(), gf.cpu().numpy()], [1.0, 0.5])
    assert np.array_equal(bits(ls), np.float32([wl]).view(np.uint32)) and np.array_equal(bits(gs), wg.view(np.uint32))
    lt, gt = eng.loss_grad_of(name, zd[0], yd[0], ignore=IGN)                    # the tensor entry, one image
    l1, g1 = eng.loss_grad_of('dice', zd[0], yd[0], ignore=IGN)
    l2, g2 = eng.loss_grad_of(N, zd[0], yd[0], ignore=IGN, cap=8)
    wl, wg = loss_sum.combine_host([float(l1), float(l2)], [g1.cpu().numpy(), g2.cpu().numpy()], [1.0, 0.5])
    assert np.array_equal(bits(lt), np.float32([wl]).view(np.uint32)) and np.array_equal(bits(gt), wg.view(np.uint32))
    both = eng.loss('surface_8+boundary_f_2', masks, ignore=IGN)                 # beside a boundary kind
    assert np.isfinite(float(both)) and len(eng.last_loss_terms()) == 2
    eng.set_loss_surface(0)
    eng.set_loss_boundary(0)


def test_cross_entropy_between_two_surface_calls_has_a_fresh_engines_bits(eng, weights):
    from eosvos_amd.engine import Engine
    z, y, zd, yd = frame_case(eng, False)
    n = z.size
    masks = yd.view(3, 1, *FRAME)
    s1 = eng.loss(N, masks)
    ce, gce = eng.loss('cross_entropy', masks), dlogits_dev(eng, n)
    s2 = eng.loss(N, masks)
    assert np.array_equal(bits(s1), bits(s2))
    fresh = Engine('resnet50', *FRAME, max_batch=3, device=DEV)
    try:
        fresh.load_model_state(*weights)
        frame_case(fresh, False)
        cf, gcf = fresh.loss('cross_entropy', masks), dlogits_dev(fresh, n)
    finally:
        fresh.close()
    assert np.array_equal(bits(ce), bits(cf)) and np.array_equal(bits(gce), bits(gcf))


@pytest.mark.parametrize('frozen', [False, True])
@pytest.mark.parametrize('ign', [None, IGN])
def test_fused_step_equals_the_separate_calls(eng, weights, ign, frozen):
    """set_loss('surface_8', ignore=v) + finetune_step == forward -> loss -> backward_step, bit for bit; also with the frozen
    encoder (eosvos_set_trainable_from)."""
    xd, yd, ym = masked_frames(4, FRAME, 0.1)
    masks = yd if ign is None else ym
    eng.load_model_state(*weights)
    eng.set_trainable_from(topology.trainable_from('resnet50', False) if frozen else 0)
    eng.set_loss_surface(5)                                  # the suffix below must win over what the engine held
    eng.set_loss(N + '_8', ignore=ign)
    try:
        fused = [eng.finetune_step(xd, masks) for _ in range(2)]
        p_fused = eng.get_params().clone()
        eng.load_model_state(*weights)
        sep = []
        for _ in range(2):
            eng.forward(xd, want_logits=False)
            sep.append(float(eng.loss(N, masks, ignore=ign, cap=8)))
            eng.backward_step()
        p_sep = eng.get_params().clone()
        eng.load_model_state(*weights)
        logits = eng.forward(xd).cpu().numpy().reshape(3, *FRAME)               # the first step's loss is the twin's on the first logits
    finally:
        eng.set_loss('cross_entropy')
        eng.set_loss_surface(0)
        eng.set_trainable_from(0)
        eng.load_model_state(*weights)
    assert np.array_equal(np.float32(fused).view(np.uint32), np.float32(sep).view(np.uint32)), (fused, sep)
    assert torch.equal(p_fused, p_sep)
    ynp = masks.cpu().numpy().reshape(3, *FRAME)
    l64 = float(surface.loss_host(logits, ynp, 8, ign)[0])
    l32 = float(surface.loss_host(logits, ynp, 8, ign, np.float32)[0])
    tol = max(2 * abs(l32 - l64), 8 * ulp32(l64))
    print(f'PARITY fused step ignore={ign} frozen={frozen}: losses {fused}; twin on the first logits {l64:.9g}; '
          f'ratio {abs(fused[0] - l64) / tol:.3f}')
    assert abs(fused[0] - l64) <= tol
    assert fused[1] != fused[0]                              # the step moved the weights


def test_meta_grad_and_the_matrix_mode_guard_run_under_the_kind(eng, weights):
    xd, yd, ym = masked_frames(8, FRAME, 0.1)
    eng.load_model_state(*weights)
    eng.set_loss('dice+0.5*surface_8', ignore=IGN)
    try:
        eng.meta_task_begin()
        eng.finetune_step(xd, ym, accumulate=True)
        flat = torch.zeros(eng.n_lr + eng.n_param, device=DEV)
        eng.meta_grad(xd, ym, flat)
        assert len(eng.last_loss_terms()) == 2
        assert bool(torch.isfinite(flat).all()) and float(flat.abs().max()) > 0
        eng.load_model_state(*weights)
        eng.set_loss(N, ignore=IGN, cap=8)
        eng.meta_task_begin()
        eng.finetune_step(xd, ym, accumulate=True)
        flat.zero_()
        ml = eng.meta_grad(xd, ym, flat)
        logits = eng.debug_tensor('logits').cpu().numpy().reshape(3, *FRAME)
        ynp = ym.cpu().numpy().reshape(3, *FRAME)
        l64 = float(surface.loss_host(logits, ynp, 8, IGN)[0])
        l32 = float(surface.loss_host(logits, ynp, 8, IGN, np.float32)[0])
        tol = max(2 * abs(l32 - l64), 8 * ulp32(l64))
        print(f'PARITY meta_grad: {ml} vs {l64}; ratio {abs(ml - l64) / tol:.3f}')
        assert abs(ml - l64) <= tol
        assert bool(torch.isfinite(flat).all()) and float(flat.abs().max()) > 0
        eng.load_model_state(*weights)
        eng.set_loss(N, cap=8)
        mode = eng.verify_matrix_mode(xd, yd)
        print(f'PARITY verify_matrix_mode under {N}: {mode} {getattr(eng, "last_step_check", None)}')
        assert mode in ('f16x3', 'bf16x6')
    finally:
        eng.set_loss('cross_entropy')
        eng.set_loss_surface(0)
        eng.load_model_state(*weights)
