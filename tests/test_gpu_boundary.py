"""The soft boundary-F loss on the MI355X: EOSVOS_LOSS_BOUNDARY_F / EOSVOS_LOSS_BCE_AND_BOUNDARY_F through eosvos_boundary_f
(any frame shape), eosvos_loss[_ignore], eosvos_loss_tensors[_ignore], eosvos_set_loss_boundary and the fused entry points,
against the torch twin `eosvos_amd.boundary.loss_host` (itself held to the closed form by tests/test_boundary_host.py).
pytest -m gpu.

Inputs.  Generic: y a centred ellipse, z = 2 N(0,1) + 4 (2y - 1) U(0,1) from a seeded torch.Generator.  Before any comparison
two conditions are asserted on the CPU from the fp64 twin's maps, because without them an arg-max could differ between fp32 and
fp64 and the comparison would mean nothing: the two largest q of every 3 x 3 window differ by at least 64 * 2^-24 relative, and
the two largest pb of every r-window centred on a pixel with gb != 0 differ by at least 1e-5.  A seed that fails a condition is
replaced by the next one (per image, seeds 0 .. 63); the conditions are never loosened.  Exact ties: logits from the three levels
{-3, -0.5, 1.25}, whose pairwise q differences are more than 1e-3 apart, so ties are the same in fp32 and fp64.

Bound (the project's rule for its float stages): device against the fp64 twin, elementwise for the gradient and absolute for
the loss, at most twice the fp32 twin's own largest error on the same input, with a floor of 8 ulp (fp32) of max |g64| for the
gradient and of the loss for the loss: one ulp per rounding of the roughly eight operations from the finished sums to dL/dz,
for inputs on which the fp32 twin happens to be nearly exact.  Every check prints its ratio to the bound (PARITY lines,
pytest -s; collected in profiles/boundary_parity.txt) before it asserts.
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
import torch.nn.functional as F

from eosvos_amd import boundary, synthetic
from loss_common import dlogits_dev as dlogits_of, masked_frames, poke_logits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME = (112, 176)                                      # batch 3 of it holds 3 x 97 x 161 pixels
DEV = 'cuda:0'
IGN = 255.0
N, C = 'boundary_f', 'cross_entropy_and_boundary_f'
SHAPES = [(1, 1, 1), (5, 7, 1), (37, 53, 2), (33, 65, 16), (20, 70, 8), (17, 130, 8), (97, 161, 8)]
LEVELS = (-3.0, -0.5, 1.25)
Q_GAP, PB_GAP = 64 * 2.0 ** -24, 1e-5
# Loss values on logits that the network produced (the fused step, meta_grad, compute_loss): no gap condition can be asserted
# there, but the loss, unlike the gradient, is continuous across an arg-max flip (a maximum is), so only rounding counts: the
# maps are fp32 (2^-24 relative each), P and R are ratios of sums of products of two maps and BF a ratio of theirs -- a few
# dozen fp32 roundings on a value of order 1 (plus the cross-entropy's 2e-6 of test_gpu_parity.py).  1e-5 = 84 ulp of 1.
NET_TOL = 1e-5


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
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ---- inputs --------------------------------------------------------------------------------------------------------------
def ellipse(B, H, W):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    y = ((((yy - (H - 1) / 2) / max(H / 3.0, 1)) ** 2 + ((xx - (W - 1) / 2) / max(W / 3.0, 1)) ** 2) <= 1).float()
    return y[None].repeat(B, 1, 1)


def add_void(y):
    """Every 7th pixel, plus a block across the seams at x = 32 and x = 64 (clipped to the frame)."""
    H, W = y.shape[-2:]
    y.view(-1)[::7] = IGN
    y[:, H // 3:H // 3 + 3, min(30, W - 1):min(67, W)] = IGN
    return y


def second_largest_gap(x, valid, r, centres, relative):
    """The smallest gap between the two largest valid values of x (H, W; fp64) in the clipped (2r+1)^2 windows centred on
    `centres` (bool H x W); windows with fewer than two valid pixels do not count."""
    if not bool(centres.any()):
        return float('inf')
    k = 2 * r + 1
    pad = F.pad(torch.where(valid, x, torch.full_like(x, -np.inf))[None, None], (r, r, r, r), value=-np.inf)
    cols = F.unfold(pad, k)[0][:, centres.reshape(-1)]                   # (k * k, centres)
    top = cols.topk(2, dim=0).values
    ok = torch.isfinite(top[1])
    if not bool(ok.any()):
        return float('inf')
    gap = (top[0] - top[1])[ok]
    if relative:
        gap = gap / top[0][ok].abs()
    return float(gap.min())


def gaps(z, y, r, ign):
    """(smallest relative q gap, smallest pb gap) over the images, from fp64 maps."""
    gq, gp = float('inf'), float('inf')
    for b in range(z.shape[0]):
        zz, yy = z[b].double(), y[b].double()
        valid = torch.ones_like(yy, dtype=torch.bool) if ign is None else yy != ign
        e = torch.exp(-zz.abs())
        q = torch.where(zz >= 0, e / (1 + e), 1 / (1 + e))
        pb = torch.where(valid, boundary._pool(q[None, None], valid[None, None], 1)[0, 0] - q, torch.zeros_like(q))
        h = 1 - yy
        gb = torch.where(valid, boundary._pool(h[None, None], valid[None, None], 1)[0, 0] - h, torch.zeros_like(h))
        gq = min(gq, second_largest_gap(q, valid, 1, valid, True))
        gp = min(gp, second_largest_gap(pb, valid, r, valid & (gb != 0), False))
    return gq, gp


_CASES = {}


def generic_case(B, H, W, r, void):
    """(z, y, ign, twin results): the images are drawn one by one (the conditions are per image), each from the next seed of
    0 .. 63 that meets both gap conditions; computed once and shared."""
    key = (B, H, W, r, void)
    if key not in _CASES:
        ign = IGN if void else None
        y = ellipse(1, H, W)
        if void:
            y = add_void(y)
        zs, seeds, gq, gp, seed = [], [], float('inf'), float('inf'), 0
        while len(zs) < B and seed < 64:
            g = torch.Generator().manual_seed(seed)
            z = (2 * torch.randn(1, H, W, generator=g) + 4 * (2 * ellipse(1, H, W) - 1) * torch.rand(1, H, W, generator=g)).float()
            q, p = gaps(z, y, r, ign)
            if q >= Q_GAP and p >= PB_GAP:
                zs.append(z)
                seeds.append(seed)
                gq, gp = min(gq, q), min(gp, p)
            seed += 1
        assert len(zs) == B, f'too few seeds in 0 .. 63 meet the gap conditions at {key}'
        z, y = torch.cat(zs), y.repeat(B, 1, 1)
        gq, gp = gaps(z, y, r, ign)                          # asserted on what the comparison will use
        assert gq >= Q_GAP and gp >= PB_GAP, key
        print(f'CASE B={B} {H}x{W} r={r} void={void}: seeds {seeds}, q gap {gq:.2e} (>= {Q_GAP:.2e}), pb gap {gp:.2e} (>= {PB_GAP:.0e})')
        _CASES[key] = (z, y, ign, {})
    return _CASES[key]


def tie_case(B, H, W, void):
    g = torch.Generator().manual_seed(H * W)
    z = torch.tensor(LEVELS)[torch.randint(0, 3, (B, H, W), generator=g)].float()
    y = ellipse(B, H, W)
    return z, (add_void(y) if void else y), (IGN if void else None)


def twins(z, y, r, ign, combined, cache=None):
    key = (r, combined)
    if cache is not None and key in cache:
        return cache[key]
    out = (boundary.loss_host(z, y, r, ignore=ign, combined=combined),
           boundary.loss_host(z, y, r, ignore=ign, combined=combined, dtype=torch.float32))
    if cache is not None:
        cache[key] = out
    return out


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def check(tag, loss, grad, z, y, r, ign, combined=False, cache=None):
    """Device loss / gradient against the fp64 twin under the module's bound: prints the ratios, then asserts."""
    (l64, g64, _), (l32, g32, _) = twins(z, y, r, ign, combined, cache)
    l64, g64 = float(l64), g64.reshape(-1).numpy()
    grad = np.asarray(grad, dtype=np.float64).reshape(-1)
    gmax = float(np.abs(g64).max())
    tol_g = max(2 * float(np.abs(g32.reshape(-1).double().numpy() - g64).max()), 8 * ulp32(gmax) if gmax > 0 else 0.0)
    tol_l = max(2 * abs(float(l32) - l64), 8 * ulp32(l64))
    dg, dl = float(np.abs(grad - g64).max()), abs(loss - l64)
    print(f'PARITY {tag}: loss {loss:.9g} vs {l64:.12g} diff {dl:.2e} bound {tol_l:.2e} ratio {dl / tol_l if tol_l else 0:.3f}; '
          f'dlogits diff {dg:.2e} bound {tol_g:.2e} ratio {dg / tol_g if tol_g else 0:.3f} (max |g64| {gmax:.2e})')
    assert np.isfinite(loss) and np.isfinite(grad).all(), tag
    if ign is not None:
        void = (y.reshape(-1) == ign).numpy()
        assert not grad[void].any(), f'{tag}: the gradient of a void pixel is not 0'
    assert dl <= tol_l, tag
    assert dg <= tol_g, tag


def run(e, z, y, r, ign, combined=False):
    loss, grad = e.boundary_f(z.to(DEV), y.to(DEV), radius=r, ignore=ign, combined=combined)
    return float(loss), grad.cpu().numpy()


# ---- every shape against the twin ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('combined', [False, True])
@pytest.mark.parametrize('void', [False, True])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('H,W,r', SHAPES)
def test_generic_inputs_vs_twin(eng, H, W, r, B, void, combined):
    z, y, ign, cache = generic_case(B, H, W, r, void)
    loss, grad = run(eng, z, y, r, ign, combined)
    check(f'{"combined" if combined else "boundary"} B={B} {H}x{W} r={r} void={void}', loss, grad, z, y, r, ign, combined, cache)


@pytest.mark.parametrize('void', [False, True])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('H,W,r', [(5, 7, 1), (37, 53, 2), (20, 70, 8), (33, 65, 16)])
def test_exact_ties_vs_twin(eng, H, W, r, B, void):
    z, y, ign = tie_case(B, H, W, void)
    loss, grad = run(eng, z, y, r, ign)
    check(f'ties B={B} {H}x{W} r={r} void={void}', loss, grad, z, y, r, ign)
    assert np.abs(grad).max() > 0


# ---- the exact cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('void', [False, True])
@pytest.mark.parametrize('case', ['empty_target', 'full_target', 'constant_logits', 'all_void'])
def test_degenerate_inputs(eng, case, void):
    z, y, _, _ = generic_case(3, 37, 53, 2, False)
    z, y = z.clone(), y.clone()
    if case == 'empty_target':
        y[:] = 0
    elif case == 'full_target':
        y[:] = 1
    elif case == 'constant_logits':
        z[:] = 0.75
    if void:
        y = add_void(y)
    if case == 'all_void':
        y[1] = IGN
    ign = IGN if (void or case == 'all_void') else None
    loss, grad = run(eng, z, y, 2, ign)
    if case == 'all_void':                                   # the image adds 0 to the mean and gets gradient 0
        per = boundary.loss_host(z, y, 2, ignore=ign)[2]
        assert float(per[1]) == 0.0 and not grad[1].any()
        check(f'all-void image, void={void}', loss, grad, z, y, 2, ign)
        lo, gr = run(eng, z[1:2], y[1:2], 2, ign)
        assert lo == 0.0 and not gr.any()
    else:
        assert loss == 1.0 and not grad.any() and np.isfinite(grad).all(), (case, loss)


def test_void_pixels_and_non_finite_logits(eng):
    z, y, ign, _ = generic_case(3, 37, 53, 2, True)
    void = y == IGN
    zd, yd = z.to(DEV), y.to(DEV)
    for combined in (False, True):
        la, ga = eng.boundary_f(zd, yd, radius=2, ignore=IGN, combined=combined)
        assert not ga[void.to(DEV)].any()
        bad = z.clone()
        bad[void] = torch.tensor([float('nan'), float('inf'), float('-inf')])[torch.arange(int(void.sum())) % 3]
        lb, gb = eng.boundary_f(bad.to(DEV), yd, radius=2, ignore=IGN, combined=combined)
        assert np.array_equal(bits(la), bits(lb)) and np.array_equal(bits(ga), bits(gb)) and bool(torch.isfinite(gb).all())
        nan = z.clone()
        idx = int(torch.nonzero(~void[1].reshape(-1))[5])
        nan[1].view(-1)[idx] = float('nan')
        ln, _ = eng.boundary_f(nan.to(DEV), yd, radius=2, ignore=IGN, combined=combined)
        assert bool(torch.isnan(ln).all())


def test_without_a_void_pixel_the_bits_are_those_of_the_plain_call(eng):
    z, y, _, _ = generic_case(3, 37, 53, 2, False)
    zd, yd = z.to(DEV), y.to(DEV)
    for combined in (False, True):
        la, ga = eng.boundary_f(zd, yd, radius=2, combined=combined)
        lb, gb = eng.boundary_f(zd, yd, radius=2, ignore=-1.0, combined=combined)
        assert np.array_equal(bits(la), bits(lb)) and np.array_equal(bits(ga), bits(gb))


# ---- reproducibility -----------------------------------------------------------------------------------------------------
def repro_case():
    z, y, _ = tie_case(3, 97, 161, True)
    g = torch.Generator().manual_seed(77)
    return (z + 0.25 * torch.randn(z.shape, generator=g)).float(), y


def repro_digest(e, z, y):
    out = []
    for combined in (False, True):
        loss, grad = e.boundary_f(z.to(DEV), y.to(DEV), radius=8, ignore=IGN, combined=combined)
        out += [int(bits(loss)[0]), hashlib.sha256(grad.cpu().numpy().tobytes()).hexdigest()]
    return out


CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from eosvos_amd.engine import Engine
import test_gpu_boundary as T
eng = Engine('resnet50', *T.FRAME, max_batch=3, device='cuda:0')
print(json.dumps(T.repro_digest(eng, *T.repro_case())))
eng.close()
'''


def test_two_evaluations_are_bit_identical_also_from_dirty_or_nan_filled_scratch(eng):
    z, y = repro_case()
    got = [repro_digest(eng, z, y)]
    other, yo, _, _ = generic_case(3, 97, 161, 8, False)
    eng.boundary_f(other.to(DEV), yo.to(DEV), radius=16)                    # another input through the scratch in between
    got.append(repro_digest(eng, z, y))
    assert got[0] == got[1], got
    env = dict(os.environ, EOSVOS_MODE_GUARD='0', EOSVOS_DEBUG_FILL='7fc00000')      # every engine buffer starts out as NaN words
    p = subprocess.run([sys.executable, '-c', CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [l for l in p.stdout.splitlines() if l.startswith('[')]
    assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert json.loads(lines[-1]) == got[0]


# ---- the setter, the names -----------------------------------------------------------------------------------------------
def frame_case(eng, void=False):
    """Batch 3 at the engine's frame size, poked in as the logits of the last forward; radius 2 is the frame's default.  No gap
    condition holds on 3 x 19712 random pixels, so these inputs are compared path against path on the device, bit for bit,
    with eosvos_boundary_f, which the cases above hold to the twin."""
    g = torch.Generator().manual_seed(5)
    y = ellipse(3, *FRAME)
    z = (2 * torch.randn(3, *FRAME, generator=g) + 4 * (2 * y - 1) * torch.rand(3, *FRAME, generator=g)).float()
    if void:
        y = add_void(y)
    poke_logits(eng, z.to(DEV))
    return z.to(DEV), y.to(DEV)


def test_the_setter_and_the_default_radius(eng):
    z, y = frame_case(eng)
    assert boundary.default_radius(*FRAME) == 2
    masks = y.view(3, 1, *FRAME)
    n = z.numel()
    eng.set_loss_boundary(5)
    l5, g5 = eng.loss(N, masks), dlogits_of(eng, n)
    r5 = eng.boundary_f(z, y, radius=5)
    assert np.array_equal(bits(l5), bits(r5[0])) and np.array_equal(bits(g5), bits(r5[1].reshape(-1)))
    eng.set_loss_boundary(0)                                 # back to the frame-size default
    l0, g0 = eng.loss(N, masks), dlogits_of(eng, n)
    for r0 in (eng.boundary_f(z, y, radius=2), eng.boundary_f(z, y)):
        assert np.array_equal(bits(l0), bits(r0[0])) and np.array_equal(bits(g0), bits(r0[1].reshape(-1)))
    assert not np.array_equal(bits(g0), bits(g5))
    ref = float(boundary.loss_host(z, y, 2)[0])
    print(f'PARITY engine frame, default radius: loss {float(l0):.9g} vs {ref:.12g}')
    assert abs(float(l0) - ref) <= NET_TOL
    l2, g2 = eng.loss(N, masks, radius=2), dlogits_of(eng, n)
    assert np.array_equal(bits(l0), bits(l2)) and np.array_equal(bits(g0), bits(g2))
    for bad in (17, -1):
        assert eng.lib.eosvos_set_loss_boundary(eng.h, bad) != 0 and b'radius' in eng.lib.eosvos_last_error()
        with pytest.raises(ValueError):
            eng.set_loss_boundary(bad)
        with pytest.raises(ValueError):
            eng.loss(N, masks, radius=bad)
    l2b = eng.loss(N, masks)                                 # still usable, the radius unchanged
    assert np.array_equal(bits(l2b), bits(l2))
    eng.set_loss_boundary(0)
    assert eng.lib.eosvos_set_loss(eng.h, 7) != 0 and b'unknown loss kind' in eng.lib.eosvos_last_error()      # kind 7 stays unknown
    out = torch.empty(1, device=DEV)
    assert eng.lib.eosvos_loss(eng.h, 7, ctypes.c_void_p(masks.data_ptr()), 3, ctypes.c_void_p(out.data_ptr())) != 0


def test_the_name_suffix_equals_the_keyword_and_the_tensor_entry_takes_one_frame_only(eng):
    zd, yd = frame_case(eng, void=True)
    n = FRAME[0] * FRAME[1]
    for name in (N, C):
        a, ga = eng.loss_of(name + '_3', zd[0], yd[0], ignore=IGN), dlogits_of(eng, n)
        eng.set_loss_boundary(0)
        b, gb = eng.loss_of(name, zd[0], yd[0], ignore=IGN, radius=3), dlogits_of(eng, n)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(ga), bits(gb))
        ref = eng.boundary_f(zd[0], yd[0], radius=3, ignore=IGN, combined=name == C)
        assert np.array_equal(bits(a), bits(ref[0])) and np.array_equal(bits(ga), bits(ref[1].reshape(-1)))
        with pytest.raises(ValueError):
            eng.loss_of(name + '_3', zd[0], yd[0], radius=4)
        for m in (n - 1, 2 * n, 1):
            with pytest.raises(RuntimeError, match='H \\* W'):
                eng.loss_of(name, zd.reshape(-1)[:m], yd.reshape(-1)[:m])
    eng.set_loss_boundary(0)
    with pytest.raises(ValueError):
        eng.loss_of('dice', zd[0], yd[0], radius=3)


# ---- integration ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ign', [None, IGN])
def test_fused_step_equals_the_separate_calls(eng, weights, ign):
    """set_loss('cross_entropy_and_boundary_f_2', ignore=v) + finetune_step == forward -> loss -> backward_step, bit for bit."""
    xd, yd, ym = masked_frames(4, FRAME, 0.1)
    masks = yd if ign is None else ym
    eng.load_model_state(*weights)
    eng.set_loss_boundary(5)                                 # the suffix below must win over what the engine held
    eng.set_loss(C + '_2', ignore=ign)
    try:
        fused = [eng.finetune_step(xd, masks) for _ in range(2)]
        p_fused = eng.get_params().clone()
    finally:
        eng.set_loss('cross_entropy')
    eng.load_model_state(*weights)
    sep = []
    for _ in range(2):
        eng.forward(xd, want_logits=False)
        sep.append(float(eng.loss(C, masks, ignore=ign, radius=2)))
        eng.backward_step()
    p_sep = eng.get_params()
    eng.load_model_state(*weights)
    eng.set_loss_boundary(0)
    assert np.array_equal(np.float32(fused).view(np.uint32), np.float32(sep).view(np.uint32)), (fused, sep)
    assert torch.equal(p_fused, p_sep)
    logits = eng.forward(xd).cpu()                           # the first step's loss is the twin's on the first logits
    ref = float(boundary.loss_host(logits.view(3, *FRAME), masks.cpu().view(3, *FRAME), 2, ignore=ign, combined=True)[0])
    print(f'PARITY fused step ignore={ign}: losses {fused}; twin on the first logits {ref:.9g}')
    assert abs(fused[0] - ref) <= NET_TOL * max(1.0, abs(ref))


def test_meta_grad_and_the_matrix_mode_guard_run_under_the_kind(eng, weights):
    xd, yd, ym = masked_frames(8, FRAME, 0.1)
    eng.load_model_state(*weights)
    eng.set_loss(N, ignore=IGN, radius=2)
    try:
        eng.meta_task_begin()
        eng.finetune_step(xd, ym, accumulate=True)
        flat = torch.zeros(eng.n_lr + eng.n_param, device=DEV)
        ml = eng.meta_grad(xd, ym, flat)
        logits = eng.debug_tensor('logits').cpu()
        ref = float(boundary.loss_host(logits.view(3, *FRAME), ym.cpu().view(3, *FRAME), 2, ignore=IGN)[0])
        print(f'PARITY meta_grad: {ml} vs {ref}')
        assert abs(ml - ref) <= NET_TOL * max(1.0, abs(ref))
        assert bool(torch.isfinite(flat).all()) and float(flat.abs().max()) > 0
        eng.load_model_state(*weights)
        eng.set_loss(C, radius=2)
        mode = eng.verify_matrix_mode(xd, yd)
        print(f'PARITY verify_matrix_mode under {C}: {mode} {getattr(eng, "last_step_check", None)}')
        assert mode in ('f16x3', 'bf16x6')
    finally:
        eng.set_loss('cross_entropy')
        eng.set_loss_boundary(0)
        eng.load_model_state(*weights)


def test_compute_loss_per_image_values(eng, weights):
    from eosvos_amd.helper_func import compute_loss
    xd, yd, _ = masked_frames(12, FRAME, 0.1)
    eng.load_model_state(*weights)
    out = eng.forward(xd)
    out._eosvos_engine = eng
    z, y = out.cpu().view(3, *FRAME), yd.cpu().view(3, *FRAME)
    a = compute_loss(N, out, yd, {'radius': 3})
    ga = dlogits_of(eng, out.numel())
    eng.set_loss_boundary(0)
    b = compute_loss(N + '_3', out, yd)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(ga), bits(dlogits_of(eng, out.numel())))
    ref, _, per_ref = boundary.loss_host(z, y, 3)
    assert abs(float(a) - float(ref)) <= NET_TOL
    per = compute_loss(N + '_3', out, yd, {'batch_average': False})
    print(f'PARITY compute_loss per image: {per.cpu().numpy()} vs {per_ref.numpy()}')
    assert per.shape == (3,) and np.abs(per.cpu().numpy() - per_ref.numpy()).max() <= NET_TOL
    perc = compute_loss(C, out, yd, {'batch_average': False, 'radius': 3})
    refc = [float(boundary.loss_host(z[i], y[i], 3, combined=True)[0]) for i in range(3)]
    assert np.abs(perc.cpu().numpy() - np.array(refc)).max() <= NET_TOL * max(1.0, max(refc))
    eng.set_loss_boundary(0)
    with pytest.raises(ValueError):
        compute_loss(N + '_3', out, yd, {'radius': 2})
