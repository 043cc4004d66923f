"""Weighted sums of the device losses on the MI355X: eosvos_loss_sum / eosvos_loss_sum_tensors / eosvos_set_loss_sum /
eosvos_last_loss_terms through `Engine.loss / loss_of / loss_grad_of / set_loss / last_loss_terms` and `compute_loss`.
pytest -m gpu.

The reference is the engine itself: every term evaluated alone by the existing entry points, combined on the host by
`eosvos_amd.loss_sum.combine_host` (held to the two-rounding rule of include/eosvos.h by tests/test_loss_sum_host.py).  Every
comparison is bit for bit -- there is no tolerance -- with NaN equal to NaN.  Every term list carries a weight that is no power
of two on a term after the first, so a combine launch contracted to fused multiply-adds would be caught.
"""
import ctypes

import numpy as np
import pytest
import torch

from eosvos_amd import loss_sum, synthetic
from loss_common import dlogits_dev as dlogits_of, masked_frames, poke_logits

pytestmark = pytest.mark.gpu

FRAME = (112, 176)
DEV = 'cuda:0'
IGN = 255.0
SUMS = ['lovasz_hinge+0.3*boundary_f_2',
        '0.3*cross_entropy+0.7*dice',
        'class_balanced_cross_entropy+0.3*bootstrapped_cross_entropy_25+lovasz_hinge_flat',
        '0.7*cross_entropy_and_dice+0.3*dice+0.6*lovasz_hinge+0.9*cross_entropy_and_boundary_f_3']
TAILS = '0.3*dice+lovasz_hinge_flat+0.7*bootstrapped_cross_entropy_50+0.9*class_balanced_cross_entropy'
JF = '0.5*lovasz_hinge+0.3*boundary_f_2'


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


def same_bits(a, b):
    """fp32 arrays (or scalars) equal bit for bit, NaN equal to NaN."""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float32)), np.atleast_1d(np.asarray(b, dtype=np.float32))
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint32), b[ok].view(np.uint32))


def f32(t):
    return t.detach().cpu().contiguous().numpy().astype(np.float32, copy=False)


def terms_alone(e, spelled, masks, ign):
    """Every term of `spelled` by `Engine.loss` on the last forward: (values, gradients, weights)."""
    n = masks.numel()
    vals, grads, ws = [], [], []
    for w, term in loss_sum.parse(spelled):
        vals.append(f32(e.loss(term, masks, ignore=ign))[0])
        grads.append(f32(dlogits_of(e, n)))
        ws.append(w)
    return vals, grads, ws


def check_sum_on_forward(e, spelled, masks, ign):
    vals, grads, ws = terms_alone(e, spelled, masks, ign)
    want_loss, want_grad = loss_sum.combine_host(vals, grads, ws)
    got = f32(e.loss(spelled, masks, ignore=ign))[0]
    got_grad = f32(dlogits_of(e, masks.numel()))
    got_terms = e.last_loss_terms()
    print(f'SUM {spelled} ignore={ign}: {got!r} = {ws} x {vals}')
    assert same_bits(got, want_loss), (got, want_loss)
    assert same_bits(got_grad, want_grad), int((got_grad.view(np.uint32) != want_grad.view(np.uint32)).sum())
    assert len(got_terms) == len(vals) and same_bits(np.float32(got_terms), np.float32(vals)), (got_terms, vals)
    if ign is not None:                                      # void pixels keep gradient +0
        assert not got_grad.view(np.uint32)[f32(masks).reshape(-1) == ign].any()
    return got, got_grad


# ---- 1. the rule, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spelled', SUMS)
@pytest.mark.parametrize('void', [False, True])
@pytest.mark.parametrize('B', [1, 3])
def test_the_sum_is_combine_host_of_its_terms(eng, B, void, spelled):
    xd, yd, ym = masked_frames(5, FRAME, 0.1)
    masks = (ym if void else yd)[:B].contiguous()
    ign = IGN if void else None
    try:
        eng.forward(xd[:B].contiguous(), want_logits=False)
        loss, grad = check_sum_on_forward(eng, spelled, masks, ign)
        assert np.isfinite(loss) and grad.any()
        # once more on N(0, 4^2) logits, which keep the hinge and the selection busy
        z = 4.0 * torch.randn(B, 1, *FRAME, generator=torch.Generator().manual_seed(17 + B))
        poke_logits(eng, z.to(DEV).contiguous())
        check_sum_on_forward(eng, spelled, masks, ign)
    finally:
        eng.set_loss_boundary(0)


def test_a_nan_term_makes_the_sum_nan(eng):
    xd, yd, _ = masked_frames(5, FRAME, 0.1)
    eng.forward(xd, want_logits=False)
    z = torch.randn(3, 1, *FRAME, generator=torch.Generator().manual_seed(3))
    z[1, 0, 7, 9] = float('nan')
    poke_logits(eng, z.to(DEV).contiguous())
    loss, _ = check_sum_on_forward(eng, '0.3*cross_entropy+0.7*dice', yd, None)
    assert np.isnan(loss)


# ---- 2. tails and alignment ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [2, 3, 5, 1023, 2049, 4099])
def test_tails_and_an_unaligned_gradient_pointer(eng, n):
    g = torch.Generator().manual_seed(n)
    z = (2.0 * torch.randn(n, generator=g)).to(DEV)
    y = (torch.rand(n, generator=g) < 0.4).float()
    y[0], y[1] = 1.0, 0.0                                   # both classes present
    y = y.to(DEV)
    vals, grads, ws = [], [], []
    for w, term in loss_sum.parse(TAILS):
        vals.append(f32(eng.loss_of(term, z, y))[0])
        grads.append(f32(dlogits_of(eng, n)))
        ws.append(w)
        one, one_grad = eng.loss_grad_of(term, z, y)        # a single kind through the new entry: that kind's bits
        assert same_bits(f32(one), vals[-1]) and same_bits(f32(one_grad), grads[-1]), term
    want_loss, want_grad = loss_sum.combine_host(vals, grads, ws)
    loss, grad = eng.loss_grad_of(TAILS, z, y)
    assert grad.shape == z.shape
    assert same_bits(f32(loss), want_loss) and same_bits(f32(grad), want_grad)
    assert same_bits(np.float32(eng.last_loss_terms()), np.float32(vals))
    assert same_bits(f32(eng.loss_of(TAILS, z, y)), want_loss)              # the value-only entry, gradient in the scratch
    assert same_bits(f32(dlogits_of(eng, n)), want_grad)
    # the same call with dlogits_out one element into a larger buffer: 4-byte aligned only, and nothing written around it
    kinds, weights, _, _, _ = loss_sum.resolve(TAILS)
    sentinel = np.float32(-12345.678)
    buf = torch.full((n + 9,), float(sentinel), device=DEV)
    out = torch.empty(1, device=DEV)
    assert buf.data_ptr() % 16 == 0
    rc = eng.lib.eosvos_loss_sum_tensors(eng.h, len(kinds), (ctypes.c_int * len(kinds))(*kinds),
                                         (ctypes.c_float * len(kinds))(*weights), ctypes.c_void_p(z.data_ptr()),
                                         ctypes.c_void_p(y.data_ptr()), n, 0, 0.0, ctypes.c_void_p(out.data_ptr()),
                                         ctypes.c_void_p(buf.data_ptr() + 4))
    assert rc == 0, eng.lib.eosvos_last_error()
    eng.synchronize()
    got = f32(buf)
    assert same_bits(got[1:n + 1], want_grad) and same_bits(f32(out), want_loss)
    assert same_bits(got[:1], [sentinel]) and same_bits(got[n + 1:], np.full(8, sentinel, np.float32))


# ---- 3. a single name goes where it went ------------------------------------------------------------------------------------
def test_a_single_name_keeps_its_bits_and_twice_dice_is_twice_dice(eng):
    xd, yd, ym = masked_frames(6, FRAME, 0.1)
    eng.forward(xd, want_logits=False)
    n = ym.numel()
    before = f32(eng.loss('dice', ym, ignore=IGN)), f32(dlogits_of(eng, n))
    twice = f32(eng.loss('2*dice', ym, ignore=IGN)), f32(dlogits_of(eng, n))
    assert eng.last_loss_terms() == [float(before[0][0])]
    eng.loss(SUMS[3], ym, ignore=IGN)
    eng.set_loss_boundary(0)
    after = f32(eng.loss('dice', ym, ignore=IGN)), f32(dlogits_of(eng, n))
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    assert same_bits(twice[0], np.float32(2) * before[0]) and same_bits(twice[1], np.float32(2) * before[1])


# ---- 4. the fused step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ign', [None, IGN])
def test_fused_step_equals_the_separate_calls(eng, weights, ign):
    """set_loss(sum, ignore=v) + finetune_step == forward -> loss(sum) -> backward_step, bit for bit; set_loss('dice') then
    leaves no trace of the sum."""
    xd, yd, ym = masked_frames(4, FRAME, 0.1)
    masks = yd if ign is None else ym
    try:
        eng.load_model_state(*weights)
        eng.set_loss_boundary(5)                             # the suffix must win over what the engine held
        eng.set_loss(JF, ignore=ign)
        fused = [eng.finetune_step(xd, masks) for _ in range(2)]
        fused_terms = eng.last_loss_terms()
        p_fused = eng.get_params().clone()
        eng.set_loss('dice', ignore=ign)
        fused.append(eng.finetune_step(xd, masks))
        p_fused_dice = eng.get_params().clone()

        eng.load_model_state(*weights)
        sep = []
        for _ in range(2):
            eng.forward(xd, want_logits=False)
            sep.append(float(eng.loss(JF, masks, ignore=ign)))
            eng.backward_step()
        sep_terms = eng.last_loss_terms()
        p_sep = eng.get_params().clone()
        eng.forward(xd, want_logits=False)
        sep.append(float(eng.loss('dice', masks, ignore=ign)))
        eng.backward_step()
        p_sep_dice = eng.get_params().clone()
    finally:
        eng.set_loss('cross_entropy')
        eng.set_loss_boundary(0)
        eng.load_model_state(*weights)
    print(f'SUM fused step ignore={ign}: {fused} terms {fused_terms}')
    assert same_bits(np.float32(fused), np.float32(sep)), (fused, sep)
    assert len(fused_terms) == 2 and same_bits(np.float32(fused_terms), np.float32(sep_terms))
    assert torch.equal(p_fused, p_sep) and torch.equal(p_fused_dice, p_sep_dice)
    assert not torch.equal(p_fused, p_fused_dice)
    w = [np.float32(x) for x, _ in loss_sum.parse(JF)]
    assert same_bits(fused[1], np.float32(w[0] * np.float32(fused_terms[0])) + np.float32(w[1] * np.float32(fused_terms[1])))


def test_a_sum_that_was_set_leaves_no_trace_in_a_single_kind(eng, weights):
    """set_loss('2*dice') then set_loss('dice'): the fused step has the bits of an engine that never saw a sum, and
    last_loss_terms goes on reporting the last sum that was evaluated -- on an engine that evaluated none, it goes on raising."""
    from eosvos_amd.engine import Engine
    xd, yd, _ = masked_frames(10, FRAME, 0.1)
    clean = Engine('resnet50', *FRAME, max_batch=3, device=DEV)
    try:
        got = []
        for names in (('dice',), ('2*dice', 'dice')):
            clean.load_model_state(*weights)
            for name in names:
                clean.set_loss(name)
            got.append((clean.finetune_step(xd, yd), clean.get_params().clone()))
            with pytest.raises(RuntimeError, match='no loss sum'):
                clean.last_loss_terms()
    finally:
        clean.close()
    try:
        eng.load_model_state(*weights)
        eng.forward(xd, want_logits=False)
        eng.loss('2*dice', yd)
        terms = eng.last_loss_terms()
        eng.set_loss('2*dice')
        eng.set_loss('dice')
        got.append((eng.finetune_step(xd, yd), eng.get_params().clone()))
        assert len(terms) == 1 and eng.last_loss_terms() == terms
    finally:
        eng.set_loss('cross_entropy')
        eng.load_model_state(*weights)
    for loss, params in got[1:]:
        assert same_bits(loss, got[0][0]) and torch.equal(params, got[0][1])


# ---- 5. meta_grad and the matrix-mode guard ---------------------------------------------------------------------------------
def test_meta_grad_and_the_matrix_mode_guard_run_under_a_sum(eng, weights):
    xd, yd, ym = masked_frames(8, FRAME, 0.1)
    try:
        eng.load_model_state(*weights)
        eng.set_loss(JF, ignore=IGN)
        eng.meta_task_begin()
        eng.finetune_step(xd, ym, accumulate=True)
        flat = torch.zeros(eng.n_lr + eng.n_param, device=DEV)
        ml = eng.meta_grad(xd, ym, flat)
        terms = eng.last_loss_terms()
        vals, _, ws = terms_alone(eng, JF, ym, IGN)          # the single kinds on the logits of the meta forward
        want, _ = loss_sum.combine_host(vals, None, ws)
        print(f'SUM meta_grad: {ml} terms {terms}')
        assert same_bits(ml, want) and same_bits(np.float32(terms), np.float32(vals))
        assert bool(torch.isfinite(flat).all()) and float(flat.abs().max()) > 0
        eng.load_model_state(*weights)
        eng.set_loss(JF)
        mode = eng.verify_matrix_mode(xd, yd)                # the fused step in both split modes
        print(f'SUM verify_matrix_mode, fused: {mode} {getattr(eng, "last_step_check", None)}')
        assert mode in ('f16x3', 'bf16x6')
        eng.load_model_state(*weights)
        mode = eng.verify_matrix_mode(xd, yd, loss_kind=JF)   # the loss re-run by its name
        print(f'SUM verify_matrix_mode, by name: {mode} {getattr(eng, "last_step_check", None)}')
        assert mode in ('f16x3', 'bf16x6')
    finally:
        eng.set_loss('cross_entropy')
        eng.set_loss_boundary(0)
        eng.load_model_state(*weights)


# ---- 6. compute_loss -------------------------------------------------------------------------------------------------------
def test_compute_loss(eng, weights):
    from eosvos_amd.helper_func import compute_loss
    xd, yd, ym = masked_frames(12, FRAME, 0.1)
    spelled = 'lovasz_hinge+0.3*boundary_f_3'
    try:
        eng.load_model_state(*weights)
        out = eng.forward(xd)
        out._eosvos_engine = eng
        n = out.numel()
        want, want_grad = check_sum_on_forward(eng, spelled, ym, IGN)
        eng.set_loss_boundary(0)
        a = compute_loss(spelled, out, ym, {'ignore': IGN})
        assert a.dim() == 0 and a._eosvos_engine is eng
        assert same_bits(f32(a), want) and same_bits(f32(dlogits_of(eng, n)), want_grad)
        eng.set_loss_boundary(0)
        b = compute_loss('lovasz_hinge+0.3*boundary_f', out, ym, {'ignore': IGN, 'radius': 3})      # the keyword is the suffix
        assert same_bits(f32(b), want) and same_bits(f32(dlogits_of(eng, n)), want_grad)
        flat = compute_loss(spelled, out, ym, {'ignore': IGN, 'per_image': False})
        flat_ref = eng.loss('lovasz_hinge_flat+0.3*boundary_f_3', ym, ignore=IGN)
        assert same_bits(f32(flat), f32(flat_ref)) and not same_bits(f32(flat), want)
        # per sample: every term takes the sample as one set
        per = compute_loss(spelled, out, ym, {'batch_average': False, 'ignore': IGN})
        assert per.shape == (3,)
        for i in range(3):
            vals = [f32(eng.loss_of(term, out[i], ym[i], ignore=IGN))[0] for _, term in loss_sum.parse(spelled)]
            ref, _ = loss_sum.combine_host(vals, None, [w for w, _ in loss_sum.parse(spelled)])
            assert same_bits(f32(per[i]), ref), (i, per[i], ref)
        with pytest.raises(ValueError):
            compute_loss('0.3*cross_entropy+0.7*dice', out, yd, {'radius': 3})
        with pytest.raises(ValueError):
            compute_loss(spelled, out, yd, {'radius': 2})
    finally:
        eng.set_loss_boundary(0)


# ---- 7. failure is contained -----------------------------------------------------------------------------------------------
def test_a_failed_term_fails_the_sum_and_nothing_else(eng):
    xd, yd, _ = masked_frames(6, FRAME, 0.1)
    eng.forward(xd, want_logits=False)
    z, y = torch.randn(1000, device=DEV), (torch.rand(1000, device=DEV) < 0.5).float()
    with pytest.raises(RuntimeError, match='H \\* W'):
        eng.loss_of('dice+boundary_f', z, y)
    with pytest.raises(RuntimeError, match='H \\* W'):
        eng.loss_grad_of('boundary_f', z, y)
    assert np.isfinite(f32(eng.loss_of('dice', z, y))[0])
    assert np.isfinite(f32(eng.loss('0.3*cross_entropy+0.7*dice', yd))[0])
    # the library's own checks
    one = (ctypes.c_int * 5)(1, 0, 4, 6, 3), (ctypes.c_float * 5)(1, 1, 1, 1, 1)
    for n_terms, kinds, ws, msg in ((0, *one, b'1 .. 4 terms'), (5, *one, b'1 .. 4 terms'),
                                    (2, (ctypes.c_int * 2)(1, 7), one[1], b'unknown loss kind'),
                                    (2, (ctypes.c_int * 2)(1, 1), one[1], b'twice'),
                                    (2, (ctypes.c_int * 2)(8, 9), one[1], b'one boundary kind'),
                                    (2, one[0], (ctypes.c_float * 2)(1, 0), b'finite and > 0'),
                                    (2, one[0], (ctypes.c_float * 2)(1, -1), b'finite and > 0'),
                                    (2, one[0], (ctypes.c_float * 2)(float('inf'), 1), b'finite and > 0'),
                                    (2, one[0], (ctypes.c_float * 2)(float('nan'), 1), b'finite and > 0')):
        assert eng.lib.eosvos_set_loss_sum(eng.h, n_terms, kinds, ws) != 0
        assert msg in eng.lib.eosvos_last_error(), (msg, eng.lib.eosvos_last_error())
    assert np.isfinite(f32(eng.loss('dice', yd))[0])


# ---- 8. reproducible -------------------------------------------------------------------------------------------------------
def test_two_evaluations_are_bit_identical_also_from_a_dirty_scratch(eng):
    xd, _, ym = masked_frames(9, FRAME, 0.1)
    eng.forward(xd, want_logits=False)
    n = ym.numel()
    try:
        a = f32(eng.loss(SUMS[0], ym, ignore=IGN)), f32(dlogits_of(eng, n))
        b = f32(eng.loss(SUMS[0], ym, ignore=IGN)), f32(dlogits_of(eng, n))
        eng.loss(SUMS[3], ym, ignore=IGN)                    # four slices written by other kinds
        c = f32(eng.loss(SUMS[0], ym, ignore=IGN)), f32(dlogits_of(eng, n))
    finally:
        eng.set_loss_boundary(0)
    assert np.isfinite(a[0][0]) and a[1].any()
    for other in (b, c):
        assert same_bits(a[0], other[0]) and same_bits(a[1], other[1])
