"""The void label (`ignore`) of every device loss on the MI355X: eosvos_loss_ignore / eosvos_loss_tensors_ignore /
eosvos_set_loss_ignore / eosvos_propagation_targets against the fp64 restatements of tests/loss_ignore_ref.py, against the
unmasked entry points (bit for bit where no pixel is void), against the reference's `lovasz_hinge(..., ignore=255)`
(tests/golden/lovasz_ignore.npz), through the fused step, and through online adaptation with an uncertainty band.
pytest -m gpu.

Bounds.  Lovasz kinds: test_gpu_lovasz.py's (gradient 1e-6 of the fp64 value elementwise, loss 1e-5 relative, the same set of
non-zero entries; against the fixture the stored reference noise + 1e-5 relative for the loss, twice that noise + 1e-6 of
max |grad| for the gradient).  BCE, dice, BCE + dice and class-balanced BCE: what test_gpu_parity.py asserts for the unmasked
kinds against the oracle: loss within 1e-5 * max(1, |loss|) (test_dice_losses_vs_oracle; 2e-6 for BCE,
test_loss_and_grad_vs_golden), dL/dlogits within 1e-4 of max |dL/dlogits| + 1e-10.  The gradient at a void pixel is exactly +0.
Every check prints its measured margin (MARGIN lines, pytest -s) before it asserts.
"""
import ctypes

import numpy as np
import pytest
import torch

import loss_ignore_ref as R
from loss_common import dev, dlogits_of, masked_frames, poke_logits, void_mask
from eosvos_amd import synthetic

pytestmark = pytest.mark.gpu

SMALL = (96, 160)
DEV = 'cuda:0'
IGN = 255.0
GRAD_RTOL, LOSS_RTOL = 1e-6, 1e-5                       # Lovasz (test_gpu_lovasz.py)
LOSS_TOL = {'cross_entropy': 2e-6, 'dice': 1e-5, 'cross_entropy_and_dice': 1e-5, 'class_balanced_cross_entropy': 1e-5}
DLOGITS_TOL = 1e-4                                      # of max |dL/dlogits| (+ 1e-10)
LOVASZ = ('lovasz_hinge', 'lovasz_hinge_flat')
PATTERNS = ('none', 'all', 'random30', 'block', 'last_valid')


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
    x = (3.0 * rng.randn(n)).astype(np.float32)
    t = (rng.rand(n) < 0.3).astype(np.float32)
    void = void_mask(n, pattern, rng)
    t[void] = IGN
    return x, t, void


def check(tag, kind, loss, grad, ref_loss, ref_grad, void):
    """Prints the measured margins, then asserts the module's bounds."""
    grad, ref_grad = np.asarray(grad, dtype=np.float64).reshape(-1), np.asarray(ref_grad, dtype=np.float64).reshape(-1)
    void = np.asarray(void).reshape(-1)
    assert np.isfinite(loss) and np.isfinite(grad).all(), tag
    assert not grad[void].any() and not np.signbit(grad[void]).any(), f'{tag}: gradient at a void pixel is not +0'
    if kind in LOVASZ:
        nz = ref_grad != 0
        rel = float((np.abs(grad[nz] - ref_grad[nz]) / np.abs(ref_grad[nz])).max()) if nz.any() else 0.0
        lrel = abs(loss - ref_loss) / abs(ref_loss) if ref_loss != 0 else abs(loss)
        print(f'MARGIN {tag}: loss {loss:.9g} vs {ref_loss:.12g} rel {lrel:.2e}; grad worst elementwise rel {rel:.2e}')
        assert np.array_equal(grad != 0, nz), f'{tag}: the sets of non-zero gradient entries differ'
        assert rel <= GRAD_RTOL and lrel <= LOSS_RTOL, (tag, rel, lrel)
        return
    dl, dg, gmax = abs(loss - ref_loss), float(np.abs(grad - ref_grad).max()), float(np.abs(ref_grad).max())
    print(f'MARGIN {tag}: loss {loss:.9g} vs {ref_loss:.12g} diff {dl:.2e} (allowed {LOSS_TOL[kind] * max(1.0, abs(ref_loss)):.2e}); '
          f'dlogits diff {dg:.2e} (allowed {DLOGITS_TOL * gmax + 1e-10:.2e})')
    assert dl <= LOSS_TOL[kind] * max(1.0, abs(ref_loss)), tag
    assert dg <= DLOGITS_TOL * gmax + 1e-10, tag


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('n', [1, 255, 257, 769, 4097])
@pytest.mark.parametrize('kind', R.KINDS)
def test_one_set_vs_fp64_restatement(eng, kind, n, pattern):
    """eosvos_loss_tensors_ignore (`loss_of`): loss and gradient of every kind, sizes around the 256-element block; at 769 and
    4097 the 'block' pattern is a wholly void block between valid ones (up to 257 it cannot but be 'all')."""
    x, t, void = make_case(n, pattern, seed=n + 7 * PATTERNS.index(pattern))
    ref_loss, ref_grad = R.one_set(kind, x, t, IGN)
    loss = float(eng.loss_of(kind, dev(x), dev(t), ignore=IGN))
    check(f'{kind} n={n} {pattern}', kind, loss, dlogits_of(eng, n), ref_loss, ref_grad, void)
    if pattern == 'all':
        assert loss == 0.0


@pytest.mark.parametrize('kind', R.KINDS)
def test_without_a_void_pixel_the_bits_are_those_of_the_plain_call(eng, kind):
    """Both eosvos_loss*_ignore forms against eosvos_loss / eosvos_loss_tensors: loss and dlogits bit for bit."""
    n = 3 * SMALL[0] * SMALL[1]
    x, t, _ = make_case(n, 'none', seed=41)
    xd, td = dev(x), dev(t)
    for m in (4097, n):                                               # one block row of the grid, and the whole buffer
        a = eng.loss_of(kind, xd[:m], td[:m]).cpu().numpy().view(np.uint32)
        ga = dlogits_of(eng, m).view(np.uint32).copy()
        b = eng.loss_of(kind, xd[:m], td[:m], ignore=IGN).cpu().numpy().view(np.uint32)
        gb = dlogits_of(eng, m).view(np.uint32)
        assert np.array_equal(a, b) and np.array_equal(ga, gb), (kind, m)
    poke_logits(eng, xd)
    masks = td.view(3, 1, *SMALL)
    a = eng.loss(kind, masks).cpu().numpy().view(np.uint32)
    ga = dlogits_of(eng, n).view(np.uint32).copy()
    b = eng.loss(kind, masks, ignore=-1.0).cpu().numpy().view(np.uint32)
    gb = dlogits_of(eng, n).view(np.uint32)
    assert np.array_equal(a, b) and np.array_equal(ga, gb), kind


BIG = (296, 296)                                        # batch 3: the engine's scratch holds BIG_N elements
BIG_N = 1024 * 256 + 257


@pytest.fixture(scope='module')
def big_eng(weights):
    from eosvos_amd.engine import Engine
    e = Engine('resnet50', *BIG, max_batch=3, device=DEV)
    e.load_model_state(*weights)
    x, _ = synthetic.synthetic_frames(3, *BIG, seed=3)
    e.forward(x.to(DEV), want_logits=False)
    yield e
    e.close()


@pytest.mark.parametrize('pattern', ['none', 'random30'])
@pytest.mark.parametrize('kind', [k for k in R.KINDS if k not in LOVASZ])
def test_second_trip_of_the_partial_grid(big_eng, kind, pattern):
    """The partial grids cap at 1024 blocks of 256 threads: 1024 * 256 + 257 elements is the smallest size at which the
    grid-stride loop runs a second time, with a ragged tail.  (The Lovasz grids are per tile and run at 3 x 480 x 854 in
    test_gpu_lovasz.py.)  Without a void pixel: the bits of the plain call; with 30 % void: the fp64 restatement."""
    n = BIG_N
    x, t, void = make_case(n, pattern, seed=53)
    xd, td = dev(x), dev(t)
    loss = big_eng.loss_of(kind, xd, td, ignore=IGN).cpu().numpy()
    grad = dlogits_of(big_eng, n).copy()
    if pattern == 'none':
        plain = big_eng.loss_of(kind, xd, td).cpu().numpy()
        assert np.array_equal(loss.view(np.uint32), plain.view(np.uint32)), (kind, loss, plain)
        assert np.array_equal(grad.view(np.uint32), dlogits_of(big_eng, n).view(np.uint32)), kind
    else:
        ref_loss, ref_grad = R.one_set(kind, x, t, IGN)
        check(f'{kind} n={n} {pattern}', kind, float(loss[0]), grad, ref_loss, ref_grad, void)


@pytest.mark.parametrize('kind', R.KINDS)
def test_non_finite_logits_at_void_pixels_never_reach_the_loss(eng, kind):
    n = 4097
    x, t, void = make_case(n, 'random30', seed=5)
    clean = x.copy()
    clean[void] = 0.0
    bad = x.copy()
    bad[void] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[np.arange(int(void.sum())) % 3]
    a = eng.loss_of(kind, dev(clean), dev(t), ignore=IGN).cpu().numpy()
    ga = dlogits_of(eng, n).copy()
    b = eng.loss_of(kind, dev(bad), dev(t), ignore=IGN).cpu().numpy()
    gb = dlogits_of(eng, n)
    assert np.isfinite(b).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (kind, a, b)
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))


@pytest.mark.parametrize('kind', ['lovasz_hinge', 'lovasz_hinge_flat', 'cross_entropy', 'dice', 'class_balanced_cross_entropy'])
def test_batch3_through_eosvos_loss_ignore(eng, kind):
    """On the engine's own logits: image 1 all void, image 2 without void, image 0 30 % void.  Per image the Lovasz mean is
    over all 3 images; class-balanced BCE keeps the divisions by the full shape."""
    P = SMALL[0] * SMALL[1]
    x, t, void = make_case(3 * P, 'random30', seed=17)
    t, void = t.reshape(3, P), void.reshape(3, P)
    t[1], void[1] = IGN, True
    t[2] = np.where(void[2], 0.0, t[2])
    void[2] = False
    poke_logits(eng, dev(x))
    loss = float(eng.loss(kind, dev(t).view(3, 1, *SMALL), ignore=IGN))
    ref_loss, ref_grad = R.batch(kind, x.reshape(3, P), t, IGN)
    check(f'{kind} batch 3', kind, loss, dlogits_of(eng, 3 * P), ref_loss, ref_grad, void)


@pytest.mark.parametrize('tag,kind', [('per_image', 'lovasz_hinge'), ('flat', 'lovasz_hinge_flat')])
def test_vs_reference_fixture(golden_dir, weights, tag, kind):
    """The unmodified reference's `lovasz_hinge(..., ignore=255)` and its autograd gradient, B = 3 at 40 x 64."""
    import os
    from eosvos_amd.engine import Engine
    g = np.load(os.path.join(golden_dir, 'lovasz_ignore.npz'))
    x, t, ign = g['logits'], g['labels'].astype(np.float32), float(g['ignore'])
    b, h, w = x.shape
    e = Engine('resnet50', h, w, max_batch=b, device=DEV)
    try:
        e.load_model_state(*weights)
        frames, _ = synthetic.synthetic_frames(b, h, w, seed=1)
        e.forward(frames.to(DEV), want_logits=False)
        poke_logits(e, dev(x))
        loss = float(e.loss(kind, dev(t).view(b, 1, h, w), ignore=ign))
        grad = dlogits_of(e, x.size).reshape(x.shape)
    finally:
        e.close()
    ref_loss, ref_grad = float(g[f'{tag}_loss']), g[f'{tag}_dlogits']
    noise_l, noise_g = float(g[f'{tag}_ref_vs_f64_loss']), float(g[f'{tag}_ref_vs_f64_grad'])
    dl, dg = abs(loss - ref_loss), float(np.abs(grad - ref_grad).max())
    gmax = float(np.abs(ref_grad).max())
    print(f'MARGIN fixture {tag}: loss diff {dl:.2e} (allowed {noise_l + LOSS_RTOL * abs(ref_loss):.2e}); '
          f'grad diff {dg:.2e} (allowed {(2 * noise_g + 1e-6) * gmax:.2e})')
    assert dl <= noise_l + LOSS_RTOL * abs(ref_loss)
    assert dg <= (2 * noise_g + 1e-6) * gmax
    assert not grad[t == ign].any()


@pytest.mark.parametrize('bad', [0.5, 0.0, 1.0, float('nan'), float('inf')])
def test_bad_ignore_is_rejected_by_the_library(eng, bad):
    """The C entry points themselves (the Python wrapper checks first): an error, nothing launched."""
    n = 255
    xd, td, out = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(1, device=DEV)
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    assert eng.lib.eosvos_loss_tensors_ignore(eng.h, 0, p(xd), p(td), n, bad, p(out)) != 0
    assert b'ignore' in eng.lib.eosvos_last_error()
    assert eng.lib.eosvos_set_loss_ignore(eng.h, 1, bad) != 0
    assert eng.lib.eosvos_propagation_targets(eng.h, p(xd), 1, n, 0.3, 0.7, bad, p(td), None) != 0
    with pytest.raises(ValueError):
        eng.loss_of('dice', xd, td, ignore=bad)
    with pytest.raises(ValueError):
        eng.set_loss('dice', ignore=bad)


@pytest.mark.parametrize('kind', ['cross_entropy', 'dice', 'lovasz_hinge'])
def test_fused_step_equals_the_separate_calls(eng, weights, kind):
    """set_loss(kind, ignore=v) + finetune_step == forward -> loss(kind, masks, ignore=v) -> backward_step, bit for bit."""
    xd, _, ym = masked_frames(4, SMALL, 0.3)
    eng.load_model_state(*weights)
    eng.set_loss(kind, ignore=IGN)
    try:
        fused = [eng.finetune_step(xd, ym) for _ in range(2)]
        p_fused = eng.get_params().clone()
    finally:
        eng.set_loss('cross_entropy')
    eng.load_model_state(*weights)
    sep = []
    for _ in range(2):
        eng.forward(xd, want_logits=False)
        sep.append(float(eng.loss(kind, ym, ignore=IGN)))
        eng.backward_step()
    p_sep = eng.get_params()
    eng.load_model_state(*weights)
    assert np.array_equal(np.float32(fused).view(np.uint32), np.float32(sep).view(np.uint32)), (fused, sep)
    assert torch.equal(p_fused, p_sep)


def test_the_fused_flag_is_live_and_off_by_default(eng, weights):
    """One BCE step with 30 % void differs from the same step without ignore; set_loss(name) alone turns it off again."""
    xd, yd, ym = masked_frames(6, SMALL, 0.3)
    y0 = torch.where(ym == IGN, torch.zeros_like(ym), ym)               # the same targets with the void pixels as background
    got = {}
    for tag, ign, masks in (('ignore', IGN, ym), ('plain', None, y0), ('after', None, y0)):
        eng.load_model_state(*weights)
        if tag == 'ignore':
            eng.set_loss('cross_entropy', ignore=ign)
        elif tag == 'after':
            eng.set_loss('cross_entropy', ignore=IGN)
            eng.set_loss('cross_entropy')
        loss = eng.finetune_step(xd, masks)
        got[tag] = (loss, eng.get_params().clone())
        eng.set_loss('cross_entropy')
    eng.load_model_state(*weights)
    logits = eng.forward(xd).cpu().numpy()
    ref, _ = R.bce(logits, ym.cpu().numpy(), IGN)
    assert abs(got['ignore'][0] - ref) <= LOSS_TOL['cross_entropy'] * max(1.0, abs(ref))
    assert got['ignore'][0] != got['plain'][0] and not torch.equal(got['ignore'][1], got['plain'][1])
    assert got['after'][0] == got['plain'][0] and torch.equal(got['after'][1], got['plain'][1])


def test_a_new_engine_and_an_aliasing_engine_do_not_take_the_void_label_over(eng, weights):
    """The flag is per engine and off by default: a second engine (what `spawn` builds) steps on void-labelled masks as the
    plain loss does, also while it aliases the state of an engine whose flag is on; that engine's own flag stays on."""
    from eosvos_amd.engine import Engine
    xd, _, ym = masked_frames(10, SMALL, 0.3)
    got = {}
    for tag, ign in (('on', IGN), ('off', None)):
        eng.load_model_state(*weights)
        eng.set_loss('cross_entropy', ignore=ign)
        got[tag] = (eng.finetune_step(xd, ym), eng.get_params().clone())
    eng.load_model_state(*weights)
    eng.set_loss('cross_entropy', ignore=IGN)
    other = Engine('resnet50', *SMALL, max_batch=3, device=DEV)
    try:
        for tag in ('fresh', 'aliasing'):
            other.load_model_state(*weights)
            if tag == 'aliasing':
                other.alias_state(eng)
            loss = other.finetune_step(xd, ym)
            assert loss == got['off'][0] and torch.equal(other.get_params(), got['off'][1]), tag
        assert got['on'][0] != got['off'][0]
        loss = eng.finetune_step(xd, ym)                                # the source's own flag is still on
        assert loss == got['on'][0] and torch.equal(eng.get_params(), got['on'][1])
    finally:
        other.unalias_state()
        other.close()
        eng.set_loss('cross_entropy')
        eng.load_model_state(*weights)


def test_meta_grad_runs_with_the_void_label(eng, weights):
    xd, yd, ym = masked_frames(8, SMALL, 0.3)
    eng.load_model_state(*weights)
    eng.set_loss('dice', ignore=IGN)
    try:
        eng.meta_task_begin()
        eng.finetune_step(xd, ym, accumulate=True)
        flat = torch.zeros(eng.n_lr + eng.n_param, device=DEV)
        ml = eng.meta_grad(xd, ym, flat)
        logits = eng.debug_tensor('logits').cpu().numpy()
        ref, _ = R.dice(logits, ym.cpu().numpy(), IGN)
        plain, _ = R.dice(logits, torch.where(ym == IGN, torch.zeros_like(ym), ym).cpu().numpy())
        print(f'MARGIN meta_grad dice with ignore: {ml} vs {ref} (without ignore {plain})')
        assert abs(ml - ref) <= LOSS_TOL['dice'] * max(1.0, abs(ref)) and abs(ref - plain) > 1e-3
        assert bool(torch.isfinite(flat).all()) and float(flat.abs().max()) > 0
    finally:
        eng.set_loss('cross_entropy')
        eng.load_model_state(*weights)


def test_propagation_targets(eng):
    """Maps and per-frame counts for (lo, hi) = (0.3, 0.7): exact 0.3 (void: not < lo) and 0.7 (positive), a frame without
    positives, an odd pixel count with more than one block per frame; identical counts over two calls."""
    rng = np.random.RandomState(9)
    F, P = 4, 4097
    p = rng.rand(F, P).astype(np.float32)
    p[0, :4] = [0.3, 0.7, np.nextafter(np.float32(0.3), np.float32(0)), np.nextafter(np.float32(0.7), np.float32(0))]
    p[2] = np.minimum(p[2], np.float32(0.69))                          # no positive pixel
    lo, hi = np.float32(0.3), np.float32(0.7)
    want = np.where(p >= hi, np.float32(1), np.where(p < lo, np.float32(0), np.float32(IGN)))
    counts = [int((row >= hi).sum()) for row in p]
    assert want[0, :4].tolist() == [IGN, 1.0, 0.0, IGN] and counts[2] == 0 and min(counts[0], counts[1], counts[3]) > 0
    pd = dev(p)
    out1, n1 = eng.propagation_targets(pd, 0.3, 0.7, IGN)
    out2, n2 = eng.propagation_targets(pd, 0.3, 0.7, IGN)
    assert n1 == counts and n2 == counts
    assert np.array_equal(out1.cpu().numpy(), want) and torch.equal(out1, out2)
    out3, n3 = eng.propagation_targets(pd.view(F, 1, 17, 241), 0.3, 0.7, -1.0, counts=False)
    assert n3 is None and out3.shape == (F, 1, 17, 241)
    assert np.array_equal(out3.cpu().numpy().reshape(F, P), np.where(want == IGN, np.float32(-1), want))
    with pytest.raises(ValueError):
        eng.propagation_targets(pd, 0.7, 0.3, IGN)


# ---- online adaptation ------------------------------------------------------------------------------------------------
BN_CFG = {'accum_stats': False, 'learn_weight': False, 'learn_bias': False}
MO_CFG = dict(init_lr=1e-3, learn_model_init=True, second_order_gradients=False, lr_hierarchy_level='NEURON',
              use_log_init_lr=False, max_lr=None)


def finetune_object_before_the_band(model, meta_optim, meta_optim_state_dict, frames, gt, cfg):
    """`evaluate.finetune_object` as it was before `min_prop` could be a band (repeated batch, train frame 0): what a scalar
    `min_prop` must still compute."""
    from eosvos_amd.evaluate import INFER_BATCH, online_adapt_schedule
    from eosvos_amd.helper_func import compute_loss, early_stopping, set_random_seeds
    n = frames.shape[0]
    ona = cfg['eval_online_adapt']
    bsz = cfg['data_cfg']['batch_sizes']['train']
    es = cfg.get('train_early_stopping_cfg', {'patience': None, 'min_loss_improv': 0.001})
    loss_func = cfg.get('loss_func', 'cross_entropy')
    gt = gt.to(frames.device).float().view(1, 1, *gt.shape[-2:])
    masks = torch.zeros(n, 1, *frames.shape[-2:], device=frames.device)
    masks[0] = 2 * gt[0]
    hist = []
    for r, rd in enumerate(online_adapt_schedule(n, 0, ona['step'], bsz)):
        if r == 0 or ona['reset_model_mode'] == 'FULL':
            meta_optim.load_state_dict(meta_optim_state_dict)
            meta_optim.reset()
            meta_optim.eval()
        elif ona['reset_model_mode'] == 'FIRST_STEP':
            meta_optim.load_state_dict(meta_optim_state_dict)
            if model._dirty:
                model.push_state()
            model.engine.restore()
            meta_optim.eval()
        num_epochs = cfg['num_epochs']['eval'] if r == 0 else ona['num_epochs']
        model.train_without_dropout()
        round_hist = []
        if r > 0:
            round_inputs, round_gts = frames[0:1], gt
            for f in rd['propagate_frames']:
                pg = masks[f:f + 1].ge(ona['min_prop']).float()
                if pg.sum().item() != 0:
                    round_inputs = torch.cat([round_inputs, frames[f:f + 1]])
                    round_gts = torch.cat([round_gts, pg])
            round_inputs, round_gts = round_inputs.contiguous(), round_gts.contiguous()
        for epoch in range(1, num_epochs + 1):
            set_random_seeds(cfg.get('seed', 1) + epoch + r)
            if r == 0:
                inputs, gts = frames[0:1].expand(bsz, -1, -1, -1).contiguous(), gt.expand(bsz, -1, -1, -1).contiguous()
            else:
                inputs, gts = round_inputs, round_gts
            outputs = model(inputs)
            train_loss = compute_loss(loss_func, outputs[-1], gts)
            model.zero_grad()
            meta_optim.set_train_loss(train_loss)
            meta_optim.step(train_loss)
            meta_optim.meta_model.detach_param_groups()
            round_hist.append(train_loss.item())
            if early_stopping(round_hist, **es):
                break
        hist.append(round_hist)
        if r == 0:
            model.engine.snapshot()
        model.eval()
        nb = max(1, min(int(getattr(model.engine, 'max_batch', 1)), INFER_BATCH))
        for f in range(rd['eval_min'], rd['eval_max'], nb):
            g = min(f + nb, rd['eval_max'])
            masks[f:g] = model.engine.infer(frames[f:g].contiguous())
    return masks[:, 0], hist


def test_online_adaptation_with_an_uncertainty_band():
    """step 2, 2 + 2 iterations, 5 frames: the band run finishes and differs from the scalar run; the scalar run is the
    run of the code before the band existed, bit for bit."""
    from eosvos_amd import evaluate
    from eosvos_amd.helper_func import init_parent_model
    from eosvos_amd.meta_optim import MetaOptimizer
    from eosvos_amd import topology
    model, _ = init_parent_model(architecture='DeepLabV3Plus', encoder='resnet50', train_encoder=True,
                                 decoder_norm_layer='BatchNorm2d', replace_batch_with_group_norms=False, batch_norm=BN_CFG,
                                 roi_pool_output_sizes=None, eval_augment_rpn_proposals_mode=None, box_nms_thresh=None,
                                 maskrcnn_loss=None)
    sd, lrs = synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50')
    msd = {}
    for (n, _), lr in zip(topology.trainable('resnet50'), lrs):
        msd['log_init_lr_' + n.replace('.', '-')] = lr.clone()
    for n, _ in topology.trainable('resnet50'):
        msd['model_init_' + n.replace('.', '-')] = sd[n].clone()
    model.load_state_dict(sd)
    mo = MetaOptimizer(model, **MO_CFG)
    H, W, N = SMALL[0], SMALL[1], 5
    frames, gt = synthetic.synthetic_frames(1, H, W, seed=3)
    seq = torch.cat([torch.roll(frames, shifts=4 * i, dims=3) for i in range(N)]).to(DEV)
    cfg = {'eval_online_adapt': {'step': 2, 'reset_model_mode': 'FIRST_STEP', 'num_epochs': 2, 'min_prop': 0.5},
           'data_cfg': {'batch_sizes': {'train': 3}, 'random_train_transform': False}, 'num_epochs': {'eval': 2},
           'loss_func': 'cross_entropy', 'seed': 1}
    try:
        scalar, hist_s = evaluate.finetune_object(model, mo, msd, seq, gt[0], cfg)
        before, hist_b = finetune_object_before_the_band(model, mo, msd, seq, gt[0], cfg)
        assert torch.equal(scalar, before) and hist_s == hist_b
        cfg['eval_online_adapt']['min_prop'] = [0.3, 0.7]
        band, hist = evaluate.finetune_object(model, mo, msd, seq, gt[0], cfg)
        assert [len(h) for h in hist] == [len(h) for h in hist_s] and bool(torch.isfinite(band).all())
        assert np.isfinite(np.concatenate(hist)).all()
        assert torch.equal(band[:3], scalar[:3])                    # round 0 knows no band
        assert not torch.equal(band[3:], scalar[3:])
    finally:
        if model.engine is not None:
            model.engine.close()
