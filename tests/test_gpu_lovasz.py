"""The Lovasz hinge kinds (`loss_func: lovasz_hinge` / `lovasz_hinge_flat`, networks/loss_lovasz.py:78-111) on the MI355X:
the HIP pipeline of csrc/lovasz_kernels.hip against the fp64 stable-sort restatement (tests/lovasz_ref.py), against the
reference's own values (tests/golden/lovasz.npz), and through the network against the CPU oracle.  pytest -m gpu.

Bounds.  Gradient, elementwise: 1e-6 of the fp64 value (the closed-form weight is at most 4 fp32 roundings = 2.4e-7 from
it; x4), exactly 0 where e <= 0, and the same set of non-zero entries.  Loss: 1e-5 relative (a fixed-order sum of <= 1.23 M
non-negative terms is within log2(n) * 2^-24 = 1.2e-6; x8).  Against the reference fixture the bound is the reference's own
stored distance to the restatement (it forms its weights by subtracting fp32 numbers near 1): loss within that distance
+ 1e-5 relative, gradient within twice that noise + 1e-6 of max |grad|.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lovasz_ref
from loss_common import dlogits_of, dlogits_raw, poke_logits  # noqa: F401  (the child process reads T.dlogits_raw)
from eosvos_amd import synthetic, topology

pytestmark = pytest.mark.gpu

SMALL, FULL = (96, 160), (480, 854)
DEV = 'cuda:0'
GRAD_RTOL, LOSS_RTOL = 1e-6, 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def weights():
    return synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50')


@pytest.fixture(scope='module')
def small_engine(weights):
    from eosvos_amd.engine import Engine
    eng = Engine('resnet50', *SMALL, max_batch=3, device=DEV)
    eng.load_model_state(*weights)
    yield eng
    eng.close()


@pytest.fixture(scope='module')
def full_engine(weights):
    """480 x 854, batch 3, after one batch-3 forward: `debug_tensor('dlogits')` then shows all 3 x 480 x 854 elements."""
    from eosvos_amd.engine import Engine
    eng = Engine('resnet50', *FULL, max_batch=3, device=DEV)
    eng.load_model_state(*weights)
    x, _ = synthetic.synthetic_frames(3, *FULL, seed=3)
    eng.forward(x.to(DEV), want_logits=False)
    yield eng
    eng.close()


def make_case(n, target, scale, seed, quantise=False):
    rng = np.random.RandomState(seed)
    x = (scale * rng.randn(n)).astype(np.float32)
    if quantise:
        x = (np.round(x * 8) / 8).astype(np.float32)          # thousands of equal errors across both labels
    if target == 'zeros':
        t = np.zeros(n, dtype=np.float32)
    elif target == 'ones':
        t = np.ones(n, dtype=np.float32)
    else:
        t = (rng.rand(n) < 0.3).astype(np.float32)
    return x, t


def check(tag, loss, grad, ref_loss, ref_grad, margins=None):
    """The issue's op-level bounds; prints the measured margins before asserting."""
    grad, ref_grad = np.asarray(grad, dtype=np.float64).reshape(-1), np.asarray(ref_grad, dtype=np.float64).reshape(-1)
    nz = ref_grad != 0
    rel = float((np.abs(grad[nz] - ref_grad[nz]) / np.abs(ref_grad[nz])).max()) if nz.any() else 0.0
    lrel = abs(loss - ref_loss) / max(abs(ref_loss), 1e-30) if ref_loss != 0 else abs(loss)
    print(f'MARGIN {tag}: loss {loss:.9g} vs {ref_loss:.12g} rel {lrel:.2e}; grad worst elementwise rel {rel:.2e}; '
          f'non-zero {int(nz.sum())} of {nz.size}')
    if margins is not None:
        margins.append((tag, lrel, rel))
    assert np.array_equal(grad != 0, nz), f'{tag}: the sets of non-zero gradient entries differ'
    assert rel <= GRAD_RTOL, (tag, rel)
    assert lrel <= LOSS_RTOL, (tag, loss, ref_loss)


@pytest.mark.parametrize('scale', [3.0, 80.0])
@pytest.mark.parametrize('target', ['zeros', 'ones', 'mixed'])
@pytest.mark.parametrize('n', [1, 255, 257, 480 * 854])
def test_one_set_vs_fp64_restatement(full_engine, n, target, scale):
    """eosvos_loss_tensors (`loss_of`): the n elements are one set for either kind."""
    eng = full_engine
    x, t = make_case(n, target, scale, seed=n % 1000 + int(scale))
    ref_loss, ref_grad = lovasz_ref.lovasz_flat_f64(x, t)
    for kind in ('lovasz_hinge', 'lovasz_hinge_flat'):
        loss = float(eng.loss_of(kind, torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)))
        check(f'{kind} n={n} {target} scale={scale:g}', loss, dlogits_of(eng, n), ref_loss, ref_grad)


@pytest.mark.parametrize('n', [257, 480 * 854])
def test_heavy_ties_rank_by_pixel_index(full_engine, n):
    """Logits quantised to 1/8: thousands of equal errors on both labels; their order is the pixel index."""
    x, t = make_case(n, 'mixed', 3.0, seed=11, quantise=True)
    e, g, _ = lovasz_ref.errors_f32(x, t)
    if n > 1000:
        both = np.intersect1d(e[g & (e > 0)], e[~g & (e > 0)])
        assert both.size >= 20 and np.isin(e, both).sum() > 1000       # the case is what it says
    ref_loss, ref_grad = lovasz_ref.lovasz_flat_f64(x, t)
    loss = float(full_engine.loss_of('lovasz_hinge', torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)))
    check(f'ties n={n}', loss, dlogits_of(full_engine, n), ref_loss, ref_grad)


@pytest.mark.parametrize('scale', [3.0, 80.0])
@pytest.mark.parametrize('kind', ['lovasz_hinge', 'lovasz_hinge_flat'])
def test_batch3_full_size_through_eosvos_loss(full_engine, kind, scale):
    """eosvos_loss on the engine's own logits buffer: batch 3 at 480 x 854, per image (mean, gradients / 3) and flat."""
    eng = full_engine
    n = 3 * FULL[0] * FULL[1]
    x, t = make_case(n, 'mixed', scale, seed=5)
    t = t.reshape(3, -1)
    t[1] = 0.0                                                         # one all-background image in the batch
    t = t.reshape(-1)
    poke_logits(eng, torch.from_numpy(x).to(DEV))
    loss = float(eng.loss(kind, torch.from_numpy(t).to(DEV).view(3, 1, *FULL)))
    ref_loss, ref_grad = lovasz_ref.lovasz_hinge_f64(x.reshape(3, -1), t.reshape(3, -1), per_image=(kind == 'lovasz_hinge'))
    check(f'{kind} batch 3 full size scale={scale:g}', loss, dlogits_of(eng, n), ref_loss, ref_grad)


@pytest.mark.parametrize('tag,kind', [('per_image', 'lovasz_hinge'), ('flat', 'lovasz_hinge_flat'), ('zero', 'lovasz_hinge')])
def test_vs_reference_fixture(golden_dir, tag, kind):
    """The unmodified reference's loss and autograd gradient, B = 3 at 48 x 80, through eosvos_loss on a 48 x 80 engine whose
    logits buffer holds the fixture's logits."""
    from eosvos_amd.engine import Engine
    g = np.load(os.path.join(golden_dir, 'lovasz.npz'))
    x, t = g['logits'], g['labels'].astype(np.float32)
    if tag == 'zero':
        x, t = x[:1], np.zeros_like(t[:1])
    eng = Engine('resnet50', 48, 80, max_batch=3, device=DEV)
    try:
        eng.load_model_state(synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50'))
        b = x.shape[0]
        frames, _ = synthetic.synthetic_frames(b, 48, 80, seed=1)
        eng.forward(frames.to(DEV), want_logits=False)
        poke_logits(eng, torch.from_numpy(np.ascontiguousarray(x)).to(DEV))
        loss = float(eng.loss(kind, torch.from_numpy(np.ascontiguousarray(t)).to(DEV).view(b, 1, 48, 80)))
        grad = dlogits_of(eng, x.size).reshape(x.shape)
    finally:
        eng.close()
    ref_loss, ref_grad = float(g[f'{tag}_loss']), g[f'{tag}_dlogits']
    noise_l, noise_g = float(g[f'{tag}_ref_vs_f64_loss']), float(g[f'{tag}_ref_vs_f64_grad'])
    dl, dg = abs(loss - ref_loss), float(np.abs(grad - ref_grad).max())
    gmax = float(np.abs(ref_grad).max())
    print(f'MARGIN fixture {tag}: loss diff {dl:.2e} (allowed {noise_l + LOSS_RTOL * abs(ref_loss):.2e}); '
          f'grad diff {dg:.2e} (allowed {(2 * noise_g + 1e-6) * gmax:.2e})')
    assert dl <= noise_l + LOSS_RTOL * abs(ref_loss)
    assert dg <= (2 * noise_g + 1e-6) * gmax


def test_two_evaluations_are_bit_identical(full_engine):
    n = 3 * FULL[0] * FULL[1]
    x, t = make_case(n, 'mixed', 3.0, seed=21, quantise=True)
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    got = []
    for _ in range(2):
        loss = full_engine.loss_of('lovasz_hinge_flat', xd, td).cpu().numpy().view(np.uint32)
        got.append((loss.copy(), dlogits_of(full_engine, n).view(np.uint32).copy()))
        full_engine.loss_of('dice', xd, td)                            # something else through the gradient buffer in between
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


CHILD = r'''
import hashlib, json, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from eosvos_amd.engine import Engine
import test_gpu_lovasz as T
eng = Engine('resnet50', 96, 160, max_batch=3, device='cuda:0')
out = {}
for kind, n in (('lovasz_hinge_flat', 3 * 96 * 160), ('lovasz_hinge', 96 * 160 - 3)):
    x, t = T.make_case(n, 'mixed', 3.0, seed=33, quantise=True)
    loss = eng.loss_of(kind, torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda())
    eng.synchronize()
    ptr_grad = T.dlogits_raw(eng, n)
    out[kind] = [int(loss.cpu().numpy().view(np.uint32)[0]), hashlib.sha256(ptr_grad.tobytes()).hexdigest()]
print(json.dumps(out))
'''


def test_nan_filled_buffers_give_the_same_bits():
    """The same evaluation in a process whose engine buffers (the sort scratch included) start out as NaN words, and in one
    that gets the allocator's pages as they come: a kernel that reads a slot nothing wrote would differ."""
    res = []
    for fill in (None, '7fc00000'):
        env = dict(os.environ, EOSVOS_MODE_GUARD='0')
        env.pop('EOSVOS_DEBUG_FILL', None)
        if fill:
            env['EOSVOS_DEBUG_FILL'] = fill
        p = subprocess.run([sys.executable, '-c', CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
        assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        res.append(json.loads(lines[-1]))
    assert res[0] == res[1], res
    for kind, n in (('lovasz_hinge_flat', 3 * 96 * 160), ('lovasz_hinge', 96 * 160 - 3)):          # ... and they are the right bits
        x, t = make_case(n, 'mixed', 3.0, seed=33, quantise=True)
        ref_loss, _ = lovasz_ref.lovasz_flat_f64(x, t)
        loss = float(np.array([res[0][kind][0]], dtype=np.uint32).view(np.float32)[0])
        assert abs(loss - ref_loss) <= LOSS_RTOL * ref_loss


@pytest.mark.parametrize('bad', [float('nan'), float('-inf')])
def test_non_finite_logit_gives_non_finite_loss_and_leaves_no_trace(small_engine, bad):
    n = 96 * 160
    x, t = make_case(n, 'mixed', 3.0, seed=8)
    clean_x = torch.from_numpy(x).to(DEV)
    td = torch.from_numpy(t).to(DEV)
    before = float(small_engine.loss_of('lovasz_hinge', clean_x, td))
    grad_before = dlogits_raw(small_engine, n)
    xb = x.copy()
    xb[int(np.flatnonzero(t > 0.5)[5])] = bad                          # on a foreground pixel
    loss = float(small_engine.loss_of('lovasz_hinge', torch.from_numpy(xb).to(DEV), td))
    assert not np.isfinite(loss)
    after = float(small_engine.loss_of('lovasz_hinge', clean_x, td))
    assert np.float32(after).view(np.uint32) == np.float32(before).view(np.uint32)
    assert np.array_equal(dlogits_raw(small_engine, n).view(np.uint32), grad_before.view(np.uint32))


@pytest.fixture
def oracle_knows_lovasz(monkeypatch):
    """Teach the CPU oracle's `loss_fn` the two names at test time (the oracle files stay as they are)."""
    from oracle import deeplab
    orig = deeplab.loss_fn

    def loss_fn(name, logits, gt):
        if name in ('lovasz_hinge', 'lovasz_hinge_flat'):
            return lovasz_ref.lovasz_hinge_torch(logits, gt, per_image=(name == 'lovasz_hinge'))
        return orig(name, logits, gt)
    monkeypatch.setattr(deeplab, 'loss_fn', loss_fn)
    return deeplab


@pytest.mark.parametrize('name', ['lovasz_hinge', 'lovasz_hinge_flat'])
def test_loss_gradient_and_finetune_vs_oracle(small_engine, weights, oracle_knows_lovasz, name):
    """Value and dL/dlogits on the engine's own logits at the tolerances test_dice_losses_vs_oracle uses for dice (1e-5 of the
    loss, 1e-4 of max |dL/dlogits|); first-step parameter gradients and the parameters after 3 fine-tune steps against
    oracle.meta at the bounds test_gradients_and_finetune_small_vs_golden holds the BCE path to (2e-3 of a tensor's largest
    gradient entry, 3e-6 of its largest parameter)."""
    from oracle import meta
    deeplab = oracle_knows_lovasz
    eng = small_engine
    eng.load_model_state(*weights)
    x, y = synthetic.synthetic_frames(2, *SMALL, seed=9)
    logits = eng.forward(x.to(DEV))
    loss = eng.loss(name, y.to(DEV))
    lg = logits.cpu().clone().requires_grad_(True)
    ref = deeplab.loss_fn(name, lg, y)
    (dref,) = torch.autograd.grad(ref, lg)
    ref = ref.detach()
    d = eng.debug_tensor('dlogits').cpu()
    print(f'MARGIN {name} on engine logits: loss diff {abs(float(loss) - float(ref)):.2e}, dlogits diff '
          f'{float((d - dref).abs().max()):.2e} of max {float(dref.abs().max()):.2e}')
    assert abs(float(loss) - float(ref)) < 1e-5 * max(1.0, abs(float(ref)))
    assert float((d - dref).abs().max()) <= 1e-4 * float(dref.abs().max()) + 1e-10

    tr = topology.trainable('resnet50')
    offs = np.cumsum([0] + [int(np.prod(s)) for _, s in tr])
    eng.load_model_state(*weights)
    eng.set_loss(name)
    try:
        eng.keep_grads(True)
        losses = []
        for it in range(3):
            losses.append(eng.finetune_step(x.to(DEV), y.to(DEV)))
            if it == 0:
                grads = eng.get_grads().cpu()
        eng.keep_grads(False)
        params = eng.get_params().cpu()
    finally:
        eng.set_loss('cross_entropy')
        eng.load_model_state(*weights)
    P = dict(weights[0])
    ref_losses = []
    for it in range(3):
        rl, rg, P = meta.finetune_step(P, weights[1], x, y, loss_name=name)
        ref_losses.append(float(rl))
        if it == 0:
            ref_grads = rg
    worst_g = worst_p = 0.0
    for i, (n, s) in enumerate(tr):
        got, r = grads[offs[i]:offs[i + 1]].view(*s), ref_grads[i]
        worst_g = max(worst_g, float((got - r).abs().max() / (r.abs().max() + 1e-20)))
        assert float((got - r).abs().max()) <= 2e-3 * float(r.abs().max()) + 1e-7, n
        gp, rp = params[offs[i]:offs[i + 1]].view(*s), P[n]
        worst_p = max(worst_p, float((gp - rp).abs().max() / (rp.abs().max() + 1e-20)))
        assert float((gp - rp).abs().max()) <= 3e-6 * float(rp.abs().max()), n
    print(f'MARGIN {name} through the network: losses {losses} vs {ref_losses}; worst gradient {worst_g:.2e} of the tensor max, '
          f'worst parameter after 3 steps {worst_p:.2e}')
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-5)


def test_meta_task_with_lovasz_vs_oracle(small_engine, weights, oracle_knows_lovasz):
    """K = 2 meta task through eosvos_set_loss + finetune_step + meta_grad, at test_meta_task_with_dice_loss_vs_oracle's bounds."""
    from oracle import meta
    eng = small_engine
    eng.load_model_state(*weights)
    eng.set_loss('lovasz_hinge')
    try:
        x, y = synthetic.synthetic_frames(1, *SMALL, seed=77)
        xm, ym = torch.flip(x, dims=[3]).contiguous(), torch.flip(y, dims=[3]).contiguous()
        ref = meta.meta_task(weights[0], weights[1], [(x, y)] * 2, (xm, ym), loss_name='lovasz_hinge')
        eng.meta_task_begin()
        tl = [eng.finetune_step(x.to(DEV), y.to(DEV), accumulate=True) for _ in range(2)]
        flat = torch.zeros(eng.n_lr + eng.n_param, device=DEV)
        ml = eng.meta_grad(xm.to(DEV), ym.to(DEV), flat)
        r = torch.cat([t.flatten() for t in ref['g_lr']]).numpy()
        got = flat[:eng.n_lr].cpu().numpy()
        print(f'MARGIN lovasz meta task: train losses {tl} vs {ref["train_losses"]}; meta loss {ml} vs {ref["meta_loss"]}; '
              f'lr gradient diff {np.abs(got - r).max() / np.abs(r).max():.2e} of max')
        np.testing.assert_allclose(tl, ref['train_losses'], rtol=1e-5)
        assert abs(ml - ref['meta_loss']) <= 5e-4 * abs(ref['meta_loss'])
        assert np.abs(got - r).max() <= 2.5e-3 * np.abs(r).max()
    finally:
        eng.set_loss('cross_entropy')
        eng.load_model_state(*weights)


def test_fused_step_equals_the_separate_calls(small_engine, weights):
    """finetune_step with the kind selected == forward -> compute_loss -> backward_step, bit for bit."""
    eng = small_engine
    x, y = synthetic.synthetic_frames(3, *SMALL, seed=4)
    xd, yd = x.to(DEV), y.to(DEV)
    eng.load_model_state(*weights)
    eng.set_loss('lovasz_hinge')
    try:
        fused = [eng.finetune_step(xd, yd) for _ in range(2)]
        p_fused = eng.get_params().clone()
    finally:
        eng.set_loss('cross_entropy')
    eng.load_model_state(*weights)
    sep = []
    for _ in range(2):
        eng.forward(xd, want_logits=False)
        sep.append(float(eng.loss('lovasz_hinge', yd)))
        eng.backward_step()
    p_sep = eng.get_params()
    eng.load_model_state(*weights)
    assert np.array_equal(np.float32(fused).view(np.uint32), np.float32(sep).view(np.uint32)), (fused, sep)
    assert torch.equal(p_fused, p_sep)


def test_compute_loss_names_and_kwargs(small_engine, weights):
    """The drop-in surface: both names, `per_image: False` as the flat kind, `batch_average: False` per sample."""
    from eosvos_amd.helper_func import compute_loss
    eng = small_engine
    eng.load_model_state(*weights)
    x, y = synthetic.synthetic_frames(2, *SMALL, seed=2)
    logits = eng.forward(x.to(DEV))
    logits._eosvos_engine = eng                     # what networks.DeepLabV3Plus attaches to its outputs
    yd = y.to(DEV)
    lg, yn = logits.cpu().numpy()[:, 0], y.numpy()[:, 0]
    a = float(compute_loss('lovasz_hinge', logits, yd))
    b = float(compute_loss('lovasz_hinge', logits, yd, {'per_image': False}))
    c = float(compute_loss('lovasz_hinge_flat', logits, yd))
    per = compute_loss('lovasz_hinge', logits, yd, {'batch_average': False}).cpu().numpy()
    ra, _ = lovasz_ref.lovasz_hinge_f64(lg, yn, True)
    rb, _ = lovasz_ref.lovasz_hinge_f64(lg, yn, False)
    rp = [lovasz_ref.lovasz_flat_f64(lg[i], yn[i])[0] for i in range(2)]
    assert abs(a - ra) <= LOSS_RTOL * ra and abs(b - rb) <= LOSS_RTOL * rb and b == c
    np.testing.assert_allclose(per, rp, rtol=LOSS_RTOL)
    with pytest.raises(NotImplementedError):
        compute_loss('lovasz', logits, yd)
