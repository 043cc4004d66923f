"""Frozen-encoder fine-tuning on the engine (`eosvos_set_trainable_from`, `parent_model.train_encoder: False`) against the
reference trajectories of fixture G24 (tests/golden/make_g24.py), in every matrix mode.  Needs an MI355X: pytest -m gpu.

Tolerances are the ones tests/test_gpu_parity.py holds G45 (fine-tune) and G7 (meta task) to; the 480 x 854 batch-3
trajectory is held to 1e-3 (losses relative, logits absolute)."""
import math
import os

import numpy as np
import pytest
import torch

from eosvos_amd import synthetic, topology

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SMALL = (96, 160)
FULL = (480, 854)
MODES = ['f16x3', 'bf16x6', 'f32']
BN_CFG = {'accum_stats': False, 'learn_weight': False, 'learn_bias': False}
MO_CFG = dict(init_lr=1e-3, learn_model_init=True, second_order_gradients=False, lr_hierarchy_level='NEURON',
              use_log_init_lr=False, max_lr=None)


@pytest.fixture(scope='module')
def g24(golden_dir):
    return np.load(os.path.join(golden_dir, 'g24_frozen_encoder.npz'))


@pytest.fixture(params=MODES)
def mode(request):
    from eosvos_amd.engine import get_matrix_mode, set_matrix_mode
    prev = get_matrix_mode()
    set_matrix_mode(request.param)
    yield request.param
    set_matrix_mode(prev)


def _engine(encoder, hw, batch, frozen=True, norm='bn'):
    from eosvos_amd.engine import Engine
    eng = Engine(encoder, *hw, max_batch=batch, device=DEV, norm=norm)
    if frozen:
        eng.set_trainable_from(topology.trainable_from(encoder, False))
    sd = synthetic.synthetic_state(encoder)
    eng.load_model_state(sd, synthetic.synthetic_lrs(encoder))
    return eng, sd


def _offsets(encoder):
    return np.cumsum([0] + [int(np.prod(s)) for _, s in topology.trainable(encoder)])


def _l2(flat, offs, i):
    return float(flat[offs[i]:offs[i + 1]].double().norm())


def _frozen_prefix_is_init(eng, encoder, sd):
    nf = topology.frozen_tensors(encoder, False)
    offs = _offsets(encoder)
    init = torch.cat([sd[n].reshape(-1).float() for n, _ in topology.trainable(encoder)[:nf]])
    return torch.equal(eng.get_params()[:offs[nf]].cpu(), init)


def test_finetune_vs_g24(g24, mode):
    """V3+ R50, T = 10 at 96 x 160, batch 3 (G45's small case); the frozen weights stay the init bit for bit."""
    eng, sd = _engine('resnet50', SMALL, 3)
    try:
        nf = topology.frozen_tensors('resnet50', False)
        offs = _offsets('resnet50')
        tr = topology.trainable('resnet50')
        batches = [synthetic.synthetic_frames(3, *SMALL, seed=2400 + it) for it in range(10)]
        eng.reset()
        eng.keep_grads(True)
        losses = []
        for it, (x, y) in enumerate(batches):
            losses.append(eng.finetune_step(x.to(DEV), y.to(DEV)))
            if it == 0:
                grads = eng.get_grads().cpu()
        eng.keep_grads(False)
        np.testing.assert_allclose(losses, g24['ft_losses'], rtol=1e-5)
        assert not bool(grads[:offs[nf]].any())                       # the frozen tensors have no gradient
        for k, i in enumerate(range(nf, len(tr))):
            r = g24['ft_grad_fp'][k][1]
            assert abs(_l2(grads, offs, i) - r) <= 6e-4 * r + 1e-9, (tr[i][0], _l2(grads, offs, i), r)
        params = eng.get_params().cpu()
        for k, i in enumerate(range(nf, len(tr))):
            r = g24['ft_param_fp'][k][1]
            assert abs(_l2(params, offs, i) - r) <= 3e-6 * r, tr[i][0]
        assert _frozen_prefix_is_init(eng, 'resnet50', sd)
        out = eng.forward(batches[0][0].to(DEV)).cpu().numpy()
        assert np.abs(out - g24['ft_final_logits']).max() < 1e-4
    finally:
        eng.close()


def test_meta_task_vs_g24(g24, mode):
    """One K = 2 meta task (G7): the meta-gradient of the trainable subset, nothing in the frozen part."""
    eng, _ = _engine('resnet50', SMALL, 1)
    try:
        nf = topology.frozen_tensors('resnet50', False)
        tr = topology.trainable('resnet50')
        x, y = synthetic.synthetic_frames(1, *SMALL, seed=2450)
        xm, ym = torch.flip(x, dims=[3]).contiguous(), torch.flip(y, dims=[3]).contiguous()
        eng.meta_task_begin()
        tl = [eng.finetune_step(x.to(DEV), y.to(DEV), accumulate=True) for _ in range(2)]
        flat = torch.zeros(eng.n_lr + eng.n_param, device=DEV)
        ml = eng.meta_grad(xm.to(DEV), ym.to(DEV), flat)
        np.testing.assert_allclose(tl, g24['k2_train_losses'], rtol=1e-5)
        assert abs(ml - g24['k2_meta_loss'][0]) <= 3e-5 * abs(g24['k2_meta_loss'][0])
        flat = flat.cpu()
        r0 = sum(s[0] for _, s in tr[:nf])
        offs = _offsets('resnet50') + eng.n_lr
        assert not bool(flat[:r0].any()) and not bool(flat[eng.n_lr:offs[nf]].any())
        ref = g24['k2_lr_grad']
        got = flat[r0:eng.n_lr].numpy()
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 2.5e-3 * np.abs(ref).max(), np.abs(got - ref).max() / np.abs(ref).max()
        for k, i in enumerate(range(nf, len(tr))):
            r = g24['k2_init_grad_fp'][k][1]
            l2 = float(flat[offs[i]:offs[i + 1]].double().norm())
            assert abs(l2 - r) <= 4e-4 * r + 1e-9, (tr[i][0], l2, r)
    finally:
        eng.close()


def test_full_size_batch3_trajectory_vs_g24(g24, mode):
    eng, sd = _engine('resnet50', FULL, 3)
    try:
        nf = topology.frozen_tensors('resnet50', False)
        offs = _offsets('resnet50')
        eng.reset()
        losses = []
        for it in range(10):
            x, y = synthetic.synthetic_frames(3, *FULL, seed=2460 + it)
            losses.append(eng.finetune_step(x.to(DEV), y.to(DEV)))
            if it == 0:
                x0 = x[:1].contiguous()
        np.testing.assert_allclose(losses, g24['full_losses'], rtol=1e-3)
        out = eng.forward(x0.to(DEV)).cpu()
        assert np.abs(out[0, 0, ::8, ::7].numpy() - g24['full_final_logits_sub']).max() < 1e-3
        params = eng.get_params().cpu()
        for k, i in enumerate(range(nf, len(offs) - 1)):
            r = g24['full_param_fp'][k][1]
            assert abs(_l2(params, offs, i) - r) <= 1e-3 * r
        assert _frozen_prefix_is_init(eng, 'resnet50', sd)
    finally:
        eng.close()


@pytest.mark.parametrize('encoder,norm', [('resnet50', 'bn'), ('resnet50', 'gn'), ('deeplabv3_resnet50', 'bn')])
def test_trainable_gradients_equal_the_full_engine(mode, encoder, norm):
    """First-step gradients of the trainable tensors: the same launches and plans as with the encoder trainable, so the same
    bits; the frozen ones are zero.  (GroupNorm mode and plain DeepLabV3 included.)"""
    nf = topology.frozen_tensors(encoder, False)
    offs = _offsets(encoder)
    x, y = synthetic.synthetic_frames(2, *SMALL, seed=2480)
    got = {}
    for frozen in (False, True):
        eng, sd = _engine(encoder, SMALL, 2, frozen=frozen, norm=norm)
        try:
            eng.keep_grads(True)
            eng.reset()
            got[frozen] = (eng.finetune_step(x.to(DEV), y.to(DEV)), eng.get_grads().cpu())
            for _ in range(2):
                eng.finetune_step(x.to(DEV), y.to(DEV))
            if frozen:
                assert _frozen_prefix_is_init(eng, encoder, sd)
        finally:
            eng.close()
    (la, ga), (lb, gb) = got[False], got[True]
    assert la == lb
    assert not bool(gb[:offs[nf]].any())
    diff = float((ga[offs[nf]:] - gb[offs[nf]:]).abs().max())
    assert diff == 0.0, diff


def test_deeplabv3_finetune_vs_g24(g24):
    eng, sd = _engine('deeplabv3_resnet50', SMALL, 2)
    try:
        enc = 'deeplabv3_resnet50'
        nf = topology.frozen_tensors(enc, False)
        offs = _offsets(enc)
        tr = topology.trainable(enc)
        batches = [synthetic.synthetic_frames(2, *SMALL, seed=2470 + it) for it in range(5)]
        eng.reset()
        eng.keep_grads(True)
        losses = []
        for it, (x, y) in enumerate(batches):
            losses.append(eng.finetune_step(x.to(DEV), y.to(DEV)))
            if it == 0:
                grads = eng.get_grads().cpu()
        eng.keep_grads(False)
        np.testing.assert_allclose(losses, g24['v3_losses'], rtol=1e-5)
        for k, i in enumerate(range(nf, len(tr))):
            r = g24['v3_grad_fp'][k][1]
            assert abs(_l2(grads, offs, i) - r) <= 6e-4 * r + 1e-9, (tr[i][0], _l2(grads, offs, i), r)
        params = eng.get_params().cpu()
        for k, i in enumerate(range(nf, len(tr))):
            r = g24['v3_param_fp'][k][1]
            assert abs(_l2(params, offs, i) - r) <= 3e-6 * r, tr[i][0]
        assert _frozen_prefix_is_init(eng, enc, sd)
        out = eng.forward(batches[0][0].to(DEV)).cpu().numpy()
        assert np.abs(out - g24['v3_final_logits']).max() < 1e-4
    finally:
        eng.close()


def test_boundary_rejects_other_convs_and_aliases_must_agree():
    from eosvos_amd import _ffi
    eng, _ = _engine('resnet50', SMALL, 1, frozen=False)
    other, _ = _engine('resnet50', SMALL, 1, frozen=True)
    try:
        with pytest.raises(_ffi.EosvosError):
            eng.set_trainable_from(5)
        with pytest.raises(_ffi.EosvosError):
            eng.alias_state(other)
        eng.set_trainable_from(other.train_from)
        eng.alias_state(other)
        with pytest.raises(_ffi.EosvosError):
            other.set_trainable_from(0)
        eng.unalias_state()
    finally:
        eng.close()
        other.close()


def _model_and_optim():
    from eosvos_amd.helper_func import init_parent_model
    from eosvos_amd.meta_optim import MetaOptimizer
    model, _ = init_parent_model(architecture='DeepLabV3Plus', encoder='resnet50', train_encoder=False, batch_norm=BN_CFG)
    sd = synthetic.synthetic_state('resnet50')
    model.load_state_dict(sd)
    mo = MetaOptimizer(model, **MO_CFG)
    lrs = dict(zip([n for n, _ in topology.trainable('resnet50')], synthetic.synthetic_lrs('resnet50')))
    msd = {}
    for k in mo.state_dict():
        lr = k.startswith('log_init_lr_')
        n = k[len('log_init_lr_' if lr else 'model_init_'):].replace('-', '.')
        msd[k] = (lrs[n] if lr else sd[n]).clone()
    return model, mo, msd, sd


def _sequence():
    H, W, N = SMALL[0], SMALL[1], 6
    frames, gt = synthetic.synthetic_frames(1, H, W, seed=3, second_object=True)
    seq = torch.cat([torch.roll(frames, shifts=4 * i, dims=3) for i in range(N)]).to(DEV)
    rows = torch.arange(H).view(-1, 1)
    return seq, [(gt[0] * (rows < H // 2)).float(), (gt[0] * (rows >= H // 2)).float()]


def test_evaluate_sequence_with_online_adaptation_and_objects_in_flight():
    from eosvos_amd import config
    from eosvos_amd.evaluate import evaluate_sequence, finetune_object, object_workers, run_objects_in_flight
    model, mo, msd, sd = _model_and_optim()
    cfg = config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS-OnA', 'num_epochs.eval=3', 'eval_online_adapt.num_epochs=2',
                            'eval_online_adapt.step=3', 'parent_model.train_encoder=False'])
    seq, objs = _sequence()
    labels, probs, hist = evaluate_sequence(model, mo, msd, seq, objs, cfg)
    assert labels.shape == (6, *SMALL) and [len(h) for h in hist[0]] == [3, 2]
    assert model.engine.train_from == 43
    assert all(bool(torch.isfinite(p).all()) for p in probs)
    nf = topology.frozen_tensors('resnet50', False)
    offs = _offsets('resnet50')
    init = torch.cat([sd[n].reshape(-1).float() for n, _ in topology.trainable('resnet50')[:nf]])
    assert torch.equal(model.engine.get_params()[:offs[nf]].cpu(), init)
    # objects side by side on spawned models (their engines take the boundary too) == one after the other at that budget
    workers = object_workers(model, mo, MO_CFG, 2)
    res = run_objects_in_flight(workers, msd, seq, objs, cfg)
    assert all(w.model.engine.train_from == 43 for w in workers)
    model._ensure_engine(*SMALL, 3)
    model.set_wg_budget(256)
    model.set_side_stream(False)
    torch.cuda.synchronize()
    one = [finetune_object(model, mo, msd, seq, g, cfg) for g in objs]
    for (p2, h2), (p1, h1) in zip(res, one):
        assert h2 == h1 and torch.equal(p2, p1)
    model.set_wg_budget(0)
    model.set_side_stream(True)
    for w in workers:
        w.model.close_engines()
    model.close_engines()


def test_meta_trainer_on_the_subset():
    """MetaTrainer with a frozen-encoder engine: subset vectors, the separate RAdam calls, frozen init untouched."""
    from eosvos_amd.meta_run import MetaTrainer
    eng, sd = _engine('resnet50', SMALL, 1)
    try:
        mt = MetaTrainer(eng, meta_batch_size=2, freeze_encoder=True)
        tr = topology.trainable('resnet50')[43:]
        assert mt.state.numel() == sum(s[0] for _, s in tr) + sum(math.prod(s) for _, s in tr)
        lrs = synthetic.synthetic_lrs('resnet50')[43:]
        mt.load_state(sd, lrs)
        before = mt.state.clone()
        tasks = []
        for t in range(2):
            x, y = synthetic.synthetic_frames(1, *SMALL, seed=2490 + t)
            tasks.append((x.to(DEV), y.to(DEV), torch.flip(x, dims=[3]).contiguous().to(DEV), torch.flip(y, dims=[3]).contiguous().to(DEV)))
        losses = mt.meta_iteration(tasks, inner_steps=2)
        assert all(math.isfinite(l) for l in losses)
        torch.cuda.synchronize()
        moved = (mt.state - before).abs()
        assert float(moved.max()) > 0
        nb = mt._backbone_lr                    # freeze_encoder: layer4's lrs and init take lr 0
        assert not bool(moved[:nb].any()) and not bool(moved[mt.n_lr:mt.n_lr + mt._backbone_param].any())
        assert _frozen_prefix_is_init(eng, 'resnet50', sd)
    finally:
        eng.close()
