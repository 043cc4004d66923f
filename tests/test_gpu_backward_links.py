"""Per-link fp64 audit of the backward pass and the fused update INSIDE the network (frozen BatchNorm, resnet50).

The op-level suites check each kernel on a scratch engine that holds one convolution.  A real `finetune_step` runs the same
kernels through the stage-grouped weight-gradient launches and their tables, the side-stream queue, the pre-split pair path
(from the second iteration of a trajectory on, alternating buffers), the two update tables built once per (batch, part), the
cached plans, the merged ASPP data gradient and the accumulate / add / partial-mask forms of the data gradient.  Here every
LINK of that pass (tests/backward_links_ref.py, proved against autograd in tests/test_backward_links_host.py) is recomputed
in float64 on the CPU from the engine's own operands -- the buffers `eosvos_debug_tensor` names, which stay in place after the
step -- and compared elementwise with what the engine left:

    err = max|gpu - ref64| / max|ref64|  <=  max(K * err_torch32, floor)

err_torch32: the same link function in float32 on the CPU from the same operands; K and the floors are the op suites' own
(test_gpu_misc_ops.K / FLOOR, test_gpu_conv_algos.TOL).  Every link is local, so no ReLU gate flips and the kernel-level
bounds apply unchanged.  ReLU masks are exact.  The update is checked per element, all 40 289 729 scalars.

One MARGIN line per link group (profiles/backward_links_margins.txt holds a run's lines).

Not covered: GroupNorm mode (it overwrites the stored raw outputs with dz and exposes neither), resnet101, plain DeepLabV3.
The accumulating (`gsum`) meta path and the trainable boundary: tests/test_gpu_meta_links.py.
"""
import numpy as np
import pytest
import torch

import backward_links_ref as R
from eosvos_amd import _ffi, synthetic
from eosvos_amd.engine import Engine
from test_gpu_conv_algos import TOL
from test_gpu_misc_ops import FLOOR, K

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H, W = 65, 97               # stride-2 / 4 / 8 / 16 maps of 33 x 49, 17 x 25, 9 x 13, 5 x 7: every tile is ragged
WINO_F4_MINDIM = 64         # EOSVOS_WINO_F4_MINDIM (engine.cpp): undilated maps from here on take F(4,3)
# Max-pool backward: an input pixel lies in at most 4 windows (3 x 3, stride 2), so its gradient is a sum of at most 4 routed
# terms -- 3 fp32 additions, each within 2^-24 of a partial sum <= sum|terms| <= 4 max|g|: 3 * 4 * 2^-24 < 2^-20 of the scale.
MAXPOOL_FLOOR = 2.0 ** -20
NET = R.Net('resnet50')
WLINKS = R.weight_links(NET)
DLINKS = R.data_links(NET)


def _conv_floor(ci, out_hw):
    """The op suites' floor of conv ci on an output map of out_hw."""
    c = NET.convs[ci]
    if ci == NET.pool:
        return FLOOR['pool_dw']
    if ci == NET.last:
        return FLOOR['head_dw']
    wino_shape = c.k == 3 and c.stride == 1 and c.pad == c.dil and 1 <= c.dil <= 8 and c.cin % 4 == 0 and c.cout % 4 == 0
    if not wino_shape:
        return TOL['direct']
    f4 = c.dil == 1 and out_hw[0] >= WINO_F4_MINDIM and out_hw[1] >= WINO_F4_MINDIM
    return TOL['wino_f4'] if f4 else TOL['wino_f2']


def _out_hw(run, ci):
    return tuple(run['T'][WLINKS[ci].g].shape[-2:])


def _errs(gpu, ref64, ref32):
    scale = float(ref64.abs().max())
    assert scale > 0 and gpu.shape == ref64.shape, (scale, gpu.shape, ref64.shape)
    return float((gpu.double() - ref64).abs().max()) / scale, float((ref32.double() - ref64).abs().max()) / scale


def _where(gpu, ref64, n=6):
    """The worst elements of a failed link: index (NCHW / OIHW), engine value, reference."""
    d = (gpu.double() - ref64).abs().flatten()
    top = torch.topk(d, min(n, d.numel())).indices
    idx = np.stack(np.unravel_index(top.numpy(), tuple(gpu.shape)), axis=1)
    return '; '.join(f'{tuple(int(v) for v in i)}: {float(gpu.flatten()[t]):.6e} vs {float(ref64.flatten()[t]):.6e}' for i, t in zip(idx, top))


def _capture(eng, x, y):
    """One fine-tune step on (x, y), then everything the links read, on the CPU."""
    before = eng.get_params().cpu()
    eng.profile_launches(True)
    loss = eng.finetune_step(x.to(DEV), y.to(DEV))
    eng.synchronize()
    kernels = sorted(eng.profile_read())
    eng.profile_launches(False)
    T = {n: eng.debug_tensor(n).cpu() for n in R.buffer_names(NET)}
    T['x'] = x
    run = dict(T=T, before=before, grads=eng.get_grads().cpu(), after=eng.get_params().cpu(), loss=loss, kernels=kernels,
               norm_a=eng.debug_tensor('norm_a').reshape(-1).cpu())
    assert np.isfinite(loss) and bool(torch.isfinite(run['grads']).all())
    return run


def _audit_weights(run, label, cis, floor_of=None):
    """Weight links of the convs `cis` of a captured step: prints the group's MARGIN line, then asserts every link."""
    T64, T32 = R.Cast(run['T'], torch.float64), R.Cast(run['T'], torch.float32)
    A64, A32 = NET.scales(run['norm_a'].double()), NET.scales(run['norm_a'])
    G = NET.weights(run['grads'])
    rows, bad = [], []
    for ci in cis:
        l, c = WLINKS[ci], NET.convs[ci]
        dw64, db64 = R.weight_link(NET, l, T64, A64)
        dw32, db32 = R.weight_link(NET, l, T32, A32)
        floor = floor_of(ci) if floor_of else _conv_floor(ci, _out_hw(run, ci))
        parts = [(c.name + '.weight', G[ci][0], dw64, dw32)] + ([(c.name + '.bias', G[ci][1], db64, db32)] if c.bias else [])
        for name, got, r64, r32 in parts:
            eg, e32 = _errs(got, r64, r32)
            bound = max(K * e32, floor)
            rows.append((eg / bound, name, eg, e32, bound))
            if not eg <= bound:
                bad.append(f'{name}: {eg:.3e} > {bound:.3e} (torch32 {e32:.2e}) at {_where(got, r64)}')
    worst = max(rows)
    print(f'MARGIN {label} weight links ({len(rows)}): worst {worst[1]} {worst[2]:.2e} (torch32 {worst[3]:.2e}, bound {worst[4]:.2e})')
    assert not bad, (label, bad)


def _audit_data(run, label, stage):
    T64, T32 = R.Cast(run['T'], torch.float64), R.Cast(run['T'], torch.float32)
    A64, A32 = NET.scales(run['norm_a'].double()), NET.scales(run['norm_a'])
    W32 = NET.weights(run['before'])
    W64 = NET.weights(run['before'].double())
    rows, bad = [], []
    for l in DLINKS:
        if l.stage != stage:
            continue
        got = run['T'][l.out]
        r64, r32 = l.fn(T64, W64, A64), l.fn(T32, W32, A32)
        eg, e32 = _errs(got, r64, r32)
        if l.misc:
            floor = MAXPOOL_FLOOR if l.misc == 'maxpool_bwd' else FLOOR[l.misc]
        else:
            floor = max(_conv_floor(ci, _out_hw(run, ci)) for ci in l.convs)
        bound = max(K * e32, floor)
        rows.append((eg / bound, l.out, eg, e32, bound))
        if not eg <= bound:
            bad.append(f'{l.out}: {eg:.3e} > {bound:.3e} (torch32 {e32:.2e}) at {_where(got, r64)}')
        if l.mask:                      # exact: no gradient where the masking activation is <= 0
            act, c0 = l.mask
            leak = (got[:, c0:] != 0) & (run['T'][act][:, c0:] <= 0)
            if bool(leak.any()):
                bad.append(f'{l.out}: {int(leak.sum())} nonzero gradients where {act} <= 0, first at {tuple(int(v[0]) for v in torch.nonzero(leak)[:1].T)}')
    worst = max(rows)
    print(f'MARGIN {label} data links ({len(rows)}): worst {worst[1]} {worst[2]:.2e} (torch32 {worst[3]:.2e}, bound {worst[4]:.2e})')
    assert not bad, (label, bad)


def _convs_of(*stages):
    return [l.ci for l in WLINKS if l.stage in stages]


def _new_engine(height=H, width=W, max_batch=3):
    eng = Engine('resnet50', height, width, max_batch=max_batch, device=DEV)
    eng.load_model_state(synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50'))
    eng._verify_pending = False
    eng.keep_grads(True)
    return eng


@pytest.fixture(scope='module')
def eng():
    e = _new_engine()
    yield e
    e.close()


# ---- main audit: every link, first iteration, three modes, batch 1 and 3 ---------------------------------------------------------
@pytest.fixture(scope='module')
def main_runs(eng):
    cache = {}

    def get(mode, batch):
        if (mode, batch) not in cache:
            cache.clear()               # the runs are visited one after the other: keep one
            eng.set_engine_matrix_mode(mode)
            eng.set_lr(torch.zeros(eng.n_lr))
            eng.reset()
            x, y = synthetic.synthetic_frames(batch, H, W, seed=11 + batch)
            cache[(mode, batch)] = _capture(eng, x, y)
        return cache[(mode, batch)]
    return get


@pytest.mark.parametrize('stage', R.STAGES)
@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('mode', ['f16x3', 'bf16x6', 'f32'])
def test_every_link_of_a_first_step(main_runs, mode, batch, stage):
    run = main_runs(mode, batch)
    assert torch.equal(run['before'], run['after']), 'a step with zero learning rates moved the weights'
    label = f'{mode} batch {batch} {stage}'
    _audit_weights(run, label, _convs_of(stage))
    _audit_data(run, label, stage)


# ---- later iterations: the pre-split pair path, both buffer parities ----------------------------------------------------------------
@pytest.fixture(scope='module')
def later_runs(eng):
    lib = _ffi.load()
    prev = lib.eosvos_set_presplit(2)
    try:
        eng.set_engine_matrix_mode('f16x3')
        eng.set_lr(torch.zeros(eng.n_lr))
        eng.reset()
        runs = [_capture(eng, *synthetic.synthetic_frames(3, H, W, seed=21 + it)) for it in range(3)]
    finally:
        lib.eosvos_set_presplit(prev)
    for r in runs[:1]:
        r['T'] = None                   # only its kernel list is needed
    return runs


@pytest.mark.parametrize('step', [2, 3])
def test_weight_links_of_later_iterations_on_the_presplit_path(later_runs, step):
    used = [[k for k in r['kernels'] if k.startswith('wgrad_p')] for r in later_runs]
    assert not used[0] and used[1] and used[2], ('the pre-split path: not in step 1, in steps 2 and 3', used)
    run = later_runs[step - 1]
    assert torch.equal(run['before'], run['after'])
    _audit_weights(run, f'f16x3 batch 3 presplit step {step} layer1..3 ({used[step - 1]})', _convs_of('layer1', 'layer2', 'layer3'),
                   floor_of=lambda ci: TOL['direct'])


# ---- stale plans and tables: one engine through batch, budget, mode and stream switches ---------------------------------------------
STALE_STEPS = ['batch 3', 'batch 1', 'batch 3 again', 'budget 256, batch 3', 'bf16x6, batch 3', 'no side stream, batch 3',
               'no side stream, batch 1', 'side stream again, batch 1']


@pytest.fixture(scope='module')
def stale_runs():
    e = _new_engine()
    try:
        e.set_engine_matrix_mode('f16x3')
        e.set_lr(torch.zeros(e.n_lr))
        e.reset()
        f3, f1 = synthetic.synthetic_frames(3, H, W, seed=31), synthetic.synthetic_frames(1, H, W, seed=32)
        runs = [_capture(e, *f3), _capture(e, *f1), _capture(e, *f3)]
        assert e.set_wg_budget(256) == 256
        runs.append(_capture(e, *f3))
        e.set_engine_matrix_mode('bf16x6')
        runs.append(_capture(e, *f3))
        assert e.set_side_stream(False) is False
        runs.append(_capture(e, *f3))
        runs.append(_capture(e, *f1))
        assert e.set_side_stream(True) is True
        runs.append(_capture(e, *f1))
    finally:
        e.close()
    return runs


@pytest.mark.parametrize('step', range(len(STALE_STEPS)), ids=[s.replace(' ', '_').replace(',', '') for s in STALE_STEPS])
def test_weight_links_after_plan_and_table_switches(stale_runs, step):
    run = stale_runs[step]
    assert torch.equal(run['before'], run['after'])
    _audit_weights(run, f'switches: {STALE_STEPS[step]}', range(len(NET.convs)))


def _same(a, b):
    """What two captured steps do not share bit for bit: (buffers, weight-gradient tensors)."""
    bufs = [n for n in R.buffer_names(NET) if not torch.equal(a['T'][n], b['T'][n])]
    ga, gb = NET.weights(a['grads']), NET.weights(b['grads'])
    return bufs, [ci for ci in range(len(NET.convs)) if not (torch.equal(ga[ci][0], gb[ci][0]) and (ga[ci][1] is None or torch.equal(ga[ci][1], gb[ci][1])))]


def test_side_stream_switch_changes_what_the_header_says(stale_runs):
    """include/eosvos.h, eosvos_set_side_stream: the loss, every data gradient and every weight gradient but layer1's at batch > 1
    (and the pre-split path's in f16x3 -- not taken here: bf16x6) are bit-identical with and without the stream.  Steps 5 / 6
    (batch 3) and 7 / 8 (batch 1) of the sequence differ in nothing else.  Layer1's gradients of step 6 pass the fp64 audit above."""
    layer1 = set(_convs_of('layer1'))
    for a, b, allowed in ((stale_runs[4], stale_runs[5], layer1), (stale_runs[6], stale_runs[7], set())):
        bufs, convs = _same(a, b)
        print(f'MARGIN side stream on vs off, batch {a["T"]["x"].shape[0]}: buffers that differ {bufs}, weight gradients {[NET.convs[ci].name for ci in convs]}')
        assert a['loss'] == b['loss'] and not bufs, bufs
        assert set(convs) <= allowed, [NET.convs[ci].name for ci in convs if ci not in allowed]


# ---- F(4,3) decoder ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['f16x3', 'f32'])
def test_decoder_links_on_an_f43_map(mode):
    """257 x 261: a stride-4 map of 65 x 66 >= EOSVOS_WINO_F4_MINDIM, the decoder's 3x3 convs take F(4,3)."""
    e = _new_engine(257, 261, max_batch=1)
    try:
        e.set_engine_matrix_mode(mode)
        e.set_lr(torch.zeros(e.n_lr))
        e.reset()
        run = _capture(e, *synthetic.synthetic_frames(1, 257, 261, seed=41))
    finally:
        e.close()
    assert tuple(run['T']['d1'].shape[-2:]) == (65, 66)
    assert _conv_floor(NET.dec_a, (65, 66)) == TOL['wino_f4'] and _conv_floor(NET.dec_b, (17, 25)) == TOL['wino_f2']
    assert torch.equal(run['before'], run['after'])
    _audit_weights(run, f'{mode} 257x261 decoder', _convs_of('decoder'))
    _audit_data(run, f'{mode} 257x261 decoder', 'decoder')


# ---- the update link ------------------------------------------------------------------------------------------------------------------
def test_update_of_every_scalar(eng):
    """Second step of a trajectory, real learning rates, batch 3, f16x3: params_after == params_before - lr * grad per element
    (fp64 from the engine's own fp32 gradient, lr per output channel), to 2^-23 (|w| + |lr g|) -- see R.update_reference."""
    eng.set_engine_matrix_mode('f16x3')
    lr = torch.cat([l.reshape(-1).float() for l in synthetic.synthetic_lrs('resnet50')])
    eng.set_lr(lr)
    eng.reset()
    try:
        x, y = synthetic.synthetic_frames(3, H, W, seed=51)
        eng.finetune_step(x.to(DEV), y.to(DEV))
        x, y = synthetic.synthetic_frames(3, H, W, seed=52)
        before = eng.get_params().cpu()
        eng.finetune_step(x.to(DEV), y.to(DEV))
        grads, after = eng.get_grads().cpu(), eng.get_params().cpu()
    finally:
        eng.set_lr(torch.zeros(eng.n_lr))
        eng.reset()
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
    ref, bound = R.update_reference(NET, before, lr, grads)
    err = (after.double() - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    ratio[(err == 0)] = 0
    i = int(ratio.argmax())
    name, off = R.tensor_of(NET, i)
    moved = int((after != before).sum())
    print(f'MARGIN update link, {after.numel()} scalars ({moved} moved): worst {float(ratio[i]):.3f} of the bound at index {i} '
          f'({name} + {off}): {float(after[i]):.9e} vs {float(ref[i]):.9e}, w {float(before[i]):.9e}, g {float(grads[i]):.3e}')
    assert moved > 0
    assert bool((err <= bound).all()), (i, name, off, float(err[i]), float(bound[i]), int((err > bound).sum()))
