"""Per-link fp64 audit of the backward pass and the fused update INSIDE the network (resnet50 with frozen BatchNorm and with
GroupNorm, resnet101 with frozen BatchNorm).

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

GroupNorm mode runs code the frozen mode never touches: every normalised conv writes its raw output z (tiled epilogue,
Winograd output transform or the pooling branch's gemv), `launch_gn_forward` makes the activation and the mask bytes,
`launch_gn_backward` overwrites z with dz (and, in f16x3 mode, reduces the absmax that scales the fp16 operands of the weight and
data gradients that follow), and those gradients run without a folded scale.  The engine names that buffer `z<ci>`
(include/eosvos.h), so a GroupNorm step is captured in two phases -- forward, copy z and the activations, loss, backward_step,
copy dz and the gradients -- and one fused `finetune_step` from the same state must give the same loss and gradients bit for
bit.  Its links: the weight and data links on dz, and per normalised conv a GN forward link (activation from z) and a GN
backward link (dz from z and g), against torch's `F.group_norm` in float64:

    err <= max(K * err_torch32, FLOOR['gn_fwd' / 'gn_bwd']),  under the condition  K * err_torch32 <= GN_CAP = 1e-4

The cap (25 floors; torch fp32 on well-conditioned maps of these sizes is about 1e-7) keeps an ill-conditioned group from
widening its own bound until a wrong kernel passes; tests/test_backward_links_host.py asserts it on the oracle's buffers for
the frames used here, and every GN link asserts it on the engine's operands before it compares.

One MARGIN line per link group (profiles/backward_links_margins.txt holds a run's lines).

Not covered: the backward pass of plain DeepLabV3 (its own head graph, no GroupNorm variant).
The forward pass these links start from, plain DeepLabV3's included: tests/test_gpu_forward_links.py.
The accumulating (`gsum`) meta path and the trainable boundary: tests/test_gpu_meta_links.py.
"""
import functools

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
GN_CAP = 1e-4               # K * err_torch32 of a GN link may not exceed this (module docstring)


class Links:
    """One audited configuration: its graph and link tables."""

    def __init__(self, encoder, norm):
        self.encoder, self.norm = encoder, norm
        self.net = R.Net(encoder, norm)
        self.wlinks, self.dlinks = R.weight_links(self.net), R.data_links(self.net)
        self.gnlinks = R.gn_links(self.net) if norm == 'gn' else []


BN50, GN50, BN101 = Links('resnet50', 'bn'), Links('resnet50', 'gn'), Links('resnet101', 'bn')
NET = BN50.net


@functools.lru_cache(maxsize=None)
def _state(encoder):
    return synthetic.synthetic_state(encoder)


def _conv_floor(ci, out_hw, cx=BN50):
    """The op suites' floor of conv ci on an output map of out_hw."""
    net = cx.net
    c = net.convs[ci]
    if ci == net.pool:
        return FLOOR['pool_dw']
    if ci == net.last:
        return FLOOR['head_dw']
    wino_shape = c.k == 3 and c.stride == 1 and c.pad == c.dil and 1 <= c.dil <= 8 and c.cin % 4 == 0 and c.cout % 4 == 0
    if not wino_shape:
        return TOL['direct']
    f4 = c.dil == 1 and out_hw[0] >= WINO_F4_MINDIM and out_hw[1] >= WINO_F4_MINDIM
    return TOL['wino_f4'] if f4 else TOL['wino_f2']


def _out_hw(run, ci, cx=BN50):
    return tuple(run['T'][cx.wlinks[ci].g].shape[-2:])


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


def _capture(eng, x, y, cx=BN50):
    """One fine-tune step on (x, y), then everything the links read, on the CPU."""
    before = eng.get_params().cpu()
    eng.profile_launches(True)
    loss = eng.finetune_step(x.to(DEV), y.to(DEV))
    eng.synchronize()
    kernels = sorted(eng.profile_read())
    eng.profile_launches(False)
    T = {n: eng.debug_tensor(n).cpu() for n in R.buffer_names(cx.net)}
    T['x'] = x
    run = dict(T=T, before=before, grads=eng.get_grads().cpu(), after=eng.get_params().cpu(), loss=loss, kernels=kernels,
               norm_a=eng.debug_tensor('norm_a').reshape(-1).cpu())
    assert np.isfinite(loss) and bool(torch.isfinite(run['grads']).all())
    return run


def _capture_gn(eng, x, y, cx=GN50):
    """A GroupNorm step on (x, y) from the engine's current state, in two phases, because the backward pass overwrites every raw
    output z with dz: forward, copy z and the activations; loss, backward_step, copy dz and the gradients.  The learning
    rates are zero (asserted), so the fused `finetune_step` taken first ran from the same state: same loss and gradients, bit
    for bit."""
    net = cx.net
    xd, yd = x.to(DEV), y.to(DEV)
    before = eng.get_params().cpu()
    fused_loss = eng.finetune_step(xd, yd)
    fused_grads = eng.get_grads().cpu()
    assert torch.equal(eng.get_params().cpu(), before), 'a step with zero learning rates moved the weights'
    eng.reset()
    names = R.buffer_names(net)
    eng.forward(xd, want_logits=False)
    T = {n: eng.debug_tensor(n).cpu() for n in names if not n.split('.')[-1].startswith('g') and n != 'dlogits'}
    T.update({n: eng.debug_tensor(n).cpu() for n in R.z_names(net)})
    loss = float(eng.loss_bce(yd))
    eng.backward_step()
    eng.synchronize()
    T.update({n: eng.debug_tensor(n).cpu() for n in names if n not in T})
    T.update({'d' + n: eng.debug_tensor(n).cpu() for n in R.z_names(net)})
    T['x'] = x
    assert sorted(T) == sorted(names + ['x'] + R.z_names(net) + ['d' + n for n in R.z_names(net)])
    run = dict(T=T, before=before, grads=eng.get_grads().cpu(), after=eng.get_params().cpu(), loss=loss, kernels=[], norm_a=None)
    assert np.isfinite(loss) and bool(torch.isfinite(run['grads']).all())
    assert np.float32(loss).view(np.uint32) == np.float32(fused_loss).view(np.uint32), ('fused vs two-phase loss', fused_loss, loss)
    assert torch.equal(fused_grads, run['grads']), 'the fused step and the two-phase step differ in a gradient'
    return run


def _scales(run, cx, dtype):
    """Per conv: the folded scale of a frozen norm; None everywhere in GroupNorm mode (the links read dz)."""
    if cx.net.gn:
        return [None] * len(cx.net.convs)
    return cx.net.scales(run['norm_a'].to(dtype))


def _audit_weights(run, label, cis, floor_of=None, cx=BN50):
    """Weight links of the convs `cis` of a captured step: prints the group's MARGIN line, then asserts every link."""
    net = cx.net
    T64, T32 = R.Cast(run['T'], torch.float64), R.Cast(run['T'], torch.float32)
    A64, A32 = _scales(run, cx, torch.float64), _scales(run, cx, torch.float32)
    G = net.weights(run['grads'])
    rows, bad = [], []
    for ci in cis:
        l, c = cx.wlinks[ci], net.convs[ci]
        dw64, db64 = R.weight_link(net, l, T64, A64)
        dw32, db32 = R.weight_link(net, l, T32, A32)
        floor = floor_of(ci) if floor_of else _conv_floor(ci, _out_hw(run, ci, cx), cx)
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


def _audit_data(run, label, stage, cx=BN50):
    net = cx.net
    T64, T32 = R.Cast(run['T'], torch.float64), R.Cast(run['T'], torch.float32)
    A64, A32 = _scales(run, cx, torch.float64), _scales(run, cx, torch.float32)
    W32 = net.weights(run['before'])
    W64 = net.weights(run['before'].double())
    rows, bad = [], []
    for l in cx.dlinks:
        if l.stage != stage:
            continue
        got = run['T'][l.out]
        r64, r32 = l.fn(T64, W64, A64), l.fn(T32, W32, A32)
        eg, e32 = _errs(got, r64, r32)
        if l.misc:
            floor = MAXPOOL_FLOOR if l.misc == 'maxpool_bwd' else FLOOR[l.misc]
        else:
            floor = max(_conv_floor(ci, _out_hw(run, ci, cx), cx) for ci in l.convs)
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


def _audit_gn(run, label, stages=None, forward=True, cx=GN50, backward=True):
    """GN links of a captured GroupNorm step (of the convs of `stages`, default all): the backward links unless backward=False
    (a capture of a forward alone), and the forward links unless forward=False.  Each asserts the cap on torch32's own error on
    the engine's operands, then the bound; a forward link with a ReLU also that no output is negative."""
    net = cx.net
    T64, T32 = R.Cast(run['T'], torch.float64), R.Cast(run['T'], torch.float32)
    GB64, GB32 = R.affines(net, _state(cx.encoder), torch.float64), R.affines(net, _state(cx.encoder), torch.float32)
    for kind, fn in (('gn_fwd', R.gn_fwd_link), ('gn_bwd', R.gn_bwd_link)):
        if not (forward if kind == 'gn_fwd' else backward):
            continue
        rows, bad = [], []
        for l in cx.gnlinks:
            if stages is not None and l.stage not in stages:
                continue
            name = net.convs[l.ci].name
            r64, got = fn(net, l, T64, GB64)
            eg, e32 = _errs(got, r64, fn(net, l, T32, GB32)[0])
            if not K * e32 <= GN_CAP:
                bad.append(f'{name}: torch32 {e32:.2e} breaks the cap {GN_CAP:.0e} / {K}: an ill-conditioned group')
            bound = max(K * e32, FLOOR[kind])
            rows.append((eg / bound, name, eg, e32, bound))
            if not eg <= bound:
                bad.append(f'{name}: {eg:.3e} > {bound:.3e} (torch32 {e32:.2e}) at {_where(got, r64)}')
            if kind == 'gn_fwd' and l.relu and not bool((got >= 0).all()):
                bad.append(f'{name}: {int((got < 0).sum())} negative ReLU outputs')
        worst = max(rows)
        print(f'MARGIN {label} {kind} links ({len(rows)}): worst {worst[1]} {worst[2]:.2e} (torch32 {worst[3]:.2e}, bound {worst[4]:.2e})')
        assert not bad, (label, kind, bad)


def _convs_of(*stages, cx=BN50):
    return [l.ci for l in cx.wlinks if l.stage in stages]


def _new_engine(height=H, width=W, max_batch=3, cx=BN50):
    eng = Engine(cx.encoder, height, width, max_batch=max_batch, device=DEV, norm=cx.norm)
    eng.load_model_state(_state(cx.encoder), synthetic.synthetic_lrs(cx.encoder))
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
def _audit_update(eng, cx, label):
    """Second step of a trajectory, real learning rates, batch 3, f16x3: params_after == params_before - lr * grad per element
    (fp64 from the engine's own fp32 gradient, lr per output channel), to 2^-23 (|w| + |lr g|) -- see R.update_reference."""
    net = cx.net
    eng.set_engine_matrix_mode('f16x3')
    lr = torch.cat([l.reshape(-1).float() for l in synthetic.synthetic_lrs(cx.encoder)])
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
    ref, bound = R.update_reference(net, before, lr, grads)
    err = (after.double() - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    ratio[(err == 0)] = 0
    i = int(ratio.argmax())
    name, off = R.tensor_of(net, i)
    moved = int((after != before).sum())
    print(f'MARGIN update link{label}, {after.numel()} scalars ({moved} moved): worst {float(ratio[i]):.3f} of the bound at index {i} '
          f'({name} + {off}): {float(after[i]):.9e} vs {float(ref[i]):.9e}, w {float(before[i]):.9e}, g {float(grads[i]):.3e}')
    assert moved > 0
    assert bool((err <= bound).all()), (i, name, off, float(err[i]), float(bound[i]), int((err > bound).sum()))


def test_update_of_every_scalar(eng):
    """`_audit_update` on the frozen-BatchNorm resnet50 engine, all 40 289 729 scalars."""
    _audit_update(eng, BN50, '')


# ---- GroupNorm mode ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def eng_gn():
    e = _new_engine(cx=GN50)
    yield e
    e.close()


def _gn_run(e, mode, batch, seed, height=H, width=W):
    e.set_engine_matrix_mode(mode)
    e.set_lr(torch.zeros(e.n_lr))
    e.reset()
    return _capture_gn(e, *synthetic.synthetic_frames(batch, height, width, seed=seed))


@pytest.fixture(scope='module')
def gn_runs(eng_gn):
    cache = {}

    def get(mode, batch):
        if (mode, batch) not in cache:
            cache.clear()               # the runs are visited one after the other: keep one
            cache[(mode, batch)] = _gn_run(eng_gn, mode, batch, 11 + batch)
        return cache[(mode, batch)]
    return get


@pytest.mark.parametrize('stage', R.STAGES)
@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('mode', ['f16x3', 'bf16x6', 'f32'])
def test_groupnorm_every_link_of_a_first_step(gn_runs, mode, batch, stage):
    """Weight, data, GN forward and GN backward links of one stage; frames and seeds as the frozen-BatchNorm audit."""
    run = gn_runs(mode, batch)
    assert torch.equal(run['before'], run['after']), 'a step with zero learning rates moved the weights'
    label = f'gn {mode} batch {batch} {stage}'
    _audit_gn(run, label, (stage,))
    _audit_weights(run, label, _convs_of(stage, cx=GN50), cx=GN50)
    _audit_data(run, label, stage, cx=GN50)


@pytest.mark.parametrize('mode', ['f16x3', 'f32'])
def test_groupnorm_decoder_links_on_an_f43_map(mode):
    """257 x 261: the decoder's first 3x3 conv takes F(4,3) on its 65 x 66 map, whose output transform writes z."""
    e = _new_engine(257, 261, max_batch=1, cx=GN50)
    try:
        run = _gn_run(e, mode, 1, 41, 257, 261)
    finally:
        e.close()
    assert tuple(run['T']['d1'].shape[-2:]) == (65, 66) and tuple(run['T'][f'z{GN50.net.dec_a}'].shape) == (1, 256, 65, 66)
    assert _conv_floor(GN50.net.dec_a, (65, 66), GN50) == TOL['wino_f4'] and _conv_floor(GN50.net.dec_b, (17, 25), GN50) == TOL['wino_f2']
    assert torch.equal(run['before'], run['after'])
    label = f'gn {mode} 257x261 decoder'
    _audit_gn(run, label, ('decoder',))
    _audit_weights(run, label, _convs_of('decoder', cx=GN50), cx=GN50)
    _audit_data(run, label, 'decoder', cx=GN50)


GN_SWITCH_STEPS = ['batch 3', 'batch 1', 'batch 3 again']


@pytest.fixture(scope='module')
def gn_switch_runs():
    """One engine through batch 3, batch 1, batch 3: the GroupNorm statistics, the absmax slots and the update tables are per
    batch.  (Each capture resets the weights between its fused and its two-phase step; plans and tables stay.)"""
    e = _new_engine(cx=GN50)
    try:
        e.set_engine_matrix_mode('f16x3')
        e.set_lr(torch.zeros(e.n_lr))
        e.reset()
        f3, f1 = synthetic.synthetic_frames(3, H, W, seed=31), synthetic.synthetic_frames(1, H, W, seed=32)
        runs = [_capture_gn(e, *f3), _capture_gn(e, *f1), _capture_gn(e, *f3)]
    finally:
        e.close()
    return runs


@pytest.mark.parametrize('step', range(len(GN_SWITCH_STEPS)), ids=[s.replace(' ', '_') for s in GN_SWITCH_STEPS])
def test_groupnorm_links_after_batch_switches(gn_switch_runs, step):
    run = gn_switch_runs[step]
    assert torch.equal(run['before'], run['after'])
    label = f'gn switches: {GN_SWITCH_STEPS[step]}'
    _audit_gn(run, label, forward=False)
    _audit_weights(run, label, range(len(GN50.net.convs)), cx=GN50)


def test_raw_output_names(eng, eng_gn):
    """`z<ci>` (include/eosvos.h): the dense raw output of every normalised conv of a GroupNorm engine; an unknown name on a
    frozen-BatchNorm engine, for the classifier, past the last conv and for a malformed index."""
    net = GN50.net
    x, _ = synthetic.synthetic_frames(1, H, W, seed=12)
    eng_gn.forward(x.to(DEV), want_logits=False)
    assert tuple(eng_gn.debug_tensor('z0').shape) == (1, 64, 33, 49)
    assert tuple(eng_gn.debug_tensor(f'z{net.pool}').shape) == (1, 256, 1, 1)
    assert tuple(eng_gn.debug_tensor(f'z{net.dec1}').shape) == (1, 48, 17, 25)
    for e, name in ((eng, 'z0'), (eng, f'z{net.pool}'), (eng_gn, f'z{net.last}'), (eng_gn, f'z{len(net.convs)}'), (eng_gn, 'z'),
                    (eng_gn, 'z-1'), (eng_gn, 'z1x'), (eng_gn, 'z99999999999')):
        with pytest.raises(_ffi.EosvosError, match='unknown debug tensor'):
            e.debug_tensor(name)


def test_groupnorm_update_of_every_scalar(eng_gn):
    """`_audit_update` on the second step of a GroupNorm trajectory (no folded scale in the update table)."""
    _audit_update(eng_gn, GN50, ' gn')


# ---- ResNet-101, frozen BatchNorm: the 23-block layer3, its stage-grouped launches and its update tables ------------------------------
@pytest.fixture(scope='module')
def eng_101():
    e = _new_engine(cx=BN101)
    yield e
    e.close()


@pytest.fixture(scope='module')
def run_101(eng_101):
    eng_101.set_engine_matrix_mode('f16x3')
    eng_101.set_lr(torch.zeros(eng_101.n_lr))
    eng_101.reset()
    return _capture(eng_101, *synthetic.synthetic_frames(3, H, W, seed=14), cx=BN101)


@pytest.mark.parametrize('stage', R.STAGES)
def test_resnet101_every_link_of_a_first_step(run_101, stage):
    assert torch.equal(run_101['before'], run_101['after']), 'a step with zero learning rates moved the weights'
    label = f'resnet101 f16x3 batch 3 {stage}'
    _audit_weights(run_101, label, _convs_of(stage, cx=BN101), cx=BN101)
    _audit_data(run_101, label, stage, cx=BN101)


def test_resnet101_update_of_every_scalar(eng_101):
    _audit_update(eng_101, BN101, ' resnet101')
