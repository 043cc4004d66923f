"""Per-link fp64 audit of the forward pass INSIDE the network: DeepLabV3+ on resnet50 (frozen BatchNorm and GroupNorm) and
resnet101, and plain DeepLabV3 on resnet50.

The backward audits (tests/test_gpu_backward_links.py, tests/test_gpu_meta_links.py) take the forward activations as given, the
op suites run each kernel on a scratch engine that holds one conv, and the end-to-end parity tests are 5 to 50 times looser than
a kernel's own bound.  What `forward_impl` adds inside the network -- the side-stream forks and joins, the channel-slice views
into `cat` / `dcat`, the residual from `dsb` or the block's input, the cached Winograd-domain weights and their `us_valid` flags,
the absmax slots of the f16x3 mode, the pre-split siblings, the inference form without mask writes -- is checked here: after
`eng.forward(x)` every LINK (tests/forward_links_ref.py, proved against the oracle network in
tests/test_forward_links_host.py) is recomputed in float64 on the CPU from the engine's own operands, weights and folded
norm scale / shift, and compared elementwise with the buffer or channel slice the engine left:

    err = max|gpu - ref64| / max|ref64|  <=  max(K * err_torch32, floor),  under the condition  K * err_torch32 <= CAP_RATIO * floor

K and the floors are the op suites' own (test_gpu_misc_ops.K / FLOOR, test_gpu_conv_algos.TOL / STEM_FLOOR, chosen per conv as
test_gpu_backward_links._conv_floor chooses them); CAP_RATIO = 25 is the ratio of GN_CAP to the GroupNorm floors.  In GroupNorm
mode a conv's link targets its raw output `z<ci>`; the activation from z is the existing GN forward link.  The max-pool and the
broadcast of the pooling branch are exact, every ReLU output is >= 0, and the tensor `forward()` returns has the bits of
`logits`.

One MARGIN line per link group (profiles/forward_links_margins.txt holds a run's lines).
"""
import functools
import types

import pytest
import torch

import backward_links_ref as R
import forward_links_ref as FR
from eosvos_amd import _ffi, synthetic, topology
from test_gpu_backward_links import GN_CAP, H, W, _audit_gn, _conv_floor, _errs, _new_engine, _where
from test_gpu_conv_algos import STEM_FLOOR, TOL
from test_gpu_misc_ops import FLOOR, K

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CAP_RATIO = 25              # K * err_torch32 <= CAP_RATIO * floor: GN_CAP / FLOOR['gn_fwd'] (asserted below)
assert abs(GN_CAP / FLOOR['gn_fwd'] - CAP_RATIO) < 1e-9 and FLOOR['gn_fwd'] == FLOOR['gn_bwd']
MODES = ['f16x3', 'bf16x6', 'f32']
DEFAULT_MODE = 'f16x3'
EXACT = ('maxpool_fwd', 'bcast')


def _cx(encoder, norm):
    net = R.Net(encoder, norm)
    return types.SimpleNamespace(encoder=encoder, norm=norm, net=net, links=FR.forward_links(net),
                                 gnlinks=R.gn_links(net) if norm == 'gn' else [])


BN50, GN50, BN101, V3 = _cx('resnet50', 'bn'), _cx('resnet50', 'gn'), _cx('resnet101', 'bn'), _cx('deeplabv3_resnet50', 'bn')
# (configuration, height, width, batch, frame seed, stages) of every first-forward run below: the host file asserts the cap on
# the oracle's buffers of each
FRAMES = ([(cx, H, W, b, 11 + b, R.STAGES) for cx in ('BN50', 'GN50') for b in (1, 3)] + [('BN101', H, W, 3, 14, R.STAGES)]
          + [('V3', H, W, b, 11 + b, R.STAGES) for b in (1, 2)] + [('V3', 97, 161, 1, 12, R.STAGES)]
          + [(cx, 257, 261, 1, 41, ('decoder',)) for cx in ('BN50', 'GN50')]
          + [('BN50', H, W, 3, 31, R.STAGES), ('BN50', H, W, 1, 32, R.STAGES)])


def link_floor(cx, l, out_hw):
    """The op suites' floor of link l on an output map of out_hw; None for an exact link."""
    if l.kind in EXACT:
        return None
    if l.kind == 'stem':
        return STEM_FLOOR
    if l.kind == 'conv':
        return _conv_floor(l.ci, out_hw, cx)
    return FLOOR[l.kind]


def link_name(cx, l):
    return (cx.net.convs[l.ci].name if l.ci >= 0 else l.kind) + f' -> {l.out}[{l.c0}:{l.c1}]'


@functools.lru_cache(maxsize=None)
def _state(encoder):
    return synthetic.synthetic_state(encoder)


def _capture(eng, x, cx, form='forward'):
    """One forward of x in the given form, then everything the links read, on the CPU."""
    xd = x.to(DEV)
    if form == 'forward':
        out = eng.forward(xd)
    elif form == 'infer':
        out = eng.infer(xd)
    else:
        eng.infer_view(xd, mirror=False)
        out = None
    eng.synchronize()
    net = cx.net
    T = {n: eng.debug_tensor(n).cpu() for n in FR.forward_buffer_names(net) + (R.z_names(net) if net.gn else [])}
    T['x'] = x
    run = dict(T=T, out=None if out is None else out.cpu(), params=eng.get_params().cpu())
    if not net.gn:
        run['norm_a'], run['norm_b'] = eng.debug_tensor('norm_a').reshape(-1).cpu(), eng.debug_tensor('norm_b').reshape(-1).cpu()
    assert all(bool(torch.isfinite(t).all()) for t in T.values())
    return run


def _operands(run, cx, dtype, params=None, norm_a=None):
    net = cx.net
    p = run['params'] if params is None else params
    Wt = net.weights(p.to(dtype))
    if net.gn:
        none = [None] * len(net.convs)
        return Wt, none, none
    a = run['norm_a'] if norm_a is None else norm_a
    return Wt, net.scales(a.to(dtype)), net.scales(run['norm_b'].to(dtype))


def _rows(run, cx, links, params=None, norm_a=None):
    """Per link (name, err_gpu, err_torch32, bound, floor, problems): the comparison of the module docstring."""
    T64, T32 = R.Cast(run['T'], torch.float64), R.Cast(run['T'], torch.float32)
    O64, O32 = _operands(run, cx, torch.float64, params, norm_a), _operands(run, cx, torch.float32, params, norm_a)
    rows = []
    for l in links:
        name, got, bad = link_name(cx, l), FR.target(l, run['T']), []
        r32 = l.fn(T32, *O32)
        if l.kind in EXACT:
            if not torch.equal(got, r32):
                bad.append(f'{name}: not bit-equal, {int((got != r32).sum())} elements differ, worst at {_where(got, r32.double(), 3)}')
            rows.append((name, 0.0, 0.0, 0.0, None, bad))
            continue
        r64 = l.fn(T64, *O64)
        eg, e32 = _errs(got, r64, r32)
        floor = link_floor(cx, l, tuple(got.shape[-2:]))
        if not K * e32 <= CAP_RATIO * floor:
            bad.append(f'{name}: torch32 {e32:.2e} breaks the cap {CAP_RATIO} * {floor:.1e} / {K}: an ill-conditioned link')
        bound = max(K * e32, floor)
        if not eg <= bound:
            bad.append(f'{name}: {eg:.3e} > {bound:.3e} (torch32 {e32:.2e}) at {_where(got, r64)}')
        if l.relu and not bool((got >= 0).all()):
            bad.append(f'{name}: {int((got < 0).sum())} negative ReLU outputs')
        rows.append((name, eg, e32, bound, floor, bad))
    return rows


def _audit(run, cx, label, stages=R.STAGES, conv_only=False):
    links = [l for l in cx.links if l.stage in stages and not (conv_only and l.ci < 0)]
    assert links
    rows = _rows(run, cx, links)
    inexact = [r for r in rows if r[4] is not None]
    worst = max(inexact, key=lambda r: r[1] / r[3])
    by_torch = [r[0] for r in inexact if r[3] > r[4]]
    print(f'MARGIN {label} forward links ({len(rows)}, {len(rows) - len(inexact)} exact): worst {worst[0]} {worst[1]:.2e} '
          f'(torch32 {worst[2]:.2e}, bound {worst[3]:.2e}, {worst[1] / worst[3]:.2f} of it); bound set by torch32: {by_torch or "none"}')
    bad = [b for r in rows for b in r[5]]
    assert not bad, (label, bad)


def _set_mode(eng, mode):
    eng.set_engine_matrix_mode(mode)
    eng.set_lr(torch.zeros(eng.n_lr))
    eng.reset()
    eng._verify_pending = False


def _first_runs(eng, cx, height=H, width=W):
    cache = {}

    def get(mode, batch):
        if (mode, batch) not in cache:
            cache.clear()               # the runs are visited one after the other: keep one
            _set_mode(eng, mode)
            x, _ = synthetic.synthetic_frames(batch, height, width, seed=11 + batch)
            cache[(mode, batch)] = _capture(eng, x, cx)
        return cache[(mode, batch)]
    return get


def _logits_bits(run):
    assert torch.equal(run['out'], run['T']['logits']), 'forward() returned other bits than the engine\'s logits buffer'


# ---- every link of a first forward --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def eng():
    e = _new_engine(cx=BN50)
    yield e
    e.close()


@pytest.fixture(scope='module')
def eng_gn():
    e = _new_engine(cx=GN50)
    yield e
    e.close()


@pytest.fixture(scope='module')
def eng_v3():
    e = _new_engine(max_batch=2, cx=V3)
    yield e
    e.close()


@pytest.fixture(scope='module')
def bn_runs(eng):
    return _first_runs(eng, BN50)


@pytest.fixture(scope='module')
def gn_runs(eng_gn):
    return _first_runs(eng_gn, GN50)


@pytest.fixture(scope='module')
def v3_runs(eng_v3):
    return _first_runs(eng_v3, V3)


@pytest.mark.parametrize('stage', R.STAGES)
@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('mode', MODES)
def test_every_forward_link(bn_runs, mode, batch, stage):
    run = bn_runs(mode, batch)
    _logits_bits(run)
    _audit(run, BN50, f'{mode} batch {batch} {stage}', (stage,))


@pytest.mark.parametrize('stage', R.STAGES)
@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('mode', MODES)
def test_groupnorm_every_forward_link(gn_runs, mode, batch, stage):
    """conv -> z links (the raw outputs, which no backward audit can see: the backward pass overwrites them), the exact and misc
    links, and the activation from z."""
    run = gn_runs(mode, batch)
    _logits_bits(run)
    label = f'gn {mode} batch {batch} {stage}'
    _audit(run, GN50, label, (stage,))
    _audit_gn(run, label, (stage,), cx=GN50, backward=False)


@pytest.fixture(scope='module')
def run_101():
    e = _new_engine(cx=BN101)
    try:
        _set_mode(e, DEFAULT_MODE)
        return _capture(e, synthetic.synthetic_frames(3, H, W, seed=14)[0], BN101)
    finally:
        e.close()


@pytest.mark.parametrize('stage', R.STAGES)
def test_resnet101_every_forward_link(run_101, stage):
    _logits_bits(run_101)
    _audit(run_101, BN101, f'resnet101 {DEFAULT_MODE} batch 3 {stage}', (stage,))


@pytest.mark.parametrize('stage', R.STAGES)
@pytest.mark.parametrize('batch', [1, 2])
@pytest.mark.parametrize('mode', MODES)
def test_deeplabv3_every_forward_link(v3_runs, mode, batch, stage):
    """Output stride 8: a 9 x 13 ASPP map, on which almost every non-centre tap of the rate 12 / 24 / 36 convs is padding."""
    run = v3_runs(mode, batch)
    assert tuple(run['T']['cat'].shape) == (batch, 1280, 9, 13) and tuple(run['T']['d1'].shape) == (batch, 256, 9, 13)
    _logits_bits(run)
    _audit(run, V3, f'deeplabv3 {mode} batch {batch} {stage}', (stage,))


@pytest.fixture(scope='module')
def run_v3_wide():
    e = _new_engine(97, 161, max_batch=1, cx=V3)
    try:
        _set_mode(e, DEFAULT_MODE)
        return _capture(e, synthetic.synthetic_frames(1, 97, 161, seed=12)[0], V3)
    finally:
        e.close()


@pytest.mark.parametrize('stage', R.STAGES)
def test_deeplabv3_every_forward_link_with_rate12_taps_inside(run_v3_wide, stage):
    """97 x 161: a 13 x 21 ASPP map, rate-12 taps land inside the map."""
    assert tuple(run_v3_wide['T']['cat'].shape) == (1, 1280, 13, 21)
    _logits_bits(run_v3_wide)
    _audit(run_v3_wide, V3, f'deeplabv3 {DEFAULT_MODE} 97x161 {stage}', (stage,))


@pytest.mark.parametrize('mode', ['f16x3', 'f32'])
@pytest.mark.parametrize('cx', [BN50, GN50], ids=['bn', 'gn'])
def test_decoder_forward_links_on_an_f43_map(cx, mode):
    """257 x 261: a stride-4 map of 65 x 66 >= EOSVOS_WINO_F4_MINDIM, the decoder's first 3x3 conv takes F(4,3)."""
    e = _new_engine(257, 261, max_batch=1, cx=cx)
    try:
        _set_mode(e, mode)
        run = _capture(e, synthetic.synthetic_frames(1, 257, 261, seed=41)[0], cx)
    finally:
        e.close()
    assert tuple(run['T']['d1'].shape[-2:]) == (65, 66) and _conv_floor(cx.net.dec_a, (65, 66), cx) == TOL['wino_f4']
    label = f'{cx.norm} {mode} 257x261 decoder'
    _logits_bits(run)
    _audit(run, cx, label, ('decoder',))
    if cx.net.gn:
        _audit_gn(run, label, ('decoder',), cx=cx, backward=False)


# ---- the fold of a frozen norm -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['resnet50', 'deeplabv3_resnet50'])
def test_fold_link(eng, eng_v3, which):
    """`norm_a` / `norm_b` per element against the float64 fold, to the bound of the kernel's own roundings
    (`forward_links_ref.fold_reference`)."""
    e, cx = (eng, BN50) if which == 'resnet50' else (eng_v3, V3)
    sd = _state(cx.encoder)
    cat = lambda suf: torch.cat([sd[p + suf].reshape(-1).float() for p, _ in topology.norm_layers(cx.encoder)])
    a, b, ba, bb = FR.fold_reference(cat('.weight'), cat('.bias'), cat('.running_mean'), cat('.running_var'))
    ga, gb = e.debug_tensor('norm_a').reshape(-1).cpu().double(), e.debug_tensor('norm_b').reshape(-1).cpu().double()
    assert ga.numel() == cx.net.nnorm == a.numel()
    ra, rb = ((ga - a).abs() / ba.clamp_min(1e-300)).max(), ((gb - b).abs() / bb.clamp_min(1e-300)).max()
    print(f'MARGIN fold link {which} ({a.numel()} channels): a worst {float(ra):.3f} of its bound, b worst {float(rb):.3f} of its bound')
    assert bool(((ga - a).abs() <= ba).all()) and bool(((gb - b).abs() <= bb).all()), (float(ra), float(rb))


# ---- forms of the forward that must give the same bits ---------------------------------------------------------------------------
def _differ(a, b):
    return [n for n in a['T'] if not torch.equal(a['T'][n], b['T'][n])]


@pytest.mark.parametrize('cx', [BN50, GN50], ids=['bn', 'gn'])
def test_forward_infer_and_infer_view_leave_the_same_bits(eng, eng_gn, cx):
    """Two plain forwards of one input are bit-identical (so equality is the right bound); then `forward`, `infer` and
    `infer_view(mirror=False)` from one state leave every named forward buffer bit-identical: the inference form skips only the
    mask writes."""
    e = eng if cx is BN50 else eng_gn
    _set_mode(e, DEFAULT_MODE)
    x = synthetic.synthetic_frames(3, H, W, seed=14)[0]
    a, b = _capture(e, x, cx), _capture(e, x, cx)
    assert not _differ(a, b) and torch.equal(a['out'], b['out']), ('two plain forwards differ', _differ(a, b))
    inf, view, again = _capture(e, x, cx, 'infer'), _capture(e, x, cx, 'infer_view'), _capture(e, x, cx)
    print(f'MARGIN {cx.norm} forward vs infer vs infer_view: buffers that differ {_differ(a, inf)} {_differ(a, view)} {_differ(a, again)}')
    assert not _differ(a, inf), _differ(a, inf)
    # (`infer` returns sigmoid(logits), not the logits: its sign is the logits')
    assert bool((a['out'][inf['out'] > 0.5] > 0).all()) and bool((a['out'][inf['out'] < 0.5] < 0).all())
    assert bool(((inf['out'] >= 0) & (inf['out'] <= 1)).all())
    assert not _differ(a, view), _differ(a, view)
    assert not _differ(a, again), _differ(a, again)


@pytest.mark.parametrize('batch', [1, 3])
def test_side_stream_on_and_off_leave_the_same_bits(eng, batch):
    """`eosvos_set_side_stream`: "Scheduling only -- results are bit-identical", in every forward buffer."""
    _set_mode(eng, DEFAULT_MODE)
    x = synthetic.synthetic_frames(batch, H, W, seed=11 + batch)[0]
    on = _capture(eng, x, BN50)
    assert eng.set_side_stream(False) is False
    try:
        off = _capture(eng, x, BN50)
    finally:
        assert eng.set_side_stream(True) is True
    back = _capture(eng, x, BN50)
    print(f'MARGIN side stream on vs off, forward, batch {batch}: buffers that differ {_differ(on, off)} {_differ(on, back)}')
    assert not _differ(on, off) and torch.equal(on['out'], off['out']), _differ(on, off)
    assert not _differ(on, back), _differ(on, back)


@pytest.fixture(scope='module')
def dirty_runs():
    """Forwards on buffers left dirty by a batch-3 step: batch 1, then batch 3 again (`lastB` switches, `pair_reset`)."""
    e = _new_engine(cx=BN50)
    try:
        _set_mode(e, DEFAULT_MODE)
        x3, y3 = synthetic.synthetic_frames(3, H, W, seed=31)
        x1, _ = synthetic.synthetic_frames(1, H, W, seed=32)
        e.finetune_step(x3.to(DEV), y3.to(DEV))
        return [_capture(e, x1, BN50), _capture(e, x3, BN50)]
    finally:
        e.close()


@pytest.mark.parametrize('step', [0, 1], ids=['batch_1_after_a_batch_3_step', 'batch_3_again'])
def test_forward_links_on_dirty_buffers_after_batch_switches(dirty_runs, step):
    _logits_bits(dirty_runs[step])
    _audit(dirty_runs[step], BN50, f'dirty buffers: {["batch 1 after a batch-3 step", "batch 3 again"][step]}')


# ---- stale forward caches --------------------------------------------------------------------------------------------------------
WALK = ['a fresh load', 'one finetune_step', 'a second finetune_step', 'set_params with perturbed weights',
        'snapshot, step, forward, restore_params', 'step, forward, reset', 'set_norm with a changed gamma', 'a step with layer4.. trainable']
WALK_CHANGES_WEIGHTS = [False, True, True, True, True, True, False, True]


def _wino_convs(cx, run):
    """The convs whose forward may read a cached Winograd-domain weight: those with a Winograd floor on their map."""
    out = []
    for l in cx.links:
        if l.kind == 'conv' and link_floor(cx, l, tuple(FR.target(l, run['T']).shape[-2:])) != TOL['direct']:
            out.append(l.ci)
    return out


def _walk(mode):
    cx, net = BN50, BN50.net
    e = _new_engine(max_batch=1, cx=cx)
    runs = []
    try:
        e.set_engine_matrix_mode(mode)
        lr = torch.cat([l.reshape(-1).float() for l in synthetic.synthetic_lrs(cx.encoder)])
        e.set_lr(lr)
        e.reset()
        e._verify_pending = False
        x, y = synthetic.synthetic_frames(1, H, W, seed=12)
        xd, yd = x.to(DEV), y.to(DEV)

        def cap(prev=None, prev_a=None):
            run = _capture(e, x, cx)
            if prev is not None:        # the weights of the Winograd-eligible convs before the step, for the control
                now, was = net.weights(run['params']), net.weights(prev)
                run['prev'] = {ci: was[ci][0].clone() for ci in _wino_convs(cx, run) if not torch.equal(now[ci][0], was[ci][0])}
                run['same'] = [ci for ci in range(len(net.convs)) if torch.equal(now[ci][0], was[ci][0])]
            run['prev_a'] = prev_a
            runs.append(run)

        cap()                                                   # 1
        for _ in range(2):                                      # 2, 3 (the pre-split path is live from the second step on)
            p = e.get_params().cpu()
            e.finetune_step(xd, yd)
            cap(p)
        p = e.get_params().cpu()                                # 4
        g = torch.Generator().manual_seed(4)
        e.set_params(p * (1 + 1e-3 * torch.randn(p.numel(), generator=g)))
        cap(p)
        # 5 and 6: the step's own update has already cleared the flags of every trainable conv, so a forward runs between
        # the step and the audited call: the cached transformed weights are then valid, for the post-step weights p, when
        # restore_params / reset runs, and p is what a forward that kept them would have used
        snap = e.get_params().cpu()                             # 5
        e.snapshot()
        e.finetune_step(xd, yd)
        e.forward(xd)
        p = e.get_params().cpu()
        e.restore()
        cap(p)
        assert torch.equal(runs[-1]['params'], snap), 'restore_params did not bring the snapshot back'
        e.finetune_step(xd, yd)                                 # 6
        e.forward(xd)
        p = e.get_params().cpu()
        e.reset()
        cap(p)
        assert torch.equal(runs[-1]['params'], runs[0]['params']), 'reset did not bring the initial weights back'
        sd = _state(cx.encoder)                                 # 7
        cat = lambda suf: torch.cat([sd[q + suf].reshape(-1).float() for q, _ in topology.norm_layers(cx.encoder)])
        a0 = runs[-1]['norm_a']
        e.set_norm(cat('.weight') * 1.01, cat('.bias'), cat('.running_mean'), cat('.running_var'))
        e._verify_pending = False
        cap(prev_a=a0)
        assert not torch.equal(runs[-1]['norm_a'], a0)
        first = topology.trainable_from(cx.encoder, train_encoder=False)      # 8
        e.set_trainable_from(first)
        p = e.get_params().cpu()
        e.finetune_step(xd, yd)
        cap(p)
        assert set(range(first)) <= set(runs[-1]['same']), 'a frozen conv moved'
    finally:
        e.close()
    return runs


@pytest.fixture(scope='module')
def walk_runs():
    cache = {}

    def get(mode):
        if mode not in cache:
            cache.clear()
            cache[mode] = _walk(mode)
        return cache[mode]
    return get


@pytest.mark.parametrize('step', range(len(WALK)), ids=[s.replace(' ', '_').replace(',', '').replace('.', '') for s in WALK])
@pytest.mark.parametrize('mode', [DEFAULT_MODE, 'f32'])
def test_conv_links_after_every_call_that_clears_the_forward_caches(walk_runs, mode, step):
    """One engine, batch 1: after each call that clears `us_valid` (through `wino_weights_changed`, or per conv in the fused
    update) the next forward passes every conv link against the weights and `norm_a` / `norm_b` read back after the call.
    A forward has run on the weights from before each audited call, so the transformed weights of that state are cached and
    valid when the call runs: in steps 5 and 6 that is a forward between the step and restore_params / reset.
    Control, to prove the walk sees staleness: recomputed with the weights (step 7: the scales) from before the call, every
    changed Winograd-eligible conv's link breaks its bound -- a forward that reused the transformed weight would look so."""
    cx = BN50
    run = walk_runs(mode)[step]
    label = f'walk {mode} step {step + 1} ({WALK[step]})'
    _audit(run, cx, label, conv_only=True)
    stale = None
    if WALK_CHANGES_WEIGHTS[step]:
        changed = sorted(run['prev'])
        assert changed, 'the step changed no Winograd-eligible conv'
        if step == 7:
            assert all(cx.net.stage_of(ci) in ('layer4', 'aspp', 'decoder') for ci in changed)
        params = run['params'].clone()
        for ci, w in zip(range(len(cx.net.convs)), cx.net.weights(params)):
            if ci in run['prev']:
                w[0].copy_(run['prev'][ci])
        stale = _rows(run, cx, [l for l in cx.links if l.kind == 'conv' and l.ci in run['prev']], params=params)
    elif run['prev_a'] is not None:
        wino = set(_wino_convs(cx, run))
        stale = _rows(run, cx, [l for l in cx.links if l.kind == 'conv' and l.ci in wino], norm_a=run['prev_a'])
    if stale is not None:
        weakest = min(stale, key=lambda r: r[1] / r[3])
        print(f'MARGIN {label} control ({len(stale)} links with the operands from before): weakest {weakest[0]} {weakest[1]:.2e} '
              f'({weakest[1] / weakest[3]:.1f} of its bound {weakest[3]:.2e})')
        unseen = [r[0] for r in stale if r[1] <= r[3]]
        assert not unseen, ('stale operands pass the bound', unseen)


# ---- the debug accessor on a plain DeepLabV3 engine ----------------------------------------------------------------------------
def test_deeplabv3_debug_tensor_names(eng_v3):
    """include/eosvos.h: on a plain DeepLabV3 engine `d1` / `g_d1` and `lowlog` / `g_low` live on the ASPP (stride-8) map;
    the decoder's buffers are unknown names."""
    x, _ = synthetic.synthetic_frames(2, H, W, seed=13)
    eng_v3.forward(x.to(DEV), want_logits=False)
    for name, ch in (('d1', 256), ('g_d1', 256), ('lowlog', 1), ('g_low', 1), ('proj', 256), ('cat', 1280)):
        assert tuple(eng_v3.debug_tensor(name).shape) == (2, ch, 9, 13), name
    assert tuple(eng_v3.debug_tensor('logits').shape) == (2, 1, H, W)
    for name in ('dcat', 'g_dcat', 'd2', 'g_d2'):
        with pytest.raises(_ffi.EosvosError, match='unknown debug tensor'):
            eng_v3.debug_tensor(name)
