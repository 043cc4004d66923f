"""Per-link fp64 audit of the meta-gradient path and the outer step: `finetune_step(accumulate=True)` -> `gsum`,
`eosvos_meta_grad_ex` -> lr gradient and init gradient, `eosvos_outer_step` -> RAdam on the learned state.

Every link (tests/meta_links_ref.py, proved against autograd and the oracle's RAdam in tests/test_meta_links_host.py) is
recomputed on the CPU in float64 from the engine's own operands -- `get_grads` after each step, `debug_gsum`, the caller's
buffers -- and compared per row / per element with what the engine left.  No reference goes through a convolution, so no
test depends on conv accuracy and none flips a ReLU gate.

    |gpu - ref64| <= max(K * |ref32 - ref64|, floor)          K = test_gpu_misc_ops.K, ref32: the same link in float32

Floors, in U = 2^-24 (one fp32 rounding), counted from the kernels (meta_links_ref.rows_n_round and its neighbours):

* lr gradient, per row (`meta_lr_grad_all_kernel`): n_round * U * S_abs + 2 U (|prior| + |result|), S_abs = |weight| sum |gsum G|
  over the row, n_round = ceil(rowlen / 256) (the per-thread fma chain) + 6 (shuffle levels) + 2 (the 4 wave sums) + 1 (times
  `weight`) + 1 (the subtract).  Log storage (`lr_grad_neuron_kernel`): + 1 (times lr_eff) + 2 (the device expf behind lr_eff,
  1 ulp), S_abs times lr_eff.  TENSOR / SINGLE (`lr_grad_reduce_kernel`): the largest row count of the group + ceil(rows / 256)
  + 6 + 2, S_abs summed over the group.
* PARAM (`meta_lr_grad_elem_kernel` + the adding export) and the init gradient: 2^-23 (|prior| + |term|) per element.  The
  caller's buffer is pre-filled with `cycle * |what a first call adds|`: rows with factors of 0.25 ... 2, PARAM elements with
  5 ... 7 -- the element bound covers the term's up to 3 + 2 roundings only where |prior| >= 4 |term| (meta_links_ref.elem_floor)
  and a larger prior would hide the term behind its own rounding.
* accumulate: bit for bit (one rounding per `+=`, torch's fp32 add reproduces it); float4 path and the classifier's odd 257.
* update of an accumulating step: backward_links_ref.update_reference, 2^-23 (|w| + |lr g|).
* outer step: 2^-22 (|p| + |delta|) for the state, 2^-22 (|beta1 m| + |(1 - beta1) g'|) for m, 2^-22 (|beta2 v| + |(1 - beta2) g'^2|)
  for v (meta_links_ref.outer_floors); frozen values, the zeroed gradient and the Winit / Wp scatter are exact.  The kernel is
  the float32 restatement operation by operation (sqrt and divide correctly rounded) but for the contraction of its final
  multiply-add, so m and v come out bit-identical to the restatement and the state within U |delta| + 2 U (|p| + |delta|) of
  it -- inside max(K err32, floor) for any err32.  (Before this audit the kernels also contracted the m, v and weight-decay
  updates, and the restatement took torch's float32 sqrt, which is not correctly rounded on the CPU: one element in 40 M
  then passed the bound by 7 %.)

One MARGIN line per link group (profiles/meta_links_margins.txt holds a run's lines).  The outer step runs every combination
of step {1, 5, 6, 40}, grad_clip {0, 1e-3} and use_log on the lr state alone (learn_model_init off), and four combinations with
the init part that cover every value of step, grad_clip, wd {0, 1e-3} and use_log, not their full product (each of those
compares 4 x 40 M elements in two precisions on the CPU).

Not covered: the per-tensor fallback loop of `eosvos_meta_grad_ex` (it only runs if the one-launch tables cannot be made: an
allocation failure or more than 160 tensors, which no supported topology reaches) and the RCCL exchange.
"""
import numpy as np
import pytest
import torch

import backward_links_ref as R
import meta_links_ref as M
from eosvos_amd import synthetic, topology
from eosvos_amd.engine import Engine
from test_gpu_misc_ops import K

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H, W = 65, 97                   # the audit's ragged size (tests/test_gpu_backward_links.py)
STEPS = 3
SENTINEL = 7.0                  # finite: a NaN would hide a `+= 0`
ROW_CYCLE = torch.tensor([1.0, -1.5, 0.5, -0.25, 2.0])
ELEM_CYCLE = torch.tensor([5.0, -6.0, 7.0, -5.0])
LR_CASES = [(l, u) for l in ('NEURON', 'TENSOR', 'SINGLE', 'PARAM') for u in (False, True)]


def _new_engine(encoder='resnet50', norm='bn'):
    eng = Engine(encoder, H, W, max_batch=1, device=DEV, norm=norm)
    eng.load_model_state(synthetic.synthetic_state(encoder), synthetic.synthetic_lrs(encoder))
    eng._verify_pending = False
    eng.keep_grads(True)
    return eng


def _frames(seed=61):
    x, y = synthetic.synthetic_frames(1, H, W, seed=seed)
    xm, ym = torch.flip(x, dims=[3]).contiguous(), torch.flip(y, dims=[3]).contiguous()
    return x.to(DEV), y.to(DEV), xm.to(DEV), ym.to(DEV)


def _flat_lrs(encoder='resnet50'):
    return torch.cat([l.reshape(-1).float() for l in synthetic.synthetic_lrs(encoder)])


def _store(level, use_log, encoder='resnet50'):
    s = synthetic.synthetic_lr_state(encoder, level, use_log)
    return (torch.cat([t.flatten() for t in s]) if isinstance(s, list) else s.flatten()).float()


def _accumulate(eng, x, y, steps, with_params=False):
    """`steps` accumulating steps; per step the engine's gradient and gradient sum (and the parameters around the step)."""
    out = []
    for _ in range(steps):
        before = eng.get_params().cpu() if with_params else None
        loss = eng.finetune_step(x, y, accumulate=True)
        assert np.isfinite(loss)
        out.append(dict(before=before, grad=eng.get_grads().cpu(), gsum=eng.debug_gsum().cpu(),
                        after=eng.get_params().cpu() if with_params else None))
    return out


def _cycle(n, cyc):
    return cyc.repeat((n + cyc.numel() - 1) // cyc.numel())[:n]


def _meta(eng, net, xm, ym, level, weight, frozen_store=0, frozen_param=0, **flags):
    """One meta_grad into a pre-filled buffer: (prior, result, G) on the CPU.  The fill: `cycle * |what a first call into
    zeros adds|` (module docstring), SENTINEL on the frozen part."""
    ns = net.store_count(level)
    probe = torch.zeros(ns + net.nparam, device=DEV)
    eng.meta_grad(xm, ym, probe, weight=weight)
    cyc = torch.cat([_cycle(ns, ELEM_CYCLE if level == 'PARAM' else ROW_CYCLE), _cycle(net.nparam, ROW_CYCLE)])
    prior = cyc.to(DEV) * probe.abs()
    prior[:frozen_store] = SENTINEL
    prior[ns:ns + frozen_param] = SENTINEL
    buf = prior.clone()
    loss = eng.meta_grad(xm, ym, buf, weight=weight, **flags)
    assert np.isfinite(loss)
    return prior.cpu(), buf.cpu(), eng.get_grads().cpu()


def _margin(label, got, r64, r32, floor):
    """Prints the MARGIN line of one link group; returns the number of values outside max(K |ref32 - ref64|, floor)."""
    assert got.shape == r64.shape and bool(torch.isfinite(got).all())
    err, e32 = (got.double() - r64).abs(), (r32.double() - r64).abs()
    bound = torch.maximum(K * e32, floor)
    ratio = err / bound.clamp_min(1e-300)
    ratio[err == 0] = 0
    i = int(ratio.argmax())
    bad = int((err > bound).sum())
    print(f'MARGIN {label} ({got.numel()} values, {int((r64 != 0).sum())} nonzero): worst {float(ratio[i]):.3f} of the bound at {i}: '
          f'{float(got[i]):.9e} vs {float(r64[i]):.9e} (torch32 off by {float(e32[i]):.2e}, floor {float(floor[i]):.2e}); outside: {bad}')
    return bad


def _audit_meta(net, label, level, use_log, weight, store, gsum, prior, got, G, check_init=True):
    """The lr gradient and the init gradient of one meta_grad call against their links."""
    ns, w = net.store_count(level), M.f32(weight)

    def link(dt):
        gs, Gd, st, pr = gsum.to(dt), G.to(dt), store.to(dt), prior[:ns].to(dt)
        if level == 'PARAM':
            term = M.lr_grad_param(gs, Gd, st.exp() if use_log else None, w)
            return pr + term, term, None
        glr, sabs = M.lr_grad_neuron(gs, Gd, w, net)
        lr_eff = M.expand_lr(st, level, use_log, net)
        return pr + M.lr_grad_store(glr, lr_eff, level, use_log, net), sabs, lr_eff

    r64, s64, lr64 = link(torch.float64)
    r32 = link(torch.float32)[0]
    p64 = prior[:ns].double()
    floor = M.elem_floor(p64, s64) if level == 'PARAM' else M.store_floor(net, level, use_log, s64, lr64, p64, r64)
    assert bool((r64 != p64).any()), 'the link adds nothing'
    bad = [_margin(f'{label}: lr gradient {level}{" log" if use_log else ""} weight {weight}', got[:ns], r64, r32, floor)]
    if check_init:
        pi, G64 = prior[ns:].double(), G.double()
        bad.append(_margin(f'{label}: init gradient weight {weight}', got[ns:], M.init_grad_link(pi, G64, w),
                           M.init_grad_link(prior[ns:], G, w), M.elem_floor(pi, w * G64)))
    assert bad == [0] * len(bad), (label, bad)


# ---- the shared engine and trajectory -------------------------------------------------------------------------------------------------
class Base:
    pass


@pytest.fixture(scope='module')
def base():
    b = Base()
    b.net = M.Layout.of('resnet50')
    b.eng = _new_engine()
    b.lr = _flat_lrs()
    b.x, b.y, b.xm, b.ym = _frames()
    with pytest.raises(Exception, match='meta_task_begin'):
        b.eng.debug_gsum()
    b.eng.meta_task_begin()
    b.steps = _accumulate(b.eng, b.x, b.y, STEPS, with_params=True)
    yield b
    b.eng.close()


def test_layout_matches_the_engine(base):
    assert (base.net.nparam, base.net.nlr) == (base.eng.n_param, base.eng.n_lr)
    for level in ('NEURON', 'TENSOR', 'SINGLE', 'PARAM'):
        assert base.net.store_count(level) == base.eng.lr_store_count(level)


def test_accumulate_link_is_bit_exact(base):
    """`debug_gsum()` after step k == the fp32 sequential sum of the k captured gradients, all 40 289 729 elements: the float4
    path of `sgd_update_all_kernel` and its odd-size path (the classifier's 256 weights + 1 bias)."""
    grads = [s['grad'] for s in base.steps]
    for k in range(1, STEPS + 1):
        want, got = M.accumulate_link(grads[:k]), base.steps[k - 1]['gsum']
        diff = int((want != got).sum())
        print(f'MARGIN accumulate link, step {k}: {got.numel()} elements, {int((got != 0).sum())} nonzero, differing {diff}')
        assert diff == 0
    assert not torch.equal(grads[0], grads[1]) and int(torch.count_nonzero(base.steps[-1]['gsum'][-257:])) > 100      # the odd tensor took part


@pytest.mark.parametrize('k', range(STEPS))
def test_update_link_of_an_accumulating_step(base, k):
    s = base.steps[k]
    ref, bound = R.update_reference(base.net, s['before'], base.lr, s['grad'])
    err = (s['after'].double() - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    ratio[err == 0] = 0
    i = int(ratio.argmax())
    print(f'MARGIN update link of accumulating step {k + 1}: {int((s["after"] != s["before"]).sum())} of {err.numel()} moved, '
          f'worst {float(ratio[i]):.3f} of the bound at {i}')
    assert not torch.equal(s['before'], s['after'])
    assert bool((err <= bound).all()), (i, float(err[i]), float(bound[i]), int((err > bound).sum()))


# ---- the lr gradient at every level ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('level,use_log', LR_CASES)
def test_lr_gradient_link(base, level, use_log):
    eng, net, store = base.eng, base.net, _store(level, use_log)
    eng.set_lr_state(level, use_log, store)
    try:
        eng.meta_task_begin()
        gsum = _accumulate(eng, base.x, base.y, STEPS)[-1]['gsum']
        for weight in (1.0, 0.3):
            prior, got, G = _meta(eng, net, base.xm, base.ym, level, weight)
            _audit_meta(net, 'resnet50', level, use_log, weight, store, gsum, prior, got, G, check_init=(level == 'NEURON'))
        assert torch.equal(eng.debug_gsum().cpu(), gsum), 'meta_grad without new_segment moved gsum'
    finally:
        eng.set_lr(base.lr)


# ---- flags ---------------------------------------------------------------------------------------------------------------------------------
def test_flags_init_grad_off_and_new_segment(base):
    eng, net = base.eng, base.net
    eng.set_lr(base.lr)
    eng.meta_task_begin()
    _accumulate(eng, base.x, base.y, STEPS)
    buf = torch.full((net.nlr + net.nparam,), SENTINEL, device=DEV)
    eng.meta_grad(base.xm, base.ym, buf, weight=0.3, init_grad=False, new_segment=True)
    assert int((buf[net.nlr:] != SENTINEL).sum()) == 0, 'init_grad=False wrote into the init part'
    assert int((buf[:net.nlr] != SENTINEL).sum()) > 0
    assert int(torch.count_nonzero(eng.debug_gsum())) == 0, 'new_segment=True left something in gsum'
    two = _accumulate(eng, base.x, base.y, 2)
    gsum = M.accumulate_link([s['grad'] for s in two])
    assert torch.equal(two[-1]['gsum'], gsum)
    prior, got, G = _meta(eng, net, base.xm, base.ym, 'NEURON', 1.0)
    _audit_meta(net, 'new segment, its two steps alone', 'NEURON', False, 1.0, base.lr, gsum, prior, got, G)


# ---- the trainable boundary ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def bound_eng():
    e = _new_engine()
    yield e
    e.close()


BOUNDARIES = {'layer4': topology.trainable_from('resnet50', train_encoder=False), 'aspp': 'classifier.0.convs.0.0'}


@pytest.mark.parametrize('level,use_log', [('NEURON', False), ('NEURON', True), ('TENSOR', True), ('PARAM', False)])
@pytest.mark.parametrize('where', list(BOUNDARIES))
def test_trainable_boundary(base, bound_eng, where, level, use_log):
    eng, net, store = bound_eng, base.net, _store(level, use_log)
    ci = BOUNDARIES[where] if isinstance(BOUNDARIES[where], int) else net.conv_index(BOUNDARIES[where])
    p0, r0 = net.poff[ci], net.lroff[ci]
    fs = {'NEURON': r0, 'TENSOR': net.tensor_row0.index(r0), 'PARAM': p0}[level]
    ns = net.store_count(level)
    eng.set_trainable_from(ci)
    try:
        eng.set_lr_state(level, use_log, store)
        eng.meta_task_begin()
        steps = _accumulate(eng, base.x, base.y, STEPS, with_params=True)
        gsum = steps[-1]['gsum']
        assert torch.equal(gsum, M.accumulate_link([s['grad'] for s in steps]))
        assert int(torch.count_nonzero(gsum[:p0])) == 0 and int(torch.count_nonzero(gsum[p0:])) > 0
        for s in steps:
            assert int(torch.count_nonzero(s['grad'][:p0])) == 0
            assert torch.equal(s['after'][:p0], s['before'][:p0]) and not torch.equal(s['after'][p0:], s['before'][p0:])
        prior, got, G = _meta(eng, net, base.xm, base.ym, level, 0.3, frozen_store=fs, frozen_param=p0)
        for part, n in ((got[:fs], fs), (got[ns:ns + p0], p0)):
            assert part.numel() == n and n > 0 and int((part != SENTINEL).sum()) == 0, 'a frozen entry of the buffer changed'
            assert torch.equal(part, torch.full((n,), SENTINEL))
        _audit_meta(net, f'boundary {where}', level, use_log, 0.3, store, gsum, prior, got, G)
    finally:
        eng.set_trainable_from(0)
        eng.set_lr(base.lr)


# ---- other topologies ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('encoder,norm', [('resnet101', 'bn'), ('deeplabv3_resnet50', 'bn'), ('resnet50', 'gn')])
def test_other_topologies(encoder, norm):
    net, lr = M.Layout.of(encoder), _flat_lrs(encoder)
    x, y, xm, ym = _frames()
    eng = _new_engine(encoder, norm)
    try:
        assert (net.nparam, net.nlr) == (eng.n_param, eng.n_lr)
        eng.meta_task_begin()
        steps = _accumulate(eng, x, y, STEPS)
        gsum = steps[-1]['gsum']
        assert torch.equal(gsum, M.accumulate_link([s['grad'] for s in steps]))
        prior, got, G = _meta(eng, net, xm, ym, 'NEURON', 0.3)
    finally:
        eng.close()
    _audit_meta(net, f'{encoder} {norm}', 'NEURON', False, 0.3, lr, gsum, prior, got, G)


# ---- the outer step ------------------------------------------------------------------------------------------------------------------------
OUTER_CASES = [dict(step=1, grad_clip=0.0, wd=0.0, use_log=False, init=True, finetune=False),
               dict(step=5, grad_clip=1e-3, wd=1e-3, use_log=True, init=True, finetune=False),
               dict(step=6, grad_clip=1e-3, wd=0.0, use_log=False, init=True, finetune=True),
               dict(step=40, grad_clip=0.0, wd=1e-3, use_log=True, init=True, finetune=True)]
OUTER_CASES += [dict(step=s, grad_clip=gc, wd=1e-3 if (i + j) % 2 else 0.0, use_log=ul, init=False, finetune=False)
                for s in (1, 5, 6, 40) for i, gc in enumerate((0.0, 1e-3)) for j, ul in enumerate((False, True))]
FROZEN_LR, FROZEN_PARAM = 1077, 300003          # both end inside a 256-thread group, neither on a 1024 boundary
GRAD_SCALE, CLIP = 0.5, 1e-3


@pytest.fixture(scope='module')
def outer_eng():
    e = _new_engine()
    e.init0 = e.get_params().clone()            # every case starts from the same init, whatever ran before it
    yield e
    e.close()


def _outer_inputs(eng, net, c):
    """State, gradient and moments on the device from a fixed seed, with the edges planted behind the frozen prefixes."""
    g = torch.Generator(device=DEV).manual_seed(77)
    n_lr, n = net.nlr, net.nlr + (net.nparam if c['init'] else 0)
    lo, hi = 6e-4, 1.4e-3
    state = torch.empty(n, device=DEV)
    state[:n_lr] = 1e-3 * (0.5 + torch.rand(n_lr, device=DEV, generator=g))                 # some beyond either clamp
    if c['use_log']:
        state[:n_lr] = state[:n_lr].log()                                                   # negative states
        lo, hi = float(np.log(lo)), float(np.log(hi))
    lo, hi = M.f32(lo), M.f32(hi)
    state[:FROZEN_LR] = state[:FROZEN_LR].clamp(lo, hi)                                     # the clamp reaches frozen values too
    if c['init']:
        state[n_lr:] = eng.init0
    grad = torch.randn(n, device=DEV, generator=g) * 2e-3
    m = torch.randn(n, device=DEV, generator=g) * 1e-3
    v = torch.rand(n, device=DEV, generator=g) * 1e-6
    edge = torch.tensor(CLIP, dtype=torch.float32) / GRAD_SCALE                              # exact: a power of two
    inside, outside = torch.nextafter(edge, torch.tensor(0.0)), torch.nextafter(edge, torch.tensor(1.0))
    plant = torch.stack([edge, -edge, inside, -inside, outside, -outside]).to(DEV)
    for a in (FROZEN_LR + 3,) + ((n_lr + FROZEN_PARAM + 3,) if c['init'] else ()):
        grad[a:a + 6] = plant
        v[a + 8:a + 10] = 0.0                                                               # v = 0 with m != 0: the denominator is eps
        m[a + 8:a + 10] = torch.tensor([1e-3, -1e-3], device=DEV)
        grad[a + 8:a + 10] = 0.0
    a = FROZEN_LR + 20                                                                      # states that land exactly on the clamps
    state[a:a + 2] = torch.tensor([lo, hi], device=DEV)
    grad[a:a + 2] = 0.0
    m[a:a + 2] = 0.0
    v[a:a + 2] = 1.0
    hyper = dict(step=c['step'], lr_lr=1e-3, init_lr=1e-3, wd=c['wd'], betas=(0.9, 0.999), eps=1e-8, grad_scale=GRAD_SCALE,
                 grad_clip=c['grad_clip'], lr_lo=lo, lr_hi=hi, use_log=c['use_log'], frozen_lr=FROZEN_LR, frozen_param=FROZEN_PARAM)
    return state, grad, m, v, hyper


@pytest.mark.parametrize('c', OUTER_CASES, ids=lambda c: f'step{c["step"]}_clip{c["grad_clip"]:g}_wd{c["wd"]:g}_{"log" if c["use_log"] else "plain"}'
                                                          f'_{"init" if c["init"] else "lr_only"}')
def test_outer_step_link(base, outer_eng, c):
    eng, net = outer_eng, base.net
    n_lr = net.nlr
    state, grad, m, v, h = _outer_inputs(eng, net, c)
    old = [t.to('cpu', copy=True) for t in (state, grad, m, v)]
    params_before = eng.get_params().clone()
    eng.outer_step(state, grad, m, v, n_lr, c['init'], h['step'], h['lr_lr'], h['init_lr'], h['wd'], grad_scale=h['grad_scale'],
                   grad_clip=h['grad_clip'], lr_lo=h['lr_lo'], lr_hi=h['lr_hi'], use_log=h['use_log'], frozen_lr=FROZEN_LR,
                   frozen_param=FROZEN_PARAM, betas=h['betas'], eps=h['eps'])
    eng.synchronize()
    assert int(torch.count_nonzero(grad)) == 0, 'the gradient buffer is not zeroed'
    # the Winit / Wp scatter: 1x1, 3x3, 7x7 tensors and the bias, now (Wp) and after a reset (Winit)
    if c['init']:
        assert torch.equal(eng.get_params(), state[n_lr:])
        eng.reset()
        assert torch.equal(eng.get_params(), state[n_lr:]) and not torch.equal(params_before, state[n_lr:])
    else:
        assert torch.equal(eng.get_params(), params_before)
        eng.reset()
        assert torch.equal(eng.get_params(), params_before)
    new = [t.cpu() for t in (state, m, v)]
    ref = M.outer_step_link(*(t.double() for t in old), h, net)
    r32 = M.outer_step_link(*old, h, net)
    floors = M.outer_floors(*(t.double() for t in old), ref[0], h)
    tag = f'outer step {c["step"]}, clip {c["grad_clip"]:g}, wd {c["wd"]:g}, {"log" if c["use_log"] else "plain"}, {"lr + init" if c["init"] else "lr only"}'
    bad = [_margin(f'{tag}: {name}', new[i], ref[i], r32[i], floors[i]) for i, name in enumerate(('state', 'm', 'v'))]
    assert bad == [0, 0, 0], (tag, bad)
    # frozen prefixes: the value stays, the moments move
    cuts = [(0, FROZEN_LR)] + ([(n_lr, n_lr + FROZEN_PARAM)] if c['init'] else [])
    for a, b in cuts:
        assert torch.equal(new[0][a:b], old[0][a:b]), 'a frozen value moved'
        assert int((new[1][a:b] != old[2][a:b]).sum()) > (b - a) // 2 and int((new[2][a:b] != old[3][a:b]).sum()) > (b - a) // 2
    assert int((new[0][FROZEN_LR:n_lr] != old[0][FROZEN_LR:n_lr]).sum()) > (n_lr - FROZEN_LR) // 2
    a = FROZEN_LR + 20
    assert new[0][a] == h['lr_lo'] and new[0][a + 1] == h['lr_hi']
    assert float(new[0][:n_lr].min()) == h['lr_lo'] and float(new[0][:n_lr].max()) == h['lr_hi']
    assert int((ref[0][:n_lr] == h['lr_lo']).sum()) > 100 and int((ref[0][:n_lr] == h['lr_hi']).sum()) > 100      # the clamp cut many
    if c['grad_clip'] > 0:
        g1 = old[1] * GRAD_SCALE
        assert int((g1.abs() == M.f32(CLIP)).sum()) >= 2 and int((g1.abs() > M.f32(CLIP)).sum()) > 0
    if c['finetune']:
        # the lr the engine now uses: exp(state) or state, through one update (lr_eff from the same expf: torch's on the device)
        lr_eff = (state[:n_lr].exp() if c['use_log'] else state[:n_lr]).cpu()
        before = eng.get_params().cpu()
        loss = eng.finetune_step(base.x, base.y)
        grads, after = eng.get_grads().cpu(), eng.get_params().cpu()
        assert np.isfinite(loss)
        want, bound = R.update_reference(net, before, lr_eff, grads)
        err = (after.double() - want).abs()
        print(f'MARGIN {tag}: update with the new lr, worst {float((err / bound.clamp_min(1e-300)).max()):.3f} of the bound, '
              f'{int((after != before).sum())} moved')
        assert bool((err <= bound).all()) and not torch.equal(after, before)
        eng.reset()
