"""The restatement of the meta-gradient path and the outer step (tests/meta_links_ref.py) proved on the CPU before
tests/test_gpu_meta_links.py trusts it:

* against autograd: a tiny two-conv + bias model in float64, K = 3 inner SGD steps with learned lrs and first-order
  (`second_order_gradients=False`: detached) gradients; the lr gradient at every level and storage form and the init
  gradient equal `torch.autograd.grad` of the weighted meta loss to 1e-12;
* against the project's torch RAdam (`oracle.meta.radam_step`, itself pinned to the reference's RAdam by fixture G8; the
  package's `radam.RAdam` is the device kernel and cannot run here): 8 steps across the N_sma >= 5 switch;
* the bounds are not vacuous: the float32 restatement with one planted mistake -- a row one element short, bias rows paired
  with the wrong base, `weight` applied twice, beta1 for beta2, no clamp, I and T exchanged in the init scatter -- exceeds
  the bound the GPU test applies; without the mistake it stays inside.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import meta_links_ref as M
from eosvos_amd import topology
from oracle import meta as ometa
from test_gpu_misc_ops import K

TINY = M.Layout([M.Conv('a', 3, 4, 3, False), M.Conv('b', 4, 2, 1, True)])
LEVELS = [(l, u) for l in ('NEURON', 'TENSOR', 'SINGLE', 'PARAM') for u in (False, True)]


def _split(flat, net=TINY):
    out = []
    for c, po in zip(net.convs, net.poff):
        n = c.cout * c.cin * c.k * c.k
        out.append(flat[po:po + n].view(c.cout, c.cin, c.k, c.k))
        if c.bias:
            out.append(flat[po + n:po + n + c.cout])
    return out


def _loss(flat, x, y):
    wa, wb, bb = _split(flat)
    z = F.conv2d(F.relu(F.conv2d(x, wa, padding=1)), wb, bb)
    return F.binary_cross_entropy_with_logits(z, y)


def _lr_elem(store, level, use_log):
    """Per-element effective lr of a stored state, differentiable."""
    if level == 'PARAM':
        return store.exp() if use_log else store
    lr = store.exp() if use_log else store
    if level == 'TENSOR':
        r0 = TINY.tensor_row0
        lr = torch.cat([lr[t].expand(b - a) for t, (a, b) in enumerate(zip(r0[:-1], r0[1:]))])
    elif level == 'SINGLE':
        lr = lr.expand(TINY.nlr)
    return torch.cat([lr[r].expand(int(n)) for r, n in enumerate(TINY.row_len)])     # rows are contiguous in the flat layout


@pytest.mark.parametrize('level,use_log', LEVELS)
def test_links_equal_autograd(level, use_log):
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, xm = rnd(2, 3, 6, 7), rnd(2, 3, 6, 7)
    y, ym = (rnd(2, 2, 6, 7) > 0).double(), (rnd(2, 2, 6, 7) > 0).double()
    init = (rnd(TINY.nparam) * 0.3).requires_grad_(True)
    val = 0.05 * (1 + torch.rand(TINY.store_count(level), generator=g, dtype=torch.float64))
    store = (val.log() if use_log else val).requires_grad_(True)
    weight = 0.3
    lr = _lr_elem(store, level, use_log)
    theta, grads = init, []
    for _ in range(3):
        d = theta.detach().requires_grad_(True)
        grads.append(torch.autograd.grad(_loss(d, x, y), d)[0])
        theta = theta - lr * grads[-1]
    d = theta.detach().requires_grad_(True)
    G = torch.autograd.grad(_loss(d, xm, ym), d)[0]
    a_lr, a_init = torch.autograd.grad(weight * _loss(theta, xm, ym), (store, init))
    gsum = M.accumulate_link(grads)
    if level == 'PARAM':
        got = M.lr_grad_param(gsum, G, lr.detach() if use_log else None, weight)
    else:
        glr, _ = M.lr_grad_neuron(gsum, G, weight, TINY)
        got = M.lr_grad_store(glr, M.expand_lr(store.detach(), level, use_log, TINY), level, use_log, TINY)
    assert float(a_lr.abs().max()) > 0
    assert float((got - a_lr).abs().max()) <= 1e-12 * float(a_lr.abs().max())
    prior = rnd(TINY.nparam)
    ref = prior + a_init
    assert float((M.init_grad_link(prior, G, weight) - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


HYP = dict(lr=M.f32(1e-3), wd=M.f32(1e-3), betas=(M.f32(0.9), M.f32(0.999)), eps=M.f32(1e-8), grad_scale=0.25, grad_clip=M.f32(0.1))


def test_radam_link_equals_the_oracle_radam():
    g = torch.Generator().manual_seed(8)
    p = torch.randn(300, generator=g, dtype=torch.float64)
    po, st = p.clone(), {}
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    branches = set()
    for step in range(1, 9):
        gr = torch.randn(300, generator=g, dtype=torch.float64)
        p, m, v = M.radam_link(p, gr, m, v, step, HYP['lr'], HYP['wd'], HYP['betas'], HYP['eps'], HYP['grad_scale'], HYP['grad_clip'])
        gc = (gr * HYP['grad_scale']).clamp(-HYP['grad_clip'], HYP['grad_clip'])
        assert bool((gc.abs() == HYP['grad_clip']).any()) and bool((gc.abs() < HYP['grad_clip']).any())
        ometa.radam_step(po, gc, st, HYP['lr'], HYP['wd'], HYP['betas'], HYP['eps'])
        branches.add((step, M.radam_scalars(step, HYP['betas'])[0] >= 5))
        for a, b in ((p, po), (m, st['exp_avg']), (v, st['exp_avg_sq'])):
            assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), step
    assert (5, False) in branches and (6, True) in branches


def _outer_case(use_log, n_extra=0):
    net = TINY
    g = torch.Generator().manual_seed(13)
    n = net.nlr + net.nparam
    state = torch.randn(n, generator=g) * 0.1
    state[:net.nlr] = (torch.rand(net.nlr, generator=g) * 1e-3 + 5e-4)
    if use_log:
        state[:net.nlr] = state[:net.nlr].log()
    grad, m, v = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
    lo, hi = (float(state[:net.nlr].min()) + 1e-4 * (7 if use_log else 1), float(state[:net.nlr].max()) - 1e-4 * (7 if use_log else 1))
    hyper = dict(step=6, lr_lr=1e-3, init_lr=1e-3, wd=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_scale=0.5, grad_clip=0.25,
                 lr_lo=lo, lr_hi=hi, use_log=use_log, frozen_lr=2, frozen_param=50)
    return net, state, grad, m, v, hyper


@pytest.mark.parametrize('use_log', [False, True])
def test_outer_step_link_is_radam_per_group_plus_clamp(use_log):
    net, state, grad, m, v, h = _outer_case(use_log)
    s64, g64, m64, v64 = (t.double() for t in (state, grad, m, v))
    new, nm, nv, lr_eff, init = M.outer_step_link(s64, g64, m64, v64, h, net)
    n, kw = net.nlr, dict(betas=h['betas'], eps=h['eps'], grad_scale=h['grad_scale'], grad_clip=h['grad_clip'])
    a, fa = M.radam_link(s64[:n], g64[:n], m64[:n], v64[:n], 6, h['lr_lr'], 0.0, **kw), h['frozen_lr']
    b, fb = M.radam_link(s64[n:], g64[n:], m64[n:], v64[n:], 6, h['init_lr'], h['wd'], **kw), h['frozen_param']
    want = a[0].clamp(M.f32(h['lr_lo']), M.f32(h['lr_hi']))
    assert bool((want != a[0]).any()), 'the clamp cuts nothing'
    assert torch.equal(new[fa:n], want[fa:]) and torch.equal(new[:fa], s64[:fa])
    assert torch.equal(new[n + fb:], b[0][fb:]) and torch.equal(new[n:n + fb], s64[n:n + fb]) and torch.equal(init, new[n:])
    assert torch.equal(nm, torch.cat([a[1], b[1]])) and torch.equal(nv, torch.cat([a[2], b[2]]))
    assert not torch.equal(nm[:fa], m64[:fa]) and not torch.equal(nv[n:n + fb], v64[n:n + fb])      # frozen: m and v still move
    assert torch.equal(lr_eff, new[:n].exp() if use_log else new[:n])
    only_lr = M.outer_step_link(s64[:n], g64[:n], m64[:n], v64[:n], h, net)
    assert only_lr[4] is None and torch.equal(only_lr[0], new[:n])


# ---- the bounds see the planted mistakes ------------------------------------------------------------------------------------
def _lr_case(level, use_log, weight, **mistake):
    """(|x - ref64|, bound) per stored value, x the float32 restatement (with a planted mistake), on random operands."""
    net = TINY
    g = torch.Generator().manual_seed(21)
    gsum, G = torch.randn(net.nparam, generator=g), torch.randn(net.nparam, generator=g)
    val = 1e-3 * (1 + torch.rand(net.store_count(level), generator=g))
    store = val.log() if use_log else val
    prior = torch.randn(net.store_count(level), generator=g) * (8 if level == 'PARAM' else 1)

    def link(dt, **kw):
        gs, Gd, st, pr = gsum.to(dt), G.to(dt), store.to(dt), prior.to(dt)
        if level == 'PARAM':
            w = weight * weight if kw.get('weight_twice') else weight
            term = M.lr_grad_param(gs, Gd, st.exp() if use_log else None, w)
            return pr + term, term, None
        glr, sabs = M.lr_grad_neuron(gs, Gd, weight, net, **kw)
        lr_eff = M.expand_lr(st, level, use_log, net)
        return pr + M.lr_grad_store(glr, lr_eff, level, use_log, net), sabs, lr_eff

    r64, s64, lr64 = link(torch.float64)
    r32 = link(torch.float32)[0]
    x = link(torch.float32, **mistake)[0]
    if level == 'PARAM':
        floor = M.elem_floor(prior.double(), s64)
    else:
        floor = M.store_floor(net, level, use_log, s64, lr64, prior.double(), r64)
    return (x.double() - r64).abs(), torch.maximum(K * (r32.double() - r64).abs(), floor)


@pytest.mark.parametrize('level,use_log', LEVELS)
def test_lr_gradient_bounds_are_not_vacuous(level, use_log):
    err, bound = _lr_case(level, use_log, 0.3)
    assert bool((err <= bound).all())
    mistakes = [dict(weight_twice=True)]
    if level != 'PARAM':            # (PARAM has no rows: the element-wise product cannot lose or mispair one)
        mistakes += [dict(drop_last_of=1), dict(drop_last_of=TINY.nlr - 1), dict(bias_shift=1)]
    for mk in mistakes:
        err, bound = _lr_case(level, use_log, 0.3, **mk)
        assert bool((err > bound).any()), (mk, float((err / bound).max()))


@pytest.mark.parametrize('use_log', [False, True])
def test_outer_step_bounds_are_not_vacuous(use_log):
    net, state, grad, m, v, h = _outer_case(use_log)
    ref = M.outer_step_link(*(t.double() for t in (state, grad, m, v)), h, net)
    r32 = M.outer_step_link(state, grad, m, v, h, net)
    floors = M.outer_floors(*(t.double() for t in (state, grad, m, v)), ref[0], h)

    def exceeds(x):
        return [bool(((x[i].double() - ref[i]).abs() > torch.maximum(K * (r32[i].double() - ref[i]).abs(), floors[i])).any()) for i in range(3)]

    assert exceeds(r32) == [False, False, False]
    assert exceeds(M.outer_step_link(state, grad, m, v, h, net, beta1_for_beta2=True))[2]
    assert exceeds(M.outer_step_link(state, grad, m, v, h, net, skip_clamp=True))[0]
    init = r32[4]
    assert torch.equal(M.flat_layout(M.engine_layout(init, net), net), init)
    assert not torch.equal(M.flat_layout(M.engine_layout(init, net, swap_it=True), net), init)     # that link's bound is equality


def test_layouts_of_the_supported_topologies():
    for enc in ('resnet50', 'resnet101', 'deeplabv3_resnet50'):
        net = M.Layout.of(enc)
        sizes = [int(np.prod(s)) for _, s in topology.trainable(enc)]
        assert net.nparam == sum(sizes) and net.ntensors == len(sizes)
        assert net.tensor_poff[:-1] == list(np.cumsum([0] + sizes[:-1]))
        assert int(net.row_len.sum()) == net.nparam and net.row_base.numel() == net.nlr
