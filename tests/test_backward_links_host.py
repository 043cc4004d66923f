"""The link functions of tests/backward_links_ref.py against autograd, on the CPU in float64.

The oracle network (oracle/deeplab.py, frozen BatchNorm, synthetic weights) runs at 33 x 49, batch 2, with the BCE loss; every
conv's input and every norm layer's output is captured with its gradient.  Each link -- fed with those captured tensors under
the engine's buffer names -- must reproduce autograd's own gradient of the buffer it recomputes (a data link) or of the conv's
weight (a weight link) to 1e-12 of the largest entry.  That proves the formulas and the operand table of the GPU audit
(tests/test_gpu_backward_links.py) before any kernel is involved.
"""
import pytest
import torch
import torch.nn.functional as F

import backward_links_ref as R
from eosvos_amd import synthetic
from oracle import deeplab

H, W, B = 33, 49, 2
TOL = 1e-12


def capture(h, w, batch):
    """(net, buffers under the engine's names, weights, scales, autograd's weight gradients) of one forward + loss + backward."""
    net = R.Net('resnet50')
    sd = synthetic.synthetic_state('resnet50', dtype=torch.float64)
    trainable = {c.name + s for c in net.convs for s in ('.weight', '.bias')}
    P = {k: (v.double().clone().requires_grad_(True) if k in trainable else v) for k, v in sd.items()}
    x, y = synthetic.synthetic_frames(batch, h, w, seed=7)
    x, y = x.double(), y.double()
    X, N = [], []                       # per conv, in call order (= topology.conv_infos order): its input, its norm's output
    conv0, norm0 = deeplab._conv, deeplab._norm

    def conv(P_, t, c):
        if t.requires_grad:
            t.retain_grad()
        X.append(t)
        return conv0(P_, t, c)

    def norm(P_, t, prefix, mode):
        r = norm0(P_, t, prefix, mode)
        r.retain_grad()
        N.append(r)
        return r

    taps = {}
    deeplab._conv, deeplab._norm = conv, norm
    try:
        logits = deeplab.forward(P, x, 'resnet50', 'bn', taps=taps)
    finally:
        deeplab._conv, deeplab._norm = conv0, norm0
    assert len(X) == len(net.convs) and len(N) == len(net.convs) - 1
    assert [t.shape[1] for t in X] == [c.cin for c in net.convs]
    N.append(None)                      # the classifier has no norm
    logits.retain_grad()
    taps['low_logits'].retain_grad()
    deeplab.bce_loss(logits, y).backward()

    nb = len(net.blocks)
    T = {'x': x, 'c1': F.relu(N[0]), 'p1': X[1], 'g_c1': N[0].grad, 'g_p1': X[1].grad}
    for i, b in enumerate(net.blocks):
        nxt = net.blocks[i + 1]['c1'] if i + 1 < nb else net.aspp[0]
        T[f'blk{i}.t1'], T[f'blk{i}.t2'], T[f'blk{i}.out'] = X[b['c2']], X[b['c3']], X[nxt]
        T[f'blk{i}.g_t1'], T[f'blk{i}.g_t2'], T[f'blk{i}.g_out'] = N[b['c1']].grad, N[b['c2']].grad, N[b['c3']].grad
        if b['ds'] >= 0:
            assert torch.equal(N[b['ds']].grad, N[b['c3']].grad)
    assert X[net.dec1] is X[net.blocks[net.tap + 1]['c1']]
    cat = X[net.project]
    T.update({'cat': cat, 'g_cat': R.relumask(cat) * cat.grad, 'vec': X[net.pool], 'gvec': X[net.pool].grad,
              'poolout': F.relu(N[net.pool]), 'gp': N[net.pool].grad, 'proj': F.relu(N[net.project]), 'g_proj': N[net.project].grad,
              'dcat': X[net.dec_a], 'g_dcat': torch.cat((X[net.dec_a].grad[:, :256], N[net.dec1].grad), dim=1),
              'd1': X[net.dec_b], 'd2': X[net.last], 'g_d1': N[net.dec_a].grad, 'g_d2': N[net.dec_b].grad,
              'g_low': taps['low_logits'].grad, 'dlogits': logits.grad})
    T = {k: v.detach() for k, v in T.items()}
    assert sorted(T) == sorted(R.buffer_names(net) + ['x'])
    Wt = [(P[c.name + '.weight'].detach(), P[c.name + '.bias'].detach() if c.bias else None) for c in net.convs]
    A = [P[c.norm + '.weight'].detach() / torch.sqrt(P[c.norm + '.running_var'] + deeplab.EPS) if c.norm else None for c in net.convs]
    Gw = [(P[c.name + '.weight'].grad, P[c.name + '.bias'].grad if c.bias else None) for c in net.convs]
    return net, T, Wt, A, Gw


@pytest.fixture(scope='module')
def captured():
    return capture(H, W, B)


def _err(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = float(ref.abs().max())
    assert scale > 0
    return float((got - ref).abs().max()) / scale


@pytest.mark.parametrize('stage', R.STAGES)
def test_weight_links_reproduce_autograd(captured, stage):
    net, T, Wt, A, Gw = captured
    links = [l for l in R.weight_links(net) if l.stage == stage]
    assert links and all(net.stage_of(l.ci) == stage for l in links)
    for l in links:
        dw, db = R.weight_link(net, l, T, A)
        assert _err(dw, Gw[l.ci][0]) <= TOL, net.convs[l.ci].name
        if net.convs[l.ci].bias:
            assert _err(db, Gw[l.ci][1]) <= TOL, net.convs[l.ci].name


@pytest.mark.parametrize('stage', R.STAGES)
def test_data_links_reproduce_autograd(captured, stage):
    net, T, Wt, A, Gw = captured
    links = [l for l in R.data_links(net) if l.stage == stage]
    assert links
    for l in links:
        got = l.fn(T, Wt, A)
        assert _err(got, T[l.out]) <= TOL, l.out
        if l.mask:
            act, c0 = l.mask
            assert bool((got[:, c0:][T[act][:, c0:] <= 0] == 0).all()), l.out


def test_link_tables_cover_the_network(captured):
    """One weight link per conv, in conv order; every gradient buffer is the output of exactly one data link."""
    net = captured[0]
    wl = R.weight_links(net)
    assert [l.ci for l in wl] == list(range(63)) and net.nparam == 40289729 and net.nlr == 28658
    outs = [l.out for l in R.data_links(net)]
    grads = [n for n in R.buffer_names(net) if n.split('.')[-1].startswith('g')]
    assert sorted(outs) == sorted(n for n in grads if n != 'dlogits'), set(outs) ^ set(grads)


def test_update_reference_layout(captured):
    """The lr broadcast of the update reference: one value per output channel, one for the classifier's bias."""
    net = captured[0]
    w = torch.zeros(net.nparam)
    g = torch.ones(net.nparam)
    lr = torch.arange(1, net.nlr + 1, dtype=torch.float64)
    ref, bound = R.update_reference(net, w, lr, g)
    c = net.convs[1]
    per = c.cin * c.k * c.k
    assert torch.equal(-ref[net.poff[1]:net.poff[1] + c.cout * per].view(c.cout, per)[:, 0], lr[net.lroff[1]:net.lroff[1] + c.cout])
    assert float(-ref[-1]) == net.nlr and float(-ref[-2]) == net.nlr - 1 and float(-ref[-257]) == net.nlr - 1
    assert float(-ref[-258]) == net.nlr - 2
    assert R.tensor_of(net, net.nparam - 1) == ('decoder.last_conv.8.bias', 0)
    assert R.tensor_of(net, net.poff[5] + 3) == (net.convs[5].name + '.weight', 3)
    assert float(bound[-1]) == 2.0 ** -23 * net.nlr
