"""The link functions of tests/backward_links_ref.py against autograd, on the CPU in float64.

The oracle network (oracle/deeplab.py, synthetic weights; resnet50 and resnet101 with frozen BatchNorm, resnet50 with
GroupNorm) runs at 33 x 49, batch 2, with the BCE loss; every conv's input and every norm layer's input and output is captured
with its gradient.  Each link -- fed with those captured tensors under the engine's buffer names -- must reproduce autograd's
own gradient of the buffer it recomputes (a data link, a GN backward link), of the conv's weight (a weight link) or the
activation itself (a GN forward link) to 1e-12 of the largest entry.  That proves the formulas and the operand table of the
GPU audit (tests/test_gpu_backward_links.py) before any kernel is involved.

The GroupNorm links' bound there is max(4 * err_torch32, floor), err_torch32 torch's own float32 group norm on the same
operands, under the condition 4 * err_torch32 <= GN_CAP = 1e-4 (25 floors; torch fp32 on well-conditioned maps of these sizes
is about 1e-7): an ill-conditioned group must not widen its own bound until a wrong kernel passes.  `test_gn_cap_*` assert
that condition here on the oracle's own float64 buffers, for the engine's float32 state and every frame the GPU tests use.
"""
import pytest
import torch
import torch.nn.functional as F

import backward_links_ref as R
from eosvos_amd import synthetic
from oracle import deeplab

H, W, B = 33, 49, 2
TOL = 1e-12
GN_K, GN_CAP = 4, 1e-4                  # the GroupNorm links' K and the cap on K * err_torch32 (module docstring)
# (height, width, batch, frame seed) of every GroupNorm run of tests/test_gpu_backward_links.py whose GN links are audited
GN_GPU_FRAMES = [(65, 97, 1, 12), (65, 97, 3, 14), (257, 261, 1, 41), (65, 97, 3, 31), (65, 97, 1, 32)]


def capture(h, w, batch, encoder='resnet50', norm='bn', seed=7, engine_state=False, fwd=None):
    """(net, buffers under the engine's names, weights, scales, autograd's weight gradients, (gamma, beta) per conv) of one
    forward + loss + backward.  engine_state: the float32 state the GPU tests load, cast to float64.  fwd: a dict that
    receives what the forward links (tests/forward_links_ref.py) read beyond that: 'S', the folded shift per conv, and 'T',
    the forward buffers no backward link names (`blk<i>.dsb` under a frozen norm, `lowlog`, `logits`).  Plain DeepLabV3
    has no backward links: it needs fwd, and the result holds its forward buffers only and None for the weight gradients."""
    net = R.Net(encoder, norm)
    assert fwd is not None or not net.v3, 'plain DeepLabV3 has forward links only: pass fwd'
    if engine_state:
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in synthetic.synthetic_state(encoder).items()}
    else:
        sd = synthetic.synthetic_state(encoder, dtype=torch.float64)
    trainable = {c.name + s for c in net.convs for s in ('.weight', '.bias')}
    P = {k: (v.double().clone().requires_grad_(True) if k in trainable else v) for k, v in sd.items()}
    x, y = synthetic.synthetic_frames(batch, h, w, seed=seed)
    x, y = x.double(), y.double()
    X, Z, N = [], [], []                # per conv, in call order (= topology.conv_infos order): its input, its norm's input / output
    conv0, norm0 = deeplab._conv, deeplab._norm

    def conv_hook(P_, t, c):
        if t.requires_grad:
            t.retain_grad()
        X.append(t)
        return conv0(P_, t, c)

    def norm_hook(P_, t, prefix, mode):
        t.retain_grad()
        Z.append(t)
        r = norm0(P_, t, prefix, mode)
        r.retain_grad()
        N.append(r)
        return r

    taps = {}
    deeplab._conv, deeplab._norm = conv_hook, norm_hook
    try:
        logits = deeplab.forward(P, x, encoder, norm, taps=taps)
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
            if net.gn:
                T[f'blk{i}.dsb'] = N[b['ds']]
            elif fwd is not None:
                fwd.setdefault('T', {})[f'blk{i}.dsb'] = N[b['ds']].detach()
    cat = X[net.project]
    if fwd is not None:
        fwd.setdefault('T', {}).update(lowlog=taps['low_logits'].detach(), logits=logits.detach())
        fwd['S'] = [None] * len(net.convs) if net.gn else [
            (P[c.norm + '.bias'] - P[c.norm + '.running_mean'] * P[c.norm + '.weight'].detach() / torch.sqrt(P[c.norm + '.running_var'] + deeplab.EPS)).detach()
            if c.norm else None for c in net.convs]
    if net.v3:
        T = {k: v for k, v in T.items() if not k.split('.')[-1].startswith('g')}
        T.update({'cat': cat, 'vec': X[net.pool], 'poolout': F.relu(N[net.pool]), 'proj': F.relu(N[net.project]), 'd1': X[net.last]})
        T = {k: v.detach() for k, v in T.items()}
        Wt = [(P[c.name + '.weight'].detach(), P[c.name + '.bias'].detach() if c.bias else None) for c in net.convs]
        A = [P[c.norm + '.weight'].detach() / torch.sqrt(P[c.norm + '.running_var'] + deeplab.EPS) if c.norm else None for c in net.convs]
        return net, T, Wt, A, None, R.affines(net, sd, torch.float64)
    assert X[net.dec1] is X[net.blocks[net.tap + 1]['c1']]
    T.update({'cat': cat, 'g_cat': R.relumask(cat) * cat.grad, 'vec': X[net.pool], 'gvec': X[net.pool].grad,
              'poolout': F.relu(N[net.pool]), 'gp': N[net.pool].grad, 'proj': F.relu(N[net.project]), 'g_proj': N[net.project].grad,
              'dcat': X[net.dec_a], 'g_dcat': torch.cat((X[net.dec_a].grad[:, :256], N[net.dec1].grad), dim=1),
              'd1': X[net.dec_b], 'd2': X[net.last], 'g_d1': N[net.dec_a].grad, 'g_d2': N[net.dec_b].grad,
              'g_low': taps['low_logits'].grad, 'dlogits': logits.grad})
    if net.gn:
        for ci, c in enumerate(net.convs):
            if c.norm:
                T[f'z{ci}'], T[f'dz{ci}'] = Z[ci], Z[ci].grad
    T = {k: v.detach() for k, v in T.items()}
    assert sorted(T) == sorted(R.buffer_names(net) + ['x'] + (R.z_names(net) + ['d' + n for n in R.z_names(net)] if net.gn else []))
    Wt = [(P[c.name + '.weight'].detach(), P[c.name + '.bias'].detach() if c.bias else None) for c in net.convs]
    if net.gn:
        A = [None] * len(net.convs)     # no folded scale: the links read dz
    else:
        A = [P[c.norm + '.weight'].detach() / torch.sqrt(P[c.norm + '.running_var'] + deeplab.EPS) if c.norm else None for c in net.convs]
    Gw = [(P[c.name + '.weight'].grad, P[c.name + '.bias'].grad if c.bias else None) for c in net.convs]
    return net, T, Wt, A, Gw, R.affines(net, sd, torch.float64)


@pytest.fixture(scope='module')
def captured():
    return capture(H, W, B)


@pytest.fixture(scope='module')
def captured_101():
    return capture(H, W, B, 'resnet101', 'bn')


@pytest.fixture(scope='module')
def captured_gn():
    return capture(H, W, B, 'resnet50', 'gn')


def _err(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = float(ref.abs().max())
    assert scale > 0
    return float((got - ref).abs().max()) / scale


def _weight_links_reproduce_autograd(captured, stage):
    net, T, Wt, A, Gw, _ = captured
    links = [l for l in R.weight_links(net) if l.stage == stage]
    assert links and all(net.stage_of(l.ci) == stage for l in links)
    for l in links:
        dw, db = R.weight_link(net, l, T, A)
        assert _err(dw, Gw[l.ci][0]) <= TOL, net.convs[l.ci].name
        if net.convs[l.ci].bias:
            assert _err(db, Gw[l.ci][1]) <= TOL, net.convs[l.ci].name


def _data_links_reproduce_autograd(captured, stage):
    net, T, Wt, A, Gw, _ = captured
    links = [l for l in R.data_links(net) if l.stage == stage]
    assert links
    for l in links:
        got = l.fn(T, Wt, A)
        assert _err(got, T[l.out]) <= TOL, l.out
        if l.mask:
            act, c0 = l.mask
            assert bool((got[:, c0:][T[act][:, c0:] <= 0] == 0).all()), l.out


@pytest.mark.parametrize('stage', R.STAGES)
def test_weight_links_reproduce_autograd(captured, stage):
    _weight_links_reproduce_autograd(captured, stage)


@pytest.mark.parametrize('stage', R.STAGES)
def test_data_links_reproduce_autograd(captured, stage):
    _data_links_reproduce_autograd(captured, stage)


@pytest.mark.parametrize('stage', R.STAGES)
def test_resnet101_links_reproduce_autograd(captured_101, stage):
    """The block discovery, the low-level tap and the link tables on the 33-block graph."""
    _weight_links_reproduce_autograd(captured_101, stage)
    _data_links_reproduce_autograd(captured_101, stage)


@pytest.mark.parametrize('stage', R.STAGES)
def test_groupnorm_weight_and_data_links_reproduce_autograd(captured_gn, stage):
    """The weight and data links on dz (no folded scale) under norm='gn'."""
    _weight_links_reproduce_autograd(captured_gn, stage)
    _data_links_reproduce_autograd(captured_gn, stage)


def test_link_tables_cover_the_network(captured):
    """One weight link per conv, in conv order; every gradient buffer is the output of exactly one data link."""
    _link_tables_cover_the_network(captured[0])


def test_link_tables_cover_resnet101_and_groupnorm(captured_101, captured_gn):
    _link_tables_cover_the_network(captured_101[0])
    _link_tables_cover_the_network(captured_gn[0])
    assert 'blk0.dsb' in R.buffer_names(captured_gn[0]) and 'blk1.dsb' not in R.buffer_names(captured_gn[0])
    assert not any(n.endswith('.dsb') for n in R.buffer_names(captured_101[0]))


def _link_tables_cover_the_network(net):
    wl = R.weight_links(net)
    nconv, nblock, nparam, nlr = {'resnet50': (63, 16, 40289729, 28658), 'resnet101': (114, 33, 59229633, 54770)}[net.encoder]
    assert [l.ci for l in wl] == list(range(nconv)) and len(net.blocks) == nblock and net.nparam == nparam and net.nlr == nlr
    assert [b['stage'] for b in net.blocks].count('layer3') == nblock - 10 and net.tap == 2
    outs = [l.out for l in R.data_links(net)]
    grads = [n for n in R.buffer_names(net) if n.split('.')[-1].startswith('g')]
    assert sorted(outs) == sorted(n for n in grads if n != 'dlogits'), set(outs) ^ set(grads)
    assert [l.ci for l in R.gn_links(net)] == list(range(nconv - 1)) and R.z_names(net) == [f'z{ci}' for ci in range(nconv - 1)]


# ---- GroupNorm links ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stage', R.STAGES)
def test_gn_links_reproduce_autograd(captured_gn, stage):
    """Forward link: the stored activation from z; backward link: autograd's own dL/dz from z and the buffer's g."""
    net, T, Wt, A, Gw, GB = captured_gn
    links = [l for l in R.gn_links(net) if l.stage == stage]
    assert links and all(net.stage_of(l.ci) == stage for l in links)
    for l in links:
        y, stored = R.gn_fwd_link(net, l, T, GB)
        assert _err(y, stored) <= TOL, ('forward', net.convs[l.ci].name)
        dz, stored = R.gn_bwd_link(net, l, T, GB)
        assert _err(dz, stored) <= TOL, ('backward', net.convs[l.ci].name)


def gn_torch32_errors(net, T, GB64):
    """Per GN link (name, err_torch32 forward, err_torch32 backward): torch's float32 links against the float64 ones on the
    same operands, relative to the float64 result's largest entry."""
    T32 = R.Cast(T, torch.float32)
    GB32 = [None if gb is None else (gb[0].float(), gb[1].float()) for gb in GB64]
    rows = []
    for l in R.gn_links(net):
        y64, y32 = R.gn_fwd_link(net, l, T, GB64)[0], R.gn_fwd_link(net, l, T32, GB32)[0]
        d64, d32 = R.gn_bwd_link(net, l, T, GB64)[0], R.gn_bwd_link(net, l, T32, GB32)[0]
        rows.append((net.convs[l.ci].name, _err(y32.double(), y64), _err(d32.double(), d64)))
    return rows


@pytest.mark.parametrize('h,w,batch,seed', GN_GPU_FRAMES)
def test_gn_cap_on_the_frames_of_the_gpu_tests(h, w, batch, seed):
    """K * err_torch32 <= GN_CAP on every GN link of the oracle's own buffers (float32 buffers of a float64 pass from the
    state the engine loads), for each frame and seed the GPU tests audit GN links on."""
    net, T, Wt, A, Gw, GB = capture(h, w, batch, 'resnet50', 'gn', seed=seed, engine_state=True)
    T = {k: v.float().double() for k, v in T.items()}         # what an engine holds: float32 values
    rows = gn_torch32_errors(net, T, GB)
    wf, wb = max(rows, key=lambda r: r[1]), max(rows, key=lambda r: r[2])
    print(f'GN torch32 {h}x{w} batch {batch} seed {seed}: forward worst {wf[0]} {wf[1]:.2e}, backward worst {wb[0]} {wb[2]:.2e} (cap {GN_CAP / GN_K:.1e})')
    bad = [r for r in rows if not (GN_K * r[1] <= GN_CAP and GN_K * r[2] <= GN_CAP)]
    assert not bad, bad


def test_update_reference_layout():
    """The lr broadcast of the update reference: one value per output channel, one for the classifier's bias."""
    net = R.Net('resnet50')
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
