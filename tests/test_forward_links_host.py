"""The forward link table of tests/forward_links_ref.py against the oracle network, on the CPU in float64.

The oracle (oracle/deeplab.py, synthetic weights) runs at 33 x 49, batch 2, for resnet50 with frozen BatchNorm and with
GroupNorm, resnet101 and plain DeepLabV3 on resnet50; `test_backward_links_host.capture` records every buffer under the engine's
names.  Each link, fed those tensors, must reproduce the captured buffer (or its channel slice) to 1e-12 of its largest entry,
and all links composed from the frame alone must reproduce `deeplab.forward`'s logits.  That proves the formulas and the operand
table of the GPU audit (tests/test_gpu_forward_links.py) before any kernel is involved.

SENSITIVITY: the GPU audit's bound max(K * err_torch32, floor) must be able to see a wrong kernel.  On the oracle's buffers
rounded to float32, one link of each class (1x1, 3x3 direct, 3x3 Winograd-eligible, dilated, strided, stem) is mutated -- one
tap dropped on one border row of a 3x3 conv, the residual left out of one output channel, one channel's shift replaced by its
neighbour's -- and each mutation must land above that link's bound.

CAP: K * err_torch32 <= 25 * floor for every link (the ratio of GN_CAP to the GroupNorm floors), so an ill-conditioned link
cannot widen its own bound until a wrong kernel passes.  A condition, not a measurement: asserted here on the oracle's buffers
for every (size, batch, seed) the GPU file uses, and there again on the engine's operands.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import backward_links_ref as R
import forward_links_ref as FR
import test_gpu_forward_links as G
from test_backward_links_host import H, W, B, TOL, _err, capture
from test_gpu_misc_ops import K

GRAPHS = {'resnet50-bn': ('resnet50', 'bn'), 'resnet50-gn': ('resnet50', 'gn'), 'resnet101-bn': ('resnet101', 'bn'),
          'deeplabv3_resnet50': ('deeplabv3_resnet50', 'bn')}
CX = {'BN50': G.BN50, 'GN50': G.GN50, 'BN101': G.BN101, 'V3': G.V3}


@functools.lru_cache(maxsize=None)
def _captured(graph, h=H, w=W, batch=B, seed=7, engine_state=False):
    """(net, T with every forward buffer, weights, scales, shifts, (gamma, beta))."""
    fwd = {}
    net, T, Wt, A, _, GB = capture(h, w, batch, *GRAPHS[graph], seed=seed, engine_state=engine_state, fwd=fwd)
    T = {k: v for k, v in T.items() if not k.split('.')[-1].startswith('g') and k != 'dlogits' and not k.startswith('dz')}
    T.update(fwd['T'])
    assert sorted(T) == sorted(FR.forward_buffer_names(net) + ['x'] + (R.z_names(net) if net.gn else []))
    return net, T, Wt, A, fwd['S'], GB


@pytest.mark.parametrize('stage', R.STAGES)
@pytest.mark.parametrize('graph', GRAPHS)
def test_forward_links_reproduce_the_oracle(graph, stage):
    net, T, Wt, A, S, GB = _captured(graph)
    links = [l for l in FR.forward_links(net) if l.stage == stage]
    assert links and all(l.ci < 0 or net.stage_of(l.ci) == stage for l in links)
    for l in links:
        got = l.fn(T, Wt, A, S)
        assert got.shape[1] == l.c1 - l.c0
        assert _err(got, FR.target(l, T)) <= TOL, (l.out, l.c0)
        assert all(s in T for s in l.src)


@pytest.mark.parametrize('graph', GRAPHS)
def test_composition_of_all_links_reproduces_the_logits(graph):
    from eosvos_amd import synthetic
    from oracle import deeplab
    net, T, Wt, A, S, GB = _captured(graph)
    C = FR.compose(net, T['x'], Wt, A, S, GB)
    sd = synthetic.synthetic_state(GRAPHS[graph][0], dtype=torch.float64)
    with torch.no_grad():
        logits = deeplab.forward(sd, T['x'], *GRAPHS[graph])
    assert _err(C['logits'], logits) <= TOL
    assert sorted(C) == sorted(T)
    for n in T:
        assert _err(C[n], T[n]) <= TOL, n


@pytest.mark.parametrize('graph', GRAPHS)
def test_forward_link_table_covers_the_network(graph):
    """Every conv exactly once; every forward buffer (GroupNorm: with the existing GN forward links, which make the activations
    from z); the slices of `cat` / `dcat` disjoint and complete."""
    net = _captured(graph)[0]
    links = FR.forward_links(net)
    assert sorted(l.ci for l in links if l.ci >= 0) == list(range(len(net.convs)))
    assert all(l.stage in R.STAGES and l.kind in ('conv', 'stem', 'maxpool_fwd', 'pool_fwd', 'bcast', 'resize_fwd', 'head_fwd') for l in links)
    outs = {l.out for l in links} | ({g.out for g in R.gn_links(net)} if net.gn else set())
    assert outs == set(FR.forward_buffer_names(net)) | (set(R.z_names(net)) if net.gn else set()), outs ^ set(FR.forward_buffer_names(net))
    width = {'cat': 1280} if net.v3 else {'cat': 1280, 'dcat': 304}
    for name, n in width.items():
        owners = sorted((l.c0, l.c1) for l in links if l.out == name) if not net.gn else sorted(
            [(l.c0, l.c1) for l in links if l.out == name] + [(g.out_c0, g.out_c0 + net.convs[g.ci].cout) for g in R.gn_links(net) if g.out == name])
        assert owners[0][0] == 0 and owners[-1][1] == n and all(a[1] == b[0] for a, b in zip(owners, owners[1:])), (name, owners)
    for l in links:
        if l.out not in width and not l.out.startswith('z'):
            assert l.c0 == 0, l.out
    if net.v3:
        assert net.convs[net.aspp[1]].dil == 12 and net.convs[net.aspp[3]].dil == 36 and net.head3 == net.project + 1
        assert 'dcat' not in outs and 'd2' not in outs


# ---- sensitivity --------------------------------------------------------------------------------------------------------------
def _f32(T):
    return {k: v.float().double() for k, v in T.items()}


def _classes(net, T):
    """class -> the index of one conv link of it (resnet50, frozen BatchNorm)."""
    links = FR.forward_links(net)
    by_name = {net.convs[l.ci].name: i for i, l in enumerate(links) if l.ci >= 0}
    cls = {'1x1': by_name['backbone.layer1.1.conv3'],             # identity-residual block
           '3x3 direct': by_name['classifier.0.convs.2.0'],        # rate 12: outside the Winograd range
           '3x3 Winograd-eligible': by_name['backbone.layer1.0.conv2'],
           'dilated': by_name['backbone.layer4.0.conv2'],          # rate 2 on the 3 x 4 map: the left-column tap is inside from column 2 on
           'strided': by_name['backbone.layer2.0.conv2'],
           'stem': by_name['backbone.conv1']}
    cx = G.BN50
    floors = {k: G.link_floor(cx, links[i], tuple(FR.target(links[i], T).shape[-2:])) for k, i in cls.items()}
    assert floors['3x3 direct'] == G.TOL['direct'] and floors['strided'] == G.TOL['direct']
    assert floors['3x3 Winograd-eligible'] == G.TOL['wino_f2'] and floors['dilated'] == G.TOL['wino_f2']
    return links, cls, floors


def _bound(l, T, Wt, A, S, floor):
    """The GPU test's bound of link l on these (float32-valued) operands, and the float64 result."""
    r64 = l.fn(T, Wt, A, S)
    T32 = R.Cast(T, torch.float32)
    f = lambda v: None if v is None else v.float()
    r32 = l.fn(T32, [(w.float(), f(b)) for w, b in Wt], [f(a) for a in A], [f(s) for s in S])
    return max(K * _err(r32.double(), r64), floor), r64


WIDE = 225                  # a 3 x 15 ASPP map: the rate-12 conv's left-column tap lies inside the map from output column 12 on


@functools.lru_cache(maxsize=None)
def _rounded(w):
    net, T, Wt, A, S, GB = _captured('resnet50-bn', w=w, engine_state=True)
    r = lambda v: None if v is None else v.float().double()
    return net, _f32(T), [(r(w_), r(b)) for w_, b in Wt], [r(a) for a in A], [r(s) for s in S]


@pytest.mark.parametrize('klass', ['1x1', '3x3 direct', '3x3 Winograd-eligible', 'dilated', 'strided', 'stem'])
def test_the_bound_sees_a_wrong_kernel(klass):
    net, T, Wt, A, S = _rounded(WIDE if klass == '3x3 direct' else W)
    links, cls, floors = _classes(net, T)
    l = links[cls[klass]]
    c = net.convs[l.ci]
    bound, ref = _bound(l, T, Wt, A, S, floors[klass])
    x, w, a, b = T[l.src[0]], Wt[l.ci][0], A[l.ci], S[l.ci]
    finish = lambda y: F.relu(y + T[l.res]) if l.res else F.relu(y)
    seen = {}
    # one channel's shift replaced by its neighbour's
    b2 = b.clone()
    i = int(torch.nonzero(b[:-1] != b[1:])[0])           # the first channel whose neighbour has another shift
    b2[i] = b[i + 1]
    seen['one channel\'s shift replaced by its neighbour\'s'] = _err(finish(FR.affine(FR.conv(x, w, c), a, b2)), ref)
    if c.k == 3:        # one tap (centre row, left column: inside the map on the top border row) dropped on output row 0
        w1 = torch.zeros_like(w)
        w1[:, :, 1, 0] = w[:, :, 1, 0]
        y = FR.conv(x, w, c)
        y[:, :, 0] -= FR.conv(x, w1, c)[:, :, 0]
        seen['one tap dropped on the top border row'] = _err(finish(FR.affine(y, a, b)), ref)
    if l.res:           # the residual left out of one output channel
        res = T[l.res].clone()
        res[:, 0] = 0
        seen['residual left out of channel 0'] = _err(F.relu(FR.affine(FR.conv(x, w, c), a, b) + res), ref)
    print(f'SENSITIVITY {klass} ({c.name}), bound {bound:.2e}: ' + ', '.join(f'{k} {v:.2e}' for k, v in seen.items()))
    assert bound <= G.CAP_RATIO * floors[klass]
    assert all(v > bound for v in seen.values()), (klass, bound, seen)
    assert ('residual left out of channel 0' in seen) == (klass == '1x1')
    assert ('one tap dropped on the top border row' in seen) == (c.k == 3)


# ---- cap ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('frame', G.FRAMES, ids=lambda f: f'{f[0]}-{f[1]}x{f[2]}-b{f[3]}-s{f[4]}' + ('' if len(f[5]) > 1 else '-' + f[5][0]))
def test_cap_on_the_frames_of_the_gpu_tests(frame):
    """K * err_torch32 <= CAP_RATIO * floor on every link the GPU file audits on this frame, on the oracle's own buffers (float32
    values of a float64 pass from the state the engine loads)."""
    name, h, w, batch, seed, stages = frame
    cx = CX[name]
    graph = {'BN50': 'resnet50-bn', 'GN50': 'resnet50-gn', 'BN101': 'resnet101-bn', 'V3': 'deeplabv3_resnet50'}[name]
    fwd = {}
    net, T, Wt, A, _, GB = capture(h, w, batch, *GRAPHS[graph], seed=seed, engine_state=True, fwd=fwd)
    T = dict(T, **fwd['T'])
    r = lambda v: None if v is None else v.float().double()
    T, Wt, A, S = _f32(T), [(r(a), r(b)) for a, b in Wt], [r(a) for a in A], [r(s) for s in fwd['S']]
    rows = []
    for l in cx.links:
        floor = G.link_floor(cx, l, tuple(FR.target(l, T).shape[-2:]))
        if l.stage not in stages or floor is None:
            continue
        bound, _ = _bound(l, T, Wt, A, S, 0.0)
        rows.append((bound / floor, G.link_name(cx, l), bound, floor))
    worst = max(rows)
    print(f'CAP {name} {h}x{w} batch {batch} seed {seed}: worst K * torch32 / floor {worst[0]:.3f} ({worst[1]}: {worst[2]:.2e} vs floor {worst[3]:.1e})')
    bad = [r for r in rows if not r[0] <= G.CAP_RATIO]
    assert not bad, bad


def test_fold_reference_bounds_hold_for_a_float32_fold():
    """The fold's bound admits a plain float32 evaluation of the same three lines, and not a swapped channel."""
    from eosvos_amd import synthetic, topology
    sd = synthetic.synthetic_state('resnet50')
    cat = lambda suf: torch.cat([sd[p + suf].reshape(-1).float() for p, _ in topology.norm_layers('resnet50')])
    g, be, mu, v = cat('.weight'), cat('.bias'), cat('.running_mean'), cat('.running_var')
    a, b, ba, bb = FR.fold_reference(g, be, mu, v)
    a32 = (1.0 / torch.sqrt(v + 1e-5)) * g
    b32 = be - mu * a32
    assert bool(((a32.double() - a).abs() <= ba).all()) and bool(((b32.double() - b).abs() <= bb).all())
    assert not bool(((a32.roll(1).double() - a).abs() <= ba).all())
