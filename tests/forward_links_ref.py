"""The links of the engine's forward pass (`forward_impl`, e-osvos_amd/csrc/engine.cpp), one plain torch function each.

A forward LINK recomputes one forward buffer -- or the channel slice of `cat` / `dcat` that one launch owns -- from the
buffers upstream of it (the engine's own operands, `eosvos_debug_tensor`), the weights in `eosvos_get_params` layout and
the folded frozen-norm scale / shift (`norm_a` / `norm_b`), so an error of one kernel, a missing stream join, a stale
Winograd-domain weight or a write across a slice boundary shows in its own link and in no other.

* frozen BatchNorm: a conv link is relu?(a * conv(x) + b (+ residual)), the residual `blk<i>.dsb` or the block's input;
* GroupNorm (`Net(encoder, 'gn')`): the same graph, but a normalised conv's link targets its RAW output `z<ci>` (no scale,
  no shift, no ReLU, no residual); the activation from z is `backward_links_ref.gn_fwd_link`;
* plain DeepLabV3 (`Net('deeplabv3_resnet50')`): strides and dilations from `topology.conv_infos`, ASPP on the stride-8
  map, `d1` from `proj` (the head's 3x3), `lowlog` from `d1` on that map, `logits` from `lowlog`.

Every link names its stage (one of `backward_links_ref.STAGES`), its kind ('conv', or the misc kind 'stem', 'maxpool_fwd',
'pool_fwd', 'bcast', 'resize_fwd', 'head_fwd'), its conv (or -1), the buffer it recomputes and the channel slice it owns.

Dtype-generic, CPU only, no engine call.  tests/test_forward_links_host.py proves the table against the oracle network;
tests/test_gpu_forward_links.py feeds it the engine's buffers.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

import backward_links_ref as R

# fn(T, W, A, S) -> the link's slice T[out][:, c0:c1]; T: name -> NCHW tensor, W: per conv (weight, bias), A / S: per conv
# folded scale / shift (None in GroupNorm mode and for the classifier).  src: the buffers it reads; res: the residual's name
FwdLink = namedtuple('FwdLink', 'stage kind ci out c0 c1 fn src res relu')


def conv(x, w, c):
    return F.conv2d(x, w, None, stride=c.stride, padding=c.pad, dilation=c.dil)


def affine(y, a, b):
    return y * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def conv_link_fn(net, ci, x, res, relu):
    """relu?(a * conv(T[x]) + b (+ T[res])) of a frozen norm; the raw conv in GroupNorm mode."""
    c = net.convs[ci]

    def fn(T, W, A, S):
        y = conv(T[x], W[ci][0], c)
        if net.gn:
            return y
        y = affine(y, A[ci], S[ci])
        if res:
            y = y + T[res]
        return F.relu(y) if relu else y
    return fn


def forward_links(net):
    """Every forward link in the order `forward_impl` launches them (main stream)."""
    cv = net.convs
    L = []

    def add_conv(stage, ci, x, out, c0=0, res=None, relu=True, kind='conv'):
        if net.gn:      # the conv's launch writes z; the activation (residual and ReLU included) is the GN forward link's
            L.append(FwdLink(stage, kind, ci, f'z{ci}', 0, cv[ci].cout, conv_link_fn(net, ci, x, None, False), (x,), None, False))
        else:
            L.append(FwdLink(stage, kind, ci, out, c0, c0 + cv[ci].cout, conv_link_fn(net, ci, x, res, relu), (x,) + ((res,) if res else ()), res, relu))

    add_conv('stem', 0, 'x', 'c1', kind='stem')
    L.append(FwdLink('stem', 'maxpool_fwd', -1, 'p1', 0, 64, lambda T, W, A, S: F.max_pool2d(T['c1'], 3, 2, 1), ('c1',), None, False))
    for i, b in enumerate(net.blocks):
        st, xin = b['stage'], net.xin(i)
        if b['ds'] >= 0:
            add_conv(st, b['ds'], xin, f'blk{i}.dsb', relu=False)
        add_conv(st, b['c1'], xin, f'blk{i}.t1')
        add_conv(st, b['c2'], f'blk{i}.t1', f'blk{i}.t2')
        add_conv(st, b['c3'], f'blk{i}.t2', f'blk{i}.out', res=f'blk{i}.dsb' if b['ds'] >= 0 else xin)
    l4 = f'blk{len(net.blocks) - 1}.out'
    for j, ci in enumerate(net.aspp):
        add_conv('aspp', ci, l4, 'cat', 256 * j)
    L.append(FwdLink('aspp', 'pool_fwd', -1, 'vec', 0, 2048, lambda T, W, A, S: T[l4].mean(dim=(2, 3), keepdim=True), (l4,), None, False))
    add_conv('aspp', net.pool, 'vec', 'poolout', kind='pool_fwd')

    def bcast(T, W, A, S):
        return T['poolout'].expand(-1, -1, *T['cat'].shape[-2:])
    L.append(FwdLink('aspp', 'bcast', -1, 'cat', 1024, 1280, bcast, ('poolout',), None, False))
    add_conv('aspp', net.project, 'cat', 'proj')
    if net.v3:
        add_conv('decoder', net.head3, 'proj', 'd1')
        feat = 'd1'
    else:
        add_conv('decoder', net.dec1, f'blk{net.tap}.out', 'dcat', 256)

        def up(T, W, A, S):
            return F.interpolate(T['proj'], size=T[f'blk{net.tap}.out'].shape[-2:], mode='bilinear', align_corners=True)
        L.append(FwdLink('decoder', 'resize_fwd', -1, 'dcat', 0, 256, up, ('proj', f'blk{net.tap}.out'), None, False))
        add_conv('decoder', net.dec_a, 'dcat', 'd1')
        add_conv('decoder', net.dec_b, 'd1', 'd2')
        feat = 'd2'

    def head(T, W, A, S):
        return conv(T[feat], W[net.last][0], cv[net.last]) + W[net.last][1].view(1, -1, 1, 1)
    L.append(FwdLink('decoder', 'head_fwd', net.last, 'lowlog', 0, 1, head, (feat,), None, False))

    def final(T, W, A, S):
        return F.interpolate(T['lowlog'], size=T['x'].shape[-2:], mode='bilinear', align_corners=False)
    L.append(FwdLink('decoder', 'resize_fwd', -1, 'logits', 0, 1, final, ('lowlog', 'x'), None, False))
    return L


def forward_buffer_names(net):
    """Every named buffer a forward pass writes, the raw outputs `z<ci>` of a GroupNorm engine aside: the forward buffers of
    `backward_links_ref.buffer_names` (DeepLabV3: without the decoder's), every `blk<i>.dsb` (named in both norm modes),
    `lowlog` and `logits`."""
    names = [n for n in R.buffer_names(net) if not n.split('.')[-1].startswith('g') and n != 'dlogits']
    if net.v3:
        names = [n for n in names if n not in ('dcat', 'd2')]
    names += [f'blk{i}.dsb' for i, b in enumerate(net.blocks) if b['ds'] >= 0 and f'blk{i}.dsb' not in names]
    return names + ['lowlog', 'logits']


def target(l, T):
    """The stored slice a link is compared with."""
    return T[l.out][:, l.c0:l.c1]


def compose(net, x, W, A, S, GB=None):
    """The whole forward pass from the frame alone, link by link: name -> buffer.  GB: per conv (gamma, beta), GroupNorm mode
    (the activation from z: `backward_links_ref.gn_fwd`, the operation of its GN forward link)."""
    T = {'x': x}
    width = {'cat': 1280, 'dcat': 304}

    def store(name, c0, y):
        if name in width:
            if name not in T:
                T[name] = torch.zeros(y.shape[0], width[name], *y.shape[-2:], dtype=y.dtype)
            T[name][:, c0:c0 + y.shape[1]] = y
        else:
            T[name] = y

    gnl = {g.ci: g for g in R.gn_links(net)} if net.gn else {}
    for l in forward_links(net):
        store(l.out, l.c0, l.fn(T, W, A, S))
        g = gnl.get(l.ci) if l.out.startswith('z') else None
        if g is not None:
            store(g.out, g.out_c0, R.gn_fwd(T[l.out], GB[g.ci][0], GB[g.ci][1], T[g.res] if g.res else None, g.relu))
    return T


# ---- frozen-norm fold ---------------------------------------------------------------------------------------------------------
def fold_reference(gamma, beta, mean, var, eps=1e-5):
    """fp64 folded scale / shift of a frozen norm and the per-element bounds of the fp32 fold (`fold_norm_kernel`):

        inv = 1 / sqrt(var + eps);  a = inv * gamma;  b = beta - mean * a

    a: four fp32 roundings in a row (the sum var + eps, the square root, the reciprocal, the product with gamma), each within
    2^-24 relative, so |a32 - a| <= 4 * 2^-24 |a| to first order.
    b: the product mean * a32 carries a's error, |mean| * bound(a), plus its own rounding 2^-24 |mean a|; the difference is
    rounded once more, 2^-24 |beta - mean a| <= 2^-24 (|beta| + |mean a|).  2^-23 (|beta| + |mean a|) + |mean| * bound(a)
    covers both roundings with a factor to spare (a fused multiply-add rounds once: covered as well)."""
    g, be, mu, v = gamma.double(), beta.double(), mean.double(), var.double()
    a = g / torch.sqrt(v + eps)
    b = be - mu * a
    bound_a = 4 * 2.0 ** -24 * a.abs()
    bound_b = 2.0 ** -23 * (be.abs() + (mu * a).abs()) + mu.abs() * bound_a
    return a, b, bound_a, bound_b
