"""The links of the engine's backward pass (`backward_impl`, e-osvos_amd/csrc/engine.cpp), one plain torch function each.

A LINK recomputes one buffer of the backward pass from the buffers upstream of it -- the operands the engine's own kernels
read, which stay in place after a step (`eosvos_debug_tensor`) -- so an error in one kernel shows in its own link and in no
other: no ReLU gate flips anywhere, because every mask is taken from the activation the kernel masked with.

* gradient convention: every `g_*` buffer is dL/d(post-norm, pre-ReLU output) of the layer that wrote the activation; the
  gradient on the conv side of a frozen norm is `a * g`, `a` the folded scale gamma / sqrt(var + eps) per output channel;
* a WEIGHT link (one per conv): dW = wgrad(x, a * g), OIHW; the classifier's bias gradient is the pixel sum of its g;
* a DATA link: one `g_*` buffer (or `gp` / `gvec` of the image-pooling branch) from the gradients and weights it is made of;
* GroupNorm mode (`Net(encoder, 'gn')`): same convention for `g_*`.  Every normalised conv ci keeps its raw output z in one
  buffer (`z<ci>` after the forward pass) that the backward pass overwrites with dL/dz (here `dz<ci>`: the same engine buffer,
  read after the step).  A GN FORWARD link recomputes the stored activation from z, a GN BACKWARD link recomputes dz from z
  and the conv's g (a whole buffer or its channel slice); the weight and data links read dz where the frozen form reads
  `a * g`, with no scale.

Everything here is dtype-generic (fp64 for the reference, fp32 for torch's own error on the same operands), runs on the
CPU and makes no engine call.  tests/test_backward_links_host.py proves every function against autograd on the oracle
network; tests/test_gpu_backward_links.py feeds them the engine's buffers.

Scope: DeepLabV3+ on ResNet-50 / ResNet-101, frozen BatchNorm or GroupNorm.  Not covered: the backward pass of plain
DeepLabV3 (`Net` describes its graph for the forward links, tests/forward_links_ref.py).  The accumulating
(`gsum`) meta path and the trainable boundary: tests/meta_links_ref.py.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from eosvos_amd import topology

STAGES = ('stem', 'layer1', 'layer2', 'layer3', 'layer4', 'aspp', 'decoder')

WeightLink = namedtuple('WeightLink', 'ci stage x g g_c0')       # dW[ci] = wgrad(T[x], a * T[g][:, g_c0:g_c0 + cout])
# out: the buffer the link recomputes; fn(T, W, A): its reference; mask: (activation, first masked channel) or None -- the
# gradient is zero wherever that activation is <= 0; convs: the convs whose data gradient it holds; misc: the kind of a
# link that is no convolution (a key of test_gpu_misc_ops.FLOOR, or 'maxpool_bwd')
DataLink = namedtuple('DataLink', 'out stage fn mask convs misc')
# GroupNorm links of conv ci: T[out][:, out_c0:out_c0 + cout] = relu?(gn(T[z<ci>]) (+ T[res])); dz = d(sum(g * gn(z))) / dz with
# g = T[g][:, g_c0:g_c0 + cout]
GNLink = namedtuple('GNLink', 'ci stage out out_c0 res relu g g_c0')
GN_GROUPS, GN_EPS = 16, 1e-5


class Net:
    """Indices of the graph's convs (`topology.conv_infos` order, the engine's) and its bottleneck blocks."""

    def __init__(self, encoder='resnet50', norm='bn'):
        assert norm in ('bn', 'gn'), norm
        self.encoder, self.gn, self.v3 = encoder, norm == 'gn', topology.is_v3(encoder)
        assert not (self.v3 and self.gn), 'plain DeepLabV3 has no GroupNorm variant'
        self.convs = topology.conv_infos(encoder)
        idx = {c.name: i for i, c in enumerate(self.convs)}
        self.blocks = []
        for i, c in enumerate(self.convs):
            if c.name.startswith('backbone.layer') and c.name.endswith('.conv1'):
                p = c.name[:-len('.conv1')]
                self.blocks.append(dict(c1=i, c2=idx[p + '.conv2'], c3=idx[p + '.conv3'], ds=idx.get(p + '.downsample.0', -1),
                                        stage='layer' + p.split('.')[1][-1]))
        self.tap = max(i for i, b in enumerate(self.blocks) if b['stage'] == 'layer1')      # the low-level feature
        a = 'classifier.0'
        self.aspp = [idx[f'{a}.convs.{j}.0'] for j in range(4)]
        self.pool, self.project = idx[a + '.convs.4.1'], idx[a + '.project.0']
        if self.v3:             # plain DeepLabV3: no decoder; DeepLabHead's 3x3 conv and classifier on the ASPP map
            self.dec1 = self.dec_a = self.dec_b = -1
            self.head3, self.last = idx['classifier.1'], idx['classifier.4']
        else:
            self.dec1, self.dec_a = idx['decoder.conv1'], idx['decoder.last_conv.0']
            self.dec_b, self.last, self.head3 = idx['decoder.last_conv.4'], idx['decoder.last_conv.8'], -1
        self.poff, self.lroff, self.noff = [], [], []
        p = l = n = 0
        for c in self.convs:
            self.poff.append(p); self.lroff.append(l); self.noff.append(n if c.norm else -1)
            p += c.cout * c.cin * c.k * c.k + (c.cout if c.bias else 0)
            l += c.cout + (1 if c.bias else 0)
            n += c.cout if c.norm else 0
        self.nparam, self.nlr, self.nnorm = p, l, n

    def xin(self, i):
        return 'p1' if i == 0 else f'blk{i - 1}.out'

    def g_xin(self, i):
        return 'g_p1' if i == 0 else f'blk{i - 1}.g_out'

    def stage_of(self, ci):
        if ci == 0:
            return 'stem'
        for b in self.blocks:
            if ci in (b['c1'], b['c2'], b['c3'], b['ds']):
                return b['stage']
        return 'aspp' if ci <= self.project else 'decoder'

    def weights(self, flat):
        """Per conv (OIHW weight, bias or None): views of the flat parameter vector (`eosvos_get_params` layout)."""
        out = []
        for c, o in zip(self.convs, self.poff):
            n = c.cout * c.cin * c.k * c.k
            out.append((flat[o:o + n].view(c.cout, c.cin, c.k, c.k), flat[o + n:o + n + c.cout] if c.bias else None))
        return out

    def scales(self, norm_a):
        """Per conv: its slice of the concatenated folded norm scales (norm-layer order), None for the classifier.  The folded
        shifts `norm_b` have the same layout and are sliced the same way."""
        return [norm_a[o:o + c.cout] if c.norm else None for c, o in zip(self.convs, self.noff)]


# ---- the operations ---------------------------------------------------------------------------------------------------------
def wgrad(x, g, c):
    return torch.nn.grad.conv2d_weight(x, (c.cout, c.cin, c.k, c.k), g, stride=c.stride, padding=c.pad, dilation=c.dil)


def dgrad(g, w, c, in_hw):
    return torch.nn.grad.conv2d_input((g.shape[0], c.cin) + tuple(in_hw), w, g, stride=c.stride, padding=c.pad, dilation=c.dil)


def scaled(g, a):
    return g if a is None else g * a.view(1, -1, 1, 1)


def conv_side(net, ci, g, T, A):
    """The gradient on the conv side of conv ci's norm layer: a * g (frozen BatchNorm; g itself for the classifier), or the
    engine's dz (GroupNorm)."""
    if net.gn and net.convs[ci].norm:
        return T[f'dz{ci}']
    return scaled(g, A[ci])


def gn_fwd(z, gamma, beta, res=None, relu=True):
    y = F.group_norm(z, GN_GROUPS, gamma, beta, GN_EPS)
    if res is not None:
        y = y + res
    return F.relu(y) if relu else y


def gn_bwd(z, g, gamma):
    """d(sum(g * group_norm(z))) / dz (the shift does not enter)."""
    z = z.detach().clone().requires_grad_(True)
    return torch.autograd.grad(F.group_norm(z, GN_GROUPS, gamma, None, GN_EPS), z, g)[0]


def relumask(act):
    return (act > 0).to(act.dtype)


def resize_bwd(g, in_hw, align_corners):
    """The adjoint of the bilinear resize (in_hw -> g's size): linear, so its input's values do not matter."""
    x = torch.zeros(g.shape[:2] + tuple(in_hw), dtype=g.dtype, requires_grad=True)
    y = F.interpolate(x, size=g.shape[-2:], mode='bilinear', align_corners=align_corners)
    return torch.autograd.grad(y, x, g)[0]


def maxpool_bwd(c1, g):
    """3x3 / stride 2 / pad 1 max-pool backward onto the stem's ReLU output, times that ReLU's mask (the kernel routes a
    gradient only to an argmax whose value is > 0)."""
    x = c1.detach().clone().requires_grad_(True)
    y = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    return torch.autograd.grad(y, x, g)[0] * relumask(c1)


# ---- weight links -----------------------------------------------------------------------------------------------------------
def weight_links(net):
    assert not net.v3, 'the backward links cover DeepLabV3+ only'
    L = [None] * len(net.convs)
    L[0] = WeightLink(0, 'stem', 'x', 'g_c1', 0)
    for i, b in enumerate(net.blocks):
        st = b['stage']
        L[b['c1']] = WeightLink(b['c1'], st, net.xin(i), f'blk{i}.g_t1', 0)
        L[b['c2']] = WeightLink(b['c2'], st, f'blk{i}.t1', f'blk{i}.g_t2', 0)
        L[b['c3']] = WeightLink(b['c3'], st, f'blk{i}.t2', f'blk{i}.g_out', 0)
        if b['ds'] >= 0:
            L[b['ds']] = WeightLink(b['ds'], st, net.xin(i), f'blk{i}.g_out', 0)
    l4 = f'blk{len(net.blocks) - 1}.out'
    for j, ci in enumerate(net.aspp):
        L[ci] = WeightLink(ci, 'aspp', l4, 'g_cat', 256 * j)
    L[net.pool] = WeightLink(net.pool, 'aspp', 'vec', 'gp', 0)
    L[net.project] = WeightLink(net.project, 'aspp', 'cat', 'g_proj', 0)
    L[net.dec1] = WeightLink(net.dec1, 'decoder', f'blk{net.tap}.out', 'g_dcat', 256)
    L[net.dec_a] = WeightLink(net.dec_a, 'decoder', 'dcat', 'g_d1', 0)
    L[net.dec_b] = WeightLink(net.dec_b, 'decoder', 'd1', 'g_d2', 0)
    L[net.last] = WeightLink(net.last, 'decoder', 'd2', 'g_low', 0)
    assert all(l is not None for l in L)
    return L


def weight_link(net, link, T, A):
    """(dW OIHW, dbias or None) of one conv from the buffers T (name -> NCHW tensor) and the per-conv scales A."""
    c = net.convs[link.ci]
    g = conv_side(net, link.ci, T[link.g][:, link.g_c0:link.g_c0 + c.cout], T, A)
    return wgrad(T[link.x], g, c), (g.sum(dim=(0, 2, 3)) if c.bias else None)


# ---- data links -------------------------------------------------------------------------------------------------------------
def _hw(t):
    return tuple(t.shape[-2:])


def data_links(net):
    """Every data link, in the order `backward_impl` runs them.  fn(T, W, A) -> the link's buffer; T: name -> NCHW tensor,
    W: per conv (weight, bias), A: per conv scale."""
    assert not net.v3, 'the backward links cover DeepLabV3+ only'
    cv = net.convs
    L = []

    def conv_dg(ci, g, T, W, A, in_hw):
        return dgrad(conv_side(net, ci, g, T, A), W[ci][0], cv[ci], in_hw)

    L.append(DataLink('g_low', 'decoder', lambda T, W, A: resize_bwd(T['dlogits'], _hw(T['d2']), False), None, (), 'resize_bwd'))
    L.append(DataLink('g_d2', 'decoder', lambda T, W, A: relumask(T['d2']) * conv_dg(net.last, T['g_low'], T, W, A, _hw(T['d2'])),
                      ('d2', 0), (), 'head_gx'))
    L.append(DataLink('g_d1', 'decoder', lambda T, W, A: relumask(T['d1']) * conv_dg(net.dec_b, T['g_d2'], T, W, A, _hw(T['d1'])),
                      ('d1', 0), (net.dec_b,), None))

    def g_dcat(T, W, A):
        r = conv_dg(net.dec_a, T['g_d1'], T, W, A, _hw(T['dcat'])).clone()
        r[:, 256:] *= relumask(T['dcat'][:, 256:])            # channels [0, 256): the upsampled ASPP output, no ReLU of its own
        return r
    L.append(DataLink('g_dcat', 'decoder', g_dcat, ('dcat', 256), (net.dec_a,), None))
    L.append(DataLink('g_proj', 'decoder',
                      lambda T, W, A: relumask(T['proj']) * resize_bwd(T['g_dcat'][:, :256], _hw(T['proj']), True),
                      ('proj', 0), (), 'resize_bwd'))
    L.append(DataLink('g_cat', 'aspp', lambda T, W, A: relumask(T['cat']) * conv_dg(net.project, T['g_proj'], T, W, A, _hw(T['cat'])),
                      ('cat', 0), (net.project,), None))
    L.append(DataLink('gp', 'aspp', lambda T, W, A: T['g_cat'][:, 1024:1280].sum(dim=(2, 3), keepdim=True), None, (), 'pool_bwd'))
    L.append(DataLink('gvec', 'aspp', lambda T, W, A: conv_dg(net.pool, T['gp'], T, W, A, (1, 1)), None, (), 'pool_bwd'))
    last = len(net.blocks) - 1

    def g_l4(T, W, A):
        l4 = T[f'blk{last}.out']
        s = (T['gvec'] / (l4.shape[2] * l4.shape[3])).expand_as(l4).clone()
        for j, ci in enumerate(net.aspp):
            s += conv_dg(ci, T['g_cat'][:, 256 * j:256 * j + 256], T, W, A, _hw(l4))
        return relumask(l4) * s
    L.append(DataLink(f'blk{last}.g_out', 'aspp', g_l4, (f'blk{last}.out', 0), tuple(net.aspp), None))
    for i in range(last, -1, -1):
        b = net.blocks[i]
        st = b['stage']
        L.append(DataLink(f'blk{i}.g_t2', st,
                          lambda T, W, A, i=i, b=b: relumask(T[f'blk{i}.t2']) * conv_dg(b['c3'], T[f'blk{i}.g_out'], T, W, A, _hw(T[f'blk{i}.t2'])),
                          (f'blk{i}.t2', 0), (b['c3'],), None))
        L.append(DataLink(f'blk{i}.g_t1', st,
                          lambda T, W, A, i=i, b=b: relumask(T[f'blk{i}.t1']) * conv_dg(b['c2'], T[f'blk{i}.g_t2'], T, W, A, _hw(T[f'blk{i}.t1'])),
                          (f'blk{i}.t1', 0), (b['c2'],), None))

        def g_xin(T, W, A, i=i, b=b):
            xin = T[net.xin(i)]
            s = conv_dg(b['c1'], T[f'blk{i}.g_t1'], T, W, A, _hw(xin))
            if b['ds'] >= 0:        # downsample form
                s = s + conv_dg(b['ds'], T[f'blk{i}.g_out'], T, W, A, _hw(xin))
            else:                   # identity form
                s = s + T[f'blk{i}.g_out']
            if i == net.tap + 1:    # the low-level feature also feeds the decoder's conv1
                s = s + conv_dg(net.dec1, T['g_dcat'][:, 256:304], T, W, A, _hw(xin))
            return s if i == 0 else relumask(xin) * s         # p1 is a max-pool output: its mask is the stem's, in maxpool_bwd
        convs = (b['c1'],) + ((b['ds'],) if b['ds'] >= 0 else ()) + ((net.dec1,) if i == net.tap + 1 else ())
        L.append(DataLink(net.g_xin(i), st, g_xin, None if i == 0 else (net.xin(i), 0), convs, None))
    L.append(DataLink('g_c1', 'stem', lambda T, W, A: maxpool_bwd(T['c1'], T['g_p1']), ('c1', 0), (), 'maxpool_bwd'))
    return L


def gn_links(net):
    """One GNLink per normalised conv, in conv order."""
    L = {0: GNLink(0, 'stem', 'c1', 0, None, True, 'g_c1', 0)}
    for i, b in enumerate(net.blocks):
        st = b['stage']
        L[b['c1']] = GNLink(b['c1'], st, f'blk{i}.t1', 0, None, True, f'blk{i}.g_t1', 0)
        L[b['c2']] = GNLink(b['c2'], st, f'blk{i}.t2', 0, None, True, f'blk{i}.g_t2', 0)
        L[b['c3']] = GNLink(b['c3'], st, f'blk{i}.out', 0, f'blk{i}.dsb' if b['ds'] >= 0 else net.xin(i), True, f'blk{i}.g_out', 0)
        if b['ds'] >= 0:
            L[b['ds']] = GNLink(b['ds'], st, f'blk{i}.dsb', 0, None, False, f'blk{i}.g_out', 0)
    for j, ci in enumerate(net.aspp):
        L[ci] = GNLink(ci, 'aspp', 'cat', 256 * j, None, True, 'g_cat', 256 * j)
    L[net.pool] = GNLink(net.pool, 'aspp', 'poolout', 0, None, True, 'gp', 0)
    L[net.project] = GNLink(net.project, 'aspp', 'proj', 0, None, True, 'g_proj', 0)
    L[net.dec1] = GNLink(net.dec1, 'decoder', 'dcat', 256, None, True, 'g_dcat', 256)
    L[net.dec_a] = GNLink(net.dec_a, 'decoder', 'd1', 0, None, True, 'g_d1', 0)
    L[net.dec_b] = GNLink(net.dec_b, 'decoder', 'd2', 0, None, True, 'g_d2', 0)
    assert sorted(L) == [ci for ci, c in enumerate(net.convs) if c.norm]
    return [L[ci] for ci in sorted(L)]


def gn_fwd_link(net, l, T, GB):
    """(recomputed, stored) activation of GN link l; GB: per conv (gamma, beta)."""
    cout = net.convs[l.ci].cout
    y = gn_fwd(T[f'z{l.ci}'], GB[l.ci][0], GB[l.ci][1], T[l.res] if l.res else None, l.relu)
    return y, T[l.out][:, l.out_c0:l.out_c0 + cout]


def gn_bwd_link(net, l, T, GB):
    """(recomputed, stored) dz of GN link l."""
    cout = net.convs[l.ci].cout
    return gn_bwd(T[f'z{l.ci}'], T[l.g][:, l.g_c0:l.g_c0 + cout], GB[l.ci][0]), T[f'dz{l.ci}']


def affines(net, state, dtype):
    """Per conv (gamma, beta) of its norm layer from a model state dict, None for the classifier."""
    return [(state[c.norm + '.weight'].to(dtype), state[c.norm + '.bias'].to(dtype)) if c.norm else None for c in net.convs]


def z_names(net):
    """The engine's names (`z<ci>`) of the raw-output buffers of a GroupNorm engine."""
    return [f'z{ci}' for ci, c in enumerate(net.convs) if c.norm]


def buffer_names(net):
    """Every named buffer the links read or recompute, the input frame ('x') and the z / dz buffers of a GroupNorm engine
    (`z_names`) aside."""
    names = ['c1', 'p1', 'g_c1', 'g_p1', 'cat', 'g_cat', 'vec', 'gvec', 'poolout', 'gp', 'proj', 'g_proj', 'dcat', 'g_dcat',
             'd1', 'd2', 'g_d1', 'g_d2', 'g_low', 'dlogits']
    for i in range(len(net.blocks)):
        names += [f'blk{i}.{k}' for k in ('t1', 't2', 'out', 'g_t1', 'g_t2', 'g_out')]
        if net.gn and net.blocks[i]['ds'] >= 0:
            names.append(f'blk{i}.dsb')                     # the shortcut's output: the residual of the block's last GroupNorm
    return names


class Cast:
    """name -> tensor in one dtype, converted on first use (a stage's test touches only its own buffers)."""

    def __init__(self, tensors, dtype):
        self.src, self.dtype, self.done = tensors, dtype, {}

    def __getitem__(self, name):
        if name not in self.done:
            self.done[name] = self.src[name].to(self.dtype)
        return self.done[name]


def update_reference(net, before, lr, grad):
    """fp64 `w - lr * g` of every scalar, lr per output channel (`eosvos_set_lr`: one value per conv output channel, one for
    the classifier's bias), and the per-element bound 2^-23 (|w| + |lr g|): one fp32 rounding of the product (relative
    2^-24 of |lr g|) plus one of the difference (2^-24 of |w - lr g| <= |w| + |lr g|), with a factor two to spare."""
    w, g = before.double(), grad.double()
    lre = torch.empty_like(w)
    for c, po, lo in zip(net.convs, net.poff, net.lroff):
        n = c.cout * c.cin * c.k * c.k
        lre[po:po + n].view(c.cout, -1).copy_(lr[lo:lo + c.cout].double().view(-1, 1).expand(c.cout, n // c.cout))
        if c.bias:
            lre[po + n:po + n + c.cout] = lr[lo + c.cout].double()
    step = lre * g
    return w - step, 2.0 ** -23 * (w.abs() + step.abs())


def tensor_of(net, index):
    """(trainable tensor's name, offset inside it) of a flat parameter index."""
    for c, po in zip(reversed(net.convs), reversed(net.poff)):
        if index >= po:
            n = c.cout * c.cin * c.k * c.k
            return (c.name + '.weight', index - po) if index < po + n else (c.name + '.bias', index - po - n)
    raise IndexError(index)
