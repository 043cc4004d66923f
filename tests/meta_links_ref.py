"""The links of the meta-gradient path (`eosvos_meta_grad_ex`) and of the outer step (`eosvos_outer_step`), one plain torch
function each (e-osvos_amd/csrc/engine.cpp, misc_kernels.hip).

Every link is linear or elementwise and local: it recomputes one vector from the vectors upstream of it -- the engine's own
operands (`get_grads` after each step, `debug_gsum`, the caller's buffers) -- so an error in one kernel shows in its own link
and in no other, and no link depends on the accuracy of a convolution.

Everything is dtype-generic: called with float64 tensors a function is the reference, with float32 tensors it is torch's own
error on the same operands (the `err_torch32` yardstick).  Nothing here needs a GPU.  All vectors are in the flat layout of
`get_grads` / `flat_meta_grad`: OIHW, weight then bias per conv, tensors in `topology.trainable` order.
tests/test_meta_links_host.py proves the functions against autograd and the oracle's RAdam; tests/test_gpu_meta_links.py
feeds them the engine's buffers.

The bounds (`rows_n_round`, `row_floor`, ...) are counted from the kernels' summation structure, in units of U = 2^-24 (one
fp32 rounding, relative); no measured constant enters them.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from eosvos_amd import topology

U = 2.0 ** -24                  # one fp32 rounding, relative to the rounded value
EXP_ULPS = 2                    # expf of the device library: 1 ulp = 2 U (HIP math API accuracy table)
Conv = namedtuple('Conv', 'name cin cout k bias')


class Layout:
    """Offsets of the flat vectors: per conv `poff` (parameters) and `lroff` (per-neuron lr rows: cout weight rows, then cout
    bias rows); per lr row its first element and length; per state-dict tensor its first row."""

    def __init__(self, convs):
        self.convs = [Conv(c.name, c.cin, c.cout, c.k, bool(c.bias)) for c in convs]
        self.poff, self.lroff, self.tensor_row0, self.tensor_poff = [], [], [], []
        base, length = [], []
        p = l = 0
        for c in self.convs:
            rl, w = c.cin * c.k * c.k, c.cout * c.cin * c.k * c.k
            self.poff.append(p); self.lroff.append(l)
            self.tensor_row0.append(l); self.tensor_poff.append(p)
            base += [p + r * rl for r in range(c.cout)]; length += [rl] * c.cout
            if c.bias:
                self.tensor_row0.append(l + c.cout); self.tensor_poff.append(p + w)
                base += [p + w + r for r in range(c.cout)]; length += [1] * c.cout
            p += w + (c.cout if c.bias else 0)
            l += c.cout * (2 if c.bias else 1)
        self.nparam, self.nlr, self.ntensors = p, l, len(self.tensor_row0)
        self.tensor_row0.append(l); self.tensor_poff.append(p)
        self.row_base, self.row_len = torch.tensor(base), torch.tensor(length)

    @classmethod
    def of(cls, encoder):
        return cls(topology.conv_infos(encoder))

    def store_count(self, level):
        return {'NEURON': self.nlr, 'TENSOR': self.ntensors, 'SINGLE': 1, 'PARAM': self.nparam}[level]

    def group_row0(self, level):
        """First row of every stored value's group of lr rows (+ the end), TENSOR and SINGLE."""
        return self.tensor_row0 if level == 'TENSOR' else [0, self.nlr]

    def conv_index(self, name):
        return [c.name for c in self.convs].index(name)


# ---- the inner loop's sum ---------------------------------------------------------------------------------------------------
def accumulate_link(grads_per_step):
    """gsum_K = ((g_1 + g_2) + ...), elementwise and in this order (`gsum[e] += g` of the fused update, from zero)."""
    s = grads_per_step[0].clone()
    for g in grads_per_step[1:]:
        s = s + g
    return s


# ---- the lr gradient --------------------------------------------------------------------------------------------------------
def lr_grad_neuron(gsum, G, weight, net, drop_last_of=None, bias_shift=0, weight_twice=False):
    """Per lr row: -weight * sum_e gsum[row, e] * G[row, e] (weight rows: T * cin elements, bias rows: 1), and
    S_abs[row] = |weight| * sum_e |gsum * G|, the scale its error is measured against (the sum cancels).
    The keyword arguments plant the mistakes the bounds must see (test_meta_links_host): the last element of one row dropped,
    the bias rows paired with a base `bias_shift` elements early, `weight` applied twice."""
    prod = gsum * G
    if drop_last_of is not None:
        prod = prod.clone()
        prod[int(net.row_base[drop_last_of] + net.row_len[drop_last_of]) - 1] = 0
    w = weight * weight if weight_twice else weight
    glr, sabs = prod.new_zeros(net.nlr), prod.new_zeros(net.nlr)
    for c, po, lo in zip(net.convs, net.poff, net.lroff):
        n = c.cout * c.cin * c.k * c.k
        rows = prod[po:po + n].view(c.cout, -1)
        glr[lo:lo + c.cout] = -w * rows.sum(dim=1)
        sabs[lo:lo + c.cout] = abs(w) * rows.abs().sum(dim=1)
        if c.bias:
            b = prod[po + n - bias_shift:po + n - bias_shift + c.cout]
            glr[lo + c.cout:lo + 2 * c.cout] = -w * b
            sabs[lo + c.cout:lo + 2 * c.cout] = abs(w) * b.abs()
    return glr, sabs


def lr_grad_store(glr_neuron, lr_eff, level, use_log, net):
    """The chain from the per-neuron d/d lr to the stored level (meta_optim.py:27-67,157-163,180-185): times lr_eff for log
    storage (d exp(s) / d s), then identity (NEURON), the sum over the rows of each state-dict tensor (TENSOR; weight and
    bias are separate tensors) or over all rows (SINGLE).  Also right for S_abs (every factor is >= 0)."""
    g = glr_neuron * lr_eff if use_log else glr_neuron
    if level == 'NEURON':
        return g
    r0 = net.group_row0(level)
    return torch.stack([g[a:b].sum() for a, b in zip(r0[:-1], r0[1:])])


def lr_grad_param(gsum, G, lr_elem, weight):
    """PARAM level: -weight * gsum * G (* lr_elem for log storage), elementwise, in the kernel's order."""
    v = -gsum * G
    if lr_elem is not None:
        v = v * lr_elem
    return weight * v


def init_grad_link(prior, G, weight):
    return prior + weight * G


def expand_lr(store, level, use_log, net):
    """Effective per-neuron lr of a stored state (NEURON / TENSOR / SINGLE): `lr_expand_kernel`."""
    if level == 'TENSOR':
        r0 = net.tensor_row0
        store = torch.cat([store[t].expand(b - a) for t, (a, b) in enumerate(zip(r0[:-1], r0[1:]))])
    elif level == 'SINGLE':
        store = store.reshape(1).expand(net.nlr)
    return store.exp() if use_log else store.clone()


# ---- bounds of the lr gradient ----------------------------------------------------------------------------------------------
def rows_n_round(net, level, use_log):
    """Roundings on the way to one per-neuron row (`meta_lr_grad_all_kernel`), per row: the per-thread fma chain of
    ceil(rowlen / 256) terms, the 6 shuffle levels of the wave sum, the 2 additions of the 4 wave sums (counted as a tree;
    the kernel adds them left to right, three deep: the bound is the tighter one), the multiply by `weight` and the subtract.
    Log storage: + the multiply by lr_eff and the device expf that made lr_eff (EXP_ULPS)."""
    n = torch.ceil(net.row_len.double() / 256) + 6 + 2 + 1 + 1
    return n + (1 + EXP_ULPS if use_log else 0)


def reduce_n_round(nrows, use_log):
    """The same count for `lr_grad_reduce_kernel` over the `nrows` rows of a group: chain, shuffles, wave sums."""
    return math.ceil(nrows / 256) + 6 + 2


def row_floor(n_round, s_abs, prior, result):
    """n_round * U * S_abs: every partial sum of the row is <= S_abs, each rounding within U of it; 2 U (|prior| + |result|):
    the rounding of the final `+=` into the caller's buffer, with a factor two to spare."""
    return n_round * U * s_abs + 2 * U * (prior.abs() + result.abs())


def store_floor(net, level, use_log, s_abs_neuron, lr_eff, prior, result):
    """Per stored value: the floor of `|gpu - ref64|` (float64 tensors).  s_abs_neuron: S_abs per row for the weight in use."""
    n_rows = rows_n_round(net, level, use_log)
    s = s_abs_neuron * lr_eff if use_log else s_abs_neuron
    if level == 'NEURON':
        return row_floor(n_rows, s, prior, result)
    r0 = net.group_row0(level)
    n = torch.tensor([float(n_rows[a:b].max()) + reduce_n_round(b - a, use_log) for a, b in zip(r0[:-1], r0[1:])], dtype=torch.float64)
    sg = torch.stack([s[a:b].sum() for a, b in zip(r0[:-1], r0[1:])])
    return row_floor(n, sg, prior, result)


def elem_floor(prior, term):
    """PARAM level and the init gradient: 2^-23 (|prior| + |term|) per element.  The init gradient has two roundings
    (weight * G, the add): U |term| + U |prior + term|.  PARAM has up to four on the term (gsum * G, * lr_elem, * weight, and
    lr_elem's expf at EXP_ULPS) and the add: (3 + EXP_ULPS) U |term| + U |prior + term| -- within the bound wherever
    |prior| >= (2 + EXP_ULPS) |term|, which is how the tests fill the buffer."""
    return 2 * U * (prior.abs() + term.abs())


# ---- RAdam and the outer step -----------------------------------------------------------------------------------------------
def f32(x):
    """A hyper-parameter as the kernel receives it: a C float."""
    return float(np.float32(x))


def radam_scalars(step, betas):
    """(N_sma, step_size) of radam.py:62-79 (degenerated_to_sgd) in Python floats, from the betas the kernel receives."""
    b1, b2 = f32(betas[0]), f32(betas[1])
    b2t = b2 ** step
    n_max = 2.0 / (1.0 - b2) - 1.0
    n_sma = n_max - 2.0 * step * b2t / (1.0 - b2t)
    if n_sma >= 5.0:
        return n_sma, math.sqrt((1.0 - b2t) * (n_sma - 4.0) / (n_max - 4.0) * (n_sma - 2.0) / n_sma * n_max / (n_max - 2.0)) / (1.0 - b1 ** step)
    return n_sma, 1.0 / (1.0 - b1 ** step)


def _sqrt(t):
    """Correctly rounded in either precision, as the kernel's sqrtf (torch's float32 sqrt on the CPU is not: it is off by one
    ulp for about one input in 150; the double root of a float rounds to the float root exactly)."""
    return t.sqrt() if t.dtype == torch.float64 else t.double().sqrt().float()


def radam_link(p, g, m, v, step, lr, wd, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, grad_clip=0.0, beta1_for_beta2=False):
    """radam.py:28-94 restated, functional: returns (p, m, v) after step number `step` (1-based).  N_sma and step_size in
    Python floats; the elementwise part in the tensors' dtype, in the order of `radam_kernel`; the N_sma < 5 branch has no
    denominator.  The scalars are the C floats the kernel receives; with float32 tensors their two products are formed in
    float32 as the kernel forms them.  (1 - beta is exact in either precision: beta >= 1/2.)"""
    lr, wd, eps, gs, clip = f32(lr), f32(wd), f32(eps), f32(grad_scale), f32(grad_clip)
    b1, b2 = f32(betas[0]), f32(betas[1])
    n_sma, step_size = radam_scalars(step, betas)
    if p.dtype == torch.float32:
        c_wd, c_step = float(np.float32(-wd) * np.float32(lr)), float(-np.float32(step_size) * np.float32(lr))
    else:
        c_wd, c_step = -wd * lr, -step_size * lr
    if beta1_for_beta2:
        b2 = b1
    gr = g * gs
    if clip > 0:
        gr = gr.clamp(-clip, clip)
    vv = v * b2 + ((1.0 - b2) * gr) * gr
    mm = m * b1 + (1.0 - b1) * gr
    pv = p
    if wd != 0:
        pv = pv + c_wd * pv
    if n_sma >= 5.0:
        pv = pv + c_step * (mm / (_sqrt(vv) + eps))
    else:
        pv = pv + c_step * mm
    return pv, mm, vv


def outer_step_link(state, grad, m, v, hyper, net, skip_clamp=False, beta1_for_beta2=False):
    """`eosvos_outer_step`: the two parameter groups of the learned state [lr state (n_lr) | init (n_param, when
    learn_model_init)].  lr state: `lr_lr`, no weight decay, then the clamp to [lr_lo, lr_hi]; init: `init_lr`, `wd`.  The
    leading frozen_lr / frozen_param elements of each take lr 0: their m and v move, their value does not.
    hyper: dict(step, lr_lr, init_lr, wd, betas, eps, grad_scale, grad_clip, lr_lo, lr_hi, use_log, frozen_lr, frozen_param).
    Returns (state, m, v, effective lr, init part or None)."""
    h = hyper
    kw = dict(betas=h['betas'], eps=h['eps'], grad_scale=h['grad_scale'], grad_clip=h['grad_clip'], beta1_for_beta2=beta1_for_beta2)
    n = net.nlr
    cuts = [(0, h['frozen_lr'], 0.0, 0.0), (h['frozen_lr'], n, h['lr_lr'], 0.0)]
    if state.numel() > n:
        assert state.numel() == n + net.nparam
        cuts += [(n, n + h['frozen_param'], 0.0, h['wd']), (n + h['frozen_param'], n + net.nparam, h['init_lr'], h['wd'])]
    ps, ms, vs = [], [], []
    for a, b, lr, wd in cuts:
        pv, mm, vv = radam_link(state[a:b], grad[a:b], m[a:b], v[a:b], h['step'], lr, wd, **kw)
        ps.append(pv); ms.append(mm); vs.append(vv)
    new, nm, nv = torch.cat(ps), torch.cat(ms), torch.cat(vs)
    if not skip_clamp:
        new[:n] = new[:n].clamp(f32(h['lr_lo']), f32(h['lr_hi']))
    lr_eff = new[:n].exp() if h['use_log'] else new[:n].clone()
    return new, nm, nv, lr_eff, (new[n:] if state.numel() > n else None)


def outer_floors(state, grad, m, v, new64, hyper):
    """Per element, from float64 operands: 2^-22 (|p| + |delta|) for the state (delta: what the step moved it by, before the
    clamp cut it), 2^-22 (|beta1 m| + |(1 - beta1) g'|) for m, 2^-22 (|beta2 v| + |(1 - beta2) g'^2|) for v; g' the scaled and
    clipped gradient.  m: the roundings of g' (U), (1 - beta1) g' (U), beta1 m (U) and the sum (U of the total) are within it;
    v has one more on its second term."""
    h = hyper
    b1, b2 = f32(h['betas'][0]), f32(h['betas'][1])
    gr = grad * f32(h['grad_scale'])
    if f32(h['grad_clip']) > 0:
        gr = gr.clamp(-f32(h['grad_clip']), f32(h['grad_clip']))
    fm = 4 * U * ((b1 * m).abs() + ((1 - b1) * gr).abs())
    fv = 4 * U * ((b2 * v).abs() + ((1 - b2) * gr * gr).abs())
    return 4 * U * (state.abs() + (new64 - state).abs()), fm, fv


# ---- the engine's layout ----------------------------------------------------------------------------------------------------
def engine_layout(flat, net, swap_it=False):
    """Flat OIHW -> the engine's arena, O,(kh,kw),I per conv, biases in place (the scatter of `outer_step_kernel` into Winit /
    Wp).  swap_it: the planted mistake -- I and T exchanged in the destination index."""
    out = flat.clone()
    for c, po in zip(net.convs, net.poff):
        t, n = c.k * c.k, c.cout * c.cin * c.k * c.k
        if not swap_it:                     # d = (o * T + t) * I + i; exchanged it is (o * I + i) * T + t: the source's own place
            out[po:po + n] = flat[po:po + n].view(c.cout, c.cin, t).permute(0, 2, 1).reshape(-1)
    return out


def flat_layout(arena, net):
    """The engine's arena -> flat OIHW (`get_params`)."""
    out = arena.clone()
    for c, po in zip(net.convs, net.poff):
        t, n = c.k * c.k, c.cout * c.cin * c.k * c.k
        out[po:po + n] = arena[po:po + n].view(c.cout, t, c.cin).permute(0, 2, 1).reshape(-1)
    return out
