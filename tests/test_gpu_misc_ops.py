"""Op-level parity of the non-convolution kernels (misc_kernels.hip) on the GPU, through the C-ABI test entries
(eosvos_test_groupnorm / _maxpool / _resize / _aspp_pool / _head drive the production launchers with the engine's own
geometry; the losses go through eosvos_bce / eosvos_loss_tensors).

Every case is compared ELEMENTWISE with the same torch op in float64 on the CPU (the calls oracle/deeplab.py makes,
gradients by autograd), and with the op in torch float32 on the CPU: err_gpu <= max(K * err_torch32, floor), both relative to
the reference's scale.  One MARGIN line per case.  Structural results (ReLU masks, the max-pool argmax routing, NaN
positions) are asserted exactly.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from eosvos_amd import _ffi
from eosvos_amd.engine import Engine
from oracle import deeplab

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K = 4                       # err_gpu may be K times torch fp32's error ...
FLOOR = {                   # ... or this floor (relative to the output's scale), whichever is larger
    'gn_fwd': 4e-6, 'gn_bwd': 4e-6,
    'resize_fwd': 2e-6, 'resize_bwd': 4e-6,
    'pool_fwd': 4e-6, 'pool_bwd': 4e-6, 'pool_dw': 4e-6,
    'head_fwd': 2e-6, 'head_gx': 2e-7, 'head_dw': 4e-6,
    'loss': 2e-6, 'dlogits': 2e-6,
}


@pytest.fixture(scope='module')
def eng():
    e = Engine('resnet50', 96, 160, max_batch=1, device=DEV)
    yield e
    e.close()


def _err(a, ref):
    a, ref = a.double().cpu(), ref.double()
    scale = float(ref.abs().max())
    return float((a - ref).abs().max()) / (scale if scale > 0 else 1.0)


def _check(case, cap=None, **parts):
    """parts: name -> (gpu, torch32, fp64 reference, floor key).  Prints the MARGIN line, then asserts every part.
    cap: an upper limit of every bound, for inputs on which torch fp32 itself is far from the fp64 result."""
    res = {}
    for name, (gpu, t32, ref, fk) in parts.items():
        eg, e32 = _err(gpu, ref), _err(t32, ref)
        bound = max(K * e32, FLOOR[fk])
        res[name] = (eg, e32, min(bound, max(cap, FLOOR[fk])) if cap is not None else bound)
    print(f'MARGIN {case} ' + ' '.join(f'{n} {eg:.2e} (torch32 {e32:.2e}, bound {b:.2e})' for n, (eg, e32, b) in res.items()))
    for n, (eg, e32, b) in res.items():
        assert eg <= b, (case, n, eg, e32, b)


def _relu_bits(y):
    """ReLU mask bytes of y (..., C): bit j of byte q = (channel 4q + j > 0)."""
    m = (y > 0).to(torch.uint8).reshape(*y.shape[:-1], -1, 4)
    return (m[..., 0] | (m[..., 1] << 1) | (m[..., 2] << 2) | (m[..., 3] << 3)).contiguous()


# ---- GroupNorm(16, C), frozen affine ------------------------------------------------------------------------------
def _gn_ref(z, g, gamma, beta, res, relu, dtype):
    """(y, dz) of y = relu?(group_norm(z) * gamma + beta (+ res)) on (B, P, C) tensors; dz = d(sum(g * (gn(z) gamma + beta)))/dz."""
    zz = z.to(dtype).permute(0, 2, 1).contiguous().requires_grad_(True)
    t = F.group_norm(zz, 16, gamma.to(dtype), beta.to(dtype), eps=1e-5)
    t.backward(g.to(dtype).permute(0, 2, 1))
    y = t.detach().permute(0, 2, 1)
    if res is not None:
        y = y + res.to(dtype)
    if relu:
        y = y.clamp_min(0)
    return y, zz.grad.permute(0, 2, 1)


def _run_gn(eng, case, z, gamma, beta, g, res=None, relu=False, ldz=None, ldy=None, yoff=0, cap=None):
    """z, g, res: CPU (B, P, C).  ldz / ldy: run on channel slices (at offset 4 / yoff) of wider device buffers."""
    B, P, C = z.shape
    zb = torch.full((B, P, ldz or C), float('nan'), device=DEV)
    zoff = 4 if ldz else 0
    zd = zb[:, :, zoff:zoff + C]
    zd.copy_(z)
    yb = torch.full((B, P, ldy or C), float('nan'), device=DEV)
    yd = yb[:, :, yoff:yoff + C]
    gm, bt = gamma.to(DEV), beta.to(DEV)
    resd = res.to(DEV) if res is not None else None
    m8 = torch.zeros(B, P, C // 4 + 3, dtype=torch.uint8, device=DEV) if relu else None
    y, stats = eng.test_groupnorm(zd, gm, bt, res=resd, relu=relu, y=yd, m8=m8)
    ygpu = y.cpu()
    outside = torch.cat([yb[:, :, :yoff], yb[:, :, yoff + C:]], dim=2)
    assert bool(outside.isnan().all()), 'GroupNorm wrote outside its channel slice'
    if relu:
        assert torch.equal(m8[:, :, :C // 4].cpu(), _relu_bits(ygpu)), 'm8 differs from y > 0'
        assert not bool(m8[:, :, C // 4:].any()), 'm8 written past C / 4 bytes'
    dz = eng.test_groupnorm_bwd(zd, g.to(DEV), gm, stats).cpu()
    assert torch.equal(zb[:, :, :zoff].isnan().cpu(), torch.ones(B, P, zoff, dtype=torch.bool))
    y64, dz64 = _gn_ref(z, g, gamma, beta, res, relu, torch.float64)
    y32, dz32 = _gn_ref(z, g, gamma, beta, res, relu, torch.float32)
    _check(case, cap=cap, fwd=(ygpu, y32, y64, 'gn_fwd'), bwd=(dz, dz32, dz64, 'gn_bwd'))


GN_CASES = [   # (C, B, P, residual, relu, ldz, ldy / y offset): the network's maps of 480x854 and 97x163, then the edges
    (64, 3, 49 * 82, False, True, None, None),        # stem, 97x163 (stride 2)
    (64, 1, 240 * 427, False, True, None, None),      # stem, 480x854
    (48, 1, 120 * 214, False, True, None, (304, 256)),  # decoder.conv1 into the dcat slice, 480x854 stride 4
    (64, 3, 25 * 41, True, True, None, None),
    (128, 3, 13 * 21, True, True, None, None),        # stride 8 of 97x163
    (256, 1, 120 * 214, False, True, None, None),
    (256, 3, 25 * 41, False, False, 1280, None),      # z a channel slice of a wider buffer
    (512, 1, 60 * 107, True, True, None, None),
    (1024, 3, 7 * 11, True, True, None, None),        # stride 16 of 97x163
    (1024, 1, 30 * 54, False, True, None, None),
    (2048, 1, 30 * 54, True, True, None, None),
    (2048, 3, 7 * 11, False, False, None, None),
    (256, 3, 1, False, True, None, None),             # the ASPP pooling branch's GroupNorm: one pixel
    (256, 1, 20, False, True, None, None),            # P < 8 * rows: one chunk
    (64, 1, 37, True, True, None, None),              # short last chunk
    (2048, 1, 5, False, True, None, None),
]


@pytest.mark.parametrize('case', GN_CASES, ids=lambda c: f'C{c[0]}_B{c[1]}_P{c[2]}')
def test_groupnorm_vs_fp64(eng, case):
    C, B, P, with_res, relu, ldz, ly = case
    gen = torch.Generator().manual_seed(C * 7 + P)
    z = torch.randn(B, P, C, generator=gen) * 2 + torch.randn(1, 1, C, generator=gen)       # per-channel means
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen) * 0.2
    g = torch.randn(B, P, C, generator=gen)
    res = torch.randn(B, P, C, generator=gen) if with_res else None
    _run_gn(eng, f'gn {case}', z, gamma, beta, g, res, relu, ldz=ldz, ldy=ly[0] if ly else None, yoff=ly[1] if ly else 0)


@pytest.mark.parametrize('offset', [0, 10, 100, 1000])
def test_groupnorm_mean_offset(eng, offset):
    """Groups whose mean is `offset` standard deviations from zero (the variance by E[z^2] - E[z]^2 of unshifted fp32 sums
    loses (mean / std)^2 of its precision), and one constant group (rstd = 1 / sqrt(eps)).  torch's own fp32 group_norm
    loses precision here too (1.8e-3 at 1000), so the bound is capped at 4x the rounding of the inputs themselves relative
    to their spread, offset * 2^-24: measured 1.2e-2 at 1000 and 1.1e-4 at 100 with unshifted sums, 6.6e-6 and 8.1e-7 now."""
    B, P, C = 2, 60 * 107, 256
    gen = torch.Generator().manual_seed(offset + 1)
    sign = torch.where(torch.rand(1, 1, 16, generator=gen) > 0.5, 1.0, -1.0)
    z = torch.randn(B, P, C, generator=gen) + (offset * sign).repeat_interleave(C // 16, dim=2)
    z[:, :, 5 * 16:6 * 16] = 3.25 + offset          # group 5: constant
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen) * 0.2
    g = torch.randn(B, P, C, generator=gen)
    _run_gn(eng, f'gn mean/std {offset}', z, gamma, beta, g, relu=True, cap=4 * offset * 2.0 ** -24)


# ---- max-pool 3x3 / 2 / 1 with the ReLU mask ------------------------------------------------------------------------
def _pool_ref(x, gy, dtype):
    xx = x.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.max_pool2d(xx, 3, 2, 1)
    y.backward(gy.to(dtype).permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), (xx.grad * (xx.detach() > 0)).permute(0, 2, 3, 1)


POOL_SHAPES = [(1, 1, 1), (1, 2, 2), (1, 1, 6), (2, 5, 1), (1, 3, 4), (2, 7, 9), (1, 8, 8),
               (3, 49, 81), (1, 49, 82), (2, 50, 83), (1, 50, 84),            # stem maps of 97..100 x 161..168
               (1, 240, 427), (1, 240, 428)]                                  # 480 x 853 / 855


@pytest.mark.parametrize('shape', POOL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_maxpool_vs_fp64(eng, shape):
    """Inputs on a few levels (ties among positive values are common; torch keeps the first maximum in raster order) with
    many exact zeros (a ReLU output); integer gradients, so the routed sums are exact: y and gx must match bit for bit."""
    B, H, W = shape
    C = 64
    gen = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.randint(-3, 4, (B, H, W, C), generator=gen).float().clamp_min(0) * 0.5
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randint(-8, 9, (B, Ho, Wo, C), generator=gen).float()
    y, idx, gx = eng.test_maxpool(x.to(DEV), gy.to(DEV))
    y64, gx64 = _pool_ref(x, gy, torch.float64)
    print(f'MARGIN maxpool {shape}: y {_err(y, y64):.2e} gx {_err(gx, gx64):.2e} (exact required)')
    assert torch.equal(y.cpu().double(), y64)
    assert torch.equal(gx.cpu().double(), gx64), 'argmax routing or ReLU mask differs from torch'
    assert torch.equal((idx.cpu() >= 0x80), y.cpu() > 0)


@pytest.mark.parametrize('tap', range(9))
def test_maxpool_special_values(eng, tap):
    """+inf, -inf and a NaN at every tap position of a window: y is NaN exactly where torch's is, and equal elsewhere
    (torch: `val > maxval || isnan(val)`).  The NaN's gradient routing is not asserted."""
    B, H, W, C = 1, 9, 11, 8
    gen = torch.Generator().manual_seed(tap)
    x = torch.randn(B, H, W, C, generator=gen)
    ky, kx = divmod(tap, 3)
    for c, oy, ox, v in ((0, 2, 2, float('nan')), (1, 1, 3, float('nan')), (2, 2, 2, float('inf')),
                         (3, 3, 1, float('-inf')), (4, 0, 0, float('nan')), (5, 4, 5, float('nan'))):
        iy, ix = oy * 2 - 1 + ky, ox * 2 - 1 + kx
        if 0 <= iy < H and 0 <= ix < W:
            x[0, iy, ix, c] = v
    x[0, :, :, 6] = float('-inf')                  # a channel of -inf only
    x[0, 4, 4, 7] = float('nan')
    x[0, 4, 5, 7] = float('nan')                   # two NaNs in some windows
    y, _, _ = eng.test_maxpool(x.to(DEV))
    y64, _ = _pool_ref(x, torch.zeros(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), torch.float64)
    y = y.cpu().double()
    print(f'MARGIN maxpool special tap {tap}: NaN outputs gpu {int(y.isnan().sum())} torch {int(y64.isnan().sum())}')
    assert torch.equal(y.isnan(), y64.isnan()), 'a NaN was dropped (or made up) by the max-pool'
    assert torch.equal(y.nan_to_num(0.0), y64.nan_to_num(0.0))


# ---- bilinear resize --------------------------------------------------------------------------------------------------
def _resize_ref(x, gy, mask, size, ac, dtype):
    xx = x.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.interpolate(xx, size=size, mode='bilinear', align_corners=ac)
    y.backward(gy.to(dtype).permute(0, 3, 1, 2))
    gx = xx.grad.permute(0, 2, 3, 1)
    if mask is not None:
        gx = gx * (mask.to(dtype) > 0)
    return y.detach().permute(0, 2, 3, 1), gx


RESIZE_CASES = [   # (align_corners, (hin, win), (hout, wout), B, C, ldy, masked)
    (True, (7, 11), (25, 41), 3, 256, 304, True),         # h16 -> h4 of 97x163 into the dcat slice
    (True, (30, 54), (120, 214), 1, 256, 304, True),      # 480x854
    (True, (31, 54), (121, 214), 1, 256, 304, False),
    (True, (8, 14), (29, 53), 2, 1, 1, False),            # V = 1
    (False, (25, 41), (97, 163), 3, 1, 1, False),         # h4 -> H logits
    (False, (120, 214), (480, 854), 1, 1, 1, False),
    (False, (121, 214), (481, 855), 1, 1, 1, False),
    (False, (30, 54), (120, 214), 1, 4, 4, True),
    (True, (1, 2), (5, 7), 2, 1, 1, False),               # in = 1 (align_corners: scale 0) and in = 2
    (False, (1, 2), (5, 7), 2, 4, 4, False),
    (True, (2, 1), (7, 5), 1, 4, 8, True),
    (False, (2, 3), (40, 50), 1, 1, 1, False),            # ratios > 12: resize_bwd_kernel<1> without the precomputed weights
    (True, (1, 3), (30, 40), 1, 1, 1, False),
    (False, (2, 3), (40, 50), 1, 4, 4, False),
]


@pytest.mark.parametrize('case', RESIZE_CASES, ids=lambda c: f'ac{int(c[0])}_{c[1][0]}x{c[1][1]}_{c[2][0]}x{c[2][1]}_C{c[4]}')
def test_resize_vs_fp64(eng, case):
    ac, (hin, win), (hout, wout), B, C, ldy, masked = case
    gen = torch.Generator().manual_seed(hin * 100 + hout + C)
    x = torch.randn(B, hin, win, C, generator=gen)
    gy = torch.randn(B, hout, wout, C, generator=gen)
    mask = (torch.randn(B, hin, win, C, generator=gen).clamp_min(0)) if masked else None
    yb = torch.full((B, hout, wout, ldy), float('nan'), device=DEV)
    yd = yb[..., ldy - C:]
    gyb = torch.zeros(B, hout, wout, ldy, device=DEV)
    gyb[..., ldy - C:] = gy.to(DEV)
    gx = torch.empty(B, hin, win, C, device=DEV)
    eng.test_resize(ac, x=x.to(DEV), y=yd, gy=gyb[..., ldy - C:], gx=gx, mask=mask.to(DEV) if masked else None)
    assert bool(yb[..., :ldy - C].isnan().all()), 'resize wrote outside its channel slice'
    y64, gx64 = _resize_ref(x, gy, mask, (hout, wout), ac, torch.float64)
    y32, gx32 = _resize_ref(x, gy, mask, (hout, wout), ac, torch.float32)
    if masked:
        assert bool((gx.cpu()[mask <= 0] == 0).all())
    _check(f'resize {case}', fwd=(yd.cpu(), y32, y64, 'resize_fwd'), bwd=(gx.cpu(), gx32, gx64, 'resize_bwd'))


# ---- ASPP image pooling and the head --------------------------------------------------------------------------------
def _pool_branch_ref(x, w, a, b, gy, dtype):
    """ASPPPooling: mean over pixels -> 1x1 conv (+ folded norm + ReLU) -> broadcast; the backward of the branch without its
    ReLU, given the (already masked) gradient gy of the broadcast output."""
    xx = x.to(dtype).requires_grad_(True)
    ww = w.to(dtype).requires_grad_(True)
    v = xx.mean(dim=1)
    t = v @ ww.t()
    if a is not None:
        t = t * a.to(dtype) + b.to(dtype)
    y = t.clamp_min(0) if a is not None else t
    t.unsqueeze(1).expand(-1, x.shape[1], -1).backward(gy.to(dtype))
    return v.detach(), y.detach(), xx.grad, ww.grad


@pytest.mark.parametrize('B,P,offset,folded', [(1, 2, 0.0, True), (3, 3, 50.0, True), (2, 77, 0.0, False),
                                               (3, 30 * 54, 100.0, True), (1, 30 * 54, 0.0, True), (3, 7 * 11, 20.0, False)])
def test_aspp_pool_vs_fp64(eng, B, P, offset, folded):
    Kc, N = 2048, 256
    gen = torch.Generator().manual_seed(P + B)
    x = (torch.randn(B, P, Kc, generator=gen) + offset).clamp_min(0)
    w = torch.randn(N, Kc, generator=gen) / Kc ** 0.5
    a = torch.rand(N, generator=gen) + 0.5 if folded else None
    b = torch.randn(N, generator=gen) * 0.5 if folded else None
    ldy = 1280
    yb = torch.full((B, P, ldy), float('nan'), device=DEV)
    yd = yb[:, :, 1024:1280]                        # the cat slice of the network
    m8 = torch.zeros(B, P, ldy // 4, dtype=torch.uint8, device=DEV)
    gy = torch.randn(B, P, N, generator=gen)
    # forward first: the backward's input gradient carries the ReLU mask of the GPU's own output (the consumer applies it)
    r = eng.test_aspp_pool(x.to(DEV), w.to(DEV), a.to(DEV) if folded else None, b.to(DEV) if folded else None, y=yd,
                           m8=m8[:, :, 1024 // 4:])
    ygpu = r['y'].cpu()
    gym = gy * (ygpu > 0) if folded else gy
    r = eng.test_aspp_pool(x.to(DEV), w.to(DEV), a.to(DEV) if folded else None, b.to(DEV) if folded else None, y=yd,
                           m8=m8[:, :, 1024 // 4:], gy=gym.to(DEV))
    assert bool(yb[:, :, :1024].isnan().all())
    assert torch.equal(m8[:, :, 1024 // 4:].cpu(), _relu_bits(ygpu))
    assert not bool(m8[:, :, :1024 // 4].any())
    v64, y64, gx64, dw64 = _pool_branch_ref(x, w, a, b, gym, torch.float64)
    v32, y32, gx32, dw32 = _pool_branch_ref(x, w, a, b, gym, torch.float32)
    assert torch.equal(ygpu, r['pool'].cpu().unsqueeze(1).expand(-1, P, -1))
    _check(f'aspp pool B{B} P{P} offset {offset} folded {folded}', v=(r['v'].cpu(), v32, v64, 'pool_fwd'),
           fwd=(r['pool'].cpu(), y32, y64, 'pool_fwd'),
           gx=(r['gx'].cpu(), gx32, gx64, 'pool_bwd'), dw=(r['dw'].cpu(), dw32, dw64, 'pool_dw'))


def _head_ref(x, w, b, g, dtype):
    xx = x.to(dtype).requires_grad_(True)
    ww = w.to(dtype).requires_grad_(True)
    bb = b.to(dtype).requires_grad_(True)
    y = xx @ ww + bb
    y.backward(g.to(dtype))
    return y.detach(), xx.grad * (xx.detach() > 0), torch.cat([ww.grad, bb.grad])


@pytest.mark.parametrize('B,hw', [(1, (120, 214)), (3, (120, 214)), (3, (25, 41)), (1, (7, 11)), (1, (1, 3))])
def test_head_vs_fp64(eng, B, hw):
    C = 256
    P = B * hw[0] * hw[1]
    gen = torch.Generator().manual_seed(P)
    x = torch.randn(P, C, generator=gen).clamp_min(0)                        # a ReLU output
    w = torch.randn(C, generator=gen) / C ** 0.5
    b = torch.randn(1, generator=gen)
    g = torch.randn(P, generator=gen) / P
    y, gx, dw = eng.test_head(x.to(DEV), w.to(DEV), b.to(DEV), g.to(DEV))
    y64, gx64, dw64 = _head_ref(x, w, b, g, torch.float64)
    y32, gx32, dw32 = _head_ref(x, w, b, g, torch.float32)
    assert bool((gx.cpu()[x <= 0] == 0).all())
    _check(f'head B{B} {hw}', fwd=(y.cpu(), y32, y64, 'head_fwd'), gx=(gx.cpu(), gx32, gx64, 'head_gx'),
           dw=(dw.cpu(), dw32, dw64, 'head_dw'))


# ---- losses -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def loss_eng():
    e = Engine('resnet50', 480, 854, max_batch=3, device=DEV)       # scratch for n up to 3 x 480 x 854
    yield e
    e.close()


def _loss_inputs(n, logit_scale, target, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=gen) * logit_scale
    if logit_scale >= 80:
        x = torch.where(torch.rand(n, generator=gen) > 0.5, 80.0, -80.0) * torch.rand(n, generator=gen).sqrt()
    t = {'zeros': torch.zeros(n), 'ones': torch.ones(n), 'mixed': (torch.rand(n, generator=gen) > 0.6).float()}[target]
    return x, t


LOSS_NAMES = ['cross_entropy', 'dice', 'cross_entropy_and_dice', 'class_balanced_cross_entropy']


def _oracle_loss(name, x, t, dtype):
    xx = x.to(dtype).view(1, 1, 1, -1).requires_grad_(True)
    l = deeplab.loss_fn(name, xx, t.to(dtype).view(1, 1, 1, -1))
    l.backward()
    return l.detach().view(1), xx.grad.view(-1)


@pytest.mark.parametrize('n', [1, 255, 257, 3 * 480 * 854])
@pytest.mark.parametrize('scale', [3.0, 80.0])
@pytest.mark.parametrize('target', ['zeros', 'ones', 'mixed'])
def test_losses_vs_fp64(loss_eng, n, scale, target):
    """Loss value of every kind and dlogits (BCE through eosvos_bce's caller buffer; the other kinds through the engine's
    gradient scratch, read back for n <= H * W) against the fp64 restatement in oracle/deeplab.py.
    Degenerate cases, asserted as the oracle gives them: class-balanced BCE with one class only is 0 with a zero gradient
    (the other class's count weights every term), and dice's +1 smoothing keeps all-zero targets finite."""
    e = loss_eng
    x, t = _loss_inputs(n, scale, target, seed=n + int(scale))
    xd, td = x.to(DEV), t.to(DEV)
    out = []
    for name in LOSS_NAMES:
        l64, d64 = _oracle_loss(name, x, t, torch.float64)
        l32, d32 = _oracle_loss(name, x, t, torch.float32)
        if name == 'cross_entropy':
            loss = torch.empty(1, device=DEV)
            dl = torch.empty(n, device=DEV)
            _ffi.check(e.lib.eosvos_bce(e.h, ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(td.data_ptr()), n,
                                        ctypes.c_void_p(loss.data_ptr()), ctypes.c_void_p(dl.data_ptr())))
            dl = dl.cpu()
        else:
            loss = e.loss_of(name, xd, td)
            dl = e.debug_tensor('dlogits').reshape(-1)[:n].cpu() if n <= 480 * 854 else None
        loss = loss.cpu()
        if name == 'class_balanced_cross_entropy' and target != 'mixed':
            assert float(l64) == 0.0 and float(loss) == 0.0
        out.append((name, loss, l32, l64, dl, d32, d64))
    for name, loss, l32, l64, dl, d32, d64 in out:
        parts = {'loss': (loss, l32, l64, 'loss')}
        if dl is not None:
            parts['dlogits'] = (dl, d32, d64, 'dlogits')
        _check(f'{name} n{n} scale {scale} {target}', **parts)


def test_bce_per_sample(loss_eng):
    """`batch_average: False`: eosvos_loss_tensors on each sample of a batch (run_loader's metrics)."""
    x, t = _loss_inputs(3 * 480 * 854, 6.0, 'mixed', seed=5)
    x, t = x.view(3, 1, 480, 854), t.view(3, 1, 480, 854)
    for name in LOSS_NAMES:
        ref64 = deeplab.loss_per_sample(name, x.double(), t.double())
        ref32 = deeplab.loss_per_sample(name, x, t)
        got = torch.cat([loss_eng.loss_of(name, x[b].to(DEV).contiguous(), t[b].to(DEV).contiguous()) for b in range(3)]).cpu()
        _check(f'per-sample {name}', loss=(got, ref32, ref64, 'loss'))


# ---- the plan fingerprint belongs to the engine's own passes ------------------------------------------------------
def test_plan_fingerprint_unaffected_by_other_engines():
    """Launches of a scratch engine (a test entry point) after another engine's forward must not mix into that engine's
    fingerprint, and an engine destroyed after its forward must not be written to afterwards."""
    from eosvos_amd import synthetic
    a = Engine('resnet50', 96, 160, max_batch=1, device=DEV)
    a.load_model_state(synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50'))
    x, _ = synthetic.synthetic_frames(1, 96, 160, seed=3)
    a.infer(x.to(DEV))
    torch.cuda.synchronize()
    before = a.plan_fingerprint()
    scratch = Engine('resnet50', 64, 64, max_batch=1, device=DEV)
    gen = torch.Generator().manual_seed(0)
    xs = torch.randn(1, 16, 16, 64, generator=gen).to(DEV)
    ws = torch.randn(64, 64, 3, 3, generator=gen).to(DEV)
    scratch.test_conv_algo('direct', xs, ws, None, None, None, False, 1, 1, 1)
    third = Engine('resnet50', 64, 64, max_batch=1, device=DEV)
    third.load_model_state(synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50'))
    third.infer(torch.zeros(1, 3, 64, 64, device=DEV))
    third.close()
    scratch.test_conv_algo('direct', xs, ws, None, None, None, False, 1, 1, 1)    # after a forward of a destroyed engine
    after = a.plan_fingerprint()
    scratch.close()
    a.close()
    print(f'MARGIN plan fingerprint before {before[0]:#x} after {after[0]:#x}')
    assert after == before
