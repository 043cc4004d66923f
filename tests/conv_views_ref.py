"""fp64 torch references of the convolution forms the engine's passes launch (tests/test_gpu_conv_views.py compares the HIP
kernels with them; tests/test_conv_views_host.py checks the composition formulas against autograd on the CPU).

Tensors are NHWC like the engine's; `a` / `b` are the folded frozen-norm scale / shift per output channel (None: 1 / 0).
Engine gradients are taken w.r.t. the post-norm, pre-ReLU output of a conv, so a data gradient contracts a * g.

Mask bytes: one byte per 4 channels, bit j of byte q of a pixel = (channel 4q + j of the activation > 0); bits 4..7 are zero.
"""
import torch
import torch.nn.functional as F

nchw = lambda t: t.permute(0, 3, 1, 2)
nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()


def pack_bits(mask):
    """bool (..., C) -> uint8 (..., C / 4)."""
    m = mask.to(torch.uint8).reshape(*mask.shape[:-1], -1, 4)
    return (m[..., 0] | (m[..., 1] << 1) | (m[..., 2] << 2) | (m[..., 3] << 3)).contiguous()


def unpack_bits(m8):
    """uint8 (..., C / 4) -> bool (..., C): only bits 0..3 count."""
    j = torch.arange(4, dtype=torch.uint8, device=m8.device)
    return ((m8.unsqueeze(-1) >> j) & 1).bool().reshape(*m8.shape[:-1], -1)


def relu_bytes(y):
    """The bytes a ReLU writer must leave for the activation y (..., C)."""
    return pack_bits(y > 0)


def _chan(v, n):
    return torch.ones(n, dtype=torch.float64) if v is None else v.double()


def fwd_ref(x, w, a, b, stride, dil, pad, res=None, relu=False):
    """relu?(a * conv(x, w) + b (+ res)), NHWC fp64."""
    y = F.conv2d(nchw(x.double()), w.double(), None, stride, pad, dil)
    y = y * _chan(a, w.shape[0]).view(1, -1, 1, 1)
    if b is not None:
        y = y + b.double().view(1, -1, 1, 1)
    y = nhwc(y)
    if res is not None:
        y = y + res.double()
    return F.relu(y) if relu else y


def dgrad_ref(g, w, a, in_hw, stride, dil, pad, gx0=None, add=None, m8=None, mask_c0=0):
    """gx = M * ((gx0 or 0) + (add or 0) + dgrad(a * g)); M = bits of m8 for channels >= mask_c0, 1 below (m8 None: 1)."""
    B = g.shape[0]
    Cout, Cin = w.shape[0], w.shape[1]
    ga = nchw(g.double()) * _chan(a, Cout).view(1, -1, 1, 1)
    gx = nhwc(torch.nn.grad.conv2d_input((B, Cin, in_hw[0], in_hw[1]), w.double(), ga, stride, pad, dil))
    if gx0 is not None:
        gx = gx + gx0.double()
    if add is not None:
        gx = gx + add.double()
    if m8 is not None:
        M = unpack_bits(m8)
        M[..., :mask_c0] = True
        gx = gx * M
    return gx


def wgrad_ref(g, x, wshape, a, stride, dil, pad):
    """dw [Cout][Cin][k][k] = a * wgrad(g, x)."""
    ga = nchw(g.double()) * _chan(a, wshape[0]).view(1, -1, 1, 1)
    return torch.nn.grad.conv2d_weight(nchw(x.double()), tuple(wshape), ga, stride, pad, dil)


def _rows(t, dtype):
    return t.to(dtype).reshape(-1, t.shape[-1])


def fwd_ref_mm(x, w, a, b, res=None, relu=False, dtype=torch.float64):
    """fwd_ref of a 1x1 stride-1 unpadded conv as ONE matrix product [pixels x Cin] [Cin x Cout], computed in `dtype` on the
    device the operands live on (long reductions over many pixels, where torch's CPU fp64 convolution is slow; with
    dtype = float32: the plain single-precision evaluation of the same op that an error bound can be taken from)."""
    Co, Ci = w.shape[:2]
    y = _rows(x, dtype) @ w.to(dtype).reshape(Co, Ci).t()
    if a is not None:
        y = y * a.to(dtype)
    if b is not None:
        y = y + b.to(dtype)
    if res is not None:
        y = y + _rows(res, dtype)
    return (F.relu(y) if relu else y).reshape(*x.shape[:-1], Co)


def dgrad_ref_mm(g, w, a, m8=None, mask_c0=0, dtype=torch.float64):
    """dgrad_ref (no initial contents, no added tensor) of a 1x1 stride-1 unpadded conv: M * ((a * g) [pixels x Cout] w [Cout x Cin])."""
    Co, Ci = w.shape[:2]
    ga = _rows(g, dtype) if a is None else _rows(g, dtype) * a.to(dtype)
    gx = (ga @ w.to(dtype).reshape(Co, Ci)).reshape(*g.shape[:-1], Ci)
    if m8 is not None:
        M = unpack_bits(m8)
        M[..., :mask_c0] = True
        gx = gx * M
    return gx


def wgrad_ref_mm(g, x, a, dtype=torch.float64):
    """wgrad_ref of a 1x1 stride-1 unpadded conv: dw [Cout][Cin][1][1] = (a * g)^T [Cout x pixels] x [pixels x Cin]."""
    ga = _rows(g, dtype) if a is None else _rows(g, dtype) * a.to(dtype)
    return (ga.t() @ _rows(x, dtype)).reshape(g.shape[-1], x.shape[-1], 1, 1)


def dgrad_taps_ref(g, w, a, d):
    """dgrad(a * g) of a stride-1 conv with padding = d * (k // 2), tap by tap: pixel (y, x) of g reaches input pixel
    (y + dy, x + dx), (dy, dx) = ((ky, kx) - k // 2) * d, through w[:, :, ky, kx] -- one fp64 matrix product per tap, on the
    device the operands live on (the ASPP's 2048 input channels make torch's CPU fp64 convolution slow)."""
    B, h, w_, Co = g.shape
    k = w.shape[-1]
    ga = g.double() * (1.0 if a is None else a.double().to(g.device))
    wd = w.double().to(g.device)
    out = torch.zeros(B, h, w_, w.shape[1], dtype=torch.float64, device=g.device)
    for ky in range(k):
        for kx in range(k):
            dy, dx = (ky - k // 2) * d, (kx - k // 2) * d
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w_, w_ - dx)
            if y0 < y1 and x0 < x1:
                out[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx] += ga[:, y0:y1, x0:x1] @ wd[:, :, ky, kx]
    return out


def aspp_dgrad_ref(g_cat, ws, scales, g_l4_0, m8, dils=(1, 6, 12, 18)):
    """g_l4 = M * (g_l4_0 + sum_i dgrad_i(a_i * g_cat[..., 256 i : 256 i + 256])): branch 0 is the 1x1 conv, the others 3x3 with
    padding = dilation dils[i]; channels past 256 * len(ws) of g_cat (the pooling branch) take no part."""
    acc = g_l4_0.double().clone()
    for i, (wi, ai) in enumerate(zip(ws, scales)):
        acc = acc + dgrad_taps_ref(g_cat[..., 256 * i:256 * i + wi.shape[0]], wi, ai, dils[i] if wi.shape[-1] == 3 else 1)
    return acc * unpack_bits(m8).to(acc.device)


def tile_keeps_tap(B, h, w, d, ky, kx, tile, rows=128):
    """Does the 128-pixel row tile `tile` of the (B, h, w) map, pixels taken in NHW order across the images, hold a pixel
    whose tap (ky, kx) of a 3x3 filter with dilation = padding = d lands inside its image?  (The merged ASPP launch keeps a tap
    for a tile exactly then; all other taps of the tile are skipped.)"""
    P = B * h * w
    for p in range(tile * rows, min((tile + 1) * rows, P)):
        y, x = (p % (h * w)) // w, p % w
        if 0 <= y + (ky - 1) * d < h and 0 <= x + (kx - 1) * d < w:
            return True
    return False


def tap_coverage(B, h, w, d):
    """{(ky, kx): (tiles that keep the tap, tiles that drop it)} for the vertical off-centre taps (kx = 1, ky = 0 / 2)."""
    ntile = (B * h * w + 127) // 128
    out = {}
    for ky in (0, 2):
        keep = [t for t in range(ntile) if tile_keeps_tap(B, h, w, d, ky, 1, t)]
        out[(ky, 1)] = (keep, [t for t in range(ntile) if t not in keep])
    return out


# The engines of the merged-ASPP cases of tests/test_gpu_conv_views.py: name -> (frame H, W, max_batch, batches run, dilations
# whose vertical off-centre taps some 128-pixel tile keeps AND another drops -- checked by tests/test_conv_views_host.py).
#   main:  21 x 38 map.  f16x3 merged at batch 2 then 1.  In the bf16x6 / fp32 modes the d = 6 branch of this size runs F(2,3)
#          (wino_on: B * h * w / 4 * 2048 * 256 >= 1e8, i.e. B * h * w >= 764), where the merged launch declines.
#   low:   21 x 18 map, 2 * 378 = 756 pixels: below that threshold at batch 2, so bf16x6 runs merged at batch 2 (a tile across
#          the image boundary) and then batch 1.  With h >= 21 rows and B * h * w < 764 at batch 2 a row has <= 18 pixels, a tile
#          spans >= 7 rows, and no tile can lie wholly inside rows 0..5 or 15..20: the d = 6 vertical taps are kept by EVERY
#          tile of such a map (d = 12 and 18 are kept by some and dropped by others).
#   small: 21 x 22 map, batch 1 (462 pixels): bf16x6 merged with tiles that drop the d = 6 vertical taps.
ASPP_ENGINES = {
    'main': (336, 608, 2, (2, 1), (6, 12, 18)),
    'low': (336, 288, 2, (2, 1), (12, 18)),
    'small': (336, 352, 1, (1,), (6, 12, 18)),
}


def aspp_map(name):
    """(h16, w16) of the engine `name`: two stride-2 stages by the stem and pooling, two by layer2 / layer3 (ceil each)."""
    H, W = ASPP_ENGINES[name][:2]
    for _ in range(4):
        H, W = (H + 1) // 2, (W + 1) // 2
    return H, W
