"""Soft boundary-F loss, `loss_func: boundary_f[_<r>]` / `cross_entropy_and_boundary_f[_<r>]`: the names, the radius, and the
torch twin of the device kernels (`csrc/boundary_kernels.hip`, the rule of `include/eosvos.h` at EOSVOS_LOSS_BOUNDARY_F).

Bokhovkin & Burnaev, "Boundary Loss for Remote Sensing Imagery Semantic Segmentation" (2019): the soft form of the F measure.
Per image, z the logits, y the targets, V the valid (non-void) pixels; windows are square, centred, clipped to the frame and
range over valid pixels only:
  q = sigmoid(-z) (by the branch on the sign of z),  h = 1 - y
  pb = max_{3x3} q - q,  gb = max_{3x3} h - h;  pe = max_{(2r+1)^2} pb,  ge = max_{(2r+1)^2} gb;  all 0 at void pixels
  Sp = sum_V pb + eps, Sg = sum_V gb + eps, P = sum_V pb ge / Sp, R = sum_V pe gb / Sg, BF = 2PR / (P + R + eps), eps = 1e-7
  image loss = 1 - BF (0 without a valid pixel);  `boundary_f` = the mean over the images;  `cross_entropy_and_boundary_f` =
  the `cross_entropy` value over the same valid pixels + `boundary_f`, a plain sum.
Among equal maxima the first in row-major order takes the gradient (torch's CPU max_pool2d rule).  The radius is the tolerance
of the DAVIS F measure (`data.davis_bound_pix`); the default min(16, davis_bound_pix(0.008, H, W)) is untuned: no J&F figure
exists for it."""
import math

import torch
import torch.nn.functional as F

from .loss_names import (BOUNDARY_COMBINED as COMBINED, BOUNDARY_F as NAME, BOUNDARY_KINDS as KINDS,  # noqa: F401
                         MAX_RADIUS, check_radius, parse_boundary as parse)                          # (the spelling's home)

EPS = 1e-7


def default_radius(height, width):
    """min(16, davis_bound_pix(0.008, H, W)): 8 at 480 x 854."""
    return max(1, min(MAX_RADIUS, int(math.ceil(0.008 * math.sqrt(float(height) ** 2 + float(width) ** 2)))))


def _pool(x, valid, r):
    """The (2r+1)^2 maximum over the valid pixels of each clipped window; x: (B, 1, H, W)."""
    return F.max_pool2d(torch.where(valid, x, torch.full_like(x, -math.inf)), 2 * r + 1, stride=1, padding=r)


def image_losses(logits, targets, radius, ignore=None):
    """1 - BF per image, in the dtype of `logits` ((B, H, W)), differentiable by autograd.  One source for every precision."""
    z, y = logits.unsqueeze(1), targets.unsqueeze(1)
    valid = torch.ones_like(y, dtype=torch.bool) if ignore is None else y != ignore
    zero = torch.zeros_like(z)
    e = torch.exp(-z.abs())
    q = torch.where(z >= 0, e / (1 + e), 1 / (1 + e))
    h = 1 - y
    pb = torch.where(valid, _pool(q, valid, 1) - q, zero)
    gb = torch.where(valid, _pool(h, valid, 1) - h, zero)
    pe = torch.where(valid, _pool(pb, valid, radius), zero)
    ge = torch.where(valid, _pool(gb, valid, radius), zero)
    sp, sg = pb.sum((1, 2, 3)) + EPS, gb.sum((1, 2, 3)) + EPS
    p, r = (pb * ge).sum((1, 2, 3)) / sp, (pe * gb).sum((1, 2, 3)) / sg
    loss = 1 - 2 * p * r / (p + r + EPS)
    return torch.where(valid.flatten(1).any(1), loss, torch.zeros_like(loss))


def loss_host(logits, targets, radius, ignore=None, dtype=torch.float64, combined=False):
    """The torch twin on the CPU.  logits / targets: (B, H, W) or (H, W); returns (loss, gradient of the logits' shape, the
    per-image boundary losses), all in `dtype`; the gradient is autograd's.  `combined`: `cross_entropy_and_boundary_f`."""
    radius = check_radius(radius)
    z = torch.as_tensor(logits).detach().to('cpu', torch.float32)
    y = torch.as_tensor(targets).detach().to('cpu', torch.float32)
    shape = z.shape
    if z.dim() == 2:
        z, y = z[None], y[None]
    if ignore is not None:
        z = torch.where(y != ignore, z, torch.zeros_like(z))      # a void logit never reaches the result (it may be NaN / inf)
    z = z.to(dtype).requires_grad_(True)
    y = y.to(dtype)
    per = image_losses(z, y, radius, ignore)
    loss = per.mean()
    if combined:
        valid = torch.ones_like(y, dtype=torch.bool) if ignore is None else y != ignore
        bce = torch.clamp(z, min=0) - z * y + torch.log1p(torch.exp(-z.abs()))
        n = int(valid.sum())
        if n:
            loss = loss + torch.where(valid, bce, torch.zeros_like(bce)).sum() / n
    grad, = torch.autograd.grad(loss, z)
    return loss.detach(), grad.reshape(shape), per.detach()
