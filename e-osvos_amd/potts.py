"""Image-aware pairwise (Potts) loss, `loss_func: potts[_<r>[x<d>]]`: the names, the window, and the numpy twin of the device
kernels (`csrc/potts_kernels.hip`).  Host only: importing this module needs neither torch nor the built library.

The relaxed Potts / dense-CRF regulariser evaluated as a loss on the prediction and the frame alone (Tang et al., "On
Regularized Losses for Weakly-supervised CNN Segmentation", ECCV 2018; the local-window form of Obukhov et al., "Gated CRF
Loss", 2019).  The rule (include/eosvos.h at EOSVOS_LOSS_POTTS), per image of H x W pixels, z the logits, p = sigmoid(z), I the
3-channel frame, window radius r, dilation d, N(i) the pixels i + d (dy, dx), dy, dx in [-r, r] without (0, 0), inside the frame:
    k_ij = exp(-d^2 (dy^2 + dx^2) / (2 sigma_xy^2)) exp(-|I_i - I_j|^2 / (2 sigma_rgb^2))
    S_i = sum_N k_ij;  M_i = sum_N k_ij p_j;  E = sum_i p_i (S_i - M_i);  Z = sum_i S_i
    image loss = E / Z (0 when Z = 0);  loss = the mean over the images;  dL/dz_i = (S_i - 2 M_i) p_i (1 - p_i) / (Z images)
It reads NO target: void pixels get its gradient like every other pixel, which is its purpose -- the void band of online
adaptation (`eval_online_adapt.min_prop: [lo, hi]`) trains on nothing else.  The defaults (r 3, d 2, sigma_xy = r d, sigma_rgb
0.1 in units of the frame's [0, 1] range: Obukhov's values rescaled) are untuned: no J&F figure exists for them, nor for any
weight of the term in a sum.  Out of scope: keeping k across the epochs of a round whose batch does not change, source and
destination gates, more than two classes."""
import math

import numpy as np

from .loss_names import (MAX_DILATION, MAX_HALO, MAX_WINDOW, POTTS as NAME, POTTS_KINDS as KINDS,  # noqa: F401  (the spelling's home)
                         check_window, parse_potts as parse, resolve_window)

DEFAULT_WINDOW, DEFAULT_DILATION, DEFAULT_SIGMA_RGB = 3, 2, 0.1
MAX_SIDE = 4096


def default_sigma_xy(window, dilation):
    """radius * dilation: the position kernel falls to exp(-1/2) at the window's edge along an axis."""
    return float(window * dilation)


def check_sigma(name, sigma):
    """A sigma as the float the library receives: finite and > 0 (as fp32 too)."""
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.floating, np.integer)):
        raise ValueError(f'{name}={sigma!r}: must be a number, finite and > 0')
    with np.errstate(over='ignore'):
        s = float(np.float32(sigma))
    if not (math.isfinite(s) and s > 0.0 and math.isfinite(float(sigma))):
        raise ValueError(f'{name}={sigma!r}: must be finite and > 0')
    return s


def _np(a):
    """A numpy array of a numpy array, a nested list or a torch tensor (any device)."""
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)


def _shift(a, oy, ox):
    """(the part of `a` (.., H, W) at i + (oy, ox) for the pixels i that have that neighbour, the slices of those pixels)."""
    h, w = a.shape[-2:]
    ny, nx = max(0, h - abs(oy)), max(0, w - abs(ox))        # how many rows / columns have the neighbour (0: an empty part)
    y0, x0 = max(0, -oy), max(0, -ox)
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    yn, xn = slice(y0 + oy, y0 + oy + ny) if ny else slice(0, 0), slice(x0 + ox, x0 + ox + nx) if nx else slice(0, 0)
    return a[..., yn, xn], (ys, xs)


def loss_host(logits, frames, window=DEFAULT_WINDOW, dilation=DEFAULT_DILATION, sigma_xy=None, sigma_rgb=DEFAULT_SIGMA_RGB,
              dtype=np.float64):
    """The rule on the host, one shifted-array pass per offset.  logits: (H, W) or (images, H, W); frames: (3, H, W) or
    (images, 3, H, W); returns (loss as a `dtype` scalar, the gradient of the logits' shape in `dtype`).  float32 follows the
    device step by step (its inputs, sigmas and table as fp32, the offsets in the device's order, the sigmoid from
    exp(-|z|)); float64 is the reference form."""
    dtype = np.dtype(dtype).type
    r, d = check_window(window, dilation)
    sigma_xy = default_sigma_xy(r, d) if sigma_xy is None else sigma_xy
    sxy, srgb = check_sigma('sigma_xy', sigma_xy), check_sigma('sigma_rgb', sigma_rgb)
    if dtype is np.float64:                                  # the reference form takes the sigmas as given
        sxy, srgb = float(sigma_xy), float(sigma_rgb)
    z, img = _np(logits), _np(frames)
    shape = z.shape
    if z.ndim == 2:
        z, img = z[None], img[None]
    if z.ndim != 3 or img.shape != (z.shape[0], 3) + z.shape[1:]:
        raise ValueError(f'potts: logits {shape} need frames (images, 3, H, W), got {img.shape}')
    if max(z.shape[1:]) > MAX_SIDE:
        raise ValueError(f'potts: frames larger than {MAX_SIDE} pixels a side are not supported')
    images = z.shape[0]
    z, img = z.astype(dtype), img.astype(dtype)
    inv_xy, inv_rgb = 1.0 / (2.0 * sxy * sxy), dtype(1.0 / (2.0 * srgb * srgb))
    with np.errstate(all='ignore'):
        e = np.exp(-np.abs(z))
        hi, lo = dtype(1) / (dtype(1) + e), e / (dtype(1) + e)        # sigmoid(|z|), sigmoid(-|z|)
        p = np.where(z >= 0, hi, np.where(z < 0, lo, z))              # (a NaN logit: p is that NaN)
        S, M = np.zeros_like(z), np.zeros_like(z)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dy == 0 and dx == 0:
                    continue
                pos = dtype(math.exp(-float((dy * d) ** 2 + (dx * d) ** 2) * inv_xy))
                nb, (ys, xs) = _shift(img, dy * d, dx * d)
                if nb.size == 0:
                    continue
                diff = img[..., ys, xs] - nb
                k = pos * np.exp(-(diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2]) * inv_rgb)
                S[:, ys, xs] += k
                M[:, ys, xs] += k * _shift(p, dy * d, dx * d)[0]
        loss, grad = dtype(0), np.zeros_like(z)
        for i in range(images):
            E, Z = (p[i] * (S[i] - M[i])).sum(dtype=dtype), S[i].sum(dtype=dtype)
            if Z != 0:
                loss = loss + E / Z
                grad[i] = ((S[i] - dtype(2) * M[i]) * (hi[i] * lo[i])) * (dtype(1) / (Z * dtype(images)))
        return dtype(loss / dtype(images)), grad.reshape(shape)
