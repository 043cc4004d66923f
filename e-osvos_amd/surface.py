"""Distance-weighted surface loss, `loss_func: surface[_<L>]`: the names, the cap, and the numpy twins of the device kernels
(`csrc/surface_kernels.hip`, the rule of `include/eosvos.h` at EOSVOS_LOSS_SURFACE).  Host only: numpy, no torch, no library.

Kervadec et al., "Boundary loss for highly unbalanced segmentation" (MIDL 2019): every pixel's error is weighted by its
distance to the target's boundary, so a confident blob far from the object costs more than the same blob beside the contour.
It is meant as a term beside a region loss (`dice+0.5*surface_64`).  Per image of H x W, z the logits, y the targets, v the
void label, L the cap (a whole number of pixels, 1 .. 4095):
  V = {y != v},  F = {i in V : y_i >= 0.5},  B = V \\ F;  a void pixel is in neither set and never a source of a distance
  1. D2_i = the least dy^2 + dx^2 to a pixel of the other class (infinite if that class is empty);  c_i = min(D2_i, L^2 + 1)
     as int32;  c_i = 0 at a void pixel
  2. d_i = L if c_i > L^2 else sqrt(float32(c_i));  w_i = d_i / float32(L): correctly rounded fp32, in (0, 1] on V
  3. p = sigmoid(z);  e_i = 1 - p_i on F, p_i on B;  image loss = sum_V w e / |V| (0 without a valid pixel);  `surface` = the
     mean over the images
  4. dL/dz_i = s_i w_i p_i (1 - p_i) / (|V| images), s = -1 on F, +1 on B;  exactly +0 at a void pixel
An empty target gives w = 1 everywhere and the loss is the mean foreground probability: the cap's benefit, no special case.
The default cap max(1, min(H, W) // 4) is untuned: no J&F figure exists for it, nor for any weight of the term in a sum.
Out of scope: keeping the transform across the epochs of an adaptation round whose targets do not change; the Hausdorff loss,
which also transforms the prediction; metrics other than the Euclidean one."""
import numpy as np

from .loss_names import (MAX_CAP, SURFACE as NAME, SURFACE_KINDS as KINDS, check_cap,  # noqa: F401  (the spelling's home)
                         parse_surface as parse, resolve_cap)

_FAR = np.int64(1) << 40                     # "no pixel of that class": beyond every capped distance, its square still an int64


def default_cap(height, width):
    """max(1, min(H, W) // 4), at most 4095: 120 at 480 x 854."""
    return min(MAX_CAP, max(1, min(int(height), int(width)) // 4))


def _np(a):
    """A numpy array of a numpy array, a nested list or a torch tensor (any device)."""
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)


def _images(a):
    """(the array as (images, H, W), its own shape)."""
    a = _np(a)
    if a.ndim not in (2, 3):
        raise ValueError(f'surface: maps must be (H, W) or (images, H, W), got {a.shape}')
    return (a[None] if a.ndim == 2 else a), a.shape


def classes(masks, ignore=None):
    """(valid, foreground, background) boolean maps of rule 0; a NaN target is background."""
    y = _np(masks)
    valid = np.ones(y.shape, dtype=bool) if ignore is None else y != np.float32(ignore)
    with np.errstate(invalid='ignore'):
        fg = valid & (y >= 0.5)
    return valid, fg, valid & ~fg


def _vertical(seeds):
    """Per pixel the distance to the nearest seed of its column (_FAR without one): (H, W) bool -> int64."""
    h = seeds.shape[0]
    g = np.full(seeds.shape, _FAR, dtype=np.int64)
    run = np.full(seeds.shape[1], _FAR, dtype=np.int64)
    for y in range(h):
        run = np.where(seeds[y], 0, np.minimum(run + 1, _FAR))
        g[y] = run
    run = np.full(seeds.shape[1], _FAR, dtype=np.int64)
    for y in range(h - 1, -1, -1):
        run = np.where(seeds[y], 0, np.minimum(run + 1, _FAR))
        g[y] = np.minimum(g[y], run)
    return g


def _distance_sq(seeds, limit2):
    """min(D^2 to the nearest seed, limit2) of one (H, W) map, exactly: the vertical distances, then per row the lower
    envelope over all columns."""
    g2 = np.minimum(_vertical(seeds), 1 << 20) ** 2                  # (2^20)^2 = 2^40: still "none", and no overflow below
    w = seeds.shape[1]
    dx2 = (np.arange(w, dtype=np.int64)[:, None] - np.arange(w, dtype=np.int64)[None, :]) ** 2
    out = np.empty(seeds.shape, dtype=np.int64)
    for y in range(seeds.shape[0]):
        out[y] = (dx2 + g2[y][None, :]).min(axis=1)
    return np.minimum(out, limit2)


def distance_host(masks, cap, ignore=None):
    """Rule 1: c of (H, W) or (images, H, W) targets, int32 of the same shape."""
    cap = check_cap(cap)
    y, shape = _images(masks)
    valid, fg, bg = classes(y, ignore)
    limit2 = cap * cap + 1
    c = np.zeros(y.shape, dtype=np.int32)
    for i in range(y.shape[0]):
        to_fg, to_bg = _distance_sq(fg[i], limit2), _distance_sq(bg[i], limit2)
        c[i] = np.where(fg[i], to_bg, np.where(bg[i], to_fg, 0)).astype(np.int32)
    return c.reshape(shape)


def weights_host(c, cap, dtype=np.float32):
    """Rule 2 from c.  float32 (the default) reproduces the device's w bit for bit; float64 is the reference form."""
    cap = check_cap(cap)
    c = _np(c)
    lf = dtype(cap)
    return (np.where(c > cap * cap, lf, np.sqrt(c.astype(dtype))) / lf).astype(dtype, copy=False)


def loss_host(logits, masks, cap, ignore=None, dtype=np.float64):
    """Rules 1 - 4 on the host.  logits / masks: (H, W) or (images, H, W); returns (loss as a `dtype` scalar, the gradient of
    the logits' shape in `dtype`).  The sigmoid is formed from exp(-|z|) without a cancellation, as on the device; a void
    pixel's logit never reaches the result (it may be NaN / inf)."""
    dtype = np.dtype(dtype).type
    z, shape = _images(logits)
    y, _ = _images(masks)
    if z.shape != y.shape:
        raise ValueError(f'surface: logits {z.shape} and masks {y.shape} differ in shape')
    valid, fg, _ = classes(y, ignore)
    w = weights_host(distance_host(y, cap, ignore), cap, dtype)
    images = z.shape[0]
    z = np.where(valid, z, 0).astype(dtype)
    e = np.exp(-np.abs(z))
    hi, lo = dtype(1) / (dtype(1) + e), e / (dtype(1) + e)            # sigmoid(|z|), sigmoid(-|z|)
    err = np.where((z >= 0) == fg, lo, hi)                            # 1 - p on F, p on B
    n = valid.reshape(images, -1).sum(axis=1)
    loss, grad = dtype(0), np.zeros(z.shape, dtype=dtype)
    for i in range(images):
        if n[i]:
            loss = loss + (w[i] * err[i])[valid[i]].sum(dtype=dtype) / dtype(n[i])
            g = w[i] * (hi[i] * lo[i]) / (dtype(n[i]) * dtype(images))
            grad[i] = np.where(valid[i], np.where(fg[i], -g, g), dtype(0))
    return dtype(loss / dtype(images)), grad.reshape(shape)
