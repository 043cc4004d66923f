"""Topology-aware centreline loss, `loss_func: cldice[_<k>]`: the names, the depth, and the numpy twins of the device kernels
(`csrc/cldice_kernels.hip`, the rule of `include/eosvos.h` at EOSVOS_LOSS_CLDICE).  Host only: numpy, no torch, no library.

The soft centreline Dice of Shit et al., "clDice -- a Novel Topology-Preserving Loss Function for Tubular Structure
Segmentation" (CVPR 2021): a differentiable skeleton by iterated min / max pooling, and how much of each map's skeleton lies
inside the other map.  A cut through a thin part removes skeleton, shaving a blob's edge does not, so the first costs far more
than the second at the same `dice`.  It is meant as a term beside a region loss (`dice+0.5*cldice_5`).  Per image of H x W, z
the logits, y the targets in [0, 1], V the valid pixels (y != the void label), p = sigmoid(z); every window is clipped to the
frame and ranges over pixels of V only.  For x_0 = x (p, or y) and the levels j = 0 .. k (k = the depth):
    v_j(i) = the first minimum of x_j over (up, centre, down);   h_j(i) = the first minimum over (left, centre, right)
    x_{j+1}(i) = min(v_j, h_j);   o_j(i) = the first maximum of x_{j+1} over the 3 x 3 window in row-major order
    d_j(i) = max(x_j(i) - o_j(i), 0);   u = 1, u <- u (1 - d_j) for j = 0 .. k;   S(x) = 1 - u
    Tp = (sum_V S(p) y + 1) / (sum_V S(p) + 1);   Ts = (sum_V S(y) p + 1) / (sum_V S(y) + 1)
    image loss = 1 - 2 Tp Ts / (Tp + Ts), 0 without a valid pixel;   `cldice` = the mean over the images
The gradient follows the selections (torch's CPU rules for the published `-max_pool2d(-x)` / `torch.min` / `max_pool2d`): a
window routes to its first extremum in row-major order, min(v, h) to v's pixel if v < h, to h's if h < v, half to each if
v = h.  S(y) carries none; a void pixel gets exactly +0.  The default depth clamp((min(H, W) + 48) // 96, 1, 16) is untuned: no
J&F figure exists for it, nor for any weight of the term in a sum.  Out of scope: keeping S(y) across the epochs of an
adaptation round whose targets do not change, 3-D, more than two classes."""
import numpy as np

from .loss_names import (CLDICE as NAME, CLDICE_KINDS as KINDS, MAX_DEPTH, check_depth,  # noqa: F401  (the spelling's home)
                         parse_cldice as parse, resolve_depth)

MAX_SIDE = 4096


def default_depth(height, width):
    """clamp((min(H, W) + 48) // 96, 1, 16): 5 at 480 x 854.  Untuned."""
    return min(MAX_DEPTH, max(1, (min(int(height), int(width)) + 48) // 96))


def _np(a):
    """A numpy array of a numpy array, a nested list or a torch tensor (any device)."""
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)


def _images(a):
    """(the array as (images, H, W), its own shape)."""
    a = _np(a)
    if a.ndim not in (2, 3):
        raise ValueError(f'cldice: maps must be (H, W) or (images, H, W), got {a.shape}')
    return (a[None] if a.ndim == 2 else a), a.shape


def _shift(a, dy, dx, fill):
    """b(y, x) = a(y + dy, x + dx), `fill` outside the frame; a is (images, H, W)."""
    h, w = a.shape[1:]
    b = np.full(a.shape, fill, dtype=a.dtype)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    b[:, yd, xd] = a[:, ys, xs]
    return b


def _first(a, offsets, fill, better):
    """(the first extremum of `a` over the window `offsets` in their order, its index in `offsets`): starting from `fill`,
    a candidate replaces the value only when it is strictly `better`.  The index starts out as the centre's."""
    m = np.full(a.shape, fill, dtype=a.dtype)
    arg = np.full(a.shape, offsets.index((0, 0)), dtype=np.int8)
    for n, (dy, dx) in enumerate(offsets):
        c = _shift(a, dy, dx, fill)
        take = better(c, m)
        m = np.where(take, c, m)
        arg = np.where(take, np.int8(n), arg)
    return m, arg


VERTICAL = ((-1, 0), (0, 0), (1, 0))
HORIZONTAL = ((0, -1), (0, 0), (0, 1))
SQUARE = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
CROSS = ((-1, 0), (0, -1), (0, 0), (0, 1), (1, 0))            # the pixels whose vertical or horizontal window holds the centre


def _level(x, valid):
    """One level of the chain on (images, H, W): (x_{j+1}, d_j, the vertical arg, the horizontal arg, which of v / h / both won
    as 0 / 1 / 2, the dilation arg).  Void pixels: x_{j+1} = 0, d = 0; their args are never followed."""
    dtype = x.dtype.type
    with np.errstate(invalid='ignore'):
        lo = np.where(valid, x, dtype(np.inf))
        v, av = _first(lo, VERTICAL, dtype(np.inf), np.less)
        h, ah = _first(lo, HORIZONTAL, dtype(np.inf), np.less)
        which = np.where(v < h, np.int8(0), np.where(h < v, np.int8(1), np.int8(2)))
        nxt = np.where(valid, np.where(which == 1, h, v), dtype(0))
        o, ad = _first(np.where(valid, nxt, dtype(-np.inf)), SQUARE, dtype(-np.inf), np.greater)
        t = x - o
        d = np.where(valid & (t > 0), t, dtype(0))
    return nxt, d, av, ah, which, ad


def _chain(x, valid, depth):
    """All levels: (S, the list of d_j, the list of (av, ah, which, ad))."""
    dtype = x.dtype.type
    u = np.ones(x.shape, dtype=x.dtype)
    ds, routes = [], []
    for _ in range(depth + 1):
        x, d, av, ah, which, ad = _level(x, valid)
        u = u * (dtype(1) - d)
        ds.append(d)
        routes.append((av, ah, which, ad))
    return np.where(valid, dtype(1) - u, dtype(0)), ds, routes


def _valid(y, ignore):
    return np.ones(y.shape, dtype=bool) if ignore is None else y != np.float32(ignore)


def skeleton_host(maps, depth, ignore=None, masks=None, dtype=np.float32):
    """S of maps in [0, 1], (H, W) or (images, H, W), in `dtype`; 0 at void pixels, which are where `masks` (the maps
    themselves without `masks`) equal `ignore`.  float32 (the default) reproduces the device's planes bit for bit."""
    depth = check_depth(depth)
    dtype = np.dtype(dtype).type
    x, shape = _images(maps)
    valid = _valid(x if masks is None else _images(masks)[0], ignore)
    return _chain(np.where(valid, x, 0).astype(dtype), valid, depth)[0].reshape(shape)


def sigmoid_host(z, dtype):
    """(p, p (1 - p)) from exp(-|z|) with the branch on the sign, as on the device."""
    e = np.exp(-np.abs(z))
    hi, lo = dtype(1) / (dtype(1) + e), e / (dtype(1) + e)
    return np.where(z >= 0, hi, lo), hi * lo


def coefficients(sums, dtype):
    """(the image loss, Tp, dL/dTp / Bq, dL/dTs / Sy) from (sum S(p) y, sum S(p), sum S(y) p, sum S(y)), all in `dtype`."""
    a, b, c, d = sums
    one, two = dtype(1), dtype(2)
    bq, sy = b + one, d + one
    tp, ts = (a + one) / bq, (c + one) / sy
    den = tp + ts
    return one - two * tp * ts / den, tp, -two * ts * ts / (den * den) / bq, -two * tp * tp / (den * den) / sy


def backward_host(gs, ds, routes, valid):
    """T_0 = dL/dx_0 of one chain from g_S = dL/dS, by the gathers of the rule: (images, H, W) arrays in the dtype of `gs`."""
    dtype = gs.dtype.type
    zero = dtype(0)
    k1 = len(ds)
    gd = []
    for j in range(k1):
        e = np.ones(gs.shape, dtype=gs.dtype)
        for m in range(k1):
            if m != j:
                e = e * (dtype(1) - ds[m])
        gd.append(np.where(ds[j] > 0, gs * e, zero))

    def dilation_gather(t, j):                       # t - sum over the 3 x 3 pixels i whose arg o_j is this pixel, row-major
        ad = np.where(valid, routes[j][3], np.int8(-1))
        for n, (dy, dx) in enumerate(SQUARE):
            hit = _shift(ad, dy, dx, np.int8(-1)) == 8 - n
            t = t - np.where(hit, _shift(gd[j], dy, dx, zero), zero)
        return t

    t = dilation_gather(np.zeros(gs.shape, dtype=gs.dtype), k1 - 1)          # T_{k+1}
    for j in range(k1 - 1, -1, -1):
        av, ah, which, _ = routes[j]
        wv = np.where(valid, np.where(which == 0, dtype(1), np.where(which == 2, dtype(0.5), zero)), zero)
        wh = np.where(valid, np.where(which == 1, dtype(1), np.where(which == 2, dtype(0.5), zero)), zero)
        nt = gd[j]
        for dy, dx in CROSS:                         # the pixel i = q + (dy, dx) routes to q through its own window
            w = np.zeros(gs.shape, dtype=gs.dtype)
            if dx == 0:
                w = w + np.where(_shift(av, dy, dx, np.int8(-1)) == 1 - dy, _shift(wv, dy, dx, zero), zero)
            if dy == 0:
                w = w + np.where(_shift(ah, dy, dx, np.int8(-1)) == 1 - dx, _shift(wh, dy, dx, zero), zero)
            nt = nt + w * _shift(t, dy, dx, zero)
        if j >= 1:
            nt = dilation_gather(nt, j - 1)
        t = np.where(valid, nt, zero)
    return t


def loss_host(logits, masks, depth, ignore=None, dtype=np.float64):
    """The whole rule on the host.  logits / masks: (H, W) or (images, H, W); returns (loss as a `dtype` scalar, the gradient of
    the logits' shape in `dtype`).  Every intermediate stays in `dtype`; a void pixel's logit never reaches the result."""
    depth = check_depth(depth)
    dtype = np.dtype(dtype).type
    z, shape = _images(logits)
    y, _ = _images(masks)
    if z.shape != y.shape:
        raise ValueError(f'cldice: logits {z.shape} and masks {y.shape} differ in shape')
    valid = _valid(y, ignore)
    images = z.shape[0]
    with np.errstate(invalid='ignore'):
        z = np.where(valid, z, 0).astype(dtype)
        y = np.where(valid, y, 0).astype(dtype)
        p, pq = sigmoid_host(z, dtype)
        sp, ds, routes = _chain(p, valid, depth)
        sy = _chain(y, valid, depth)[0]
        loss = dtype(0)
        gs, cs = np.zeros(z.shape, dtype=dtype), np.zeros(z.shape, dtype=dtype)
        for i in range(images):
            m = valid[i]
            if not m.any():
                continue
            sums = [a[m].sum(dtype=dtype) for a in (sp[i] * y[i], sp[i], sy[i] * p[i], sy[i])]
            li, tp, c1, c2 = coefficients(sums, dtype)
            loss = loss + li
            gs[i] = np.where(m, c1 * (y[i] - tp), dtype(0))
            cs[i] = np.where(m, c2 * sy[i], dtype(0))
        t0 = backward_host(gs, ds, routes, valid)
        grad = np.where(valid, (t0 + cs) * pq / dtype(images), dtype(0))
    return dtype(loss / dtype(images)), grad.astype(dtype, copy=False).reshape(shape)
