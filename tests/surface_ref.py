"""The surface loss by its definition (include/eosvos.h at EOSVOS_LOSS_SURFACE), as plain loops over all pairs of pixels, in
integers and fp64: the reference of tests/test_surface_host.py for `eosvos_amd.surface`, and the targets both test files share.
A plain module like lovasz_ref.py."""
import math

import numpy as np

IGN = 255.0


def classes(y, ign):
    """0 void, 1 foreground, 2 background per pixel of an (H, W) array."""
    H, W = y.shape
    out = np.zeros((H, W), dtype=np.int64)
    for i in range(H):
        for j in range(W):
            if ign is not None and y[i, j] == ign:
                continue
            out[i, j] = 1 if y[i, j] >= 0.5 else 2
    return out


def distance_loops(y, cap, ign=None):
    """c of one (H, W) target: for every valid pixel the least squared distance over ALL pixels of the other class."""
    H, W = y.shape
    cls = classes(y, ign)
    src = {k: [(i, j) for i in range(H) for j in range(W) if cls[i, j] == k] for k in (1, 2)}
    c = np.zeros((H, W), dtype=np.int32)
    for i in range(H):
        for j in range(W):
            if cls[i, j] == 0:
                continue
            best = cap * cap + 1
            for (a, b) in src[3 - cls[i, j]]:
                best = min(best, (a - i) ** 2 + (b - j) ** 2)
            c[i, j] = best
    return c


def weights_loops(c, cap):
    """w in fp64 from c."""
    w = np.zeros(c.shape, dtype=np.float64)
    for idx in np.ndindex(*c.shape):
        w[idx] = (cap if c[idx] > cap * cap else math.sqrt(int(c[idx]))) / cap
    return w


def loss_loops(z, y, cap, ign=None):
    """(loss, dL/dz) in fp64 of (images, H, W) arrays by rules 1 - 4."""
    images, H, W = z.shape
    grad = np.zeros(z.shape, dtype=np.float64)
    total = 0.0
    for b in range(images):
        cls = classes(y[b], ign)
        w = weights_loops(distance_loops(y[b], cap, ign), cap)
        n = int((cls != 0).sum())
        if n == 0:
            continue
        s = 0.0
        for i in range(H):
            for j in range(W):
                if cls[i, j] == 0:
                    continue
                p = 1.0 / (1.0 + math.exp(-float(z[b, i, j])))
                s += w[i, j] * ((1.0 - p) if cls[i, j] == 1 else p)
                grad[b, i, j] = (-1.0 if cls[i, j] == 1 else 1.0) * w[i, j] * p * (1.0 - p) / (n * images)
        total += s / n
    return total / images, grad


# ---- the targets of both test files --------------------------------------------------------------------------------------
TARGETS = ('empty', 'full', 'all_void', 'corner', 'void_band', 'checkerboard', 'blob')


def target(kind, H, W, void):
    """One (H, W) float32 target.  `void`: every 7th pixel is void as well, plus a short block (where the kind is not about
    void pixels already)."""
    y = np.zeros((H, W), dtype=np.float32)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    if kind == 'full':
        y[:] = 1
    elif kind == 'all_void':
        y[:] = IGN
    elif kind == 'corner':
        y[0, 0] = 1
    elif kind == 'void_band':                   # two regions, a foreground and a background one, separated by a void band
        if W >= 3:
            y[:, :W // 3] = 1
            y[:, W // 3:max(W // 3 + 1, 2 * W // 3)] = IGN
        else:
            y[:H // 2] = 1
            y[H // 2:H // 2 + 1] = IGN
    elif kind == 'checkerboard':
        y[:] = (ii + jj) % 2
    elif kind == 'blob':                        # a centred ellipse and a far small square
        y[:] = (((ii - (H - 1) / 2) / max(H / 3.0, 1)) ** 2 + ((jj - (W - 1) / 2) / max(W / 4.0, 1)) ** 2) <= 1
        y[:max(1, H // 8), W - max(1, W // 10):] = 1
    if void and kind not in ('all_void', 'void_band'):
        y.reshape(-1)[3::7] = IGN
        y[H // 3:H // 3 + 2, min(30, W - 1):min(67, W)] = IGN
    return y


def uses_void(kind, void):
    return void or kind in ('all_void', 'void_band')
