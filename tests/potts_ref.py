"""The pairwise (Potts) loss of include/eosvos.h (EOSVOS_LOSS_POTTS) written as plain per-pixel, per-neighbour loops in
float64: what `eosvos_amd.potts.loss_host` (one shifted-array pass per offset) is held to by tests/test_potts_host.py.  A
plain module like surface_ref.py; also the inputs the potts tests share."""
import math

import numpy as np


def loops(logits, frames, r, d, sigma_xy, sigma_rgb):
    """logits (images, H, W), frames (images, 3, H, W) -> (E per image, Z per image, loss, gradient), all float64."""
    z = np.asarray(logits, dtype=np.float64)
    img = np.asarray(frames, dtype=np.float64)
    images, H, W = z.shape
    with np.errstate(over='ignore'):
        p, q = 1.0 / (1.0 + np.exp(-z)), 1.0 / (1.0 + np.exp(z))     # q = 1 - p without the cancellation
    E, Z = np.zeros(images), np.zeros(images)
    S, M = np.zeros_like(z), np.zeros_like(z)
    for b in range(images):
        for y in range(H):
            for x in range(W):
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        yy, xx = y + d * dy, x + d * dx
                        if (dy == 0 and dx == 0) or not (0 <= yy < H and 0 <= xx < W):
                            continue
                        di = img[b, :, y, x] - img[b, :, yy, xx]
                        k = math.exp(-d * d * (dy * dy + dx * dx) / (2.0 * sigma_xy ** 2)) \
                            * math.exp(-float(di @ di) / (2.0 * sigma_rgb ** 2))
                        S[b, y, x] += k
                        M[b, y, x] += k * p[b, yy, xx]
                E[b] += p[b, y, x] * (S[b, y, x] - M[b, y, x])
                Z[b] += S[b, y, x]
    loss, grad = 0.0, np.zeros_like(z)
    for b in range(images):
        if Z[b] != 0:
            loss += E[b] / Z[b]
            grad[b] = (S[b] - 2.0 * M[b]) * p[b] * q[b] / (Z[b] * images)
    return E, Z, loss / images, grad


def case(images, H, W, seed):
    """(logits (images, H, W), frames (images, 3, H, W)) as float32: smooth colour regions with an edge and some noise, so
    that the colour kernel takes values all over (0, 1]; logits of both signs, a few of them large."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    frames = np.empty((images, 3, H, W), dtype=np.float32)
    for b in range(images):
        edge = (xx * (1 + b) + 2 * yy > (W + H) * 0.8).astype(np.float64)
        for c in range(3):
            frames[b, c] = (0.25 + 0.3 * edge * (c + 1) / 3 + 0.1 * np.sin(0.3 * xx + 0.2 * c + 0.11 * yy) + 0.04 * rng.randn(H, W))
    logits = (2.5 * rng.randn(images, H, W)).astype(np.float32)
    logits.reshape(-1)[::17] *= 4
    return logits, frames
