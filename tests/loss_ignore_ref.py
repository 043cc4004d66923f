"""fp64 restatements of the losses with a void label (`ignore`): a pixel whose target equals `ignore` is in no sum, no count and
no ranking, and its gradient is 0.  With V the valid pixels of the set being reduced:

    cross_entropy                  sum_V bce(x, t) / |V|                                   helper_func.py:32-37
    dice                           1 - (2 sum_V p t + 1) / (sum_V p + sum_V t + 1)         networks/loss_dice.py:25-30
    cross_entropy_and_dice         bce_V - log(1 - dice_V)                                 helper_func.py:45-54
    class_balanced_cross_entropy   (N_neg S_pos + N_pos S_neg) / (|V| n): counts and sums over V (num_total = N_pos + N_neg =
                                   |V|), the two trailing divisions by the FULL shape, n    networks/loss_ce.py:42-59
    lovasz_hinge[_flat]            the void pixels removed before the ranking               networks/loss_lovasz.py:78-126

An empty V gives loss 0 and an all-zero gradient.  Each function returns (loss float, dL/dx fp64 of x's shape).
"""
import numpy as np

import lovasz_ref

KINDS = ('cross_entropy', 'dice', 'cross_entropy_and_dice', 'class_balanced_cross_entropy', 'lovasz_hinge', 'lovasz_hinge_flat')


def _parts(x, t, ignore):
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    t = np.asarray(t, dtype=np.float32).reshape(-1)
    ok = np.ones(t.shape, dtype=bool) if ignore is None else (t != np.float32(ignore))
    xv = np.where(ok, x, np.float32(0)).astype(np.float64)      # a select: a NaN / inf logit at a void pixel is never read
    tv = np.where(ok, t, np.float32(0)).astype(np.float64)
    return xv, tv, ok


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _bce_terms(x, t):
    return np.maximum(x, 0.0) - x * t + np.log1p(np.exp(-np.abs(x)))


def bce(x, t, ignore=None):
    xv, tv, ok = _parts(x, t, ignore)
    V = int(ok.sum())
    if V == 0:
        return 0.0, np.zeros(np.shape(x))
    loss = float(np.sum(np.where(ok, _bce_terms(xv, tv), 0.0)) / V)
    return loss, np.where(ok, (_sigmoid(xv) - tv) / V, 0.0).reshape(np.shape(x))


def _dice_sums(xv, tv, ok):
    p = _sigmoid(xv)
    I, Sp, Sy = np.sum(np.where(ok, p * tv, 0.0)), np.sum(np.where(ok, p, 0.0)), np.sum(np.where(ok, tv, 0.0))
    return p, 2.0 * I + 1.0, Sp + Sy + 1.0


def dice(x, t, ignore=None):
    xv, tv, ok = _parts(x, t, ignore)
    p, num, D = _dice_sums(xv, tv, ok)
    dLdp = -(2.0 * tv * D - num) / (D * D)
    return float(1.0 - num / D), np.where(ok, dLdp * p * (1.0 - p), 0.0).reshape(np.shape(x))


def bce_dice(x, t, ignore=None):
    xv, tv, ok = _parts(x, t, ignore)
    V = int(ok.sum())
    if V == 0:
        return 0.0, np.zeros(np.shape(x))
    p, num, D = _dice_sums(xv, tv, ok)
    lb, gb = bce(x, t, ignore)
    dLdp = -2.0 * tv / num + 1.0 / D                            # d/dp of -log(num / D)
    return float(lb - np.log(num / D)), (gb.reshape(-1) + np.where(ok, dLdp * p * (1.0 - p), 0.0)).reshape(np.shape(x))


def class_balanced_bce(x, t, ignore=None):
    xv, tv, ok = _parts(x, t, ignore)
    V, n = int(ok.sum()), ok.size
    if V == 0:
        return 0.0, np.zeros(np.shape(x))
    lab = (tv >= 0.5) & ok
    neg = ~lab & ok
    Np, Nn = float(lab.sum()), float(neg.sum())
    v = _bce_terms(xv, lab.astype(np.float64))
    Sp, Sn = np.sum(np.where(lab, v, 0.0)), np.sum(np.where(neg, v, 0.0))
    p = _sigmoid(xv)
    grad = np.where(lab, Nn * (p - 1.0), np.where(neg, Np * p, 0.0)) / (V * float(n))
    return float((Nn * Sp + Np * Sn) / (V * float(n))), grad.reshape(np.shape(x))


def lovasz_flat(x, t, ignore=None):
    """One set of pixels: `lovasz_hinge_flat(*flatten_binary_scores(x, t, ignore))`."""
    x32 = np.asarray(x, dtype=np.float32).reshape(-1)
    t32 = np.asarray(t, dtype=np.float32).reshape(-1)
    ok = np.ones(t32.shape, dtype=bool) if ignore is None else (t32 != np.float32(ignore))
    grad = np.zeros(x32.size, dtype=np.float64)
    if not ok.any():
        return 0.0, grad.reshape(np.shape(x))
    loss, g = lovasz_ref.lovasz_flat_f64(x32[ok], t32[ok])      # boolean indexing keeps the pixel order: ties as before
    grad[ok] = g
    return loss, grad.reshape(np.shape(x))


def lovasz_hinge(x, t, ignore=None, per_image=True):
    """x, t: [B, ...].  Per image: the mean over all B images (an all-void image adds 0), gradients / B."""
    x, t = np.asarray(x, dtype=np.float32), np.asarray(t, dtype=np.float32)
    if not per_image:
        return lovasz_flat(x, t, ignore)
    B = x.shape[0]
    losses, grads = zip(*[lovasz_flat(x[b], t[b], ignore) for b in range(B)])
    return float(np.sum(losses)) / B, np.stack(grads) / B


def one_set(kind, x, t, ignore=None):
    """The n elements as ONE set (what `Engine.loss_of` evaluates for either Lovasz kind)."""
    return {'cross_entropy': bce, 'dice': dice, 'cross_entropy_and_dice': bce_dice, 'class_balanced_cross_entropy': class_balanced_bce,
            'lovasz_hinge': lovasz_flat, 'lovasz_hinge_flat': lovasz_flat}[kind](x, t, ignore)


def batch(kind, x, t, ignore=None):
    """[B, ...] tensors as `Engine.loss` evaluates them: everything over the flattened batch, the Lovasz hinge per image."""
    if kind == 'lovasz_hinge':
        return lovasz_hinge(x, t, ignore, True)
    return one_set(kind, x, t, ignore)
