"""Restatement of the Lovasz hinge (`networks/loss_lovasz.py:78-111`) that the device kernels are held to.

The errors are evaluated in fp32 exactly as torch does (`1 - x * s` with `s = +-1`: the product is exact, the subtraction
rounds once), ranked by a STABLE descending sort (ties by ascending pixel index), and the Jaccard increments are formed from
the integer counts in fp64 without the reference's cancellation (it subtracts two fp32 numbers near 1):

    g_k = 1:  w_k = 1 / U_k        g_k = 0:  w_k = I_k / (U_{k-1} U_k)        w_0 = 1 / U_0

with I_k = G - c1_k, U_k = G + c0_k, c1 / c0 the inclusive counts of foreground / background among ranks 0..k.
"""
import numpy as np


def errors_f32(logits, labels):
    x = np.asarray(logits, dtype=np.float32).reshape(-1)
    g = np.asarray(labels).reshape(-1) >= 0.5
    s = np.where(g, np.float32(1), np.float32(-1))
    return np.float32(1) - x * s, g, s


def pixel_weights(logits, labels):
    """(e fp32, s, w_rank(i) fp64 per pixel) of ONE set of pixels."""
    e, g, s = errors_f32(logits, labels)
    with np.errstate(invalid='ignore'):
        order = np.argsort(-e, kind='stable')
    gs = g[order].astype(np.int64)
    G = int(gs.sum())
    k = np.arange(e.size, dtype=np.int64)
    c1 = np.cumsum(gs)
    c0 = k + 1 - c1
    I, U = (G - c1).astype(np.float64), (G + c0).astype(np.float64)
    den = np.maximum((U - 1.0) * U, 1.0)            # (U - 1 = 0 only at rank 0 of an all-background set, replaced below)
    w = np.where(gs == 1, 1.0 / U, I / den)
    w[0] = 1.0 / U[0]
    wp = np.empty(e.size, dtype=np.float64)
    wp[order] = w
    return e, s, wp


def lovasz_flat_f64(logits, labels):
    """loss (float) and dL/dlogits (fp64, shape of `logits`) of one set of pixels."""
    e, s, wp = pixel_weights(logits, labels)
    pos = e > 0
    loss = float(np.sum(np.where(pos, e.astype(np.float64), 0.0) * wp))
    grad = np.where(pos, -s.astype(np.float64) * wp, 0.0)
    return loss, grad.reshape(np.shape(logits))


def lovasz_hinge_f64(logits, labels, per_image=True):
    """`lovasz_hinge(logits, labels, per_image)` for logits [B, ...]: per image the mean over the images (each gradient
    scaled by 1 / B), otherwise the whole batch as one set."""
    logits, labels = np.asarray(logits, dtype=np.float32), np.asarray(labels)
    if not per_image:
        return lovasz_flat_f64(logits, labels)
    B = logits.shape[0]
    losses, grads = zip(*[lovasz_flat_f64(logits[b], labels[b]) for b in range(B)])
    return float(np.sum(losses)) / B, np.stack(grads) / B


def lovasz_hinge_torch(logits, gt, per_image=True):
    """The same loss as a differentiable torch expression (the weights are constants of the order, as in the reference's
    autograd) -- what the CPU oracle's `loss_fn` is taught for the names `lovasz_hinge` / `lovasz_hinge_flat`."""
    import torch
    sets = [(logits[b], gt[b]) for b in range(logits.shape[0])] if per_image else [(logits, gt)]
    total = 0.0
    for x, t in sets:
        _, s, wp = pixel_weights(x.detach().cpu().numpy(), t.detach().cpu().numpy())
        e = 1.0 - x.reshape(-1) * torch.from_numpy(s)
        total = total + (torch.relu(e).double() * torch.from_numpy(wp)).sum()
    return (total / len(sets)).float()
