"""Bootstrapped (hard-pixel) cross-entropy, `loss_func: bootstrapped_cross_entropy[_<P>]`: the names, k, and the numpy twin of
the device kernels (`csrc/bootstrap_kernels.hip`, the rule of `include/eosvos.h` at EOSVOS_LOSS_BOOTSTRAPPED_BCE).

Per set (one image on the forward path, all n elements through `loss_of`), V the non-void pixels, n = |V|:
  key_p = -z_p * (2 * (y_p >= .5) - 1), compared as order-preserving 32-bit unsigned words (-0 -> +0, NaN -> 0xFFFFFFFF);
  q = round(fraction * 65536) in [1, 65536];  k = max(1, (n * q + 32768) >> 16);
  tau = the k-th largest key, G = #{key > tau}, T = #{key = tau}, r = k - G;
  w_p = 1 above tau, fp32 r / T at tau, 0 below and at void pixels;
  set loss = sum_V w_p bce_p / k;  loss = mean over the sets;  dL/dz_p = w_p (sigmoid(z_p) - y_p) / (k * sets).
The OnAVOS fraction 0.25 is the default; it is untuned here (no J&F figure exists for it)."""
import numpy as np

from .loss_names import BOOTSTRAP as NAME, check_fraction, parse_bootstrap as parse, q_of  # noqa: F401  (the spelling's home)

DEFAULT_FRACTION = 0.25


def k_of(n, fraction):
    """The number of pixels kept of n valid ones (0 for an empty set)."""
    n = int(n)
    return max(1, (n * q_of(fraction) + 32768) >> 16) if n > 0 else 0


def orderable(key):
    """fp32 keys -> uint32 words whose unsigned order is the keys' order: -0 as +0, NaN as 0xFFFFFFFF."""
    key = np.ascontiguousarray(key, dtype=np.float32)
    b = key.view(np.uint32).copy()
    b[b == np.uint32(0x80000000)] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    u = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    u[np.isnan(key)] = np.uint32(0xFFFFFFFF)
    return u


def keys_of(logits, targets):
    x = np.asarray(logits, dtype=np.float32)
    return orderable(np.where(np.asarray(targets) >= 0.5, -x, x))


def select(u, valid, k):
    """(tau, G, T, r, fp32 weights) of the k largest among u[valid]; k = 0 (empty set): zeros."""
    w = np.zeros(u.shape, dtype=np.float32)
    if k == 0:
        return 0, 0, 0, 0, w
    uv = u[valid]
    tau = np.partition(uv, uv.size - k)[uv.size - k]
    G, T = int((uv > tau).sum()), int((uv == tau).sum())
    r = k - G
    w[valid & (u > tau)] = 1.0
    w[valid & (u == tau)] = np.float32(r) / np.float32(T)
    return int(tau), G, T, r, w


def loss_host(logits, targets, fraction, ignore=None, dtype=np.float64):
    """The numpy twin.  logits / targets: (sets, ...) or one flat set; returns (loss, gradient of the logits' shape, fp32
    weights of that shape, [k per set]).  The selection is exact integer work on the fp32 keys; the BCE terms, the sums and
    the gradient are formed in `dtype`."""
    x32 = np.asarray(logits, dtype=np.float32)
    t32 = np.asarray(targets, dtype=np.float32)
    shape = x32.shape
    if x32.ndim < 2:
        x32, t32 = x32.reshape(1, -1), t32.reshape(1, -1)
    sets = x32.shape[0]
    x32, t32 = x32.reshape(sets, -1), t32.reshape(sets, -1)
    grad = np.zeros(x32.shape, dtype=dtype)
    weights = np.zeros(x32.shape, dtype=np.float32)
    ks, total = [], dtype(0)
    for s in range(sets):
        valid = np.ones(x32.shape[1], dtype=bool) if ignore is None else t32[s] != np.float32(ignore)
        k = k_of(int(valid.sum()), fraction)
        ks.append(k)
        if k == 0:
            continue
        _, _, _, _, w = select(keys_of(x32[s], t32[s]), valid, k)
        weights[s] = w
        on = w != 0
        x, t, wv = x32[s][on].astype(dtype), t32[s][on].astype(dtype), w[on].astype(dtype)
        with np.errstate(over='ignore', invalid='ignore'):
            e = np.exp(-np.abs(x))
            bce = np.maximum(x, 0) - x * t + np.log1p(e)
            sig = np.where(x >= 0, 1 / (1 + e), e / (1 + e))
            total += (wv * bce).sum(dtype=dtype) / dtype(k)
            grad[s][on] = wv * (sig - t) / dtype(k * sets)
    return dtype(total / dtype(sets)), grad.reshape(shape), weights.reshape(shape), ks
