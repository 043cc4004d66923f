"""Bootstrapped cross-entropy in plain loops: the oracle of the numpy twin `eosvos_amd.bootstrap.loss_host`.

One set: the valid keys as order-preserving unsigned words built bit by bit with `struct`, sorted with Python's `sorted`,
the k-th largest taken, G and T counted; k restated from the rule (q = round(fraction * 65536), k = max(1, (n q + 32768) >> 16))."""
import math
import struct

import numpy as np


def word(key):
    """One fp32 key -> its orderable 32-bit word: NaN the largest, -0 as +0, negative floats bit-flipped, others top bit set."""
    key = float(np.float32(key))
    if math.isnan(key):
        return 0xFFFFFFFF
    b = struct.unpack('<I', struct.pack('<f', key))[0]
    if b == 0x80000000:
        b = 0
    return (~b) & 0xFFFFFFFF if b & 0x80000000 else b | 0x80000000


def k_of(n, fraction):
    q = int(math.floor(float(np.float32(fraction)) * 65536.0 + 0.5))
    q = min(65536, max(1, q))
    return max(1, (n * q + 32768) // 65536) if n > 0 else 0


def one_set(logits, targets, fraction, ignore=None):
    """-> dict(k, tau, G, T, r, weights fp32 array, loss fp64, grad fp64 array) of one set."""
    x = [float(v) for v in np.asarray(logits, dtype=np.float32).reshape(-1)]
    t = [float(v) for v in np.asarray(targets, dtype=np.float32).reshape(-1)]
    n_all = len(x)
    valid = [ignore is None or t[i] != float(np.float32(ignore)) for i in range(n_all)]
    words = [word(-x[i] if t[i] >= 0.5 else x[i]) for i in range(n_all)]
    vw = sorted(words[i] for i in range(n_all) if valid[i])
    n = len(vw)
    k = k_of(n, fraction)
    w = np.zeros(n_all, dtype=np.float32)
    grad = np.zeros(n_all, dtype=np.float64)
    if k == 0:
        return dict(k=0, tau=0, G=0, T=0, r=0, weights=w, loss=0.0, grad=grad)
    tau = vw[n - k]
    G = sum(1 for v in vw if v > tau)
    T = sum(1 for v in vw if v == tau)
    r = k - G
    loss = 0.0
    for i in range(n_all):
        if not valid[i] or words[i] < tau:
            continue
        w[i] = np.float32(1.0) if words[i] > tau else np.float32(r) / np.float32(T)
        e = math.exp(-abs(x[i]))
        bce = max(x[i], 0.0) - x[i] * t[i] + math.log1p(e)
        sig = 1.0 / (1.0 + e) if x[i] >= 0 else e / (1.0 + e)
        loss += float(w[i]) * bce
        grad[i] = float(w[i]) * (sig - t[i]) / k
    return dict(k=k, tau=tau, G=G, T=T, r=r, weights=w, loss=loss / k, grad=grad)
