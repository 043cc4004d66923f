"""TEST INFRASTRUCTURE: the local dense-CRF model of `eosvos_crf_labels` (include/eosvos.h) restated pixel by pixel in
Python floats (fp64), with no tensor operation: the check of `eosvos_amd.crf.refine_host`, which in turn is the fp64
reference of the device kernels.  Also the synthetic scene both test files use."""
import math

import numpy as np
import torch


def scene(h, w, n_obj, seed, n_frames=1):
    """Coloured discs on grey with noisy probabilities: (images (n_frames, 3, h, w), probs (n_frames, n_obj, h, w)) fp32."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    images, probs = torch.full((n_frames, 3, h, w), 0.3), torch.empty(n_frames, n_obj, h, w)
    for f in range(n_frames):
        for o in range(n_obj):
            t = 0.5 if n_obj == 1 else o / (n_obj - 1)
            dist = torch.sqrt((yy - (0.3 + 0.4 * t) * h) ** 2 + (xx - (0.3 + 0.4 * t) * w) ** 2) - 0.22 * min(h, w)
            images[f][:, dist < 0] = torch.rand(3, generator=g)[:, None]
            probs[f, o] = torch.sigmoid(-0.6 * dist + 2.0 * torch.randn(h, w, generator=g))
        images[f] = (images[f] + 0.03 * torch.randn(3, h, w, generator=g)).clamp(0.0, 1.0)
    return images, probs


def refine_loops(image, probs, params):
    """One frame: image (3, H, W), probs (n_obj, H, W) array-likes -> (labels (H, W) uint8, Q^T (n_obj + 1, H, W) float64)."""
    f32 = lambda v: float(np.float32(v))                            # the parameters as the C-ABI carries them
    image, probs = np.asarray(image, dtype=np.float64), np.asarray(probs, dtype=np.float64)
    n_obj, H, W = probs.shape
    L = n_obj + 1
    T, r, d = params['iterations'], params['radius'], params['dilation']
    w_a, w_s = f32(params['w_appearance']), f32(params['w_smooth'])
    ta, tb, tg = f32(params['theta_alpha']), f32(params['theta_beta']), f32(params['theta_gamma'])
    floor = f32(1e-5)
    Q = np.zeros((L, H, W))
    U = np.zeros((L, H, W))
    for y in range(H):
        for x in range(W):
            p = [min(max(float(probs[o, y, x]), 0.0), 1.0) for o in range(n_obj)]
            s = [max(v, floor) for v in [1.0 - max(p)] + p]
            for l in range(L):
                Q[l, y, x] = s[l] / sum(s)
                U[l, y, x] = -math.log(Q[l, y, x])
    for _ in range(T):
        new = np.zeros_like(Q)
        for y in range(H):
            for x in range(W):
                acc_a, acc_s, n_a, n_s = [0.0] * L, [0.0] * L, 0.0, 0.0
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        qy, qx = y + d * dy, x + d * dx
                        if (dy, dx) == (0, 0) or not (0 <= qy < H and 0 <= qx < W):
                            continue
                        d2 = float((d * dy) ** 2 + (d * dx) ** 2)
                        col = sum((image[c, y, x] - image[c, qy, qx]) ** 2 for c in range(3))
                        k_a = math.exp(-d2 / (2 * ta * ta) - col / (2 * tb * tb))
                        k_s = math.exp(-d2 / (2 * tg * tg))
                        n_a += math.exp(-d2 / (2 * ta * ta))
                        n_s += k_s
                        for l in range(L):
                            acc_a[l] += k_a * Q[l, qy, qx]
                            acc_s[l] += k_s * Q[l, qy, qx]
                z = [-U[l, y, x] + (w_a * acc_a[l] / n_a if n_a > 0 else 0.0) + (w_s * acc_s[l] / n_s if n_s > 0 else 0.0)
                     for l in range(L)]
                e = [math.exp(v - max(z)) for v in z]
                for l in range(L):
                    new[l, y, x] = e[l] / sum(e)
        Q = new
    labels = np.zeros((H, W), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            if T == 0:                                               # merge_labels' rule on the probabilities as given
                v = [float(probs[o, y, x]) for o in range(n_obj)]
                labels[y, x] = 0 if max(v) < 0.5 else v.index(max(v)) + 1
            else:
                v = [Q[l, y, x] for l in range(1, L)]
                labels[y, x] = 0 if Q[0, y, x] > max(v) else v.index(max(v)) + 1
    return labels, Q
