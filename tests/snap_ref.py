"""The rules of `eosvos_amd/snap.py` (1-6 of its docstring) restated as plain loops over pixels and clusters: no numpy
indexing tricks, Python integers throughout, nothing shared with the twin.  What the twin is checked against; far too slow for
anything but small frames.  Also the inputs the snap tests share: noise frames, label maps, the two-disc scene."""
import numpy as np


def superpixels_ref(img, S, T, m):
    """img (3, H, W) uint8 -> (ids as H lists of W ints, the number of (iteration, cluster) updates that met n = 0)."""
    _, H, W = img.shape
    px = [[[int(img[c, y, x]) for c in range(3)] for x in range(W)] for y in range(H)]
    gy, gx = -(-H // S), -(-W // S)
    centres = []
    for cy in range(gy):
        for cx in range(gx):
            y, x = min(cy * S + S // 2, H - 1), min(cx * S + S // 2, W - 1)
            centres.append([y, x] + px[y][x])
    ids = [[0] * W for _ in range(H)]
    empty = 0
    for t in range(1, T + 1):
        for y in range(H):
            for x in range(W):
                best, best_id = None, None
                for cy in range(y // S - 1, y // S + 2):
                    for cx in range(x // S - 1, x // S + 2):
                        if not (0 <= cy < gy and 0 <= cx < gx):
                            continue
                        k = cy * gx + cx
                        c = centres[k]
                        r, g, b = px[y][x]
                        d = ((r - c[2]) ** 2 + (g - c[3]) ** 2 + (b - c[4]) ** 2) * S * S + m * m * ((y - c[0]) ** 2 + (x - c[1]) ** 2)
                        if best is None or d < best or (d == best and k < best_id):
                            best, best_id = d, k
                ids[y][x] = best_id
        if t < T:
            for k in range(gy * gx):
                n, sums = 0, [0] * 5
                for y in range(H):
                    for x in range(W):
                        if ids[y][x] == k:
                            n += 1
                            for j, v in enumerate([y, x] + px[y][x]):
                                sums[j] += v
                if n == 0:
                    empty += 1
                    continue
                centres[k] = [(2 * s + n) // (2 * n) for s in sums]
    return ids, empty


def snap_ref(rgb, labels, n_obj, S, T, m, q, keep=()):
    """rgb (N, 3, H, W) uint8, labels (N, H, W) uint8, q = round(min_share * 65536) -> (snapped maps (N, H, W) uint8, ids
    (N, H, W) int32, changed pixels per frame (N,) int64, empty-cluster updates seen)."""
    N, H, W = labels.shape
    out = labels.copy()
    ids_all = np.zeros((N, H, W), dtype=np.int32)
    changed = np.zeros(N, dtype=np.int64)
    empties = 0
    for f in range(N):
        ids, empty = superpixels_ref(rgb[f], S, T, m)
        ids_all[f] = np.array(ids, dtype=np.int32)
        empties += empty
        if f in keep:
            continue
        K = -(-H // S) * -(-W // S)
        cnt = [[0] * (n_obj + 1) for _ in range(K)]
        for y in range(H):
            for x in range(W):
                l = int(labels[f, y, x])
                if l <= n_obj:
                    cnt[ids[y][x]][l] += 1
        decision = []
        for k in range(K):
            n_c, w = sum(cnt[k]), 0
            for l in range(1, n_obj + 1):
                if cnt[k][l] > cnt[k][w]:
                    w = l
            decision.append(w if n_c > 0 and cnt[k][w] * 65536 >= q * n_c else None)
        for y in range(H):
            for x in range(W):
                l, w = int(labels[f, y, x]), decision[ids[y][x]]
                if l <= n_obj and w is not None:
                    out[f, y, x] = w
                    changed[f] += int(w != l)
    return out, ids_all, changed, empties


# ---- inputs -------------------------------------------------------------------------------------------------------------
def noise_rgb(n, h, w, seed, smooth=False):
    """Uniform uint8 noise; `smooth`: a gradient with +-20 noise instead, so that clusters are compact."""
    rng = np.random.default_rng(seed)
    if not smooth:
        return rng.integers(0, 256, size=(n, 3, h, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([yy * 255 // max(h - 1, 1), xx * 255 // max(w - 1, 1), (yy + xx) * 255 // max(h + w - 2, 1)])
    return np.clip(base[None] + rng.integers(-20, 21, size=(n, 3, h, w)), 0, 255).astype(np.uint8)


def binary_rgb(n, h, w, seed):
    """The heaviest noise: every channel of every pixel is 0 or 255."""
    rng = np.random.default_rng(seed)
    return ((rng.random((n, 3, h, w)) < 0.5) * 255).astype(np.uint8)


def blob_labels(n, h, w, n_obj, seed, above=True):
    """Label maps of blocks of 0..n_obj with speckle; with `above`, a few pixels hold values above n_obj (where one exists)."""
    rng = np.random.default_rng(seed + 1000)
    coarse = rng.integers(0, n_obj + 1, size=(n, -(-h // 6), -(-w // 6)))
    lab = np.repeat(np.repeat(coarse, 6, axis=1), 6, axis=2)[:, :h, :w].astype(np.uint8)
    speck = rng.random((n, h, w)) < 0.1
    lab[speck] = rng.integers(0, n_obj + 1, size=int(speck.sum())).astype(np.uint8)
    if above and n_obj < 255:
        over = rng.random((n, h, w)) < 0.05
        lab[over] = rng.integers(n_obj + 1, 256, size=int(over.sum())).astype(np.uint8)
    return lab


def disc_scene(h, w, seed=0):
    """Two coloured discs on a gradient with +-12 noise -> (rgb (1, 3, H, W) uint8, truth (1, H, W) uint8, prediction
    (1, H, W) uint8: the truth shifted by (2, -3) with 3 % speckle)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    r = min(h, w) // 4
    d1 = (yy - h // 2) ** 2 + (xx - w // 4) ** 2 < r * r
    d2 = (yy - h // 2) ** 2 + (xx - 3 * w // 4) ** 2 < r * r
    img = np.stack([60 + 60 * xx // max(w - 1, 1), 80 + 40 * yy // max(h - 1, 1), np.full((h, w), 100)]).astype(np.int64)
    img[:, d1] = np.array([220, 40, 40])[:, None]
    img[:, d2] = np.array([40, 60, 230])[:, None]
    img = np.clip(img + rng.integers(-12, 13, size=img.shape), 0, 255).astype(np.uint8)
    truth = np.zeros((h, w), dtype=np.uint8)
    truth[d1], truth[d2] = 1, 2
    pred = np.roll(truth, (2, -3), axis=(0, 1))
    speck = rng.random((h, w)) < 0.03
    pred[speck] = rng.integers(0, 3, size=int(speck.sum())).astype(np.uint8)
    return img[None], truth[None], pred[None]
