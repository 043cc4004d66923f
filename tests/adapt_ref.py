"""Plain-loop statement of rules 1-6 of eosvos_amd/adapt.py (the distance gate of online adaptation), and the seeded seed
patterns of its tests.  The distance is the all-pairs minimum of the definition: no two-pass trick, nothing shared with the
numpy twins or the kernels.  Slow on purpose; the tests keep the frames small."""
import numpy as np

IGN = 255.0
T = 0.5                                            # the threshold every pattern is built around


NO_SEED = 1 << 40                                  # D2 of a frame without a seed: above every cap


def distance_sq_all_pairs(seeds):
    """D2 of rule 1 before the cap: seeds (H, W) bool -> int64, by the definition (a seed is at distance 0 from itself)."""
    h, w = seeds.shape
    pts = [(int(y), int(x)) for y, x in zip(*np.nonzero(seeds))]
    out = np.full((h, w), NO_SEED, dtype=np.int64)
    for y in range(h):
        for x in range(w):
            if seeds[y, x]:
                out[y, x] = 0
                continue
            best = NO_SEED
            for qy, qx in pts:
                d = (y - qy) * (y - qy) + (x - qx) * (x - qx)
                if d < best:
                    best = d
            out[y, x] = best
    return out


def distance_sq(seeds, limit, d2=None):
    """Rule 1: seeds (H, W) bool -> min(D2, limit^2 + 1) as int64.  `d2`: the all-pairs distances of `seeds`, if at hand."""
    d2 = distance_sq_all_pairs(seeds) if d2 is None else d2
    return np.minimum(d2, limit * limit + 1)


def is_seed(p, threshold, invert):
    """`p >= t` or `!(p >= t)` on fp32 values: a NaN is never a seed of the first, always one of the second."""
    ge = bool(np.float32(p) >= np.float32(threshold))
    return (not ge) if invert else ge


def seeds_of(probs, threshold, invert=False):
    h, w = probs.shape
    out = np.zeros((h, w), dtype=bool)
    for y in range(h):
        for x in range(w):
            out[y, x] = is_seed(probs[y, x], threshold, invert)
    return out


def band_rule(probs, lo, hi, ignore=IGN):
    """The uncertainty band's targets (what `Engine.propagation_targets` is held to in test_gpu_loss_ignore.py): 1 where
    p >= hi, 0 where p < lo, void otherwise, compared as fp32."""
    p = np.asarray(probs, dtype=np.float32)
    return np.where(p >= np.float32(hi), np.float32(1), np.where(p < np.float32(lo), np.float32(0), np.float32(ignore)))


def eroded(anchor, threshold, erode):
    """Rules 2 and 3: anchor (H, W) fp32 -> E (H, W) bool."""
    A = seeds_of(anchor, threshold)
    if erode == 0:
        return A
    d_in = distance_sq(~A, erode)
    return A & (d_in > erode * erode)


def targets(probs, anchors, lo, hi, neg_dist, erode, ignore=IGN):
    """Rules 2-6: probs, anchors (F, H, W) fp32 -> (targets (F, H, W) fp32, n_pos [F])."""
    out = np.empty(probs.shape, dtype=np.float32)
    counts = []
    for f in range(probs.shape[0]):
        E = eroded(anchors[f], hi, erode)
        base = band_rule(probs[f], lo, hi, ignore)
        if not E.any():
            out[f] = base
            counts.append(0)
            continue
        far = distance_sq(E, neg_dist) > neg_dist * neg_dist
        t = base.copy()
        t[far] = 0
        out[f] = t
        counts.append(int((t == 1).sum()))
    return out, counts


# ---- patterns: probability maps whose seeds under `p >= T` form the named set ------------------------------------------------
PATTERNS = ('empty', 'full', 'corner00', 'corner0w', 'cornerh0', 'cornerhw', 'centre', 'sparse', 'blobs', 'blob_far_blob', 'nans')


def _blob(m, cy, cx, ry, rx):
    h, w = m.shape
    yy, xx = np.mgrid[0:h, 0:w]
    m |= ((yy - cy) * (yy - cy) * max(rx, 1) ** 2 + (xx - cx) * (xx - cx) * max(ry, 1) ** 2) <= max(ry, 1) ** 2 * max(rx, 1) ** 2


def pattern(name, h, w, seed=0):
    """(H, W) fp32 in [0, 1] (NaNs in 'nans'): seeds get a value in [T, 1], the rest one in [0, T)."""
    rng = np.random.RandomState(1000 * seed + 31 * h + w + len(name))
    m = np.zeros((h, w), dtype=bool)
    if name == 'full':
        m[:] = True
    elif name == 'corner00':
        m[0, 0] = True
    elif name == 'corner0w':
        m[0, w - 1] = True
    elif name == 'cornerh0':
        m[h - 1, 0] = True
    elif name == 'cornerhw':
        m[h - 1, w - 1] = True
    elif name == 'centre':
        m[h // 2, w // 2] = True
    elif name == 'sparse':
        m = rng.rand(h, w) < 0.002
    elif name in ('blobs', 'nans'):
        for _ in range(3):
            _blob(m, rng.randint(h), rng.randint(w), 1 + rng.randint(max(h // 5, 1)), 1 + rng.randint(max(w // 5, 1)))
    elif name == 'blob_far_blob':
        _blob(m, h // 3, w // 4, max(h // 5, 1), max(w // 8, 1))
        _blob(m, h - 1 - h // 8, w - 1 - w // 10, max(h // 16, 1), max(w // 20, 1))
    elif name != 'empty':
        raise KeyError(name)
    p = np.where(m, T + (1 - T) * rng.rand(h, w), T * rng.rand(h, w) * 0.999).astype(np.float32)
    p[m] = np.maximum(p[m], np.float32(T))
    if name == 'nans':
        p[rng.rand(h, w) < 0.05] = np.nan
    return p


def three_frames(h, w, nans=False, empty=1):
    """(probs, anchors) (3, H, W) for rules 2-6: a near and a far blob to judge; blobs as anchors, confident (1 on their seeds)
    so that every threshold keeps them; frame `empty` has no anchor.  With `nans`, NaNs in one map of each."""
    probs = np.stack([pattern('blob_far_blob', h, w, s) for s in range(3)])
    anchors = np.stack([pattern('nans' if nans and s == 2 else 'blobs', h, w, 10 + s) for s in range(3)])
    with np.errstate(invalid='ignore'):
        anchors[anchors >= np.float32(T)] = 1
    anchors[empty] = pattern('empty', h, w)
    if nans:
        probs[0] = pattern('nans', h, w, 4)
    return probs, anchors
