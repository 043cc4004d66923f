"""TEST INFRASTRUCTURE: the rules of `eosvos_amd/components.py` restated pixel by pixel in plain Python -- a flood fill for the
component ids and direct loops for the filter -- as the check of the numpy twin (`label_host`, `filter_host`), which in turn is
the reference of the device tests; and the pattern set both test files label."""
from collections import deque

import numpy as np

TILE_H, TILE_W = 16, 64            # the tile of csrc/ccl_kernels.hip: the patterns cross its seams


def label_ref(lab, connectivity):
    """(H, W) uint8 -> (H, W) int32 ids: raster scan, flood fill from every unvisited object pixel (the first pixel reached in
    raster order is the smallest index of its component)."""
    h, w = lab.shape
    ids = np.zeros((h, w), dtype=np.int32)
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    for y in range(h):
        for x in range(w):
            if lab[y, x] == 0 or ids[y, x]:
                continue
            ident = y * w + x + 1
            ids[y, x] = ident
            todo = deque([(y, x)])
            while todo:
                cy, cx = todo.popleft()
                for dy, dx in nb:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < h and 0 <= nx < w and not ids[ny, nx] and lab[ny, nx] == lab[y, x]:
                        ids[ny, nx] = ident
                        todo.append((ny, nx))
    return ids


def filter_ref(labels, params, prev=None, keep=()):
    """(N, H, W) uint8 -> (filtered (N, H, W) uint8, removed (N,) int64); `params` complete (`components.check`)."""
    n, h, w = labels.shape
    g, q = params['gate'], int(round(params['min_rel_area'] * 65536))
    out = labels.copy()
    removed = np.zeros(n, dtype=np.int64)
    R = prev
    for f in range(n):
        if f not in keep:
            ids = label_ref(labels[f], params['connectivity'])
            comps = {}                                    # id -> list of pixels
            for y in range(h):
                for x in range(w):
                    if ids[y, x]:
                        comps.setdefault(int(ids[y, x]), []).append((y, x))
            for o in sorted({int(v) for v in labels[f].reshape(-1)} - {0}):
                mine = {i: px for i, px in comps.items() if labels[f][px[0]] == o}
                gated = g > 0 and R is not None and bool((R == o).any())
                cand = {}
                for i, px in mine.items():
                    ok = not gated
                    for y, x in px:
                        if ok:
                            break
                        for qy in range(max(0, y - g), min(h, y + g + 1)):
                            for qx in range(max(0, x - g), min(w, x + g + 1)):
                                if R[qy, qx] == o:
                                    ok = True
                    if ok:
                        cand[i] = len(px)
                amax = max(cand.values()) if cand else 0
                first = min([i for i, a in cand.items() if a == amax]) if cand else 0
                for i, px in mine.items():
                    a = len(px)
                    kept = i in cand and a >= params['min_area'] and a * 65536 >= q * amax and \
                        (not params['largest_only'] or i == first)
                    if not kept:
                        for y, x in px:
                            out[f, y, x] = 0
                        removed[f] += a
        R = out[f]
    return out, removed


# ---- patterns ---------------------------------------------------------------------------------------------------------
def serpentine(h, w, vertical=False):
    """A one-pixel-wide path: every second row in full, joined alternately at the right and the left end (`vertical`: the same
    with columns): it crosses every tile seam and is ONE component of h * w / 2 pixels or so."""
    if vertical:
        return np.ascontiguousarray(serpentine(w, h).T)
    m = np.zeros((h, w), dtype=np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, h, 2)):
        if y + 1 < h:
            m[y, w - 1 if k % 2 == 0 else 0] = 1
    return m


def spiral(h, w):
    """A one-pixel-wide rectangular spiral with one-pixel gaps, walked inward from the top-left corner."""
    m = np.zeros((h, w), dtype=np.uint8)
    y, x, d = 0, 0, 0
    step = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    m[0, 0] = 1
    turns = 0
    while turns < 2:
        dy, dx = step[d]
        ny, nx = y + dy, x + dx
        ay, ax = ny + dy, nx + dx                         # the pixel after the next: must be free, or the arm would touch
        if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= ay < h and 0 <= ax < w and m[ay, ax]):
            y, x = ny, nx
            m[y, x] = 1
            turns = 0
        else:
            d = (d + 1) % 4
            turns += 1
    return m


def nested_u(h, w):
    """Upward-opening U shapes nested in each other, two pixels apart: the two arms of a U meet only at its bottom row, the
    case a single raster scan labels wrongly.  Every U is its own component."""
    m = np.zeros((h, w), dtype=np.uint8)
    for a in range(0, min(h, (w + 1) // 2), 2):
        lo, hi, bottom = a, w - 1 - a, h - 1 - a
        if hi < lo or bottom < 0:
            break
        m[0:bottom + 1, lo] = 1 + (a // 2) % 2
        m[0:bottom + 1, hi] = 1 + (a // 2) % 2
        m[bottom, lo:hi + 1] = 1 + (a // 2) % 2
    return m


def noise(h, w, density, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((h, w)) < density, rng.integers(1, 4, (h, w)), 0).astype(np.uint8)


def seam_quadrants(h, w):
    """Different labels meeting exactly on the tile seams (they must not join); label 1 fills two quadrants that touch only
    at the corner of four tiles: one component under 8-connectivity, two under 4."""
    m = np.zeros((h, w), dtype=np.uint8)
    m[:TILE_H, :TILE_W] = 1
    m[:TILE_H, TILE_W:] = 2
    m[TILE_H:, :TILE_W] = 3
    m[TILE_H:, TILE_W:] = 1
    return m


def patterns(h, w):
    """{name: (H, W) uint8}: the pattern set of the component tests at one size."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = {'empty': np.zeros((h, w), dtype=np.uint8), 'full': np.full((h, w), 2, dtype=np.uint8),
           'checkerboard': ((yy + xx) % 2 == 0).astype(np.uint8), 'serpentine': serpentine(h, w),
           'serpentine_v': serpentine(h, w, vertical=True), 'spiral': spiral(h, w), 'nested_u': nested_u(h, w),
           'seam_quadrants': seam_quadrants(h, w)}
    for d in (0.35, 0.5, 0.6):
        out[f'noise_{d}'] = noise(h, w, d, seed=int(d * 100) + h + w)
    return out


def chain(h, w, g, side):
    """The 6-frame gate scene: labels (6, H, W), prev (H, W), keep = (4,).  Object 1 is a side x side square drifting right by
    g - 1 < g pixels per frame from `prev` on, absent in frame 2 (the gate of frame 3 is then inactive: the object returns, and
    the distractor with it); a static distractor of label 1, larger than the object (2 side x side) and more than g away from
    every position of it, sits at the right edge; object 2 is a static square below, absent from `prev`.  Frame 4 is a `keep`
    frame."""
    assert g >= 2 and h >= 3 * side + 2 and w >= 6 * (g - 1) + side + g + 1 + 2 * side
    labels = np.zeros((6, h, w), dtype=np.uint8)
    prev = np.zeros((h, w), dtype=np.uint8)
    prev[1:1 + side, 0:side] = 1
    for f in range(6):
        x0 = (f + 1) * (g - 1)
        if f != 2:
            labels[f, 1:1 + side, x0:x0 + side] = 1
        labels[f, 0:side, w - 2 * side:w] = 1             # the distractor
        labels[f, h - side:h, 2:2 + side] = 2
    return labels, prev, (4,)
