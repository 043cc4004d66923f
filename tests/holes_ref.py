"""TEST INFRASTRUCTURE: the rules of `eosvos_amd/holes.py` restated with flood fills in plain Python -- no union-find: per frame
a breadth-first fill of label 0 from the frame border, then one fill per remaining zero region, and rules 2-5 applied
literally -- as the check of the numpy twin (`fill_host`), which in turn is the reference of the device tests; and the pattern
set both test files fill."""
from collections import deque

import numpy as np

from components_ref import TILE_H, TILE_W, spiral

CLASSES = ('border', 'several', 'large', 'overlap', 'filled')


def _neighbours(connectivity):
    """Offsets under the BACKGROUND's connectivity: the dual of the objects'."""
    return [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 4 else [])


def _flood(m, seen, y, x, nb):
    """The zero pixels of `m` reachable from (y, x), which is zero and unseen; marks them seen."""
    h, w = m.shape
    seen[y, x] = True
    todo, region = deque([(y, x)]), [(y, x)]
    while todo:
        cy, cx = todo.popleft()
        for dy, dx in nb:
            ny, nx = cy + dy, cx + dx
            if 0 <= ny < h and 0 <= nx < w and not seen[ny, nx] and m[ny, nx] == 0:
                seen[ny, nx] = True
                todo.append((ny, nx))
                region.append((ny, nx))
    return region


def fill_ref(labels, params, prev=None, keep=()):
    """(N, H, W) uint8 -> (filled maps (N, H, W) uint8, pixels filled (N,) int64, {class: background components} over all
    frames that are not kept); `params` complete (`holes.check`).  The classes are `CLASSES`: touching the border, several
    bordering labels, failing the size rule, failing the previous-frame rule, filled."""
    n, h, w = labels.shape
    nb = _neighbours(params['connectivity'])
    rq, oq = int(round(params['max_rel_area'] * 65536)), int(round(params['prev_overlap'] * 65536))
    out = labels.copy()
    filled = np.zeros(n, dtype=np.int64)
    classes = dict.fromkeys(CLASSES, 0)
    R = prev
    for f in range(n):
        if f not in keep:
            m = labels[f]                                 # every decision reads the input map
            seen = np.zeros((h, w), dtype=bool)
            for y in range(h):
                for x in range(w):
                    if (y in (0, h - 1) or x in (0, w - 1)) and m[y, x] == 0 and not seen[y, x]:
                        _flood(m, seen, y, x, nb)
                        classes['border'] += 1
            for y in range(h):
                for x in range(w):
                    if m[y, x] != 0 or seen[y, x]:
                        continue
                    region = _flood(m, seen, y, x, nb)
                    around = set()
                    for cy, cx in region:
                        for dy, dx in nb:
                            ny, nx = cy + dy, cx + dx     # inside the frame: no pixel of a hole lies on the border
                            if m[ny, nx] != 0:
                                around.add(int(m[ny, nx]))
                    assert around                         # a hole cannot have zero bordering labels
                    if len(around) != 1:
                        classes['several'] += 1
                        continue
                    o = around.pop()
                    A, S = len(region), int((m == o).sum())
                    if not (A <= params['max_area'] and A * 65536 <= rq * S):
                        classes['large'] += 1
                        continue
                    if oq > 0 and R is not None and bool((R == o).any()):
                        C = sum(1 for cy, cx in region if R[cy, cx] == o)
                        if not C * 65536 >= oq * A:
                            classes['overlap'] += 1
                            continue
                    classes['filled'] += 1
                    for cy, cx in region:
                        out[f, cy, cx] = o
                    filled[f] += A
        R = out[f]
    return out, filled, classes


# ---- patterns ---------------------------------------------------------------------------------------------------------
def _ring(m, y0, x0, y1, x1, label, t=1):
    """Rows y0..y1-1, columns x0..x1-1 hold `label`, except the interior t pixels in, which holds 0."""
    m[y0:y1, x0:x1] = label
    m[y0 + t:y1 - t, x0 + t:x1 - t] = 0
    return m


def corridor(h, w, open_to_border=False):
    """A one-pixel-wide spiral corridor of background in a frame otherwise full of label 1: one long hole over many tiles.
    `open_to_border`: the corridor's outer end reaches x = 0, so it is no hole."""
    m = np.ones((h, w), dtype=np.uint8)
    m[2:h - 2, 2:w - 2][spiral(h - 4, w - 4) == 1] = 0
    if open_to_border:
        m[2, 0:2] = 0
    return m


def patterns(h, w):
    """{name: (H, W) uint8}: the pattern set of the hole tests at one size; a pattern that does not fit the size is left out."""
    z = lambda: np.zeros((h, w), dtype=np.uint8)
    out = {'empty': z(), 'full': np.full((h, w), 255, dtype=np.uint8)}
    if h >= 5 and w >= 7:
        out['ring'] = _ring(z(), 1, 1, h - 1, w - 1, 1, t=max(1, min(h, w) // 4))       # thick: the hole is smaller than the ring
        m = z()                                           # a ring cut by the top border: its inside reaches y = 0, no hole
        m[0:4, 1:6] = 1
        m[0:3, 2:5] = 0
        out['ring_at_border'] = m
        m = _ring(z(), 1, 1, 4, 6, 3)                     # the ring's corner pixel is missing: the inside meets the outside
        m[1, 1] = 0                                       # over a corner only -- a hole for connectivity 8, none for 4
        out['corner_leak'] = m
        m = z()                                           # labels 1 and 2 side by side, a hole on their seam
        m[1:h - 1, 1:w // 2] = 1
        m[1:h - 1, w // 2:w - 1] = 2
        m[h // 2, w // 2 - 1:w // 2 + 1] = 0
        out['between_two'] = m
        out['corridor'] = corridor(h, w)
        out['corridor_open'] = corridor(h, w, open_to_border=True)
    if h >= 11 and w >= 11:
        m = _ring(z(), 1, 1, 10, 10, 1)                   # ring of 1, moat, island of 2 with its own hole
        _ring(m, 3, 3, 8, 8, 2, t=2)
        out['nested'] = m
    if w >= TILE_W + 4 and h >= 5:
        out['seam_x'] = _ring(z(), 1, TILE_W - 3, 4, TILE_W + 3, 1)         # the hole holds x = 63 and x = 64
    if h >= TILE_H + 4 and w >= 7:
        out['seam_y'] = _ring(z(), TILE_H - 3, 1, TILE_H + 3, 5, 2)         # the hole holds y = 15 and y = 16
    if h >= TILE_H + 4 and w >= TILE_W + 4:
        out['seam_xy'] = _ring(z(), TILE_H - 3, TILE_W - 3, TILE_H + 3, TILE_W + 3, 7)
    return out


def punched(h, w, p, seed):
    """Vertical thirds carry labels 1, 2 and 3, the leftmost eighth is background, and pixels are zeroed with probability p."""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), dtype=np.uint8)
    third = (w + 2) // 3
    for k in range(3):
        m[:, k * third:(k + 1) * third] = k + 1
    m[:, :w // 8] = 0
    m[rng.random((h, w)) < p] = 0
    return m


def chain(h=24, w=100):
    """The 5-frame scene of the previous-frame rule: labels (5, H, W), prev (H, W), keep = (0,), and the boxes
    (y0, y1, x0, x1) of the real hole per frame and of the spurious hole.  Object 1 is a 12 x 16 block that drifts right by one
    pixel per frame over x = 64 with a REAL hole of 3 x 4 pixels that moves with it: three quarters of it were hole in the
    frame before, so with prev_overlap 0.5 it stays open.  A SPURIOUS hole of 2 x 2 pixels sits at a fixed place inside the
    object in frames 2 and 3: in frame 3 it fills only because R is the FILLED frame 2.  Object 2 is a static block with a
    hole that `prev` does not contain.  Frame 0 is the `keep` frame; `prev` continues the drift backwards."""
    def frame(k, spurious):
        m = np.zeros((h, w), dtype=np.uint8)
        x0 = 56 + k
        m[4:16, x0:x0 + 16] = 1
        m[7:10, x0 + 5:x0 + 9] = 0                        # the real hole: columns 61 + k .. 64 + k
        if spurious:
            m[12:14, 68:70] = 0
        m[h - 6:h - 1, 2:8] = 2
        m[h - 4, 4:6] = 0
        return m
    labels = np.stack([frame(k, k in (2, 3)) for k in range(5)])
    prev = frame(-1, False)
    prev[prev == 2] = 0
    real = [(7, 10, 61 + k, 65 + k) for k in range(5)]
    return labels, prev, (0,), real, (12, 14, 68, 70)
