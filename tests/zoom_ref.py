"""TEST INFRASTRUCTURE: the box rule of the zoom pass (`eosvos_amd/zoom.py`, rules 1-5) as plain Python loops over pixels, and
the box cases shared by tests/test_zoom_host.py (numpy twin against these loops) and tests/test_gpu_zoom.py (device against the
numpy twin).  Nothing here is imported by the product."""
import numpy as np

BASE = {'max_zoom': 3, 'min_zoom': 1.5, 'threshold': 0.5, 'min_pixels': 16, 'margin': 0.5, 'margin_px': 4}
SIZES = ((32, 32), (33, 70), (97, 163))
ANCHOR = (1, 29, 49, 32, 54)             # computed by hand, see `anchor_case`


def _ceil(a, b):
    q = a // b
    return q + (1 if q * b < a else 0)


def box_ref(p0, prm):
    """One frame: p0 a (H, W) array of fp32 -> (valid, y0, x0, bh, bw), every step written out."""
    H, W = p0.shape
    thr = np.float32(prm.get('threshold', 0.5))
    cnt, my0, my1, mx0, mx1 = 0, H, -1, W, -1
    for y in range(H):
        row = p0[y]
        for x in range(W):
            if row[x] >= thr:
                cnt += 1
                my0, my1, mx0, mx1 = min(my0, y), max(my1, y), min(mx0, x), max(mx1, x)
    invalid = (0, 0, 0, H, W)
    if cnt < prm.get('min_pixels', 16):
        return invalid
    margin_q = int(round(prm.get('margin', 0.5) * 65536))
    min_q = int(round(prm.get('min_zoom', 1.5) * 65536))
    max_q = int(round(prm['max_zoom'] * 65536))
    mh, mw = my1 - my0 + 1, mx1 - mx0 + 1
    pad = ((max(mh, mw) * margin_q) >> 16) + prm.get('margin_px', 8)
    gh, gw = mh + 2 * pad, mw + 2 * pad
    bh = min(H, max(gh, _ceil(gw * H, W), _ceil(H * 65536, max_q)))
    bw = min(W, _ceil(bh * W, H))
    if bh * min_q > H * 65536:
        return invalid
    y0 = (2 * my0 + mh - bh) >> 1
    x0 = (2 * mx0 + mw - bw) >> 1
    y0 = 0 if y0 < 0 else (H - bh if y0 > H - bh else y0)
    x0 = 0 if x0 < 0 else (W - bw if x0 > W - bw else x0)
    return (1, y0, x0, bh, bw)


def boxes_ref(p0, prm):
    return np.array([box_ref(f, prm) for f in np.asarray(p0).reshape(-1, *np.asarray(p0).shape[-2:])], dtype=np.int32)


def frame(H, W, *rects, lo=0.1, hi=0.9):
    """A (H, W) fp32 probability map: `hi` inside the rectangles (y0, y1, x0, x1, inclusive), `lo` elsewhere."""
    p = np.full((H, W), lo, dtype=np.float32)
    for y0, y1, x0, x1 in rects:
        p[y0:y1 + 1, x0:x1 + 1] = hi
    return p


def anchor_case():
    """96 x 160, mask rows 40-49 and columns 70-81, margin 0.5, margin_px 4, max_zoom 3, min_zoom 1.5.  mh = 10, mw = 12,
    pad = (12 * 32768 >> 16) + 4 = 10, gh = 30, gw = 32, ceil(32 * 96 / 160) = 20, ceil(96 * 65536 / 196608) = 32: bh = 32,
    bw = ceil(32 * 160 / 96) = 54; 32 * 98304 <= 96 * 65536: valid; y0 = (80 + 10 - 32) >> 1 = 29, x0 = (140 + 12 - 54) >> 1 =
    49."""
    return 'anchor', frame(96, 160, (40, 49, 70, 81)), dict(BASE)


def cases():
    """[(name, p0 (H, W) fp32, params)]: the cases of the issue at the three sizes, and the hand-computed anchor."""
    out = [anchor_case()]
    for H, W in SIZES:
        t = f'{H}x{W}'
        one = dict(BASE, min_pixels=1)
        out.append((f'{t} pixel at the origin', frame(H, W, (0, 0, 0, 0)), one))
        out.append((f'{t} pixel at the far corner', frame(H, W, (H - 1, H - 1, W - 1, W - 1)), one))
        cy, cx = H // 2, W // 2
        out.append((f'{t} blob on the top border', frame(H, W, (0, 4, cx - 3, cx + 2)), dict(BASE)))
        out.append((f'{t} blob on the bottom border', frame(H, W, (H - 5, H - 1, cx - 3, cx + 2)), dict(BASE)))
        out.append((f'{t} blob on the left border', frame(H, W, (cy - 2, cy + 2, 0, 5)), dict(BASE)))
        out.append((f'{t} blob on the right border', frame(H, W, (cy - 2, cy + 2, W - 6, W - 1)), dict(BASE)))
        out.append((f'{t} wanted width exceeds W', frame(H, W, (cy, cy + 1, 1, W - 2)), dict(BASE, min_zoom=1)))
        out.append((f'{t} wanted width exceeds W, too large', frame(H, W, (cy, cy + 1, 1, W - 2)), dict(BASE)))
        out.append((f'{t} min_pixels - 1', frame(H, W, (cy, cy + 2, cx, cx + 4)), dict(BASE)))                 # 15 pixels
        out.append((f'{t} exactly min_pixels', frame(H, W, (cy, cy + 3, cx, cx + 3)), dict(BASE)))             # 16 pixels
        # the min_zoom boundary: no margin, a square of side k gives bh = k (H <= W); min_zoom 2 accepts k = H // 2 and
        # rejects H // 2 + 1
        edge = dict(BASE, margin=0, margin_px=0, max_zoom=4, min_zoom=2)
        k = H // 2
        out.append((f'{t} at the min_zoom boundary', frame(H, W, (3, 3 + k - 1, 5, 5 + k - 1)), edge))
        out.append((f'{t} past the min_zoom boundary', frame(H, W, (3, 3 + k, 5, 5 + k)), edge))
        tight = dict(BASE, margin=0, margin_px=0)
        out.append((f'{t} max_zoom floor active', frame(H, W, (cy - 2, cy + 1, cx - 2, cx + 1)), tight))
        out.append((f'{t} aspect term active', frame(H, W, (cy, cy + 1, cx - W // 4, cx - W // 4 + W // 2 - 1)), tight))
        out.append((f'{t} two distant blobs', frame(H, W, (0, 3, 0, 3), (H - 4, H - 1, W - 4, W - 1)), dict(BASE)))
        out.append((f'{t} empty', frame(H, W), dict(BASE)))
        p = frame(H, W, (cy - 2, cy + 2, cx - 2, cx + 2), lo=float(np.nextafter(np.float32(0.5), np.float32(0))), hi=0.5)
        out.append((f'{t} exactly at the threshold', p, dict(BASE)))
    return out


def active_term(p0, prm):
    """Which of (gh, aspect, floor) sets bh before the clamp to H -- lets a test assert that a case exercises the term it
    names."""
    H, W = p0.shape
    ys, xs = np.nonzero(p0 >= np.float32(prm['threshold']))
    mh, mw = int(ys.max() - ys.min() + 1), int(xs.max() - xs.min() + 1)
    pad = ((max(mh, mw) * int(round(prm['margin'] * 65536))) >> 16) + prm['margin_px']
    terms = {'gh': mh + 2 * pad, 'aspect': _ceil((mw + 2 * pad) * H, W), 'floor': _ceil(H * 65536, int(round(prm['max_zoom'] * 65536)))}
    best = max(terms.values())
    return [k for k, v in terms.items() if v == best], terms
