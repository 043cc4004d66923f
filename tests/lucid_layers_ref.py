"""TEST INFRASTRUCTURE: rules L2-L5 of `eosvos_amd/lucid_layers.py` as plain per-pixel loops in fp32 (np.float32 scalars, channel
vectors), the yardstick of its numpy twin, plus the synthetic inputs the CPU and the GPU tests share."""
import numpy as np

import lucid_ref
from eosvos_amd import lucid

F = np.float32


def id_map(height, width, n_ids):
    """An id map (H, W) uint8 with the ids 1 .. n_ids: overlapping rectangles laid over each other in id order, the target (id 1)
    on top of them all, one object touching a corner.  Every id keeps a pixel at every size >= 5 x 5; at 1 x 1 the pixel is 1."""
    ids = np.zeros((height, width), dtype=np.uint8)
    for i in list(range(2, n_ids + 1)) + [1]:
        y0, x0 = ((i * 5) % 7) * height // 9, ((i * 3) % 8) * width // 10
        ids[y0:y0 + max(1, height // 3), x0:x0 + max(1, width // 3)] = i
    if n_ids >= 2 and height > 4:
        ids[0:2, width - 2:] = 2
    return ids


def masks_of(ids, n_ids):
    """(target (1, H, W), others (n_ids - 1, 1, H, W)) fp32 masks whose `layer_map` is `ids`."""
    m = np.stack([(ids == i).astype(np.float32)[None] for i in range(1, n_ids + 1)])
    return m[0], m[1:]


def motion(height, width, centre, rot=0.0, factor=1.0, sy=0.0, sx=0.0):
    return lucid.invert(lucid.forward_matrix(centre[0], centre[1], rot, factor, sx * width, sy * height))


MOTIONS = [(0.0, 1.0, 0.0, 0.0), (7.0, 1.1, 0.12, -0.2), (-13.0, 0.9, -0.3, 0.45), (3.0, 1.0, 0.25, 0.3), (-5.0, 1.2, -0.1, 0.1),
           (11.0, 0.85, 0.05, -0.4), (0.0, 1.0, 0.5, 0.5), (-9.0, 1.05, -0.2, -0.15)]


def sample(height, width, order, flip=False, bg=(3.0, 1.04, 0.02, -0.03), shift=0):
    """A sample whose layers carry the ids of `order`, back to front; layer k moves by MOTIONS[(k + shift) % 8] about the frame
    centre: the layers overlap each other and some leave the frame."""
    c = (width / 2.0, height / 2.0)
    layers = [(int(i), motion(height, width, c, *MOTIONS[(k + shift) % len(MOTIONS)])) for k, i in enumerate(order)]
    return {'flip': flip, 'Bi': motion(height, width, c, *bg), 'layers': layers}


def samples(height, width, n_layers):
    """[sample]: the ids 1 .. n_layers in two depth orders, flipped and not."""
    up, down = list(range(1, n_layers + 1)), list(range(n_layers, 0, -1))
    return [sample(height, width, up), sample(height, width, down, flip=True, shift=1), sample(height, width, up[1:] + up[:1], shift=2)]


def compose_loops(fr, ids, plate, prms, target_id=1):
    """Rules L2-L5, pixel by pixel in fp32: (images (S, C, H, W), labels (S, 1, H, W), ids_out (S, H, W), counts (S, 8))."""
    c, h, w = fr.shape
    tab = lucid.cubic_table()
    images = np.zeros((len(prms), c, h, w), dtype=np.float32)
    labels = np.zeros((len(prms), 1, h, w), dtype=np.float32)
    ids_out = np.zeros((len(prms), h, w), dtype=np.uint8)
    counts = np.zeros((len(prms), 8), dtype=np.int64)
    for s, prm in enumerate(prms):
        for y in range(h):
            for x in range(w):
                xm = w - 1 - x if prm['flip'] else x
                yb, xb = lucid_ref._fix(prm['Bi'], y, xm)
                val = lucid_ref._cubic(plate, yb, xb, tab)
                top = None
                for k, (i, oi) in enumerate(prm['layers']):
                    yo, xo = lucid_ref._fix(oi, y, xm)
                    cover = 0
                    for a in (0, 1):
                        for b in (0, 1):
                            yy, xx = (yo >> 5) + a, (xo >> 5) + b
                            if 0 <= yy < h and 0 <= xx < w and ids[yy, xx] == i:
                                cover += ((yo & 31) if a else 32 - (yo & 31)) * ((xo & 31) if b else 32 - (xo & 31))
                    if cover == 1024:
                        val = lucid_ref._cubic(fr, yo, xo, tab)
                    elif cover > 0:
                        val = val + F(cover / 1024) * (lucid_ref._cubic(fr, yo, xo, tab) - val)
                    if cover >= 512:
                        top = k
                images[s, :, y, x] = val
                if top is not None:
                    ids_out[s, y, x] = prm['layers'][top][0]
                    counts[s, top] += 1
                labels[s, 0, y, x] = ids_out[s, y, x] == target_id
    return images, labels, ids_out, counts
