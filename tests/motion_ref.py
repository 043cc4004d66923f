"""TEST INFRASTRUCTURE: the rules of `eosvos_amd/motion.py` as plain loops over pixels, blocks and candidates -- the slow,
obvious statement the numpy twin (`motion.vectors_host`, `motion.warp_host`) is checked against -- and the inputs the motion
tests share."""
import numpy as np

# (H, W, B, R, bias): inside one partial block; one exact block; odd sizes; partial 16-blocks with the largest bias
SHAPES = [(7, 5, 8, 4, 0), (8, 8, 8, 1, 0), (37, 53, 8, 5, 0), (40, 56, 16, 7, 255)]
KINDS = ('noise', 'shift', 'flat', 'binary')


def luma_loops(rgb):
    """(3, H, W) uint8 -> (H, W) uint8."""
    _, h, w = rgb.shape
    out = np.zeros((h, w), dtype=np.uint8)
    for y in range(h):
        for x in range(w):
            out[y, x] = (77 * int(rgb[0, y, x]) + 150 * int(rgb[1, y, x]) + 29 * int(rgb[2, y, x]) + 128) >> 8
    return out


def match_loops(cur, ref, B, R, bias):
    """Luma planes (H, W) of frame f and f - 1 -> (by, bx, 2) int8: per block the valid candidate that is smallest under
    (cost, dy^2 + dx^2, dy, dx), compared as a Python tuple."""
    h, w = cur.shape
    by, bx = -(-h // B), -(-w // B)
    cur, ref = cur.astype(int).tolist(), ref.astype(int).tolist()
    out = np.zeros((by, bx, 2), dtype=np.int8)
    for j in range(by):
        for i in range(bx):
            y0, y1, x0, x1 = j * B, min(j * B + B, h), i * B, min(i * B + B, w)
            n = (y1 - y0) * (x1 - x0)
            best = None
            for dy in range(-R, R + 1):
                if y0 + dy < 0 or y1 - 1 + dy > h - 1:
                    continue
                for dx in range(-R, R + 1):
                    if x0 + dx < 0 or x1 - 1 + dx > w - 1:
                        continue
                    cost = 0
                    for y in range(y0, y1):
                        a, b = cur[y], ref[y + dy]
                        for x in range(x0, x1):
                            cost += abs(a[x] - b[x + dx])
                    if dy or dx:
                        cost += bias * n
                    cand = (cost, dy * dy + dx * dx, dy, dx)
                    if best is None or cand < best:
                        best = cand
            out[j, i] = best[2:]
    return out


def vectors_loops(rgb, B, R, bias, prev_rgb=None):
    """(N, 3, H, W) uint8 -> (N, by, bx, 2) int8; the first frame against `prev_rgb`, zeros without it."""
    n, _, h, w = rgb.shape
    y = [luma_loops(rgb[f]) for f in range(n)]
    mv = np.zeros((n, -(-h // B), -(-w // B), 2), dtype=np.int8)
    for f in range(n):
        ref = y[f - 1] if f else (None if prev_rgb is None else luma_loops(prev_rgb))
        if ref is not None:
            mv[f] = match_loops(y[f], ref, B, R, bias)
    return mv


def warp_loops(labels, mv, B):
    """(N, H, W), (N, by, bx, 2) -> (N, H, W): out(y, x) = lab(y + dy, x + dx) with the vector of the pixel's block."""
    n, h, w = labels.shape
    out = np.zeros_like(labels)
    for f in range(n):
        for y in range(h):
            for x in range(w):
                dy, dx = (int(v) for v in mv[f, y // B, x // B])
                out[f, y, x] = labels[f, y + dy, x + dx]
    return out


def frames_case(kind, h, w, n=3, seed=0, shift=(2, -3)):
    """n frames (n, 3, h, w) uint8.  'noise': independent noise per frame; 'shift': frame f is a large noise canvas seen
    through a window that moves by `shift` per frame, so frame f at (y, x) equals frame f - 1 at (y + shift[0], x + shift[1]);
    'flat': one colour; 'binary': 0 / 255 noise in 3 x 3 cells, the same value on the three channels -- many equal costs."""
    rng = np.random.default_rng(1000 * h + 10 * w + seed)
    if kind == 'noise':
        return rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)
    if kind == 'flat':
        return np.full((n, 3, h, w), 93, dtype=np.uint8)
    if kind == 'binary':
        cells = rng.integers(0, 2, (n, 1, -(-h // 3), -(-w // 3)), dtype=np.uint8) * 255
        return np.ascontiguousarray(np.repeat(np.repeat(np.repeat(cells, 3, axis=2), 3, axis=3)[:, :, :h, :w], 3, axis=1))
    if kind == 'shift':
        sy, sx = shift
        pad = n * max(abs(sy), abs(sx))
        canvas = rng.integers(0, 256, (3, h + 2 * pad, w + 2 * pad), dtype=np.uint8)
        # frame f shows canvas[pad + f * sy + y, pad + f * sx + x]: f(y, x) == (f - 1)(y + sy, x + sx)
        return np.stack([canvas[:, pad + f * sy:pad + f * sy + h, pad + f * sx:pad + f * sx + w] for f in range(n)])
    raise ValueError(kind)


def interior_blocks(h, w, B, shift):
    """Boolean (by, bx): the blocks for which `shift` is a valid candidate."""
    by, bx = -(-h // B), -(-w // B)
    ok = np.zeros((by, bx), dtype=bool)
    for j in range(by):
        for i in range(bx):
            y0, y1, x0, x1 = j * B, min(j * B + B, h), i * B, min(i * B + B, w)
            ok[j, i] = y0 + shift[0] >= 0 and y1 + shift[0] <= h and x0 + shift[1] >= 0 and x1 + shift[1] <= w
    return ok


def blob_labels(n, h, w, n_obj, seed=0):
    """(n, h, w) uint8 maps in 0..n_obj: a few rectangles per label and frame over a background with speckle."""
    rng = np.random.default_rng(77 * h + w + seed)
    out = np.zeros((n, h, w), dtype=np.uint8)
    for f in range(n):
        for o in range(1, n_obj + 1):
            for _ in range(3):
                y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
                out[f, y:y + int(rng.integers(1, max(2, h // 3))), x:x + int(rng.integers(1, max(2, w // 3)))] = o
        speck = rng.random((h, w)) < 0.03
        out[f][speck] = rng.integers(0, n_obj + 1, int(speck.sum()), dtype=np.uint8)
    return out


def moving_object(seed=0, n=4, h=48, w=128):
    """The scenario of a fast object: a noise background that does not move, a 12 x 12 textured square of label 1 at rows
    14..25 and columns 5 + 22 f.., and from frame 1 on a static 4 x 4 blob of label 1 at rows 40..43, columns 100..103 (a
    look-alike: the frames show nothing there).  Returns rgb (n, 3, h, w) uint8, labels (n, h, w) uint8, and the object's and
    the blob's masks (n, h, w) bool."""
    rng = np.random.default_rng(seed)
    back = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    tex = rng.integers(0, 256, (3, 12, 12), dtype=np.uint8)
    rgb = np.repeat(back[None], n, axis=0)
    lab = np.zeros((n, h, w), dtype=np.uint8)
    obj, blob = np.zeros((n, h, w), dtype=bool), np.zeros((n, h, w), dtype=bool)
    for f in range(n):
        x = 5 + 22 * f
        rgb[f, :, 14:26, x:x + 12] = tex
        obj[f, 14:26, x:x + 12] = True
        if f >= 1:
            blob[f, 40:44, 100:104] = True
    lab[obj | blob] = 1
    return rgb, lab, obj, blob
