"""Lucid first-frame synthesis for the one-shot fine-tune: some samples of every round-0 batch are composed from the annotated
frame with the object and its background moved INDEPENDENTLY.  The reference's only first-frame augmentation is the flip +
scale + rotate of the whole frame about the image centre (`custom_transforms.FirstFrameAugmenter`): in every training sample
the object sits in the same place relative to its background, with the same neighbours, while in the rest of the video it moves
against that background.  The OSVOS family's answer is "lucid data dreaming" (Khoreva et al.; the PReMVOS / OSVOS-S line of
DAVIS entries): cut the object out, fill the hole, move object and background on their own, compose them again.  This is an
opt-in extension (`config.LUCID`), off by default; the adaptation rounds and the meta-training feed are not touched.

    lucid = {'samples': 0, 'dilate': 4, 'rot': 15.0, 'scale': 0.15, 'shift': 0.1,
             'bg_rot': 5.0, 'bg_scale': 0.05, 'bg_shift': 0.05, 'min_keep': 0.5}                              (`DEFAULTS`)

  samples                     how many of a round-0 batch's samples are synthesised; 0 = off; above the batch size: cut to it
  dilate                      the hole is the mask grown by this Chebyshev radius (the object's halo leaves the background);
                              an integer in [0, 16]
  rot, scale, shift           the object's own motion about the centre of the mask's bounding box: angle in +-rot degrees,
                              factor in [1 - scale, 1 + scale], translation in +-shift * (H, W); rot in [0, 45], scale in
                              [0, 0.5], shift in [0, 1]
  bg_rot, bg_scale, bg_shift  the same for the background plate, about the frame centre; same ranges
  min_keep                    a sample is accepted only if at least this share of the mask's pixel count is still labelled;
                              in (0, 1]
`eval_lucid.samples=2 eval_lucid.shift=0.1` are example values: NOTHING here is tuned on data.

The rules (include/eosvos.h states 1-9 at `eosvos_lucid_plate` / `eosvos_lucid_compose`; the kernels are
csrc/lucid_kernels.hip; `plate_host` and `compose_host` below are the numpy twins, checked against the plain loops of
tests/lucid_ref.py; `batch_host` is rules 10-12 on the twins).  frame (C, H, W) fp32, mask (1, H, W) fp32, object = mask != 0.

PLATE, the frame with the object removed; once per (sequence, object), before round 0:
  1. hole      hole(y, x) = 1 iff a pixel with mask != 0 lies within Chebyshev distance `dilate`, inside the frame;
               known = !hole.
  2. level 0   H x W: v0 = frame where known, else 0; k0 = known.
  3. push      level l + 1 is ceil(H_l / 2) x ceil(W_l / 2): k = OR of the up to four children (2y + i, 2x + j) inside level
               l; v = the sum of the known children's v in the order (0,0), (0,1), (1,0), (1,1) divided by their number, 0 if
               none is known.  Levels go down to 1 x 1 whatever the data: their number depends on (H, W) only.
  4. pull      l = top - 1 .. 0: a pixel with k_l = 0 takes the bilinear sample of the completed level l + 1 at
               ((y + 0.5) / 2 - 0.5, (x + 0.5) / 2 - 0.5) -- a fixed ratio of 2, weights 1/4 and 3/4, both taps clamped to
               the level.  Known pixels keep their value.
  5. plate     = v0.  Known pixels carry the frame's bits; no known pixel: an all-zero plate.  fp32, no atomics,
               deterministic, independent of what the scratch held (`EOSVOS_DEBUG_FILL` changes no bit).
COMPOSE, one launch for all lucid samples of a batch; per sample `flip`, an inverse background matrix Bi and an inverse object
matrix Oi (2 x 3 doubles, built and inverted on the host: `sample_matrices`), travelling by value with the launch:
  6. coords    output pixel (y, x): xm = flip ? W - 1 - x : x; the source coordinates are the 10-bit fixed point of
               `warp_affine_kernel`, entry by entry with its roundings, the interpolating round_delta 16 and 5 fractional
               bits (`fixed_coords`), evaluated at (y, xm) once for Bi and once for Oi.
  7. coverage  A = sum over the 2 x 2 bilinear taps at the object coordinates of wy_i * wx_j * [mask != 0], integer weights
               (32 - f, f), taps outside the frame 0: an integer in [0, 1024].  label = (A >= 512), alpha = A / 1024, exact.
  8. image     Bg = bicubic sample of the plate at the background coordinates, Ob = bicubic sample of the frame at the object
               coordinates (the warp kernel's a = -0.75 table at 1/32 pixel, taps outside the frame 0; Ob only where A > 0);
               image = Ob where A == 1024, Bg where A == 0, Bg + alpha * (Ob - Bg) otherwise, in fp32.
  9. count     count[s] = the number of labelled pixels of sample s, an integer sum on a record the call zeroes itself.
BATCH (`run_batch`, shared by the twin and the device path):
 10. accept    sample s is accepted iff count[s] * 65536 >= round(min_keep * 65536) * n_mask and count[s] < H * W.  Rejected
               samples are redrawn in sample order and composed again, all rejected samples of a batch in one launch followed
               by one host read.  After `MAX_TRIES` = 8 attempts a sample takes the identity object matrix with its last
               background draw.
 11. draws     Python's `random`, in the state `set_random_seeds` left, per sample in this order: flip (`random() < 0.5`),
               bg_rot, bg_scale, bg_shift y, bg_shift x, rot, scale, shift y, shift x, each uniform in its range
               ((2 * random() - 1) * range).  A redraw repeats the four object draws only.  The forward matrix is
               T(c + t) . R . S . T(-c) in double (`forward_matrix`), cv2's sign of the angle; c = (W / 2, H / 2) for the
               background and the centre of the mask's bounding box, ((x0 + x1 + 1) / 2, (y0 + y1 + 1) / 2), for the object.
 12. layout    with k = min(samples, batch), the first batch - k samples come from today's path (`FirstFrameAugmenter`,
               `_repeat_batch` or the caller's `augment`), called for batch - k samples and not at all when that is 0; the
               last k are synthesised.  Only round 0 is touched.  A mask that is empty or fills the frame is not synthesised:
               the whole batch takes today's path.
 13. off       `None` or samples = 0: nothing new is called, nothing is drawn (`active`).
"""
import math
import numbers
import random

import numpy as np
import torch

DEFAULTS = {'samples': 0, 'dilate': 4, 'rot': 15.0, 'scale': 0.15, 'shift': 0.1, 'bg_rot': 5.0, 'bg_scale': 0.05,
            'bg_shift': 0.05, 'min_keep': 0.5}
MAX_DILATE = 16
MAX_ROT = 45
MAX_SCALE = 0.5
MAX_SIDE = 4096
MAX_TRIES = 8
MAX_SAMPLES_PER_LAUNCH = 16                              # csrc/kernels.h LUCID_MAX_SAMPLES
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
ROUND_DELTA = 16                                         # AB_SCALE / INTER_TAB_SIZE / 2 of cv::warpAffine


def _real(v):
    return not isinstance(v, bool) and isinstance(v, numbers.Real)


def _int(v):
    return not isinstance(v, bool) and isinstance(v, numbers.Integral)


def check(cfg):
    """The complete, validated parameter dictionary of `cfg` (missing keys take `DEFAULTS`); ValueError otherwise."""
    if not isinstance(cfg, dict) or set(cfg) - set(DEFAULTS):
        raise ValueError(f'lucid={cfg!r}: a dictionary with keys from {sorted(DEFAULTS)}')
    out = dict(DEFAULTS, **cfg)
    v = out['samples']
    if not _int(v) or v < 0:
        raise ValueError(f'lucid.samples={v!r}: an integer >= 0 (0 = off)')
    out['samples'] = int(v)
    v = out['dilate']
    if not _int(v) or not 0 <= v <= MAX_DILATE:
        raise ValueError(f'lucid.dilate={v!r}: an integer in [0, {MAX_DILATE}]')
    out['dilate'] = int(v)
    for k, hi in (('rot', MAX_ROT), ('bg_rot', MAX_ROT), ('scale', MAX_SCALE), ('bg_scale', MAX_SCALE), ('shift', 1), ('bg_shift', 1)):
        v = out[k]
        if not _real(v) or not 0 <= v <= hi:
            raise ValueError(f'lucid.{k}={v!r}: a number in [0, {hi}]')
        out[k] = float(v)
    v = out['min_keep']
    if not _real(v) or not 0 < v <= 1:
        raise ValueError(f'lucid.min_keep={v!r}: a number in (0, 1]')
    out['min_keep'] = float(v)
    return out


def active(cfg):
    """Validated; False when `cfg` synthesises nothing (None or samples 0)."""
    return cfg is not None and check(cfg)['samples'] != 0


# ---- the matrices: one host function for the twin and the device path -----------------------------------------------------
def forward_matrix(cx, cy, rot_deg, factor, tx, ty):
    """T(c + t) . R . S . T(-c) as (m0 .. m5), X = m0 x + m1 y + m2, Y = m3 x + m4 y + m5; cv2.getRotationMatrix2D's sign."""
    a = math.radians(rot_deg)
    al, be = math.cos(a) * factor, math.sin(a) * factor
    return (al, be, (1 - al) * cx - be * cy + tx, -be, al, be * cx + (1 - al) * cy + ty)


def invert(m):
    """The inverse of a 2 x 3 affine matrix, with cv::warpAffine's expressions."""
    d = m[0] * m[4] - m[1] * m[3]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[4] * d, m[0] * d
    m0, m1, m3, m4 = a11, m[1] * -d, m[3] * -d, a22
    return (m0, m1, -m0 * m[2] - m1 * m[5], m3, m4, -m3 * m[2] - m4 * m[5])


def mask_geometry(mask):
    """(n_mask, object centre (cx, cy) or None) of a mask (1, H, W) / (H, W), tensor or array: the count of mask != 0 and the
    centre of its bounding box."""
    m = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    m = m.reshape(m.shape[-2:]) != 0
    n = int(m.sum())
    if n == 0:
        return 0, None
    rows, cols = np.flatnonzero(m.any(axis=1)), np.flatnonzero(m.any(axis=0))
    return n, ((int(cols[0]) + int(cols[-1]) + 1) / 2.0, (int(rows[0]) + int(rows[-1]) + 1) / 2.0)


def _uniform(rng, r):
    return (2.0 * rng.random() - 1.0) * r


def draw_motion(rng, p, prefix=''):
    """The four draws of one motion, in rule 11's order: (angle, factor, shift y, shift x) with the shifts as shares."""
    return (_uniform(rng, p[prefix + 'rot']), 1.0 + _uniform(rng, p[prefix + 'scale']), _uniform(rng, p[prefix + 'shift']),
            _uniform(rng, p[prefix + 'shift']))


def draw_sample(rng, p):
    """The nine draws of one sample: {'flip', 'bg', 'ob'}."""
    flip = rng.random() < 0.5
    return {'flip': flip, 'bg': draw_motion(rng, p, 'bg_'), 'ob': draw_motion(rng, p)}


def sample_matrices(draw, height, width, centre):
    """A draw -> the compose parameters {'flip', 'Bi', 'Oi'} (the inverse matrices as 6-tuples of Python floats)."""
    rot, fac, sy, sx = draw['bg']
    bi = invert(forward_matrix(width / 2.0, height / 2.0, rot, fac, sx * width, sy * height))
    if draw['ob'] is None:                               # the fallback of rule 10
        oi = IDENTITY
    else:
        rot, fac, sy, sx = draw['ob']
        oi = invert(forward_matrix(centre[0], centre[1], rot, fac, sx * width, sy * height))
    return {'flip': bool(draw['flip']), 'Bi': bi, 'Oi': oi}


def accepted(count, n_mask, height, width, min_keep):
    """Rule 10 on integers."""
    return count * 65536 >= int(round(min_keep * 65536)) * n_mask and count < height * width


def run_batch(compose, k, params, n_mask, height, width, centre, rng=random):
    """Rules 10-11 around `compose(plist, read) -> (images, labels, counts or None)`: k synthesised samples.  Returns (images
    (k, C, H, W), labels (k, 1, H, W), records): one record per sample with its draw, its compose parameters, `tries`, `count`
    and `fallback`."""
    p = check(params)
    draws = [draw_sample(rng, p) for _ in range(k)]
    plist = [sample_matrices(d, height, width, centre) for d in draws]
    images, labels, counts = compose(plist, True)
    counts = [int(c) for c in counts]
    tries = [1] * k
    pending = [s for s in range(k) if not accepted(counts[s], n_mask, height, width, p['min_keep'])]
    attempt = 1
    while pending and attempt < MAX_TRIES:
        attempt += 1
        for s in pending:
            draws[s] = dict(draws[s], ob=draw_motion(rng, p))
            plist[s] = sample_matrices(draws[s], height, width, centre)
            tries[s] = attempt
        im, lb, cn = compose([plist[s] for s in pending], True)
        images[pending], labels[pending] = im, lb
        for s, c in zip(pending, cn):
            counts[s] = int(c)
        pending = [s for s in pending if not accepted(counts[s], n_mask, height, width, p['min_keep'])]
    fallback = set(pending)
    if pending:
        for s in pending:
            draws[s] = dict(draws[s], ob=None)
            plist[s] = sample_matrices(draws[s], height, width, centre)
        im, lb, _ = compose([plist[s] for s in pending], False)
        images[pending], labels[pending] = im, lb
    records = [dict(plist[s], draw=draws[s], tries=tries[s], count=None if s in fallback else counts[s], fallback=s in fallback)
               for s in range(k)]
    return images, labels, records


# ---- the numpy twins ------------------------------------------------------------------------------------------------------
def _np(t, dtype=None):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a if dtype is None else a.astype(dtype)


def _frame_and_mask(who, frame, mask):
    f, m = _np(frame), _np(mask)
    if f.dtype != np.float32 or f.ndim != 3:
        raise ValueError(f'{who}: frame must be (C, H, W) float32, got {f.dtype} {f.shape}')
    if m.ndim == 3 and m.shape[0] == 1:
        m = m[0]
    if m.shape != f.shape[1:] or min(m.shape) < 1 or max(m.shape) > MAX_SIDE:
        raise ValueError(f'{who}: mask must be (1, H, W) or (H, W) of the frame\'s size with 1 <= H, W <= {MAX_SIDE}, got {m.shape}')
    return f, m != 0


def levels(height, width):
    """[(H_l, W_l)] from level 0 down to 1 x 1."""
    out = [(int(height), int(width))]
    while out[-1] != (1, 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def hole_host(on, dilate):
    """Rule 1: boolean (H, W) -> the mask grown by the Chebyshev radius `dilate` (a row pass, then a column pass)."""
    h, w = on.shape
    rows = np.zeros_like(on)
    for d in range(-dilate, dilate + 1):
        src = slice(max(0, d), min(w, w + d))
        dst = slice(max(0, -d), min(w, w - d))
        rows[:, dst] |= on[:, src]
    hole = np.zeros_like(on)
    for d in range(-dilate, dilate + 1):
        src = slice(max(0, d), min(h, h + d))
        dst = slice(max(0, -d), min(h, h - d))
        hole[dst] |= rows[src]
    return hole


def plate_host(frame, mask, dilate, dtype=np.float32):
    """Rules 1-5 in numpy: frame (C, H, W) fp32, mask (1, H, W) or (H, W) -> the plate (C, H, W) of `dtype`."""
    f, on = _frame_and_mask('plate_host', frame, mask)
    if not _int(dilate) or not 0 <= dilate <= MAX_DILATE:
        raise ValueError(f'plate_host: dilate={dilate!r}: an integer in [0, {MAX_DILATE}]')
    dt = np.dtype(dtype).type
    known = ~hole_host(on, int(dilate))
    sizes = levels(*on.shape)
    v = [np.where(known[None], f.astype(dt), dt(0))]
    k = [known]
    for l in range(1, len(sizes)):
        (hl, wl), (hn, wn) = sizes[l - 1], sizes[l]
        pv = np.zeros((f.shape[0], 2 * hn, 2 * wn), dtype=dt)
        pk = np.zeros((2 * hn, 2 * wn), dtype=bool)
        pv[:, :hl, :wl], pk[:hl, :wl] = v[-1], k[-1]
        total = np.zeros((f.shape[0], hn, wn), dtype=dt)
        n = np.zeros((hn, wn), dtype=np.int64)
        for i in (0, 1):
            for j in (0, 1):
                ck = pk[i::2, j::2]
                total = total + np.where(ck[None], pv[:, i::2, j::2], dt(0))
                n += ck
        v.append(np.where(n[None] > 0, total / np.maximum(n, 1)[None].astype(dt), dt(0)).astype(dt))
        k.append(n > 0)
    for l in range(len(sizes) - 2, -1, -1):
        (hl, wl), (hn, wn) = sizes[l], sizes[l + 1]
        ys, xs = np.arange(hl), np.arange(wl)
        y0, y1 = np.clip((ys - 1) >> 1, 0, hn - 1), np.clip(((ys - 1) >> 1) + 1, 0, hn - 1)
        x0, x1 = np.clip((xs - 1) >> 1, 0, wn - 1), np.clip(((xs - 1) >> 1) + 1, 0, wn - 1)
        ly = np.where(ys & 1, dt(0.25), dt(0.75)).astype(dt)[None, :, None]
        lx = np.where(xs & 1, dt(0.25), dt(0.75)).astype(dt)[None, None, :]
        hy, hx = dt(1) - ly, dt(1) - lx
        up = v[l + 1]
        top = hx * up[:, y0][:, :, x0] + lx * up[:, y0][:, :, x1]
        bot = hx * up[:, y1][:, :, x0] + lx * up[:, y1][:, :, x1]
        v[l] = np.where(k[l][None], v[l], hy * top + ly * bot).astype(dt)
    return v[0]


def cubic_table():
    """The a = -0.75 cubic coefficients at 1/32 pixel, (32, 4) float32, in the float arithmetic of the engine's table."""
    f = np.float32
    tab = np.empty((32, 4), dtype=np.float32)
    a = f(-0.75)
    for i in range(32):
        x = f(i) * f(1.0 / 32)
        x1, xm = x + f(1), f(1) - x
        tab[i, 0] = ((a * x1 - f(5) * a) * x1 + f(8) * a) * x1 - f(4) * a
        tab[i, 1] = ((a + f(2)) * x - (a + f(3))) * x * x + f(1)
        tab[i, 2] = ((a + f(2)) * xm - (a + f(3))) * xm * xm + f(1)
        tab[i, 3] = f(1) - tab[i, 0] - tab[i, 1] - tab[i, 2]
    return tab


def fixed_coords(m, height, width, flip):
    """Rule 6: the inverse matrix m (6 doubles) -> (Y, X) int64 (H, W) with 5 fractional bits, `warp_fix` entry by entry."""
    ys = np.arange(height, dtype=np.float64)
    xm = np.arange(width, dtype=np.float64)
    if flip:
        xm = (width - 1) - xm
    m = [np.float64(v) for v in m]

    def fix_row(a, b):
        return np.rint((a * ys + b) * 1024.0).astype(np.int64) + ROUND_DELTA

    def fix_col(a):
        return np.rint((a * xm) * 1024.0).astype(np.int64)
    xf = fix_row(m[1], m[2])[:, None] + fix_col(m[0])[None, :]
    yf = fix_row(m[4], m[5])[:, None] + fix_col(m[3])[None, :]
    return yf >> 5, xf >> 5


def _cubic(src, yq, xq, tab, dt):
    """The bicubic sample of src (C, H, W) of dtype dt at the 5-bit coordinates: 16 taps added one by one, rows first."""
    _, h, w = src.shape
    sy, sx = (yq >> 5) - 1, (xq >> 5) - 1
    cy, cx = tab[yq & 31].astype(dt), tab[xq & 31].astype(dt)      # (H, W, 4)
    total = np.zeros((src.shape[0],) + yq.shape, dtype=dt)
    for i in range(4):
        yy = sy + i
        for j in range(4):
            xx = sx + j
            inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            tap = src[:, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
            total = total + np.where(inside[None], tap * (cy[..., i] * cx[..., j])[None], dt(0))
    return total


def compose_host(frame, mask, plate, params, dtype=np.float32):
    """Rules 6-9 in numpy: frame (C, H, W) fp32, mask, plate (C, H, W), params = [{'flip', 'Bi', 'Oi'}] -> (images
    (S, C, H, W) of `dtype`, labels (S, 1, H, W) float32 of 0 / 1, counts (S,) int64)."""
    f, on = _frame_and_mask('compose_host', frame, mask)
    dt = np.dtype(dtype).type
    pl = _np(plate).astype(dt)
    if pl.shape != f.shape:
        raise ValueError(f'compose_host: plate must be {f.shape}, got {pl.shape}')
    if not params:
        raise ValueError('compose_host: no sample')
    fr = f.astype(dt)
    c, h, w = f.shape
    tab = cubic_table()
    images = np.empty((len(params), c, h, w), dtype=dt)
    labels = np.empty((len(params), 1, h, w), dtype=np.float32)
    for s, prm in enumerate(params):
        yo, xo = fixed_coords(prm['Oi'], h, w, prm['flip'])
        yb, xb = fixed_coords(prm['Bi'], h, w, prm['flip'])
        oy, ox, fy, fx = yo >> 5, xo >> 5, yo & 31, xo & 31
        cover = np.zeros((h, w), dtype=np.int64)
        for i in (0, 1):
            for j in (0, 1):
                yy, xx = oy + i, ox + j
                inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
                hit = inside & on[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
                cover += np.where(hit, (fy if i else 32 - fy) * (fx if j else 32 - fx), 0)
        bg = _cubic(pl, yb, xb, tab, dt)
        ob = _cubic(fr, yo, xo, tab, dt)
        alpha = (cover.astype(dt) / dt(1024))[None]
        images[s] = np.where(cover[None] == 1024, ob, np.where(cover[None] == 0, bg, bg + alpha * (ob - bg)))
        labels[s, 0] = cover >= 512
    return images, labels, labels.reshape(len(params), -1).sum(axis=1).astype(np.int64)


def batch_host(frame, mask, params, batch, rng=random, dtype=np.float32, plain=None):
    """Rules 10-12 on the twins: a round-0 batch of `batch` samples.  `plain(n) -> (images (n, C, H, W), labels (n, 1, H, W))`
    is today's path, called for the first batch - k samples (not at all for 0, for all of them when the mask is empty or
    fills the frame).  Returns (images, labels, records): numpy arrays and the records of `run_batch` (empty without lucid
    samples)."""
    p = check(params)
    f, on = _frame_and_mask('batch_host', frame, mask)
    h, w = on.shape
    n_mask, centre = mask_geometry(on)
    k = min(p['samples'], batch) if 0 < n_mask < h * w else 0
    parts_i, parts_l, records = [], [], []
    if batch - k:
        im, lb = plain(batch - k)
        parts_i.append(_np(im, dtype))
        parts_l.append(_np(lb, np.float32))
    if k:
        plate = plate_host(f, on, p['dilate'], dtype)
        im, lb, records = run_batch(lambda plist, read: compose_host(f, on, plate, plist, dtype), k, p, n_mask, h, w, centre, rng)
        parts_i.append(im)
        parts_l.append(lb)
    return np.concatenate(parts_i), np.concatenate(parts_l), records


# ---- the device path ------------------------------------------------------------------------------------------------------
class LucidAugmenter:
    """The lucid samples of one (frame, mask) pair on the engine's GPU: the plate is built once, here; `batch(k)` composes k
    samples with one launch and one host read per attempt."""

    def __init__(self, engine, frame, mask, params, rng=random):
        """frame (C, H, W), mask (1, H, W): contiguous fp32 device tensors."""
        self.engine, self.rng = engine, rng
        self.params = check(params)
        if self.params['samples'] == 0:
            raise ValueError('lucid.LucidAugmenter: lucid.samples is 0 (off)')
        self.frame, self.mask = frame, mask
        self.height, self.width = int(frame.shape[1]), int(frame.shape[2])
        self.n_mask, self.centre = mask_geometry(mask)              # the one host read per (sequence, object)
        self.has_object = 0 < self.n_mask < self.height * self.width
        self.plate = engine.lucid_plate(frame, mask, self.params['dilate']) if self.has_object else None

    def _compose(self, plist, read):
        im, lb, cn = [], [], []
        for i in range(0, len(plist), MAX_SAMPLES_PER_LAUNCH):     # one launch up to 16 samples
            a, b, c = self.engine.lucid_compose(self.frame, self.mask, self.plate, plist[i:i + MAX_SAMPLES_PER_LAUNCH], read_counts=read)
            im.append(a)
            lb.append(b)
            cn += c or []
        return (im[0], lb[0], cn) if len(im) == 1 else (torch.cat(im), torch.cat(lb), cn)

    def batch(self, k):
        """k synthesised samples: (images (k, C, H, W), labels (k, 1, H, W), records) as `run_batch`."""
        if not self.has_object:
            raise ValueError('lucid.LucidAugmenter.batch: the mask is empty or fills the frame')
        return run_batch(self._compose, int(k), self.params, self.n_mask, self.height, self.width, self.centre, self.rng)
