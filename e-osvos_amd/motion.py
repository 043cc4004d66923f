"""Block motion between consecutive frames and the warp of a label map by it: what lets the two temporal rules of the
clean-up -- the `gate` of the component filter (`components.py`, rule 1) and `prev_overlap` of the hole filler (`holes.py`,
rule 4) -- compare a frame with the previous frame's cleaned map where the object IS now, not where it was.  Both rules read
that map at the same pixel coordinates, which is right only while an object moves less than the gate between two frames; a
fast object is removed on every second frame, and on the frames in between a static look-alike is kept because the label is
absent from the previous map.  The OSVOS / PReMVOS family propagates the previous mask by motion before it compares; this is
that step as exhaustive block matching on 8-bit luma, in integers, so that the device equals the numpy twin below bit for bit.
The reference has no such step; this is an opt-in extension (`config.MOTION`), off by default.

    motion = {'block': 0, 'radius': 16, 'bias': 2}                                                            (`DEFAULTS`)

block B: 0 = off, else 8 or 16; radius R in [1, 32]; bias in [0, 255].  Frames of at most 4096 pixels a side.
`eval_motion.block=8 eval_motion.radius=24` are example values: NOTHING here is tuned on data.

The rules (include/eosvos.h states them at `eosvos_block_motion` / `eosvos_warp_labels`; the kernels are
csrc/motion_kernels.hip; `vectors_host` / `warp_host` below are their numpy twin: the reference of the device tests and the
path of engines without the entry point; the twin itself is checked against the plain loops of tests/motion_ref.py).  Every
quantity is an integer.  Input: rgb (N, 3, H, W) uint8, planar, the frames of one sequence in order (`snap.quantise` makes
them from the engine's fp32 frames).

  1. luma     Y = (77 R + 150 G + 29 B + 128) >> 8, a uint8.
  2. blocks   by = ceil(H / B), bx = ceil(W / B); block (j, i) covers rows [jB, min(jB + B, H)) and columns
              [iB, min(iB + B, W)), n = its pixel count: the blocks at the lower and right border are smaller, and a frame
              smaller than one block is one partial block.
  3. candidates  for frame f against frame f - 1, a displacement (dy, dx) with |dy|, |dx| <= R is valid for a block when the
              whole block, shifted by it, lies inside the frame.  (0, 0) is always valid.
  4. cost     cost(d) = sum over the block of |Y_f(y, x) - Y_{f-1}(y + dy, x + dx)|, plus bias * n for d != (0, 0): the bias
              keeps flat regions at rest.
  5. choice   the valid candidate that is smallest under the lexicographic order (cost, dy^2 + dx^2, dy, dx).  It packs
              into one 64-bit key, cost << 26 | (dy^2 + dx^2) << 14 | (dy + 32) << 7 | (dx + 32) (cost <= 2 * 65280 < 2^17,
              then 12 + 7 + 7 bits), so a single integer min decides, in whatever order it is reduced.
  6. output   mv (N, by, bx, 2) int8, (dy, dx) per block.  The first frame of a call is matched against `prev_rgb`
              (3, H, W), the frame before it -- that is how a sequence is chunked; without `prev_rgb` it gets zeros.
  7. warp     out(y, x) = lab(y + dy, x + dx) with the vector of the pixel's block: the map of frame f - 1 as frame f would
              see it.  Rule 3 keeps every read inside the frame; a vector from elsewhere that leaves it is clamped to the
              border.
  8. chain    merge -> CRF -> snap -> components -> holes, with `motion` active: the vectors of all frames are computed once;
              a stage whose temporal rule is on (`gate` > 0, `prev_overlap` > 0) then runs one frame per call in ascending
              order, out[f] = stage(labels[f], prev = warp(out[f - 1], mv[f])); frame 0 has no prev, the `keep` frames pass
              unchanged and are still warped for their successor.  A stage whose temporal rule is off keeps its single
              batched call.  `motion` needs the frames, like `snap`, and at least one of the two rules to serve.
  9. off      `None` or block = 0: nothing new is called (`active`).
"""
import numbers

import numpy as np
import torch

DEFAULTS = {'block': 0, 'radius': 16, 'bias': 2}
BLOCKS = (8, 16)
MAX_RADIUS = 32
MAX_BIAS = 255
MAX_SIDE = 4096
SCRATCH_CAP = 512 << 20             # bytes of engine scratch one `eosvos_block_motion` call may take
_KEY_OFFSET = 32                    # dy and dx enter the key as dy + 32, dx + 32: 0..64, order preserved


def check(cfg):
    """The complete, validated parameter dictionary of `cfg` (missing keys take `DEFAULTS`); ValueError otherwise."""
    if not isinstance(cfg, dict) or set(cfg) - set(DEFAULTS):
        raise ValueError(f'motion={cfg!r}: a dictionary with keys from {sorted(DEFAULTS)}')
    out = dict(DEFAULTS, **cfg)
    v = out['block']
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not (v == 0 or v in BLOCKS):
        raise ValueError(f'motion.block={v!r}: 0 (off), 8 or 16')
    out['block'] = int(v)
    for k, lo, hi in (('radius', 1, MAX_RADIUS), ('bias', 0, MAX_BIAS)):
        v = out[k]
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= v <= hi:
            raise ValueError(f'motion.{k}={v!r}: an integer in [{lo}, {hi}]')
        out[k] = int(v)
    return out


def active(cfg):
    """Validated; False when `cfg` estimates nothing (None or block 0)."""
    return cfg is not None and check(cfg)['block'] != 0


def grid(height, width, block):
    """(by, bx): the blocks of a frame."""
    return (height + block - 1) // block, (width + block - 1) // block


def plane_bytes(height, width):
    """The bytes of one luma plane in the engine's scratch: rows padded to a multiple of four bytes."""
    return height * ((width + 3) // 4 * 4)


def frames_per_call(height, width):
    """How many frames one `eosvos_block_motion` call may take under the scratch cap: one luma plane per frame and one for
    the frame before the first (at least 1)."""
    return max(1, min(SCRATCH_CAP // plane_bytes(height, width) - 1, 65534))


def _as_numpy(a, dtype):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.dtype != dtype:
        raise ValueError(f'motion: expected {np.dtype(dtype).name}, got {a.dtype}')
    return a


def _check_rgb(who, rgb, prev_rgb=None):
    if rgb.ndim != 4 or rgb.shape[1] != 3 or min(rgb.shape[2:]) < 1 or max(rgb.shape[2:]) > MAX_SIDE:
        raise ValueError(f'{who}: rgb must be (N, 3, H, W) with 1 <= H, W <= {MAX_SIDE}, got {tuple(rgb.shape)}')
    if prev_rgb is not None and tuple(prev_rgb.shape) != tuple(rgb.shape[1:]):
        raise ValueError(f'{who}: prev_rgb {tuple(prev_rgb.shape)} is not one frame of rgb {tuple(rgb.shape)}')


def _check_mv(who, labels, mv, block):
    if block not in BLOCKS:
        raise ValueError(f'{who}: block={block!r}: 8 or 16')
    if labels.ndim != 3 or min(labels.shape[1:]) < 1 or max(labels.shape[1:]) > MAX_SIDE:
        raise ValueError(f'{who}: labels must be (N, H, W) with 1 <= H, W <= {MAX_SIDE}, got {tuple(labels.shape)}')
    want = (labels.shape[0],) + grid(labels.shape[1], labels.shape[2], block) + (2,)
    if tuple(mv.shape) != want:
        raise ValueError(f'{who}: mv must be {want} for labels {tuple(labels.shape)} and block {block}, got {tuple(mv.shape)}')


def luma_host(rgb):
    """Rule 1: rgb (..., 3, H, W) uint8 -> Y (..., H, W) uint8."""
    c = rgb.astype(np.int64)
    return ((77 * c[..., 0, :, :] + 150 * c[..., 1, :, :] + 29 * c[..., 2, :, :] + 128) >> 8).astype(np.uint8)


def _match(cur, ref, B, R, bias):
    """Rules 2-5 on one pair of luma planes (H, W) uint8 -> (by, bx, 2) int8.  One pass per candidate over the whole frame:
    the absolute differences where the shifted pixel exists, their sums per block by `np.add.reduceat`, the key of rule 5, a
    running minimum."""
    h, w = cur.shape
    by, bx = grid(h, w, B)
    y0, x0 = np.arange(by, dtype=np.int64) * B, np.arange(bx, dtype=np.int64) * B
    y1, x1 = np.minimum(y0 + B, h), np.minimum(x0 + B, w)                # exclusive
    n = (y1 - y0)[:, None] * (x1 - x0)[None, :]
    a, b = cur.astype(np.int64), ref.astype(np.int64)
    best = np.full((by, bx), np.iinfo(np.int64).max, dtype=np.int64)
    for dy in range(-R, R + 1):
        oky = (y0 + dy >= 0) & (y1 + dy <= h)
        if not oky.any():
            continue
        ya, yb = max(0, -dy), min(h, h - dy)                             # rows of cur whose shifted row exists
        for dx in range(-R, R + 1):
            okx = (x0 + dx >= 0) & (x1 + dx <= w)
            if not okx.any():
                continue
            xa, xb = max(0, -dx), min(w, w - dx)
            diff = np.zeros((h, w), dtype=np.int64)
            diff[ya:yb, xa:xb] = np.abs(a[ya:yb, xa:xb] - b[ya + dy:yb + dy, xa + dx:xb + dx])
            cost = np.add.reduceat(np.add.reduceat(diff, y0, axis=0), x0, axis=1)
            if dy or dx:
                cost = cost + bias * n
            key = (cost << 26) | ((dy * dy + dx * dx) << 14) | ((dy + _KEY_OFFSET) << 7) | (dx + _KEY_OFFSET)
            ok = oky[:, None] & okx[None, :]
            best = np.where(ok & (key < best), key, best)
    out = np.empty((by, bx, 2), dtype=np.int8)
    out[..., 0] = ((best >> 7) & 127) - _KEY_OFFSET
    out[..., 1] = (best & 127) - _KEY_OFFSET
    return out


def vectors_host(rgb, params, prev_rgb=None):
    """Rules 1-6 in numpy: rgb (N, 3, H, W) uint8, prev_rgb (3, H, W) uint8 or None -> mv (N, by, bx, 2) int8 (a numpy
    array)."""
    p = check(params)
    rgb = _as_numpy(rgb, np.uint8)
    prev_rgb = None if prev_rgb is None else _as_numpy(prev_rgb, np.uint8)
    _check_rgb('vectors_host', rgb, prev_rgb)
    if p['block'] == 0:
        raise ValueError('vectors_host: motion.block is 0 (off)')
    n, _, h, w = rgb.shape
    y = luma_host(rgb)
    mv = np.zeros((n,) + grid(h, w, p['block']) + (2,), dtype=np.int8)
    for f in range(n):
        ref = y[f - 1] if f else (None if prev_rgb is None else luma_host(prev_rgb))
        if ref is not None:
            mv[f] = _match(y[f], ref, p['block'], p['radius'], p['bias'])
    return mv


def warp_host(labels, mv, block):
    """Rule 7 in numpy: labels (N, H, W), mv (N, by, bx, 2) int8 -> warped maps (N, H, W) of the labels' dtype (a numpy
    array); frame n is warped by mv[n]."""
    lab = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    mv = _as_numpy(mv, np.int8)
    _check_mv('warp_host', lab, mv, block)
    n, h, w = lab.shape
    jj, ii = np.arange(h) // block, np.arange(w) // block
    out = np.empty_like(lab)
    for f in range(n):
        d = mv[f][jj][:, ii].astype(np.int64)                            # (H, W, 2): the vector of every pixel's block
        yy = np.clip(np.arange(h)[:, None] + d[..., 0], 0, h - 1)
        xx = np.clip(np.arange(w)[None, :] + d[..., 1], 0, w - 1)
        out[f] = lab[f][yy, xx]
    return out


def vectors(engine, rgb, params, prev_rgb=None):
    """The block vectors of `rgb` (N, 3, H, W) uint8 on `engine`: its `block_motion` (the device kernels) where it has the
    entry point, else `vectors_host` (stand-in engines of host tests).  Returns an int8 tensor (N, by, bx, 2) on rgb's
    device."""
    p = check(params)
    if hasattr(engine, 'block_motion'):
        return engine.block_motion(rgb, prev_rgb=prev_rgb, **p)
    return torch.from_numpy(vectors_host(rgb, p, prev_rgb=prev_rgb)).to(rgb.device)


def warp(engine, labels, mv, block):
    """`labels` (N, H, W) uint8 warped by `mv` (N, by, bx, 2) int8 on `engine`: its `warp_labels` where it has the entry
    point, else `warp_host`.  Returns a uint8 tensor on the labels' device."""
    if hasattr(engine, 'warp_labels'):
        return engine.warp_labels(labels, mv, block)
    return torch.from_numpy(warp_host(labels, mv, block)).to(labels.device)
