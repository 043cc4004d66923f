"""Hole filling of the merged label maps: the stage after the component filter (`components.py`).  The filter removes wrong
foreground; nothing before this stage adds missing foreground.  A one-shot fine-tuned net drops a few pixels inside an object
below 0.5 (highlights, motion blur, thin texture), the arg-max merge leaves a background island there, the CRF often keeps it
and the filter never looks at label 0; the OSVOS family fills such holes after the fact.  Real holes (a bicycle frame, the gap
between legs) are in the ground truth, so a hole is filled only if it is small and most of it was object in the previous
frame's FILLED map -- the chain the filter's gate uses, anchored at the train frame.  The reference has no such step; this is an
opt-in extension (`config.FILL`), off by default.

    holes = {'connectivity': 8, 'max_area': 0, 'max_rel_area': 1.0, 'prev_overlap': 0.0}                       (`DEFAULTS`)

The rules (include/eosvos.h states them at `eosvos_fill_holes`; the kernels are csrc/ccl_kernels.hip; `fill_host` below is
their numpy twin: the reference of the tests and the path of engines without the entry point).  Input: uint8 maps (N, H, W) of
one sequence in frame order, 0 = background, every other value an object label.

  1. background components  two label-0 pixels of a frame are connected under the DUAL of `connectivity`: objects 8-connected
     means background 4-connected (edge neighbours), objects 4-connected means background 8-connected (edge and corner
     neighbours).  Frames never connect.
  2. holes  a background component is a hole when none of its pixels lies on the frame border (x = 0, y = 0, x = W - 1,
     y = H - 1).  Its bordering labels are the non-zero labels among the neighbours (under the background's connectivity) of its
     pixels.  A hole with exactly one bordering label o is a candidate for o; with two or more it is left alone; it cannot
     have none.
  3. size  A = the hole's pixel count, S = the number of pixels equal to o in the frame's INPUT map.  The candidate passes iff
     A <= max_area and A * 65536 <= rq * S with rq = round(max_rel_area * 65536) (integers on every path).
  4. previous frame  R is the FILLED output of frame f - 1 (`prev` for the first frame of a call).  The rule is active for a
     candidate of o when oq = round(prev_overlap * 65536) > 0, R exists and R has a pixel equal to o; then C = the number of the
     hole's pixels p with R[p] == o, and the candidate passes iff C * 65536 >= oq * A.  Inactive: it passes.
  5. fill  pixels of holes that pass become o, everything else is copied.
  6. independence  every decision in a frame is taken on the frame's input map: holes of a frame never influence each other.
  7. keep  frames listed there (the train frames: seeded ground truth) are copied unchanged and still serve as R.
  8. off  max_area = 0 (the default) or max_rel_area = 0 switch the stage off, as does holes=None: nothing new is called
     (`active`).

Nothing here is tuned on data.
"""
import numbers

import numpy as np
import torch

from . import components

DEFAULTS = {'connectivity': 8, 'max_area': 0, 'max_rel_area': 1.0, 'prev_overlap': 0.0}
MAX_AREA = 1 << 24
SCRATCH_CAP = 512 << 20             # bytes of engine scratch one `eosvos_fill_holes` call may take
_BYTES_PER_PIXEL = 24               # parent, tile count, id, area, record, overlap count (32-bit words)
_BYTES_PER_FRAME = 1288             # 256 histogram words, one 64-bit word (pixels filled) and 256 presence bytes
_BYTES_FIXED = 264                  # the presence bytes of `prev` and the padding before the 64-bit words


def check(cfg):
    """The complete, validated parameter dictionary of `cfg` (missing keys take `DEFAULTS`); ValueError otherwise."""
    if not isinstance(cfg, dict) or set(cfg) - set(DEFAULTS):
        raise ValueError(f'holes={cfg!r}: a dictionary with keys from {sorted(DEFAULTS)}')
    out = dict(DEFAULTS, **cfg)
    v = out['max_area']
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v <= MAX_AREA:
        raise ValueError(f'holes.max_area={v!r}: an integer in [0, {MAX_AREA}]')
    out['max_area'] = int(v)
    v = out['connectivity']
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v not in (4, 8):
        raise ValueError(f'holes.connectivity={v!r}: 4 or 8')
    out['connectivity'] = int(v)
    for k in ('max_rel_area', 'prev_overlap'):
        v = out[k]
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not 0.0 <= v <= 1.0:        # a NaN fails the comparison
            raise ValueError(f'holes.{k}={v!r}: a number in [0, 1]')
        out[k] = float(v)
    return out


def active(cfg):
    """Validated; False when `cfg` fills nothing (None, max_area 0 or max_rel_area rounding to 0)."""
    if cfg is None:
        return False
    p = check(cfg)
    return bool(p['max_area'] and rel_q16(p['max_rel_area']))


def rel_q16(max_rel_area):
    """`max_rel_area` as the 16-bit fixed-point integer every path compares with."""
    return int(round(float(max_rel_area) * 65536))


def overlap_q16(prev_overlap):
    """`prev_overlap` as the 16-bit fixed-point integer every path compares with."""
    return int(round(float(prev_overlap) * 65536))


def frames_per_call(height, width):
    """How many frames one `eosvos_fill_holes` call may take under the scratch cap (at least 1)."""
    per_frame = _BYTES_PER_PIXEL * height * width + _BYTES_PER_FRAME
    return max(1, min((SCRATCH_CAP - _BYTES_FIXED) // per_frame, 65535))


def _neighbour_slices(h, w, dy, dx):
    """(slices of the pixels, slices of their neighbours dy rows down and dx columns over), both inside the frame."""
    ya, yb = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
    xa, xb = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
    return (ya, xa), (yb, xb)


def fill_host(labels, params, prev=None, keep=(), return_filled=False):
    """The rules of the module's docstring in numpy: labels (N, H, W) uint8, prev (H, W) uint8 or None -> filled maps
    (N, H, W) uint8 (a numpy array), with `return_filled` also the pixels filled per frame (N,) int64.  The background is
    labelled by `components.label_host` on the zero mask under the dual connectivity; per component a border flag, the smallest
    and largest neighbour label (one bordering label <=> they are equal) and the counts A, S, C, all as 64-bit integers."""
    p = check(params)
    lab = components._as_numpy(labels)
    prev = None if prev is None else components._as_numpy(prev)
    components._check_maps('fill_host', lab, prev)
    n, h, w = lab.shape
    keep = {int(f) for f in keep}
    rq, oq = rel_q16(p['max_rel_area']), overlap_q16(p['prev_overlap'])
    out = lab.copy()
    filled = np.zeros(n, dtype=np.int64)
    if not (p['max_area'] and rq):
        return (out, filled) if return_filled else out
    bg8 = p['connectivity'] == 4
    ids = components.label_host((lab == 0).astype(np.uint8), 8 if bg8 else 4)            # 0 on object pixels
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if bg8 else [])
    edge = np.zeros((h, w), dtype=bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    R = prev
    for f in range(n):
        if f not in keep:
            idf, m = ids[f].astype(np.int64), lab[f].astype(np.int64)
            flat = idf.reshape(-1)
            border = np.zeros(h * w + 1, dtype=bool)
            border[idf[edge]] = True
            lo = np.full(h * w + 1, 256, dtype=np.int64)
            hi = np.zeros(h * w + 1, dtype=np.int64)
            for dy, dx in steps:
                a, b = _neighbour_slices(h, w, dy, dx)
                sel = (idf[a] != 0) & (m[b] != 0)
                np.minimum.at(lo, idf[a][sel], m[b][sel])
                np.maximum.at(hi, idf[a][sel], m[b][sel])
            A = np.bincount(flat, minlength=h * w + 1).astype(np.int64)
            S = np.bincount(m.reshape(-1), minlength=256).astype(np.int64)
            o = hi                                                                       # the candidate's label where lo == hi
            ok = (A > 0) & ~border & (hi > 0) & (lo == hi) & (A <= p['max_area']) & (A * 65536 <= rq * S[o])
            ok[0] = False                                                                # id 0: the object pixels
            if oq > 0 and R is not None:
                in_R = np.bincount(R.reshape(-1), minlength=256) > 0
                C = np.bincount(flat, weights=(R.reshape(-1) == o[flat]) & (flat != 0), minlength=h * w + 1).astype(np.int64)
                ok &= ~in_R[o] | (C * 65536 >= oq * A)
            hit = ok[idf]
            out[f][hit] = o[idf][hit].astype(np.uint8)
            filled[f] = int(hit.sum())
        R = out[f]
    return (out, filled) if return_filled else out


def fill(engine, labels, params, prev=None, keep=()):
    """Filled label maps of `labels` (N, H, W) uint8 tensor on `engine`: its `fill_holes` (the device kernels) where it has the
    entry point, else `fill_host` (stand-in engines of host tests).  Returns a uint8 tensor on the labels' device."""
    p = check(params)
    if hasattr(engine, 'fill_holes'):
        return engine.fill_holes(labels, prev=prev, keep=keep, **p)
    return torch.from_numpy(fill_host(labels, p, prev=prev, keep=keep)).to(labels.device)
