"""Connected-component clean-up of the merged label maps: the region-aware last step of the OSVOS family -- drop small
components, keep the dominant component of an object, keep only components that continue the previous frame's mask -- which
removes the confident blob on a look-alike that the arg-max merge (`evaluate.py:322-326`) and the CRF both keep.  The
reference has no such step; this is an opt-in extension (`config.CLEANUP`), off by default.

    components = {'connectivity': 8, 'min_area': 0, 'min_rel_area': 0.0, 'largest_only': False, 'gate': 0}     (`DEFAULTS`)

The rules (include/eosvos.h states them at `eosvos_filter_components`; the kernels are csrc/ccl_kernels.hip; `label_host` and
`filter_host` below are their numpy twin: the reference of the tests and the path of engines without the entry point):

  components  two pixels of a frame are connected when they hold the same non-zero label and are neighbours under
              `connectivity` (4: edge neighbours, 8: edge and corner neighbours).  Different labels never connect, frames never
              connect.  The id of a component is 1 + min(y * W + x) over its pixels, background has id 0.
  filter      for frame f in ascending order, for every label o present in it:
    1. gate (`gate` = g in 0..63, 0 = off).  R is the FILTERED output of frame f - 1 (`prev` for the first frame of a call).
       The gate is active for (f, o) when g > 0, R exists and R has a pixel equal to o; then a component is a candidate only if
       one of its pixels lies within Chebyshev distance g of a pixel of R equal to o (outside the frame R counts as 0).
       Inactive: every component of o is a candidate.
    2. over the candidates of (f, o), A = pixel count, Amax = the largest candidate count: kept iff A >= min_area and
       A * 65536 >= q * Amax with q = round(min_rel_area * 65536) (integers on every path) and, with `largest_only`, A == Amax
       and the smallest id among those.
    3. pixels of components that are not kept become 0.
  keep        frames listed there (the train frames: seeded ground truth) are copied unchanged and still serve as R.

The defaults are the neutral values: nothing is filtered and callers take today's path, call for call (`active`).  Nothing
here is tuned on data.
"""
import numbers

import numpy as np
import torch

DEFAULTS = {'connectivity': 8, 'min_area': 0, 'min_rel_area': 0.0, 'largest_only': False, 'gate': 0}
MAX_GATE = 63
MAX_SIDE = 4096
MAX_PIXELS = 1 << 24                # frame-local pixel indices and areas fit 24 bits
SCRATCH_CAP = 512 << 20             # bytes of engine scratch one `eosvos_filter_components` call may take
_BYTES_PER_PIXEL = 17               # parent, tile area, id, area (int32 each) and the gate flag
_BYTES_PER_FRAME = 2312             # 257 64-bit words (largest candidate per label, pixels removed) and 256 presence bytes


def check(cfg):
    """The complete, validated parameter dictionary of `cfg` (missing keys take `DEFAULTS`); ValueError otherwise."""
    if not isinstance(cfg, dict) or set(cfg) - set(DEFAULTS):
        raise ValueError(f'components={cfg!r}: a dictionary with keys from {sorted(DEFAULTS)}')
    out = dict(DEFAULTS, **cfg)
    for k, lo, hi in (('min_area', 0, MAX_PIXELS), ('gate', 0, MAX_GATE)):
        v = out[k]
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= v <= hi:
            raise ValueError(f'components.{k}={v!r}: an integer in [{lo}, {hi}]')
        out[k] = int(v)
    v = out['connectivity']
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v not in (4, 8):
        raise ValueError(f'components.connectivity={v!r}: 4 or 8')
    out['connectivity'] = int(v)
    v = out['min_rel_area']
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not 0.0 <= v <= 1.0:        # a NaN fails the comparison
        raise ValueError(f'components.min_rel_area={v!r}: a number in [0, 1]')
    out['min_rel_area'] = float(v)
    if not isinstance(out['largest_only'], (bool, np.bool_)):
        raise ValueError(f"components.largest_only={out['largest_only']!r}: True or False")
    out['largest_only'] = bool(out['largest_only'])
    return out


def active(cfg):
    """Validated; False when `cfg` filters nothing (None, or every rule at its neutral value)."""
    if cfg is None:
        return False
    p = check(cfg)
    return bool(p['min_area'] or p['min_rel_area'] or p['largest_only'] or p['gate'])


def rel_q16(min_rel_area):
    """`min_rel_area` as the 16-bit fixed-point integer every path compares with."""
    return int(round(float(min_rel_area) * 65536))


def frames_per_call(height, width):
    """How many frames one `eosvos_filter_components` call may take under the scratch cap (at least 1)."""
    per_frame = _BYTES_PER_PIXEL * height * width + _BYTES_PER_FRAME
    return max(1, min((SCRATCH_CAP - 256) // per_frame, 65535))


def _check_maps(who, labels, prev=None):
    if labels.ndim != 3 or not str(labels.dtype).endswith('uint8') or labels.shape[1] < 1 or labels.shape[2] < 1:
        raise ValueError(f'{who}: labels must be (N, H, W) uint8, got {tuple(labels.shape)} {labels.dtype}')
    h, w = int(labels.shape[1]), int(labels.shape[2])
    if h > MAX_SIDE or w > MAX_SIDE or h * w >= MAX_PIXELS:
        raise ValueError(f'{who}: frames of {h} x {w} exceed {MAX_SIDE} pixels a side or 2^24 pixels')
    if prev is not None and (not str(prev.dtype).endswith('uint8') or tuple(prev.shape) != (h, w)):
        raise ValueError(f'{who}: prev must be ({h}, {w}) uint8')


def _as_numpy(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def label_host(labels, connectivity=8):
    """The id maps of `labels` (N, H, W) uint8 -> (N, H, W) int32, in numpy: a union-find over pixel indices with
    parent[i] <= i, all edges hooked at once (the larger root under the smaller, `np.minimum.at`) and the trees flattened by
    pointer jumping, until no edge joins two trees; the root of a tree is then the smallest index of its component."""
    lab = _as_numpy(labels)
    _check_maps('label_host', lab)
    if connectivity not in (4, 8):
        raise ValueError(f'label_host: connectivity={connectivity!r}: 4 or 8')
    n, h, w = lab.shape
    idx = np.arange(n * h * w, dtype=np.int64).reshape(n, h, w)
    fg = lab != 0
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    ea, eb = [], []
    for dy, dx in steps:                                  # a = the pixel, b = its neighbour dy rows below, dx columns over
        ya, yb = slice(0, h - dy), slice(dy, h)
        xa, xb = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
        m = fg[:, ya, xa] & (lab[:, ya, xa] == lab[:, yb, xb])
        ea.append(idx[:, ya, xa][m])
        eb.append(idx[:, yb, xb][m])
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    parent = idx.reshape(-1).copy()
    while ea.size:
        ra, rb = parent[ea], parent[eb]                   # the trees are flat: these are roots
        live = ra != rb
        if not live.any():
            break
        ea, eb, ra, rb = ea[live], eb[live], ra[live], rb[live]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:                                       # pointer jumping: depth halves per pass
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    ids = parent.reshape(n, h, w) - idx[:, :1, :1] + 1
    return np.where(fg, ids, 0).astype(np.int32)


def _near(mask, g):
    """Binary dilation of a (H, W) mask by the (2g + 1)^2 square: True within Chebyshev distance g of a True pixel."""
    h, w = mask.shape
    out = np.zeros((h + 2 * g, w), dtype=bool)
    for d in range(2 * g + 1):
        out[d:d + h] |= mask
    rows = out[g:g + h]
    out = np.zeros((h, w + 2 * g), dtype=bool)
    for d in range(2 * g + 1):
        out[:, d:d + w] |= rows
    return out[:, g:g + w]


def filter_host(labels, params, prev=None, keep=(), return_removed=False):
    """The filter of the module's docstring in numpy: labels (N, H, W) uint8, prev (H, W) uint8 or None -> filtered maps
    (N, H, W) uint8 (a numpy array), with `return_removed` also the pixels zeroed per frame (N,) int64."""
    p = check(params)
    lab = _as_numpy(labels)
    prev = None if prev is None else _as_numpy(prev)
    _check_maps('filter_host', lab, prev)
    n, h, w = lab.shape
    keep = {int(f) for f in keep}
    q, g = rel_q16(p['min_rel_area']), p['gate']
    ids = label_host(lab, p['connectivity'])
    out = lab.copy()
    removed = np.zeros(n, dtype=np.int64)
    R = prev
    for f in range(n):
        if f not in keep:
            area = np.bincount(ids[f].reshape(-1), minlength=h * w + 1).astype(np.int64)
            for o in np.unique(lab[f]):
                if o == 0:
                    continue
                of = lab[f] == o
                comp = np.unique(ids[f][of])
                if g > 0 and R is not None and (R == o).any():
                    comp = np.unique(ids[f][of & _near(R == o, g)])
                kept = np.zeros(0, dtype=comp.dtype)
                if comp.size:
                    A = area[comp]
                    amax = int(A.max())
                    ok = (A >= p['min_area']) & (A * 65536 >= q * amax)
                    if p['largest_only']:
                        ok &= comp == comp[A == amax].min()
                    kept = comp[ok]
                drop = of & ~np.isin(ids[f], kept)
                out[f][drop] = 0
                removed[f] += int(drop.sum())
        R = out[f]
    return (out, removed) if return_removed else out


def filter(engine, labels, params, prev=None, keep=()):
    """Filtered label maps of `labels` (N, H, W) uint8 tensor on `engine`: its `filter_components` (the device kernels) where it
    has the entry point, else `filter_host` (stand-in engines of host tests).  Returns a uint8 tensor on the labels' device."""
    p = check(params)
    if hasattr(engine, 'filter_components'):
        return engine.filter_components(labels, prev=prev, keep=keep, **p)
    return torch.from_numpy(filter_host(labels, p, prev=prev, keep=keep)).to(labels.device)
