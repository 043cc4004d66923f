"""Superpixel snapping of the merged label maps: the stage between the CRF (`crf.py`) and the component filter
(`components.py`).  The filter and the hole filler look at the label map alone and the CRF sees the frame only through a
pixel-pair window, so nothing else in the chain moves a label boundary onto the image edge it belongs to.  The OSVOS family
does that with superpixels ("contour snapping"): superpixels of the frame are computed and each one takes the label that holds
its majority.  The superpixels are SLIC in its GPU form (gSLIC), restricted to integers, so that the device equals the numpy
twin below bit for bit.  The reference has no such step; this is an opt-in extension (`config.SNAP`), off by default.

    snap = {'step': 0, 'iterations': 5, 'compactness': 10, 'min_share': 0.5}                                  (`DEFAULTS`)

step S: 0 = off, else an integer in [4, 64]; iterations T in [1, 20]; compactness m in [1, 64]; min_share in [0, 1].  Frames
of at most 4096 pixels a side, n_obj <= 255.  `eval_snap.step=16 eval_snap.min_share=0.6` are example values: NOTHING here is
tuned on data.

The rules (include/eosvos.h states them at `eosvos_superpixels` / `eosvos_snap_labels`; the kernels are
csrc/slic_kernels.hip; `superpixels_host` / `snap_host` below are their numpy twin: the reference of the device tests and the
path of engines without the entry point; the twin itself is checked against the plain loops of tests/snap_ref.py).  Every
quantity is an integer.  Input: rgb (N, 3, H, W) uint8, planar; labels (N, H, W) uint8, 0 = background, 1..n_obj = objects.
Frames never interact.  `quantise` makes rgb from the engine's fp32 frames.

  1. grid    gy = ceil(H / S), gx = ceil(W / S), K = gy * gx clusters per frame; the id of cell (cy, cx) is cy * gx + cx.  Its
             initial centre is the pixel (min(cy * S + S / 2, H - 1), min(cx * S + S / 2, W - 1)) (integer division) and that
             pixel's colour: a centre is five integers (y, x, R, G, B).
  2. assign  pixel (y, x) has home cell (y / S, x / S); its candidates are the clusters of the up to nine cells within +-1 of
             the home cell that exist in the grid.  D = (dR^2 + dG^2 + dB^2) * S^2 + m^2 * (dy^2 + dx^2) against the candidate's
             current centre; the pixel takes the smallest D, ties go to the smaller id.  D < 2^32 under the limits: colour gives
             <= 195075 * 4096 ~ 8.0e8, and a centre is a mean of pixels of cells within +-1 of its own, so |d| < 3 S and the
             position gives <= 2 * 192^2 * 4096 ~ 3.0e8.  The twin computes D in 64 bits, the kernel in unsigned 32.
  3. update  per cluster n and the sums of y, x, R, G, B over its pixels (each fits 32 bits: <= (3 * 64)^2 pixels * 4095); a
             new centre component is (2 * sum + n) / (2 * n), integer division (round half up); a cluster with n = 0 keeps its
             centre.
  4. schedule  for t = 1..T: assign; if t < T: update.  The ids are those of the last assign.  No connectivity enforcement: a
             cluster may be disconnected, and the vote is per id.
  5. vote    for a cluster c, cnt_c[l] = its pixels with label l <= n_obj, n_c their sum; a pixel with a label > n_obj votes
             nowhere and is copied unchanged.  The winner w is the label with the largest count, ties to the smaller label.
             With q = round(min_share * 65536), computed once on the host: if n_c > 0 and cnt_c[w] * 65536 >= q * n_c (64-bit
             products), every voting pixel of c becomes w; otherwise the pixels of c are copied.
  6. keep    frames listed there (the train frame of every object: seeded ground truth) are copied unchanged.
  7. chain   merge -> CRF -> snap -> components -> holes: the component filter and the hole filler clean what snapping leaves.
             `snap` needs the frames, like the CRF.
  8. off     `None` or step = 0: nothing new is called (`active`).
"""
import numbers

import numpy as np
import torch

DEFAULTS = {'step': 0, 'iterations': 5, 'compactness': 10, 'min_share': 0.5}
MIN_STEP, MAX_STEP = 4, 64
_INTS = {'iterations': (1, 20), 'compactness': (1, 64)}
MAX_SIDE = 4096
MAX_OBJECTS = 255
SCRATCH_CAP = 512 << 20             # bytes of engine scratch one `eosvos_snap_labels` call may take
_WORDS_PER_CLUSTER = 5 + 6          # the centre (y, x, R, G, B) and the sums (n, y, x, R, G, B), 32-bit words


def check(cfg):
    """The complete, validated parameter dictionary of `cfg` (missing keys take `DEFAULTS`); ValueError otherwise."""
    if not isinstance(cfg, dict) or set(cfg) - set(DEFAULTS):
        raise ValueError(f'snap={cfg!r}: a dictionary with keys from {sorted(DEFAULTS)}')
    out = dict(DEFAULTS, **cfg)
    v = out['step']
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not (v == 0 or MIN_STEP <= v <= MAX_STEP):
        raise ValueError(f'snap.step={v!r}: 0 (off) or an integer in [{MIN_STEP}, {MAX_STEP}]')
    out['step'] = int(v)
    for k, (lo, hi) in _INTS.items():
        v = out[k]
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= v <= hi:
            raise ValueError(f'snap.{k}={v!r}: an integer in [{lo}, {hi}]')
        out[k] = int(v)
    v = out['min_share']
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not 0.0 <= v <= 1.0:              # a NaN fails the comparison
        raise ValueError(f'snap.min_share={v!r}: a number in [0, 1]')
    out['min_share'] = float(v)
    return out


def active(cfg):
    """Validated; False when `cfg` snaps nothing (None or step 0)."""
    return cfg is not None and check(cfg)['step'] != 0


def share_q16(min_share):
    """`min_share` as the 16-bit fixed-point integer every path compares with."""
    return int(round(float(min_share) * 65536))


def grid(height, width, step):
    """(gy, gx): the cells of a frame."""
    return (height + step - 1) // step, (width + step - 1) // step


def scratch_bytes(n_frames, n_obj, height, width, step):
    """The scratch one `eosvos_snap_labels` call takes: per frame the ids (one word per pixel), 5 + 6 words per cluster,
    K * (n_obj + 1) vote words and the 64-bit count of changed pixels, 8 bytes of padding before those."""
    gy, gx = grid(height, width, step)
    k = gy * gx
    return n_frames * (4 * (height * width + k * (_WORDS_PER_CLUSTER + n_obj + 1)) + 8) + 8


def frames_per_call(n_obj, height, width, step=MIN_STEP):
    """How many frames one `eosvos_snap_labels` call may take under the scratch cap (at least 1: a single frame over the cap
    is the library's to reject).  Without `step` the bound is that of the smallest step, which has the most clusters."""
    per_frame = scratch_bytes(1, n_obj, height, width, step) - 8
    return max(1, min((SCRATCH_CAP - 8) // per_frame, 65535))


def quantise(frames, offset=None):
    """The engine's fp32 frames (N, 3, H, W) -- RGB / 255, minus `offset` / 255 per channel where the dataset subtracts its
    `mean_val` (`data_cfg.normalize`) -- as the uint8 rgb the entry points take: clamp(round(frames * 255 + offset), 0, 255).
    Separate torch ops (no fused multiply-add), so the CPU and the device agree."""
    x = frames.float() * 255.0
    if offset is not None:
        x = x + torch.as_tensor(offset, dtype=torch.float32, device=frames.device).view(1, 3, 1, 1)
    return torch.clamp(torch.round(x), 0.0, 255.0).to(torch.uint8)


def _as_numpy(a, dtype=np.uint8):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.dtype != dtype:
        raise ValueError(f'snap: expected {np.dtype(dtype).name}, got {a.dtype}')
    return a


def _check_rgb(who, rgb, labels=None):
    if rgb.ndim != 4 or rgb.shape[1] != 3 or min(rgb.shape[2:]) < 1 or max(rgb.shape[2:]) > MAX_SIDE:
        raise ValueError(f'{who}: rgb must be (N, 3, H, W) with 1 <= H, W <= {MAX_SIDE}, got {tuple(rgb.shape)}')
    if labels is not None and (labels.ndim != 3 or labels.shape[0] != rgb.shape[0] or tuple(labels.shape[1:]) != tuple(rgb.shape[2:])):
        raise ValueError(f'{who}: labels {tuple(labels.shape)} do not match rgb {tuple(rgb.shape)}')


def _check_n_obj(n_obj):
    if isinstance(n_obj, bool) or not isinstance(n_obj, numbers.Integral) or not 1 <= n_obj <= MAX_OBJECTS:
        raise ValueError(f'snap: n_obj={n_obj!r}: an integer in [1, {MAX_OBJECTS}]')
    return int(n_obj)


def _slic_frame(img, S, T, m):
    """Rules 1-4 on one frame: img (3, H, W) uint8 -> ids (H, W) int32.  Vectorised over the pixels, one pass per candidate
    offset in ascending id order with a strict `<`, so a tie keeps the smaller id."""
    _, h, w = img.shape
    gy, gx = grid(h, w, S)
    k = gy * gx
    c = img.astype(np.int64)
    cy = np.minimum(np.arange(gy, dtype=np.int64) * S + S // 2, h - 1)
    cx = np.minimum(np.arange(gx, dtype=np.int64) * S + S // 2, w - 1)
    cen = np.empty((5, k), dtype=np.int64)                               # y, x, R, G, B
    cen[0], cen[1] = np.repeat(cy, gx), np.tile(cx, gy)
    cen[2:] = c[:, cen[0], cen[1]]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    hy, hx = yy // S, xx // S
    feats = (yy, xx, c[0], c[1], c[2])
    ids = None
    for t in range(1, T + 1):
        best = np.full((h, w), np.iinfo(np.int64).max, dtype=np.int64)
        ids = np.zeros((h, w), dtype=np.int64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ny, nx = hy + dy, hx + dx
                ok = (ny >= 0) & (ny < gy) & (nx >= 0) & (nx < gx)
                cand = np.where(ok, ny * gx + nx, 0)
                d = ((c[0] - cen[2][cand]) ** 2 + (c[1] - cen[3][cand]) ** 2 + (c[2] - cen[4][cand]) ** 2) * (S * S) + \
                    (m * m) * ((yy - cen[0][cand]) ** 2 + (xx - cen[1][cand]) ** 2)
                take = ok & (d < best)
                best[take] = d[take]
                ids[take] = cand[take]
        if t < T:
            flat = ids.reshape(-1)
            n = np.bincount(flat, minlength=k).astype(np.int64)
            has = n > 0
            for j, f in enumerate(feats):                                # float64 weights: the sums are < 2^53, so exact
                s = np.bincount(flat, weights=f.reshape(-1), minlength=k).astype(np.int64)
                cen[j][has] = (2 * s[has] + n[has]) // (2 * n[has])
    return ids.astype(np.int32)


def superpixels_host(rgb, params):
    """Rules 1-4 in numpy: rgb (N, 3, H, W) uint8 -> ids (N, H, W) int32 (a numpy array)."""
    p = check(params)
    rgb = _as_numpy(rgb)
    _check_rgb('superpixels_host', rgb)
    if p['step'] == 0:
        raise ValueError('superpixels_host: snap.step is 0 (off)')
    out = np.empty((rgb.shape[0],) + rgb.shape[2:], dtype=np.int32)
    for f in range(rgb.shape[0]):
        out[f] = _slic_frame(rgb[f], p['step'], p['iterations'], p['compactness'])
    return out


def snap_host(rgb, labels, params, keep=(), n_obj=MAX_OBJECTS, return_changed=False, ids=None):
    """The rules of the module's docstring in numpy: rgb (N, 3, H, W) uint8, labels (N, H, W) uint8 -> snapped maps (N, H, W)
    uint8 (a numpy array), with `return_changed` also the pixels changed per frame (N,) int64.  `n_obj`: labels above it vote
    nowhere and pass unchanged (under the default every uint8 label votes).  `ids`: the result of `superpixels_host` on the same
    rgb and params, where the caller has it already."""
    p = check(params)
    n_obj = _check_n_obj(n_obj)
    rgb, lab = _as_numpy(rgb), _as_numpy(labels)
    _check_rgb('snap_host', rgb, lab)
    keep = {int(f) for f in keep}
    out = lab.copy()
    changed = np.zeros(lab.shape[0], dtype=np.int64)
    if p['step'] == 0:
        return (out, changed) if return_changed else out
    q = share_q16(p['min_share'])
    k = int(np.prod(grid(lab.shape[1], lab.shape[2], p['step'])))
    for f in range(lab.shape[0]):
        if f in keep:
            continue
        idf = (_slic_frame(rgb[f], p['step'], p['iterations'], p['compactness']) if ids is None else np.asarray(ids[f])).astype(np.int64)
        votes = lab[f] <= n_obj
        cnt = np.bincount(idf[votes] * (n_obj + 1) + lab[f][votes], minlength=k * (n_obj + 1)).reshape(k, n_obj + 1).astype(np.int64)
        n_c = cnt.sum(axis=1)
        win = cnt.argmax(axis=1)                                         # the first largest: ties to the smaller label
        snaps = (n_c > 0) & (cnt[np.arange(k), win] * 65536 >= q * n_c)
        hit = votes & snaps[idf]
        out[f][hit] = win[idf][hit].astype(np.uint8)
        changed[f] = int((out[f] != lab[f]).sum())
    return (out, changed) if return_changed else out


def snap(engine, rgb, labels, params, keep=(), n_obj=MAX_OBJECTS):
    """Snapped label maps of `labels` (N, H, W) uint8 against `rgb` (N, 3, H, W) uint8 on `engine`: its `snap_labels` (the device
    kernels) where it has the entry point, else `snap_host` (stand-in engines of host tests).  Returns a uint8 tensor on the
    labels' device.  `n_obj`: the number of objects of the merge (the default lets every label vote; the vote table is
    then 256 words per cluster)."""
    p = check(params)
    if hasattr(engine, 'snap_labels'):
        return engine.snap_labels(rgb, labels, n_obj=n_obj, keep=keep, **p)
    return torch.from_numpy(snap_host(rgb, labels, p, keep=keep, n_obj=n_obj)).to(labels.device)
