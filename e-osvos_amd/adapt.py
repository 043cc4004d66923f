"""Distance-gated pseudo-labels for online adaptation: what the adaptation rounds (`eval_online_adapt.step > 0`) are trained on.
Their targets come from the frame's own probabilities only -- a scalar `min_prop` makes everything below it a negative, the
`[lo, hi]` band makes the uncertain pixels void -- and neither looks at where the object was: a confident blob on a look-alike far
from the object becomes a positive target, every later round trains the net to keep it, and the clean-up stages after the merge
repair the output, not the weights.  The OSVOS family's answer is the core rule of OnAVOS (Voigtlaender & Leibe, 2017): pixels
farther than a distance from the (eroded) mask of the previous frame are negatives whatever the network says, pixels the network
is sure about and that are near are positives, the rest is void.  The reference has no such step (`evaluate.py:231-240`
thresholds and nothing else); this is an opt-in extension (`config.ADAPT`), off by default.

    adapt = {'neg_dist': 0, 'erode': 0}                                                                      (`DEFAULTS`)

`neg_dist` is an integer in [0, 4095] (0 = off), `erode` one in [0, 255]; frames are at most 4096 pixels a side.  The rules
(include/eosvos.h states them at `eosvos_distance_sq` / `eosvos_adapt_targets`; the kernels are csrc/edt_kernels.hip;
`distance_sq_host` and `targets_host` below are their numpy twins: the reference of the tests and the path of engines without
the entry point).  Everything is integer arithmetic.

  1. capped squared distance  S is a set of seed pixels of an H x W frame, L >= 1 an integer limit.  D2(p) = min over q in S of
     dy^2 + dx^2 (pixel centres, integers, within the frame only); out(p) = min(D2(p), L^2 + 1), and L^2 + 1 everywhere for an
     empty S.  int32; L <= 4095, so L^2 + 1 < 2^24 + 2^23.  The definition does not depend on the algorithm.  A NaN probability
     is never a seed under `p >= t` and always one under the inverted predicate `!(p >= t)`.
  2. anchor  for a propagated frame f the anchor is A = {p(f - 1) >= t_pos}, p(f - 1) the previous frame's probability map in
     `masks` (`masks[train_frame]` = 2 * gt, so the ground truth anchors the first frame after it; f - 1 >= the train frame
     always holds under `online_adapt_schedule`).  t_pos is the scalar `min_prop`, or `hi` of the band.
  3. erosion  with `erode` = e > 0, E = {q in A : D2_in(q) > e^2}, D2_in being rule 1 with seeds = the frame's pixels NOT in A
     and L = e.  Pixels outside the frame are not background: an object cut by the border is not eroded from the border.  With
     e = 0, E = A.
  4. far  far(p) <=> rule 1 with seeds E and L = `neg_dist` gives out(p) > neg_dist^2, i.e. out = L^2 + 1.
  5. targets of frame f (p = the frame's own probability): the base rule is the band's, 1 where p >= hi, 0 where p < lo, void
     otherwise (a NaN is void).  A scalar `min_prop` = t is the band (lo, hi) = (0, t): nothing near is negative, which is
     OnAVOS's rule; a scalar 0 (or one above 1) with `adapt` on raises ValueError.  Then far overrides: target = 0 where far.
  6. counts  n_pos[f] = the number of 1-targets after the override.  If E is empty (object lost, or eroded away) n_pos[f] = 0
     and the targets of f are the base rule's.  The caller drops frames with n_pos = 0, as it always did (OnAVOS: no adaptation
     without an anchor).
  7. off  `adapt=None` or `neg_dist` 0: nothing new is called; the code path, the batches and the random draws are what they
     were, bit for bit.  `erode` without `neg_dist` does nothing (`active` is False).
  8. train frame  the train frame's ground truth in the round's batch is never touched.

Nothing here is tuned on data; neg_dist=220 erode=15 are OnAVOS's published 480p values and serve as the example.
"""
import numbers

import numpy as np
import torch

DEFAULTS = {'neg_dist': 0, 'erode': 0}
MAX_DIST = 4095
MAX_ERODE = 255
MAX_SIDE = 4096
SCRATCH_CAP = 512 << 20             # bytes of engine scratch one `eosvos_adapt_targets` / `eosvos_distance_sq` call may take
_BYTES_PER_FRAME = 8                # the two count words


def check(cfg):
    """The complete, validated parameter dictionary of `cfg` (missing keys take `DEFAULTS`); ValueError otherwise."""
    if not isinstance(cfg, dict) or set(cfg) - set(DEFAULTS):
        raise ValueError(f'adapt={cfg!r}: a dictionary with keys from {sorted(DEFAULTS)}')
    out = dict(DEFAULTS, **cfg)
    for k, top in (('neg_dist', MAX_DIST), ('erode', MAX_ERODE)):
        v = out[k]
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v <= top:
            raise ValueError(f'adapt.{k}={v!r}: an integer in [0, {top}]')
        out[k] = int(v)
    return out


def active(cfg):
    """Validated; False when `cfg` gates nothing (None, or neg_dist 0 whatever `erode` says)."""
    if cfg is None:
        return False
    return check(cfg)['neg_dist'] > 0


def band_of(min_prop, band):
    """(lo, hi) of rule 5: the band as it is, a scalar t as (0, t); ValueError for a scalar outside (0, 1]."""
    if band is not None:
        return band
    ok = isinstance(min_prop, (int, float)) and not isinstance(min_prop, bool) and 0.0 < float(min_prop) <= 1.0
    if not ok:
        raise ValueError(f'eval_online_adapt.min_prop={min_prop!r}: with eval_adapt on a scalar must lie in (0, 1] '
                         '(it becomes the band (0, min_prop)), or be a band [lo, hi]')
    return 0.0, float(min_prop)


def frames_per_call(height, width, erode=0):
    """How many frames one device call may take under the scratch cap (at least 1)."""
    per_frame = (3 if erode else 2) * height * width + _BYTES_PER_FRAME
    return max(1, min((SCRATCH_CAP - 4) // per_frame, 65535))


def _as_numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _check_limit(who, limit):
    if isinstance(limit, bool) or not isinstance(limit, numbers.Integral) or not 1 <= limit <= MAX_DIST:
        raise ValueError(f'{who}: limit={limit!r} must be an integer in [1, {MAX_DIST}]')
    return int(limit)


def distance_sq_host(mask, limit):
    """Rule 1 in numpy: mask (..., H, W), seeds where it is non-zero / True -> min(D2, limit^2 + 1) as int64 of the same shape.
    Two passes: g = the distance to the nearest seed of the column, from the running index of the last seed seen going down and
    going up; then out = min over k of k^2 + g^2 shifted k columns either way, k = 0, 1, .. while k^2 < the largest value left."""
    L = _check_limit('distance_sq_host', limit)
    seeds = _as_numpy(mask).astype(bool)
    if seeds.ndim < 2 or min(seeds.shape[-2:]) < 1 or max(seeds.shape[-2:]) > MAX_SIDE:
        raise ValueError(f'distance_sq_host: mask must be (..., H, W) with 1 <= H, W <= {MAX_SIDE}, got {seeds.shape}')
    h, w = seeds.shape[-2:]
    cap, far = L * L + 1, 2 * MAX_SIDE
    rows = np.arange(h, dtype=np.int64).reshape(h, 1)
    above = np.maximum.accumulate(np.where(seeds, rows, -far), axis=-2)              # the last seed at or above, or far away
    below = np.minimum.accumulate(np.where(seeds, rows, far)[..., ::-1, :], axis=-2)[..., ::-1, :]
    g = np.minimum(np.minimum(rows - above, below - rows), L + 1)
    g2 = np.minimum(g * g, cap)
    best = g2.copy()
    for k in range(1, min(L, w - 1) + 1):
        if k * k >= int(best.max()):
            break
        np.minimum(best[..., k:], g2[..., :w - k] + k * k, out=best[..., k:])
        np.minimum(best[..., :w - k], g2[..., k:] + k * k, out=best[..., :w - k])
    return best


def eroded_host(anchors, threshold, erode):
    """Rules 2 and 3 in numpy: anchors (..., H, W) float -> E as a bool array."""
    a = _as_numpy(anchors)
    inside = a >= np.float32(threshold)
    if not erode:
        return inside
    return distance_sq_host(~inside, erode) > erode * erode


def targets_host(probs, anchors, lo, hi, params, ignore):
    """Rules 2-6 in numpy: probs and anchors (F, ..., H, W) fp32 (frame i's own and its previous frame's probabilities) ->
    (targets fp32 of the shape of `probs`, n_pos (F,) int64).  The thresholds are compared as fp32, as the device does."""
    p = check(params)
    if not p['neg_dist']:
        raise ValueError('targets_host: neg_dist=0 means "off"; pass a value in [1, 4095]')
    if not 0.0 <= lo < hi <= 1.0:
        raise ValueError(f'targets_host: needs 0 <= lo < hi <= 1, got {lo!r}, {hi!r}')
    x, a = _as_numpy(probs), _as_numpy(anchors)
    if x.shape != a.shape or x.ndim < 3:
        raise ValueError(f'targets_host: probs {x.shape} and anchors {a.shape} must share one shape (F, ..., H, W)')
    lo32, hi32, L = np.float32(lo), np.float32(hi), p['neg_dist']
    pos = x >= hi32
    base = np.where(pos, np.float32(1), np.where(x < lo32, np.float32(0), np.float32(ignore))).astype(np.float32)
    E = eroded_host(a, hi, p['erode'])
    far = distance_sq_host(E, L) > L * L
    out, counts = base.copy(), np.zeros(x.shape[0], dtype=np.int64)
    for f in range(x.shape[0]):
        if E[f].any():
            out[f][far[f]] = 0
            counts[f] = int((pos[f] & ~far[f]).sum())
    return out, counts


def targets(engine, probs, anchors, lo, hi, params, ignore):
    """(targets, [n_pos per frame]) of rules 2-6 for the propagated frames of one round on `engine`: its `adapt_targets` (the
    device kernels) where it has the entry point, else `targets_host` (stand-in engines of host tests)."""
    p = check(params)
    if hasattr(engine, 'adapt_targets'):
        return engine.adapt_targets(probs, anchors, lo, hi, p, ignore)
    out, counts = targets_host(probs, anchors, lo, hi, p, ignore)
    return torch.from_numpy(out).to(probs.device), [int(c) for c in counts]
