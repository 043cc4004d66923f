"""Lucid synthesis with the sequence's other objects as moving layers.  `lucid.py` moves exactly one object: on a multi-object
sequence (DAVIS-2017, YouTube-VOS) the train frame's other annotated objects stay in the plate, move rigidly with the
background, never change place relative to the target and never cover it -- and similar neighbours that cross and occlude each
other are what these sequences are hard for.  Lucid data dreaming proper (Khoreva et al.) moves every object on its own over
the filled plate, with a depth order: each object's net sees its neighbours as negatives in new places, sometimes in front of
it.  This is an opt-in extension of an opt-in extension (`config.LAYERS`, it needs `eval_lucid.samples` > 0), off by default;
other sequences' objects, the meta-training feed and the adaptation rounds are not touched, and every object's fine-tune
builds its own synthesis.

    layers = {'others': 0, 'front': 0.5}                                                                      (`DEFAULTS`)

  others   at most this many of the other objects annotated on the target's train frame become layers; an integer in [0, 7];
           0 = off
  front    the chance that an other object lies in front of the target in a sample; a number in [0, 1]
`eval_lucid_layers.others=3` is an example value: NOTHING here is tuned on data, and no J&F figure exists.

The rules (include/eosvos.h states L1-L6 at `eosvos_lucid_compose_layers`; the kernel is `lucid_layers_kernel` of
csrc/lucid_kernels.hip; `compose_host` below is the numpy twin of L2-L5, checked against the plain loops of
tests/lucid_layers_ref.py; `batch_host` is L7-L10 on the twins).  frame (C, H, W) fp32; ids (H, W) uint8: 0 = background, 1 = the
target, 2 .. M + 1 = the other objects in the order given; a pixel lying in several masks takes the target if it is in the
target's mask, else the largest id (`layer_map`).  "Rule n" without an L is a rule of `lucid.py`.

  L1. plate     rules 1-5 on the mask ids != 0: the existing `eosvos_lucid_plate`, called unchanged.  The hole is the union of
                all layered objects grown by `dilate`.
  L2. sample    `flip` and Bi as in rule 6; a layer count L in [1, 8]; per layer k = 0 .. L - 1, BACK TO FRONT, an id id_k in
                [1, 255], distinct within the sample, and an inverse matrix Oi_k.  Coordinates follow rule 6 entry by entry, once
                for Bi and once per Oi_k.
  L3. coverage  A_k = rule 7 with the tap predicate ids(tap) == id_k: an integer in [0, 1024].
  L4. image     v = Bg, the bicubic sample of the plate at the background coordinates; for k = 0 .. L - 1: A_k == 1024: v = Ob_k;
                else A_k > 0: v = v + (A_k / 1024) * (Ob_k - v); else v unchanged.  Ob_k = the rule-8 bicubic sample of the
                frame at layer k's coordinates.  fp32, every operation rounded on its own.  A kernel may skip work whose result
                is overwritten (it starts at the front-most layer with A == 1024): the bits are the rule's either way.
  L5. visible   top = the largest k with A_k >= 512, or none.  ids_out = id_top, 0 when there is none; label = 1.f iff
                id_top == target_id; counts[s][k] = the number of pixels of sample s whose top is k, an integer sum on a record
                the call zeroes itself.
  L6. one layer is today: L = 1, id_0 = 1 and ids = (mask != 0) give the images, labels and count of `eosvos_lucid_compose` bit
                for bit (the two kernels share `lucid_cubic`, the coordinate and the coverage code).
BATCH (`run_batch`, shared by the twin and the device path):
  L7. draws     Python's `random`.  Per sample, rule 11's nine draws come first, unchanged; then, for each other object in order,
                five draws: angle, factor, shift y, shift x in the OBJECT's ranges (`rot`, `scale`, `shift` of `eval_lucid`),
                about the centre of that object's own bounding box in the id map, then `front = random() < front`.  Layer order:
                the others with `front` False in order, then the target, then the others with `front` True in order.  A redraw
                repeats the target's four draws only.  After `lucid.MAX_TRIES` attempts the target takes the identity matrix and
                every other object goes behind it (with the motion it drew).
  L8. accept    rule 10 with the target's VISIBLE count counts[s][k_target] in place of count[s]; n_mask is the target's pixel
                count in the id map.
  L9. which     candidates are the objects annotated on the target's own train frame whose mask is non-empty in the id map (an
                object wholly under the target or under later objects has no pixel to move), in ascending object index; at most
                `others` of them are taken, the rest stay in the background.  With none, the whole path is today's: today's
                entry, no extra draw.  A target mask that is empty or fills the frame is not synthesised (rule 12).
 L10. off       `None` or others = 0: nothing new is called, nothing new is drawn, the batches are today's bit for bit (`active`).
"""
import random

import numpy as np
import torch

from . import lucid
from .lucid import _int, _np, _real

DEFAULTS = {'others': 0, 'front': 0.5}
MAX_OTHERS = 7
MAX_LAYERS = 8                                           # csrc/kernels.h LUCID_MAX_LAYERS
MAX_SAMPLES_PER_LAUNCH = 8                               # csrc/kernels.h LUCID_LAYERS_MAX_SAMPLES
MAX_SIDE = lucid.MAX_SIDE
TARGET = 1


def check(cfg):
    """The complete, validated parameter dictionary of `cfg` (missing keys take `DEFAULTS`); ValueError otherwise."""
    if not isinstance(cfg, dict) or set(cfg) - set(DEFAULTS):
        raise ValueError(f'lucid_layers={cfg!r}: a dictionary with keys from {sorted(DEFAULTS)}')
    out = dict(DEFAULTS, **cfg)
    v = out['others']
    if not _int(v) or not 0 <= v <= MAX_OTHERS:
        raise ValueError(f'lucid_layers.others={v!r}: an integer in [0, {MAX_OTHERS}] (0 = off)')
    out['others'] = int(v)
    v = out['front']
    if not _real(v) or not 0 <= v <= 1:
        raise ValueError(f'lucid_layers.front={v!r}: a number in [0, 1]')
    out['front'] = float(v)
    return out


def active(cfg):
    """Validated; False when `cfg` layers nothing (None or others 0)."""
    return cfg is not None and check(cfg)['others'] != 0


# ---- the id map and its geometry --------------------------------------------------------------------------------------------
def layer_map(target, others):
    """The id map of the rules from torch ops on the masks' device: target (1, H, W) or (H, W), others (M, 1, H, W) / (M, H, W) or
    a list of masks, M <= 254 -> (H, W) uint8, contiguous.  Later objects overwrite earlier ones, the target overwrites all."""
    target = target.reshape(target.shape[-2:])
    ids = torch.zeros(target.shape, dtype=torch.uint8, device=target.device)
    others = [] if others is None else list(others)
    if len(others) > 254:
        raise ValueError(f'lucid_layers.layer_map: at most 254 other objects, got {len(others)}')
    for j, o in enumerate(others):
        o = o.reshape(o.shape[-2:])
        if o.shape != target.shape:
            raise ValueError(f'lucid_layers.layer_map: object {j} is {tuple(o.shape)}, the target {tuple(target.shape)}')
        ids = torch.where(o.to(target.device) != 0, torch.full_like(ids, j + 2), ids)
    return torch.where(target != 0, torch.full_like(ids, TARGET), ids).contiguous()


def geometry(ids, n_ids=None):
    """[(pixel count, bounding-box centre (cx, cy) or None)] for the ids 0 .. n_ids (default: the largest id present) of an id
    map (H, W) uint8, tensor or array.  For a device tensor this is the one host read per (sequence, object), in place of
    `lucid.mask_geometry`'s."""
    m = _np(ids)
    m = m.reshape(m.shape[-2:])
    n_ids = int(m.max()) if n_ids is None else int(n_ids)
    return [lucid.mask_geometry(m == i) for i in range(n_ids + 1)]


def choose(geo, others):
    """Rule L9: the ids (>= 2) of the at most `others` first objects with a pixel in the id map."""
    return [i for i in range(2, len(geo)) if geo[i][0] > 0][:others]


def relabel(ids, chosen):
    """The id map with the chosen ids renumbered 2, 3, .. in order and every other id above 1 turned into background; the
    same map when nothing changes.  Tensor or array."""
    lut = np.zeros(256, dtype=np.uint8)
    lut[0:2] = (0, 1)
    for j, i in enumerate(chosen):
        lut[i] = j + 2
    if isinstance(ids, torch.Tensor):
        return torch.from_numpy(lut).to(ids.device)[ids.long()].contiguous()
    return lut[ids]


def select(ids, layer_params, n_ids):
    """Rules L9 on an id map: (the id map with only the taken objects, numbered 2 .. , its geometry [(n, centre)] for the ids
    0 .. taken + 1).  One host read for a device tensor."""
    geo = geometry(ids, n_ids)
    chosen = choose(geo, check(layer_params)['others'])
    if chosen != list(range(2, n_ids + 1)):
        ids = relabel(ids, chosen)
    return ids, [geo[0], geo[1]] + [geo[i] for i in chosen]


# ---- the draws and the depth order: one host function for the twin and the device path ------------------------------------
def draw_others(rng, p, front, n_others):
    """The five draws per other object of rule L7: [(motion, in front?)]."""
    out = []
    for _ in range(n_others):
        motion = lucid.draw_motion(rng, p)
        out.append((motion, rng.random() < front))
    return out


def draw_sample(rng, p, front, n_others):
    """Today's nine draws, then five per other object: {'flip', 'bg', 'ob', 'others'}."""
    d = lucid.draw_sample(rng, p)
    d['others'] = draw_others(rng, p, front, n_others)
    return d


def sample_layers(draw, height, width, centres):
    """A draw -> the compose parameters {'flip', 'Bi', 'layers': [(id, Oi)] back to front}; centres[i] is the bounding-box centre
    of id i.  `draw['ob']` None is the fallback of rule L7: the identity for the target, every other object behind it."""
    one = lucid.sample_matrices(draw, height, width, centres[TARGET])
    fallback = draw['ob'] is None
    behind, before = [], []
    for j, (motion, front) in enumerate(draw['others']):
        rot, fac, sy, sx = motion
        c = centres[j + 2]
        oi = lucid.invert(lucid.forward_matrix(c[0], c[1], rot, fac, sx * width, sy * height))
        (before if front and not fallback else behind).append((j + 2, oi))
    return {'flip': one['flip'], 'Bi': one['Bi'], 'layers': behind + [(TARGET, one['Oi'])] + before}


def target_layer(sample):
    return [i for i, _ in sample['layers']].index(TARGET)


def run_batch(compose, k, params, layer_params, geo, height, width, rng=random):
    """Rules L7-L8 around `compose(samples, read) -> (images, labels, counts per sample or None)`: k synthesised samples over
    the geometry `geo` = [(n, centre)] of the ids 0 .. M + 1.  Returns (images (k, C, H, W), labels (k, 1, H, W), records): one
    record per sample with its draw, its compose parameters, `tries`, `count` (the target's visible pixels) and `fallback`."""
    p, front = lucid.check(params), check(layer_params)['front']
    n_mask, centres, n_others = geo[TARGET][0], [g[1] for g in geo], len(geo) - 2

    def ok(s):
        return lucid.accepted(counts[s], n_mask, height, width, p['min_keep'])
    draws = [draw_sample(rng, p, front, n_others) for _ in range(k)]
    plist = [sample_layers(d, height, width, centres) for d in draws]
    images, labels, cn = compose(plist, True)
    counts = [int(c[target_layer(q)]) for c, q in zip(cn, plist)]
    tries = [1] * k
    pending = [s for s in range(k) if not ok(s)]
    attempt = 1
    while pending and attempt < lucid.MAX_TRIES:
        attempt += 1
        for s in pending:
            draws[s] = dict(draws[s], ob=lucid.draw_motion(rng, p))
            plist[s] = sample_layers(draws[s], height, width, centres)
            tries[s] = attempt
        im, lb, cn = compose([plist[s] for s in pending], True)
        images[pending], labels[pending] = im, lb
        for s, c in zip(pending, cn):
            counts[s] = int(c[target_layer(plist[s])])
        pending = [s for s in pending if not ok(s)]
    fallback = set(pending)
    if pending:
        for s in pending:
            draws[s] = dict(draws[s], ob=None)
            plist[s] = sample_layers(draws[s], height, width, centres)
        im, lb, _ = compose([plist[s] for s in pending], False)
        images[pending], labels[pending] = im, lb
    records = [dict(plist[s], draw=draws[s], tries=tries[s], count=None if s in fallback else counts[s], fallback=s in fallback)
               for s in range(k)]
    return images, labels, records


# ---- the numpy twin ---------------------------------------------------------------------------------------------------------
def _ids_map(who, ids, shape):
    m = _np(ids)
    if m.dtype != np.uint8 or m.shape != tuple(shape):
        raise ValueError(f'{who}: ids must be {tuple(shape)} uint8, got {m.dtype} {m.shape}')
    return m


def check_samples(who, samples):
    if not samples:
        raise ValueError(f'{who}: no sample')
    for prm in samples:
        got = [i for i, _ in prm['layers']]
        if not 1 <= len(got) <= MAX_LAYERS or len(set(got)) != len(got) or any(not _int(i) or not 1 <= i <= 255 for i in got):
            raise ValueError(f'{who}: a sample has 1 .. {MAX_LAYERS} layers with distinct ids in [1, 255], got {got}')


def coverage(on, yq, xq):
    """Rule 7 / L3: boolean (H, W) and the 5-bit coordinates -> int64 (H, W) in [0, 1024]."""
    h, w = on.shape
    oy, ox, fy, fx = yq >> 5, xq >> 5, yq & 31, xq & 31
    cover = np.zeros(yq.shape, dtype=np.int64)
    for i in (0, 1):
        for j in (0, 1):
            yy, xx = oy + i, ox + j
            inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            hit = inside & on[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
            cover += np.where(hit, (fy if i else 32 - fy) * (fx if j else 32 - fx), 0)
    return cover


def compose_host(frame, ids, plate, samples, target_id=TARGET, dtype=np.float32):
    """Rules L2-L5 in numpy: frame (C, H, W) fp32, ids (H, W) uint8, plate (C, H, W), samples = [{'flip', 'Bi', 'layers'}] ->
    (images (S, C, H, W) of `dtype`, labels (S, 1, H, W) float32 of 0 / 1, ids_out (S, H, W) uint8, counts (S, 8) int64)."""
    f = _np(frame)
    if f.dtype != np.float32 or f.ndim != 3 or min(f.shape) < 1 or max(f.shape[1:]) > MAX_SIDE:
        raise ValueError(f'lucid_layers.compose_host: frame must be (C, H, W) float32 with 1 <= H, W <= {MAX_SIDE}, got {f.dtype} {f.shape}')
    idm = _ids_map('lucid_layers.compose_host', ids, f.shape[1:])
    dt = np.dtype(dtype).type
    pl = _np(plate).astype(dt)
    if pl.shape != f.shape:
        raise ValueError(f'lucid_layers.compose_host: plate must be {f.shape}, got {pl.shape}')
    check_samples('lucid_layers.compose_host', samples)
    if not _int(target_id) or not 1 <= target_id <= 255:
        raise ValueError(f'lucid_layers.compose_host: target_id={target_id!r}: an integer in [1, 255]')
    fr = f.astype(dt)
    c, h, w = f.shape
    n = len(samples)
    tab = lucid.cubic_table()
    images = np.empty((n, c, h, w), dtype=dt)
    labels = np.empty((n, 1, h, w), dtype=np.float32)
    ids_out = np.empty((n, h, w), dtype=np.uint8)
    counts = np.zeros((n, MAX_LAYERS), dtype=np.int64)
    for s, prm in enumerate(samples):
        yb, xb = lucid.fixed_coords(prm['Bi'], h, w, prm['flip'])
        v = lucid._cubic(pl, yb, xb, tab, dt)
        top = np.full((h, w), -1, dtype=np.int64)
        for k, (i, oi) in enumerate(prm['layers']):
            yo, xo = lucid.fixed_coords(oi, h, w, prm['flip'])
            cover = coverage(idm == i, yo, xo)
            ob = lucid._cubic(fr, yo, xo, tab, dt)
            alpha = (cover.astype(dt) / dt(1024))[None]
            v = np.where(cover[None] == 1024, ob, np.where(cover[None] == 0, v, v + alpha * (ob - v)))
            top = np.where(cover >= 512, k, top)
        layer_id = np.array([0] + [i for i, _ in prm['layers']], dtype=np.uint8)       # top -1 -> 0
        images[s] = v
        ids_out[s] = layer_id[top + 1]
        labels[s, 0] = ids_out[s] == target_id
        for k in range(len(prm['layers'])):
            counts[s, k] = int((top == k).sum())
    return images, labels, ids_out, counts


def layer_map_host(target, others):
    """`layer_map` in numpy."""
    t = _np(target)
    t = t.reshape(t.shape[-2:])
    ids = np.zeros(t.shape, dtype=np.uint8)
    for j, o in enumerate([] if others is None else others):
        o = _np(o)
        ids[o.reshape(o.shape[-2:]) != 0] = j + 2
    ids[t != 0] = TARGET
    return ids


def batch_host(frame, target, others, params, layer_params, batch, rng=random, dtype=np.float32, plain=None):
    """Rules L7-L10 on the twins: a round-0 batch of `batch` samples, as `lucid.batch_host` (which this IS when the layers are
    off, no other object has a pixel, or the target is empty or fills the frame).  Returns (images, labels, records)."""
    p = lucid.check(params)
    n_others = 0 if others is None else len(others)
    if not active(layer_params) or n_others == 0:
        return lucid.batch_host(frame, target, params, batch, rng, dtype, plain)
    f = _np(frame)
    ids, geo = select(layer_map_host(target, others), layer_params, n_others + 1)
    h, w = ids.shape
    if len(geo) == 2 or not 0 < geo[TARGET][0] < h * w:
        return lucid.batch_host(frame, target, params, batch, rng, dtype, plain)
    k = min(p['samples'], batch)
    parts_i, parts_l, records = [], [], []
    if batch - k:
        im, lb = plain(batch - k)
        parts_i.append(_np(im, dtype))
        parts_l.append(_np(lb, np.float32))
    if k:
        plate = lucid.plate_host(f, ids != 0, p['dilate'], dtype)

        def compose(samples, read):
            im, lb, _, cn = compose_host(f, ids, plate, samples, TARGET, dtype)
            return im, lb, cn
        im, lb, records = run_batch(compose, k, p, layer_params, geo, h, w, rng)
        parts_i.append(im)
        parts_l.append(lb)
    return np.concatenate(parts_i), np.concatenate(parts_l), records


# ---- the device path --------------------------------------------------------------------------------------------------------
def compose_chunked(engine, frame, ids, plate, samples, read=True):
    """`Engine.lucid_compose_layers` for any number of samples, one launch per `MAX_SAMPLES_PER_LAUNCH` of them: (images,
    labels, counts per sample, or [] without `read`)."""
    im, lb, cn = [], [], []
    for i in range(0, len(samples), MAX_SAMPLES_PER_LAUNCH):
        a, b, c, _ = engine.lucid_compose_layers(frame, ids, plate, samples[i:i + MAX_SAMPLES_PER_LAUNCH], TARGET, read_counts=read)
        im.append(a)
        lb.append(b)
        cn += c or []
    return (im[0], lb[0], cn) if len(im) == 1 else (torch.cat(im), torch.cat(lb), cn)


class LayeredAugmenter:
    """The layered lucid samples of one (frame, target, others) triple on the engine's GPU: the id map, its geometry (the one
    host read) and the plate are built once, here; `batch(k)` composes k samples with one launch and one host read per attempt,
    as `lucid.LucidAugmenter.batch`.  `has_layers` False (no other object has a pixel): build a `LucidAugmenter` instead."""

    def __init__(self, engine, frame, target, others, params, layer_params, rng=random):
        """frame (C, H, W), target (1, H, W), others (M, 1, H, W): contiguous fp32 device tensors."""
        self.engine, self.rng = engine, rng
        self.params, self.layer_params = lucid.check(params), check(layer_params)
        if self.params['samples'] == 0 or self.layer_params['others'] == 0:
            raise ValueError('lucid_layers.LayeredAugmenter: lucid.samples or lucid_layers.others is 0 (off)')
        self.frame = frame
        self.height, self.width = int(frame.shape[1]), int(frame.shape[2])
        n_others = 0 if others is None else len(others)
        self.ids, self.geo = select(layer_map(target, others), self.layer_params, n_others + 1)
        self.n_mask = self.geo[TARGET][0]
        self.has_object = 0 < self.n_mask < self.height * self.width
        self.has_layers = len(self.geo) > 2
        self.plate = None
        if self.has_object and self.has_layers:
            self.plate = engine.lucid_plate(frame, (self.ids != 0).float().unsqueeze(0), self.params['dilate'])

    def _compose(self, samples, read):
        return compose_chunked(self.engine, self.frame, self.ids, self.plate, samples, read)

    def batch(self, k):
        """k synthesised samples: (images (k, C, H, W), labels (k, 1, H, W), records) as `run_batch`."""
        if not (self.has_object and self.has_layers):
            raise ValueError('lucid_layers.LayeredAugmenter.batch: no other object, or the target is empty or fills the frame')
        return run_batch(self._compose, int(k), self.params, self.layer_params, self.geo, self.height, self.width, self.rng)
