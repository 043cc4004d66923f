"""Object-centred zoom pass of the inference calls: every frame gets a second look at a crop around the object the first pass
found, magnified to the frame's own size, and the two predictions are blended inside the crop.  DeepLabV3+ runs at output
stride 16 with a stride-4 decoder: in a 480 x 854 frame a 30-pixel object is two cells of the ASPP input, and nothing that works
on label maps afterwards (CRF, snapping, component filter, hole filling) recovers what the network never resolved.  The
OSVOS / PReMVOS family answers small objects with this second look.  The zoomed view has the frame's own size, so it runs on the
model's LIVE engine with the fine-tuned weights already in it: no view engine, no `sync()`, no weight export, no new launch
plan.  The reference scores each frame once (`helper_func.py:131-142`); this is an opt-in extension (`config.ZOOM`), off by
default.

    zoom = {'max_zoom': 0, 'min_zoom': 1.5, 'threshold': 0.5, 'min_pixels': 16, 'margin': 0.5, 'margin_px': 8,
            'weight': 0.5, 'feather': 8}                                                                      (`DEFAULTS`)

  max_zoom    largest magnification; 0 = off, else in [1, 4]
  min_zoom    a frame whose box would magnify less is left alone; in [1, max_zoom]
  threshold   first-pass foreground is p >= threshold (an fp32 compare); in (0, 1)
  min_pixels  fewer foreground pixels: the frame is left alone; >= 1
  margin      context, as a share of the longer side of the mask box, per side; in [0, 4]
  margin_px   context in pixels, added to it; in [0, 256]
  weight      share of the zoomed probability inside the box; in (0, 1]
  feather     width of the linear ramp at the box edge, pixels; in [0, 64]
`eval_zoom.max_zoom=3 eval_zoom.margin=0.5` are example values: NOTHING here is tuned on data.

The rules (include/eosvos.h states them at `eosvos_zoom_boxes` .. `eosvos_zoom_blend`; the kernels are csrc/zoom_kernels.hip;
`boxes_host` below is the numpy twin of the box, bit-equal to the device and itself checked against the plain loops of
tests/zoom_ref.py; `refine_host` restates cut, put-back and blend with `F.interpolate` on slices).  Per frame, from its
first-pass probabilities p0 -- the plain inference, or the mean over the views with `tta`.  Box arithmetic is in integers only;
the two zooms and the margin enter as Q16, zq = round(z * 65536) (`q16`).

  1. mask box   my0, my1, mx0, mx1 = the inclusive bounds of {p0 >= threshold}, cnt = its size.  cnt < min_pixels: INVALID.
  2. extent     mh = my1 - my0 + 1, mw likewise; pad = ((max(mh, mw) * margin_q16) >> 16) + margin_px; gh = mh + 2 pad,
                gw = mw + 2 pad.
  3. box size   bh = min(H, max(gh, ceil(gw * H / W), ceil(H * 65536 / max_zoom_q16))); bw = min(W, ceil(bh * W / H)): the
                frame's aspect.  bh * min_zoom_q16 > H * 65536: INVALID (the object is already large, or a distant false
                positive has blown the box up).
  4. position   y0 = clamp((2 my0 + mh - bh) >> 1, 0, H - bh) with an arithmetic shift; x0 likewise.
  5. record     five int32 per frame: valid, y0, x0, bh, bw.  Invalid frames carry 0, 0, 0, H, W.
  6. cut        view = bilinear(frame[:, y0:y0+bh, x0:x0+bw] -> H x W), torch's `align_corners=False` rule applied to the slice
                (it clamps at the box edge).  An invalid frame is copied through; its forward still runs -- nothing between the
                first pass and the blended result reads from the device, and that is the price -- and nothing reads its logits.
  7. score      `Engine.infer_view(view, mirror)` on the live engine: plain, and also mirrored when `tta.flip` is on.
                `tta.scales` does not apply to the zoomed view.
  8. put back   pz = the equal-weight mean over those one or two views of sigmoid(bilinear(un-mirrored view logits,
                H x W -> bh x bw)), defined inside the box only.  Plain bilinear down-sampling: the logits are a x4 bilinear
                up-sampling of the decoder's output, so up to max_zoom 4 point sampling between them loses nothing the network
                produced.
  9. blend      fp32, in this order: out = p0 + (weight * f) * (pz - p0) inside the box, out = p0 outside.  The ramp is
                f = min(1, (d + 1) / (feather + 1)), d the smallest distance in whole pixels to a box side that is NOT on the
                frame border; no such side, or feather 0: f = 1.  Invalid frames are not written at all: their bits are p0's.
 10. off        `None` or max_zoom = 0: nothing new is called (`active`).
"""
import numbers

import numpy as np
import torch
import torch.nn.functional as F

DEFAULTS = {'max_zoom': 0, 'min_zoom': 1.5, 'threshold': 0.5, 'min_pixels': 16, 'margin': 0.5, 'margin_px': 8, 'weight': 0.5,
            'feather': 8}
MAX_ZOOM = 4
MAX_MARGIN = 4
MAX_MARGIN_PX = 256
MAX_FEATHER = 64
MAX_SIDE = 4096


def _real(v):
    return not isinstance(v, bool) and isinstance(v, numbers.Real)


def _int(v):
    return not isinstance(v, bool) and isinstance(v, numbers.Integral)


def check(cfg):
    """The complete, validated parameter dictionary of `cfg` (missing keys take `DEFAULTS`); ValueError otherwise."""
    if not isinstance(cfg, dict) or set(cfg) - set(DEFAULTS):
        raise ValueError(f'zoom={cfg!r}: a dictionary with keys from {sorted(DEFAULTS)}')
    out = dict(DEFAULTS, **cfg)
    v = out['max_zoom']
    if not _real(v) or not (v == 0 or 1 <= v <= MAX_ZOOM):
        raise ValueError(f'zoom.max_zoom={v!r}: 0 (off) or a number in [1, {MAX_ZOOM}]')
    out['max_zoom'] = float(v)
    v = out['min_zoom']
    hi = out['max_zoom'] if out['max_zoom'] else MAX_ZOOM
    if not _real(v) or not 1 <= v <= hi:
        raise ValueError(f'zoom.min_zoom={v!r}: a number in [1, max_zoom]')
    out['min_zoom'] = float(v)
    v = out['threshold']
    if not _real(v) or not 0 < v < 1:
        raise ValueError(f'zoom.threshold={v!r}: a number in (0, 1)')
    out['threshold'] = float(v)
    v = out['min_pixels']
    if not _int(v) or v < 1:
        raise ValueError(f'zoom.min_pixels={v!r}: an integer >= 1')
    out['min_pixels'] = int(v)
    v = out['margin']
    if not _real(v) or not 0 <= v <= MAX_MARGIN:
        raise ValueError(f'zoom.margin={v!r}: a number in [0, {MAX_MARGIN}]')
    out['margin'] = float(v)
    v = out['weight']
    if not _real(v) or not 0 < v <= 1:
        raise ValueError(f'zoom.weight={v!r}: a number in (0, 1]')
    out['weight'] = float(v)
    for k, hi in (('margin_px', MAX_MARGIN_PX), ('feather', MAX_FEATHER)):
        v = out[k]
        if not _int(v) or not 0 <= v <= hi:
            raise ValueError(f'zoom.{k}={v!r}: an integer in [0, {hi}]')
        out[k] = int(v)
    return out


def active(cfg):
    """Validated; False when `cfg` zooms nothing (None or max_zoom 0)."""
    return cfg is not None and check(cfg)['max_zoom'] != 0


def q16(z):
    """round(z * 65536): how the two zooms and the margin enter the integer box arithmetic."""
    return int(round(z * 65536))


def _ceil_div(a, b):
    return -((-a) // b)


def box_of_bounds(cnt, my0, my1, mx0, mx1, height, width, p):
    """Rules 1 (the count) to 5 on Python integers: the record (valid, y0, x0, bh, bw) of a frame whose foreground has `cnt`
    pixels within rows my0..my1 and columns mx0..mx1."""
    H, W = int(height), int(width)
    if cnt < p['min_pixels']:
        return (0, 0, 0, H, W)
    mh, mw = my1 - my0 + 1, mx1 - mx0 + 1
    pad = ((max(mh, mw) * q16(p['margin'])) >> 16) + p['margin_px']
    gh, gw = mh + 2 * pad, mw + 2 * pad
    bh = min(H, max(gh, _ceil_div(gw * H, W), _ceil_div(H * 65536, q16(p['max_zoom']))))
    bw = min(W, _ceil_div(bh * W, H))
    if bh * q16(p['min_zoom']) > H * 65536:
        return (0, 0, 0, H, W)
    y0 = min(max((2 * my0 + mh - bh) >> 1, 0), H - bh)
    x0 = min(max((2 * mx0 + mw - bw) >> 1, 0), W - bw)
    return (1, y0, x0, bh, bw)


def boxes_host(p0, params):
    """Rules 1-5 in numpy: p0 (N, 1, H, W) or (N, H, W) fp32 (tensor or array) -> (N, 5) int32 array, bit-equal to
    `Engine.zoom_boxes`."""
    p = check(params)
    if p['max_zoom'] == 0:
        raise ValueError('boxes_host: zoom.max_zoom is 0 (off)')
    a = p0.detach().cpu().numpy() if isinstance(p0, torch.Tensor) else np.asarray(p0)
    if a.dtype != np.float32:
        raise ValueError(f'boxes_host: expected float32, got {a.dtype}')
    if a.ndim == 4 and a.shape[1] == 1:
        a = a[:, 0]
    if a.ndim != 3 or min(a.shape[1:]) < 1 or max(a.shape[1:]) > MAX_SIDE:
        raise ValueError(f'boxes_host: p0 must be (N, 1, H, W) or (N, H, W) with 1 <= H, W <= {MAX_SIDE}, got {tuple(p0.shape)}')
    n, h, w = a.shape
    out = np.empty((n, 5), dtype=np.int32)
    for f in range(n):
        m = a[f] >= np.float32(p['threshold'])
        cnt = int(m.sum())
        if cnt:
            rows, cols = np.flatnonzero(m.any(axis=1)), np.flatnonzero(m.any(axis=0))
            out[f] = box_of_bounds(cnt, int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1]), h, w, p)
        else:
            out[f] = (0, 0, 0, h, w)
    return out


def _boxes_list(boxes):
    b = boxes.detach().cpu().numpy() if isinstance(boxes, torch.Tensor) else np.asarray(boxes)
    return [tuple(int(v) for v in row) for row in b.reshape(-1, 5)]


def crop_host(frames, boxes, dtype=torch.float64):
    """Rule 6 with `F.interpolate` on the slices: frames (B, C, H, W) -> views (B, C, H, W) of `dtype` on the CPU."""
    x = frames.detach().cpu().to(dtype)
    h, w = x.shape[2:]
    out = x.clone()
    for f, (valid, y0, x0, bh, bw) in enumerate(_boxes_list(boxes)):
        if valid:
            out[f:f + 1] = F.interpolate(x[f:f + 1, :, y0:y0 + bh, x0:x0 + bw], (h, w), mode='bilinear', align_corners=False)
    return out


def put_back_host(view_logits, boxes, dtype=torch.float64, fill=0.0):
    """Rule 8: view_logits = [(logits (B, 1, H, W) as the engine leaves them, mirrored)] -> pz (B, 1, H, W) of `dtype` on the
    CPU; `fill` outside the boxes and in invalid frames."""
    first = view_logits[0][0]
    pz = torch.full(tuple(first.shape), fill, dtype=dtype)
    wt = 1.0 / len(view_logits)
    for f, (valid, y0, x0, bh, bw) in enumerate(_boxes_list(boxes)):
        if not valid:
            continue
        acc = 0
        for logits, mirror in view_logits:
            u = logits.detach().cpu().to(dtype)[f:f + 1]
            if mirror:
                u = torch.flip(u, [3])
            acc = acc + wt * torch.sigmoid(F.interpolate(u, (bh, bw), mode='bilinear', align_corners=False))
        pz[f:f + 1, :, y0:y0 + bh, x0:x0 + bw] = acc
    return pz


def ramp_host(box, height, width, feather, dtype=torch.float64):
    """The ramp f of rule 9 over one box: (bh, bw) of `dtype`."""
    _, y0, x0, bh, bw = box
    big = height + width
    yy = torch.arange(bh).view(-1, 1).expand(bh, bw)
    xx = torch.arange(bw).view(1, -1).expand(bh, bw)
    d = torch.full((bh, bw), big, dtype=torch.int64)
    if y0 > 0:
        d = torch.minimum(d, yy)
    if y0 + bh < height:
        d = torch.minimum(d, bh - 1 - yy)
    if x0 > 0:
        d = torch.minimum(d, xx)
    if x0 + bw < width:
        d = torch.minimum(d, bw - 1 - xx)
    if feather == 0:
        return torch.ones(bh, bw, dtype=dtype)
    return torch.clamp((d + 1).to(dtype) / torch.tensor(feather + 1, dtype=dtype), max=1.0)


def blend_host(p0, pz, boxes, weight, feather, dtype=torch.float64):
    """Rule 9: p0, pz (B, 1, H, W) -> the blended probabilities (B, 1, H, W) of `dtype` on the CPU.  `weight` enters as the
    fp32 value the kernel receives."""
    out = p0.detach().cpu().to(dtype).clone()
    z = pz.detach().cpu().to(dtype)
    h, w = out.shape[2:]
    wt = torch.tensor(float(np.float32(weight)), dtype=dtype)
    for f, box in enumerate(_boxes_list(boxes)):
        valid, y0, x0, bh, bw = box
        if not valid:
            continue
        a = out[f, 0, y0:y0 + bh, x0:x0 + bw]
        out[f, 0, y0:y0 + bh, x0:x0 + bw] = a + (wt * ramp_host(box, h, w, feather, dtype)) * (z[f, 0, y0:y0 + bh, x0:x0 + bw] - a)
    return out


def refine_host(frames, p0, params, score, flip=False, dtype=torch.float64, boxes=None):
    """Rules 1-9 on the CPU in `dtype`: frames (B, 3, H, W), p0 (B, 1, H, W) fp32; `score(view, mirror)` returns the logits
    (B, 1, H, W) of a forward on the view (fed mirrored when `mirror`, logits as they come out: still mirrored).  `boxes`:
    the records to use instead of `boxes_host(p0)`.  Returns (probabilities, boxes)."""
    p = check(params)
    boxes = boxes_host(p0, p) if boxes is None else boxes
    view = crop_host(frames, boxes, dtype)
    logits = [(score(view, m), m) for m in ((False, True) if flip else (False,))]
    pz = put_back_host(logits, boxes, dtype)
    return blend_host(p0, pz, boxes, p['weight'], p['feather'], dtype), boxes


class Refiner:
    """The zoom pass of one model at one frame size, next to `tta.ViewSet`: holds the per-size temporaries (boxes, view, pz,
    one set per batch size) and does `refine(frames, p0) -> probs`.  Everything runs on the model's live engine; nothing
    between the first pass and the blended result reads from the device."""

    def __init__(self, model, height, width, zoom, tta=None):
        from . import tta as tta_views
        self.model, self.height, self.width = model, height, width
        self.params = check(zoom)
        if self.params['max_zoom'] == 0:
            raise ValueError('zoom.Refiner: zoom.max_zoom is 0 (off)')
        self.mirrors = (False, True) if tta is not None and tta_views.check(tta)[0] else (False,)
        self._tmp = {}                                              # batch -> (view, pz)

    def refine(self, frames, p0):
        """frames (B, 3, H, W), p0 (B, 1, H, W): the first pass, refined IN PLACE and returned."""
        eng = self.model.engine
        b = frames.shape[0]
        if b not in self._tmp or self._tmp[b][0].device != frames.device:
            self._tmp[b] = (torch.empty_like(frames), torch.empty_like(p0))
        view, pz = self._tmp[b]
        boxes = eng.zoom_boxes(p0, self.params)
        eng.zoom_crop(frames, boxes, out=view)
        wt = 1.0 / len(self.mirrors)
        for k, mirror in enumerate(self.mirrors):
            eng.infer_view(view, mirror)
            eng.zoom_accumulate(boxes, pz, wt, mirror=mirror, first=k == 0)
        return eng.zoom_blend(boxes, pz, p0, self.params['weight'], self.params['feather'])
