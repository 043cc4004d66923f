"""Test-time augmentation of the inference passes: every frame is scored as the mean, in probability space, of a few views
of it -- each scale of `scales`, plain and (with `flip`) mirrored left-right -- the test-time ensemble of the OSVOS / OnAVOS
family.  The reference scores one view (`helper_func.py:131-142`); this is an opt-in extension (`config.EXTENSIONS`).

    tta = {'flip': bool, 'scales': [floats]}

  views     every scale, times {plain, mirrored} with `flip`, equal weights 1 / #views (they sum to 1: the accumulator is the
            probability map, nothing divides it afterwards)
  view size round(H * s) x round(W * s); the frame is resampled to it, and the view's logits back to H x W, bilinearly with
            torch's `align_corners=False` rule (source coordinate max(0, (in / out) * (o + 0.5) - 0.5), upper neighbour
            clamped at the edge); a view of the frame's own size is not resampled at all
  per view  `Engine.resize_frames` (other sizes only) -> `Engine.infer_view` (the mirror happens in the layout pass) ->
            `Engine.tta_accumulate` (un-mirror + resize + sigmoid + weighted add, one launch)

`None` and the neutral dictionary {'flip': False, 'scales': [1.0]} mean "off": callers then take their single-view code path,
call for call (`active`).
"""
import numbers

MIN_FRAME = 32          # the smallest height / width an engine is built for (`eosvos_create_ex`)


def active(tta):
    """Validated `tta`; False when it asks for the one plain view of today's path (None or the neutral dictionary)."""
    if tta is None:
        return False
    flip, scales = check(tta)
    return flip or scales != [1.0]


def check(tta):
    """(flip, scales) of a valid `tta` dictionary; ValueError otherwise."""
    if not isinstance(tta, dict) or set(tta) - {'flip', 'scales'}:
        raise ValueError(f"tta={tta!r}: a dictionary {{'flip': bool, 'scales': [floats]}}")
    flip = tta.get('flip', False)
    scales = tta.get('scales', [1.0])
    if not isinstance(flip, bool):
        raise ValueError(f'tta.flip={flip!r}: True or False')
    if not isinstance(scales, (list, tuple)) or len(scales) == 0:
        raise ValueError(f'tta.scales={scales!r}: a non-empty list of scales')
    for s in scales:
        if isinstance(s, bool) or not isinstance(s, numbers.Real) or not s > 0 or s == float('inf'):
            raise ValueError(f'tta.scales={scales!r}: every scale must be a finite number > 0')
    return flip, [float(s) for s in scales]


def views(tta, height, width):
    """[(view height, view width, mirrored, weight)] of one height x width frame, in evaluation order."""
    flip, scales = check(tta)
    out = []
    for s in scales:
        h, w = int(round(height * s)), int(round(width * s))
        if h < MIN_FRAME or w < MIN_FRAME:
            raise ValueError(f'tta.scales: scale {s} makes a {h} x {w} view of a {height} x {width} frame; the engine needs at '
                             f'least {MIN_FRAME} x {MIN_FRAME}')
        for mirror in ((False, True) if flip else (False,)):
            out.append((h, w, mirror))
    weight = 1.0 / len(out)
    return [(h, w, m, weight) for h, w, m in out]


class ViewSet:
    """The views of one model at one frame size.  Views of the frame's own size run on the model's live engine; every other
    size has an engine of its own beside it (`model._view_engine`), which `sync()` gives the live engine's CURRENT
    (fine-tuned) weights -- call it whenever they have changed, once per run of inference calls."""

    def __init__(self, model, height, width, tta):
        self.model, self.height, self.width = model, height, width
        self.views = views(tta, height, width)
        self.engines = None                                     # view size -> engine, as of the last sync()

    def sync(self):
        main = self.model.engine
        theta = None
        self.engines = {}
        for h, w in sorted({(h, w) for h, w, _, _ in self.views if (h, w) != (self.height, self.width)}):
            if theta is None:
                theta = main.get_params()                       # one export for every view engine
            eng = self.engines[(h, w)] = self.model._view_engine(h, w, main.max_batch)
            eng.set_params(theta)

    def infer(self, frames):
        """frames (B, 3, H, W) -> probabilities (B, 1, H, W): the weighted sum over the views."""
        if self.engines is None:
            self.sync()
        main = self.model.engine
        own = (self.height, self.width)
        acc = frames.new_empty(frames.shape[0], 1, self.height, self.width)
        scaled = {}                                             # view size -> resampled frames (shared by plain / mirrored)
        for k, (h, w, mirror, weight) in enumerate(self.views):
            if (h, w) == own:
                eng, x = main, frames
            else:
                eng = self.engines[(h, w)]
                if (h, w) not in scaled:
                    scaled[(h, w)] = main.resize_frames(frames, h, w)
                x = scaled[(h, w)]
            eng.infer_view(x, mirror)
            eng.tta_accumulate(acc, weight, mirror, first=k == 0)
        return acc
