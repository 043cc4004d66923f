"""The evaluation's opt-in option groups: one table, one row per group.

A group is a dictionary of parameters that switches on one optional stage of the evaluation path (`evaluate.py`).  None of them is
part of the reference's key set (`config.BASE`): `config.parse_cli` adds a group, with the neutral values of its row, only when the
command line sets one of its keys; `from_cfg` turns the groups a config carries into the keywords of `evaluate.evaluate_dataset`.
The public functions of `evaluate.py` take the groups by keyword (`split`), consume none of them, and forward each share to its
consumer under the row's travel rule (`travelling`): an unset, `None` or -- where the rule says so -- inactive group is absent from
the consumer's call, which is then the call made before the group existed: nothing new is called, nothing is drawn.

Adding a group = a module with `DEFAULTS` / `check` / `active`, and one row here.  This module imports nothing heavy: the rows'
modules are imported when a row is used, so that `config` stays importable without torch.
"""
from collections import namedtuple
from importlib import import_module

OBJECT, MERGE = 'object', 'merge'   # the consumer: `evaluate.finetune_object_steps`, `evaluate.merge_objects`
SET, ACTIVE = 'set', 'active'       # travels when the value is not None / when the module's `active(value)` (which validates) is true

# keyword   what the functions of `evaluate.py` take               key      the config key (`key.name=value` on the command line)
# module    owns `check` (validated parameters or ValueError)       stage    which consumer the group goes to
#           and `active`                                            travels  SET or ACTIVE
# brings    what travels beside it: `lucid_others` (the other objects' masks at the object's train frame, the caller's data), or
#           `frame_offset` (what the data set subtracted from the RGB frames, when `data_cfg.normalize` is set)
# needs     (consumer(cfg), hint): an active group without its consumer in the config is an error of `check_cfg`
# example   command-line values that switch it on -- examples, untuned (eval_adapt: OnAVOS's published 480p values)
# defaults  the neutral values: with them the group is off
# about     what it does
Group = namedtuple('Group', 'keyword key module stage travels brings needs example defaults about')


def _mod(name):
    return import_module('.' + name, __package__)


def _gate_or_overlap(cfg):
    components, holes = _mod('components'), _mod('holes')
    fill = cfg.get('eval_holes', {})
    return components.check(cfg.get('eval_components', {}))['gate'] or \
        (holes.active(fill) and holes.overlap_q16(holes.check(fill)['prev_overlap']))


TABLE = (
    Group('tta', 'eval_tta', 'tta', OBJECT, SET, None, None, 'eval_tta.flip=True eval_tta.scales=[0.75,1.0,1.25]',
          {'flip': False, 'scales': [1.0]},
          'Test-time augmentation: every inference call (the propagated targets of the adaptation rounds included) averages mirrored '
          'and rescaled views in probability space with equal weights; one plain view = off.'),
    Group('crf', 'eval_crf', 'crf', MERGE, SET, None, None, 'eval_crf.iterations=5 eval_crf.w_appearance=10',
          {'iterations': 0, 'radius': 5, 'dilation': 2, 'w_appearance': 10.0, 'w_smooth': 3.0, 'theta_alpha': 8.0, 'theta_beta': 0.05,
           'theta_gamma': 3.0},
          'Local dense-CRF refinement of the merged label maps against the frames; a frame that is the train frame of every object '
          'keeps the plain merge (its seeded ground truth).  0 iterations = off; the other values are customary, not tuned on data.'),
    Group('components', 'eval_components', 'components', MERGE, SET, None, None,
          'eval_components.gate=24 eval_components.min_rel_area=0.05 eval_components.largest_only=True',
          {'connectivity': 8, 'min_area': 0, 'min_rel_area': 0.0, 'largest_only': False, 'gate': 0},
          'Connected-component filter after the merge, the CRF and the snapping: small, non-dominant and ungated components are '
          'zeroed frame by frame; the train frame passes unchanged and anchors the gate of the frame after it.'),
    Group('holes', 'eval_holes', 'holes', MERGE, ACTIVE, None, None, 'eval_holes.max_area=64 eval_holes.prev_overlap=0.5',
          {'connectivity': 8, 'max_area': 0, 'max_rel_area': 1.0, 'prev_overlap': 0.0},
          'Hole filling, last in the chain: enclosed background islands that are small and were object in the previous frame\'s '
          'filled map are filled; the train frame passes unchanged and anchors that chain.  max_area 0 = off.'),
    Group('snap', 'eval_snap', 'snap', MERGE, ACTIVE, 'frame_offset', None, 'eval_snap.step=16 eval_snap.min_share=0.6',
          {'step': 0, 'iterations': 5, 'compactness': 10, 'min_share': 0.5},
          'Superpixel snapping between the CRF and the component filter: every SLIC superpixel of the frame, quantised back to uint8 '
          'RGB, takes its majority label; the train frame passes unchanged.  step 0 = off.'),
    Group('motion', 'eval_motion', 'motion', MERGE, ACTIVE, 'frame_offset',
          (_gate_or_overlap, 'set eval_components.gate or eval_holes.prev_overlap'), 'eval_motion.block=8 eval_motion.radius=24',
          {'block': 0, 'radius': 16, 'bias': 2},
          'Motion compensation of the clean-up\'s temporal rules: the gate of the component filter and `prev_overlap` of the hole '
          'filler see the previous frame\'s cleaned map warped by block motion of the quantised frames.  block 0 = off.'),
    Group('zoom', 'eval_zoom', 'zoom', OBJECT, SET, None, None, 'eval_zoom.max_zoom=3 eval_zoom.margin=0.5',
          {'max_zoom': 0, 'min_zoom': 1.5, 'threshold': 0.5, 'min_pixels': 16, 'margin': 0.5, 'margin_px': 8, 'weight': 0.5,
           'feather': 8},
          'Object-centred zoom pass: every inference call is followed by a second look at a crop around the object its first pass '
          'found, magnified to the frame\'s size on the live engine and blended in inside the crop.  max_zoom 0 = off.'),
    Group('lucid', 'eval_lucid', 'lucid', OBJECT, SET, None, None, 'eval_lucid.samples=2 eval_lucid.shift=0.1',
          {'samples': 0, 'dilate': 4, 'rot': 15.0, 'scale': 0.15, 'shift': 0.1, 'bg_rot': 5.0, 'bg_scale': 0.05, 'bg_shift': 0.05,
           'min_keep': 0.5},
          'Lucid first-frame synthesis: the last `samples` samples of every round-0 batch are composed from the train frame -- the '
          'object cut out, the hole filled, object and background moved independently.  samples 0 = off.'),
    Group('adapt', 'eval_adapt', 'adapt', OBJECT, SET, None,
          (lambda cfg: cfg['eval_online_adapt']['step'], 'set eval_online_adapt.step'), 'eval_adapt.neg_dist=220 eval_adapt.erode=15',
          {'neg_dist': 0, 'erode': 0},
          'Distance-gated negatives for online adaptation: the propagated targets of the adaptation rounds are 0 wherever a pixel is '
          'farther than `neg_dist` from the mask of the frame before it, eroded by `erode`.  neg_dist 0 = off.'),
    Group('layers', 'eval_lucid_layers', 'lucid_layers', OBJECT, SET, 'lucid_others',
          (lambda cfg: _mod('lucid').active(cfg.get('eval_lucid')), 'set eval_lucid.samples'), 'eval_lucid_layers.others=3',
          {'others': 0, 'front': 0.5},
          'The sequence\'s other objects as moving layers of the lucid synthesis: up to `others` of the objects annotated on the '
          'target\'s train frame are cut out with it and moved on their own, each in front of it with probability `front`.  '
          'others 0 = off.'),
)
ROWS = {row.keyword: row for row in TABLE}
DEFAULTS = {row.key: row.defaults for row in TABLE}


def from_cfg(cfg):
    """The groups a config carries, as keywords of `evaluate.evaluate_dataset`."""
    return {row.keyword: cfg[row.key] for row in TABLE if cfg.get(row.key) is not None}


def check_cfg(cfg):
    """Validates every group `cfg` carries, in table order: ValueError for a bad value, and for an active group whose consumer is off."""
    for row in TABLE:
        if row.key in cfg:
            module = _mod(row.module)
            module.check(cfg[row.key])
            if row.needs and module.active(cfg[row.key]) and not row.needs[0](cfg):
                raise ValueError(f'{row.key} has no consumer: {row.needs[1]}')


def split(function, groups, merge=True):
    """(object share, merge share) of the group keywords a public function of `evaluate.py` received, unset ones dropped.  A name
    that is no group -- or a merge-stage group for a function that does not merge -- is the caller's TypeError."""
    for name in groups:
        if name not in ROWS or not (merge or ROWS[name].stage == OBJECT):
            raise TypeError(f"{function}() got an unexpected keyword argument '{name}'")
    return tuple({k: v for k, v in groups.items() if v is not None and ROWS[k].stage == stage} for stage in (OBJECT, MERGE))


def travelling(share, cfg=None, dataset=None, lucid_others=None):
    """The keywords that `share` puts into its consumer's call: every group under its travel rule (`active` validates, and may
    raise), with what it brings.  `cfg` and `dataset` (its `mean_val`, else DAVIS's) are for `frame_offset`."""
    out = {}
    for row in TABLE:
        value = share.get(row.keyword)
        if value is None or (row.travels == ACTIVE and not _mod(row.module).active(value)):
            continue
        out[row.keyword] = value
        if row.brings == 'lucid_others':
            out['lucid_others'] = lucid_others
        elif row.brings == 'frame_offset' and cfg.get('data_cfg', {}).get('normalize'):
            out['frame_offset'] = tuple(getattr(dataset, 'mean_val', _mod('data').DAVIS.mean_val))
    return out
