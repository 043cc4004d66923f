"""Sacred-compatible configuration surface of `src/train_meta.py` for the DeepLab hot path.

The reference wires `cfgs/meta.yaml` + `cfgs/torch.yaml` as base config and four named configs
(`train_meta.py:21-27`) and is driven as
    python src/train_meta.py with DAVIS-2017 e-OSVOS-OnA key=val ...
Sacred is not installed in the target image, so this module keeps the same *keys* (same names and
nesting as cfgs/meta.yaml), the same named configs and the
same `with <named...> <dotted.key=value...>` command-line grammar; an external YAML file in the
reference's format can be merged with `load_yaml`.  Values below are the reference defaults,
except that the hot-path model/loss are selected (`parent_model.architecture=DeepLabV3Plus`,
`loss_func=cross_entropy`, frozen BatchNorm) -- the reference's shipped defaults select
Mask R-CNN (`cfgs/meta.yaml:68-84`), which is out of scope.
"""
import copy

import yaml

BASE = {
    'seed': 1,
    'meta_batch_size': 4,
    'num_meta_processes_per_gpu': 1,
    'num_eval_gpus': None,
    'no_vis': True,
    'vis_interval': 10,
    'env_suffix': None,
    'save_dir': 'models',
    'resume_meta_run_epoch_mode': None,
    'increase_seed_per_meta_run': True,
    'random_frame_transform_per_task': True,
    'multi_step_bptt_loss': False,
    'random_frame_epsilon': None,
    'random_object_id_sub_group': False,
    'num_epochs': {'train': 5, 'eval': 10},
    'bptt_epochs': 5,
    'eval_online_adapt': {'step': 0, 'reset_model_mode': 'FIRST_STEP', 'num_epochs': 10, 'min_prop': 0.5},
    'meta_optim_model_file': None,
    'meta_optim_cfg': {'lr_hierarchy_level': 'NEURON', 'init_lr': 0.001, 'learn_model_init': True,
                       'second_order_gradients': False, 'use_log_init_lr': False, 'max_lr': None},
    'meta_optim_optim_cfg': {'model_init_lr': 0.00001, 'log_init_lr_lr': 0.00001, 'lr': 0.001,
                             'freeze_encoder': False, 'grad_clip': None, 'model_init_weight_decay': 0.001},
    'eval_datasets': True,
    'datasets': {'train': {'name': 'DAVIS-2016', 'split': 'train_seqs', 'eval': True},
                 'val': {'name': 'DAVIS-2016', 'split': 'val_seqs', 'eval': True},
                 'test': {'name': 'DAVIS-2016', 'split': None, 'eval': False}},
    'loss_func': 'cross_entropy',
    'parent_model': {'architecture': 'DeepLabV3Plus', 'train_encoder': True,
                     'batch_norm': {'accum_stats': False, 'learn_weight': False, 'learn_bias': False},
                     'replace_batch_with_group_norms': False, 'decoder_norm_layer': 'BatchNorm2d',
                     'eval_augment_rpn_proposals_mode': None, 'roi_pool_output_sizes': {'box': 7, 'mask': 28},
                     'maskrcnn_loss': None, 'box_nms_thresh': None, 'encoder': 'resnet50',
                     # per-dataset parent checkpoints (`init_parent_model(**datasets)`, helper_func.py:339-385)
                     'train': {'paths': [], 'val_split_files': ['data/DAVIS-2017/train_val_seqs.txt']},
                     'val': {'paths': [], 'val_split_files': ['data/DAVIS-2017/train_val_seqs.txt']},
                     'test': {'paths': [], 'val_split_files': ['data/DAVIS-2017/test-dev_seqs.txt']}},
    'train_early_stopping_cfg': {'patience': None, 'min_loss_improv': 0.001},
    'single_obj_seq_mode': 'KEEP',
    'random_flip_label': False,
    'random_no_label': False,
    'random_box_coord_perm': False,
    'data_cfg': {'multi_object': False, 'random_train_transform': False, 'num_workers': 0, 'pin_memory': False,
                 'normalize': False, 'full_resolution': False,
                 'frame_ids': {'train': 0, 'test': None, 'meta': None},
                 'batch_sizes': {'train': 1, 'test': 1, 'meta': 1},
                 'shuffles': {'train': True, 'test': False, 'meta': False},
                 'crop_sizes': {'train': None, 'test': None, 'meta': None}},
    'torch_cfg': {'print_config': False, 'device': None, 'deterministic': True, 'benchmark': False,
                  'vis': {'port': 8090, 'server': 'http://localhost'}},
}

# named configs of train_meta.py:24-27 (hot-path keys of cfgs/meta_davis-2017.yaml,
# meta_youtube-vos.yaml, eval_e-osvos.yaml, eval_e-osvos-OnA.yaml)
NAMED = {
    'DAVIS-2017': {'datasets': {'train': {'name': 'DAVIS-2017', 'split': 'train_seqs', 'eval': True},
                                'val': {'name': 'DAVIS-2017', 'split': 'val_seqs', 'eval': True},
                                'test': {'name': 'DAVIS-2017', 'split': 'test-dev_seqs', 'eval': False}},
                   'data_cfg': {'multi_object': 'single_id'}},
    'YouTube-VOS': {'datasets': {'train': {'name': ['YouTube-VOS', 'DAVIS-2017'],
                                           'split': ['train_dev_random_123_train_seqs', 'train_seqs'], 'eval': False},
                                 'val': {'name': 'YouTube-VOS', 'split': 'valid-all-frames_seqs', 'eval': False},
                                 'test': {'name': 'YouTube-VOS', 'split': None, 'eval': False},
                                 'train_dev_train_val': {'name': 'YouTube-VOS', 'split': 'train_dev_random_123_train_val_seqs',
                                                         'eval': False},
                                 'train_dev_val': {'name': 'YouTube-VOS', 'split': 'train_dev_random_123_val_seqs', 'eval': False},
                                 'val_davis16': {'name': 'DAVIS-2016', 'split': 'val_seqs', 'eval': False},
                                 'val_davis17': {'name': 'DAVIS-2017', 'split': 'val_seqs', 'eval': True}},
                    'parent_model': {'train': {'paths': [], 'val_split_files': []}, 'val': {'paths': [], 'val_split_files': []},
                                     'test': {'paths': [], 'val_split_files': []}},
                    'data_cfg': {'multi_object': 'single_id'}},
    # the iteration counts come from the command line as in the reference README
    # (`with DAVIS-2017 e-OSVOS num_epochs.eval=50`, `... e-OSVOS-OnA num_epochs.eval=100`)
    'e-OSVOS': {'no_vis': True, 'num_meta_processes_per_gpu': 0,
                'data_cfg': {'batch_sizes': {'train': 3}, 'random_train_transform': True}},
    'e-OSVOS-OnA': {'no_vis': True, 'num_meta_processes_per_gpu': 0,
                    'eval_online_adapt': {'step': 5, 'num_epochs': 10},
                    'data_cfg': {'batch_sizes': {'train': 3}, 'random_train_transform': True}},
}


# Options beyond the reference's cfgs/meta.yaml.  They are NOT part of BASE (the reference's key set): `parse_cli` adds a group
# only when the command line sets one of its keys (`eval_tta.flip=True eval_tta.scales=[0.75,1.0,1.25]`), consumers read them
# with `cfg.get(...)`.
#   eval_tta   test-time augmentation of the evaluation's inference passes (`tta.py`): mirrored and rescaled views averaged in
#              probability space with equal weights; the value below is the neutral one (one plain view = off)
EXTENSIONS = {
    'eval_tta': {'flip': False, 'scales': [1.0]},
}


# Post-processing of the evaluation's label maps, handled like EXTENSIONS (not part of BASE, added by `parse_cli` only when the
# command line sets one of its keys: `eval_crf.iterations=5 eval_crf.w_appearance=10`, read with `cfg.get(...)`).
#   eval_crf   local dense-CRF refinement of the final merge (`crf.py`); the value below is the neutral one (0 iterations = the plain
#              merge), the other keys hold `crf.DEFAULTS` -- customary values, not tuned on data
POSTPROCESS = {
    'eval_crf': {'iterations': 0, 'radius': 5, 'dilation': 2, 'w_appearance': 10.0, 'w_smooth': 3.0,
                 'theta_alpha': 8.0, 'theta_beta': 0.05, 'theta_gamma': 3.0},
}


# Region-level clean-up of the evaluation's label maps, handled like EXTENSIONS and POSTPROCESS (not part of BASE, added by
# `parse_cli` only when the command line sets one of its keys: `eval_components.gate=24 eval_components.min_rel_area=0.05
# eval_components.largest_only=True` -- example values, untuned; read with `cfg.get(...)`).
#   eval_components   connected-component filter after the merge and the CRF (`components.py`); the value below is the neutral
#                     one (`components.DEFAULTS`: nothing is filtered, nothing new is called)
CLEANUP = {
    'eval_components': {'connectivity': 8, 'min_area': 0, 'min_rel_area': 0.0, 'largest_only': False, 'gate': 0},
}


# Hole filling of the evaluation's label maps, handled like EXTENSIONS, POSTPROCESS and CLEANUP (not part of BASE, added by
# `parse_cli` only when the command line sets one of its keys: `eval_holes.max_area=64 eval_holes.prev_overlap=0.5` -- example
# values, untuned; read with `cfg.get(...)`).
#   eval_holes        enclosed background islands are filled after the component filter (`holes.py`); the value below is the
#                     neutral one (`holes.DEFAULTS`: max_area 0, nothing is filled, nothing new is called)
FILL = {
    'eval_holes': {'connectivity': 8, 'max_area': 0, 'max_rel_area': 1.0, 'prev_overlap': 0.0},
}


# Superpixel snapping of the evaluation's label maps, handled like EXTENSIONS, POSTPROCESS, CLEANUP and FILL (not part of BASE,
# added by `parse_cli` only when the command line sets one of its keys: `eval_snap.step=16 eval_snap.min_share=0.6` -- example
# values, untuned; read with `cfg.get(...)`).
#   eval_snap         between the CRF and the component filter, every SLIC superpixel of the frame takes its majority label
#                     (`snap.py`); the value below is the neutral one (`snap.DEFAULTS`: step 0, nothing new is called)
SNAP = {
    'eval_snap': {'step': 0, 'iterations': 5, 'compactness': 10, 'min_share': 0.5},
}


# Motion compensation of the clean-up's temporal rules, handled like the groups above (`eval_motion.block=8
# eval_motion.radius=24` -- example values, untuned; read with `cfg.get(...)`).
#   eval_motion       the gate of the component filter and `prev_overlap` of the hole filler see the previous frame's cleaned
#                     map warped by block motion (`motion.py`); the value below is the neutral one (`motion.DEFAULTS`: block
#                     0, nothing new is called).  Active, it needs `eval_components.gate` or `eval_holes.prev_overlap`.
MOTION = {
    'eval_motion': {'block': 0, 'radius': 16, 'bias': 2},
}


# Object-centred zoom pass of the evaluation's inference calls, handled like the groups above (not part of BASE, added by
# `parse_cli` only when the command line sets one of its keys: `eval_zoom.max_zoom=3 eval_zoom.margin=0.5` -- example values,
# untuned; read with `cfg.get(...)`).
#   eval_zoom         every frame gets a second look at a crop around the object its first pass found, magnified to the frame's
#                     own size on the live engine and blended in inside the crop (`zoom.py`); the value below is the neutral
#                     one (`zoom.DEFAULTS`: max_zoom 0, nothing new is called)
ZOOM = {
    'eval_zoom': {'max_zoom': 0, 'min_zoom': 1.5, 'threshold': 0.5, 'min_pixels': 16, 'margin': 0.5, 'margin_px': 8, 'weight': 0.5,
                  'feather': 8},
}


# Lucid first-frame synthesis for the evaluation's one-shot fine-tune, handled like the groups above (not part of BASE, added
# by `parse_cli` only when the command line sets one of its keys: `eval_lucid.samples=2 eval_lucid.shift=0.1` -- example values,
# untuned; read with `cfg.get(...)`).
#   eval_lucid        some samples of every round-0 batch are composed from the annotated frame with the object and its
#                     background moved independently (`lucid.py`); the value below is the neutral one (`lucid.DEFAULTS`:
#                     samples 0, nothing new is called, nothing is drawn)
LUCID = {
    'eval_lucid': {'samples': 0, 'dilate': 4, 'rot': 15.0, 'scale': 0.15, 'shift': 0.1, 'bg_rot': 5.0, 'bg_scale': 0.05,
                   'bg_shift': 0.05, 'min_keep': 0.5},
}


# Distance-gated negatives for online adaptation, handled like the groups above (not part of BASE, whose `eval_online_adapt`
# keeps the reference's four keys; added by `parse_cli` only when the command line sets one of its keys: `eval_adapt.neg_dist=220
# eval_adapt.erode=15` -- OnAVOS's published 480p values, an example, untuned; read with `cfg.get(...)`).
#   eval_adapt        the propagated targets of the adaptation rounds are 0 wherever a pixel is farther than `neg_dist` from the
#                     mask of the frame before it, eroded by `erode` (`adapt.py`); the value below is the neutral one
#                     (`adapt.DEFAULTS`: neg_dist 0, nothing new is called).  Active, it needs `eval_online_adapt.step` > 0.
ADAPT = {
    'eval_adapt': {'neg_dist': 0, 'erode': 0},
}


# The sequence's other objects as moving layers of the lucid synthesis, handled like the groups above (not part of BASE, added by
# `parse_cli` only when the command line sets one of its keys: `eval_lucid_layers.others=3` -- an example value, untuned; read
# with `cfg.get(...)`).  `eval_lucid` keeps its own nine keys.
#   eval_lucid_layers up to `others` of the other objects annotated on the target's train frame are cut out with it and moved on
#                     their own over the filled plate, each in front of the target with probability `front`
#                     (`lucid_layers.py`); the value below is the neutral one (`lucid_layers.DEFAULTS`: others 0, nothing new
#                     is called, nothing is drawn).  Active, it needs `eval_lucid.samples` > 0.
LAYERS = {
    'eval_lucid_layers': {'others': 0, 'front': 0.5},
}


def _merge(dst, src):
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _merge(dst[k], v)
        else:
            dst[k] = copy.deepcopy(v)
    return dst


def _set_dotted(cfg, key, value):
    parts = key.split('.')
    d = cfg
    for p in parts[:-1]:
        if p not in d or not isinstance(d[p], dict):
            raise KeyError(f'unknown config key: {key}')
        d = d[p]
    if parts[-1] not in d:
        raise KeyError(f'unknown config key: {key}')       # Sacred also rejects unknown keys
    d[parts[-1]] = value


def load_yaml(path, cfg=None):
    cfg = cfg if cfg is not None else copy.deepcopy(BASE)
    with open(path) as f:
        return _merge(cfg, yaml.safe_load(f) or {})


def parse_cli(argv):
    """`[with] <named config | key=value> ...` -> config dict (Sacred's CLI grammar, README.md:56-83)."""
    cfg = copy.deepcopy(BASE)
    args = list(argv)
    if args and args[0] == 'with':
        args = args[1:]
    updates = []
    for a in args:
        if '=' in a:
            k, v = a.split('=', 1)
            updates.append((k, yaml.safe_load(v)))
        elif a in NAMED:
            _merge(cfg, NAMED[a])
        elif a.endswith('.yaml'):
            load_yaml(a, cfg)
        else:
            raise KeyError(f'unknown named config: {a}')
    for k, v in updates:
        group = k.split('.')[0]
        for groups in (EXTENSIONS, POSTPROCESS, CLEANUP, FILL, SNAP, MOTION, ZOOM, LUCID, ADAPT, LAYERS):
            if group in groups and group not in cfg:
                cfg[group] = copy.deepcopy(groups[group])
        _set_dotted(cfg, k, v)
    if 'eval_tta' in cfg:
        from .tta import check
        check(cfg['eval_tta'])                              # ValueError: empty list, scale <= 0, ...
    if 'eval_crf' in cfg:
        from .crf import check as check_crf
        check_crf(cfg['eval_crf'])                          # ValueError: radius 0, a negative weight, ...
    if 'eval_components' in cfg:
        from .components import check as check_components
        check_components(cfg['eval_components'])            # ValueError: gate 64, connectivity 6, ...
    if 'eval_holes' in cfg:
        from .holes import check as check_holes
        check_holes(cfg['eval_holes'])                      # ValueError: max_area -1, prev_overlap 1.5, ...
    if 'eval_snap' in cfg:
        from .snap import check as check_snap
        check_snap(cfg['eval_snap'])                        # ValueError: step 3, compactness 65, ...
    if 'eval_motion' in cfg:
        from . import motion
        if motion.active(cfg['eval_motion']):               # ValueError: block 12, radius 33, bias 256, ...
            from .components import check as check_gate
            from .holes import active as fills, check as check_overlap, overlap_q16
            fill = cfg.get('eval_holes', {})
            if not check_gate(cfg.get('eval_components', {}))['gate'] and \
                    not (fills(fill) and overlap_q16(check_overlap(fill)['prev_overlap'])):
                raise ValueError('eval_motion has no consumer: set eval_components.gate or eval_holes.prev_overlap')
        else:
            motion.check(cfg['eval_motion'])
    if 'eval_zoom' in cfg:
        from .zoom import check as check_zoom
        check_zoom(cfg['eval_zoom'])                        # ValueError: max_zoom 5, min_zoom above max_zoom, weight 0, ...
    if 'eval_lucid' in cfg:
        from .lucid import check as check_lucid
        check_lucid(cfg['eval_lucid'])                      # ValueError: samples -1, dilate 17, min_keep 0, ...
    if 'eval_adapt' in cfg:
        from .adapt import active as adapts
        if adapts(cfg['eval_adapt']) and not cfg['eval_online_adapt']['step']:      # ValueError: neg_dist 4096, erode -1, a float, ...
            raise ValueError('eval_adapt has no consumer: set eval_online_adapt.step')
    if 'eval_lucid_layers' in cfg:
        from .lucid import active as lucid_on
        from .lucid_layers import active as layered
        if layered(cfg['eval_lucid_layers']) and not lucid_on(cfg.get('eval_lucid')):   # ValueError: others 8, front 1.5, a float, ...
            raise ValueError('eval_lucid_layers has no consumer: set eval_lucid.samples')
    unsupported(cfg)
    return cfg


def unsupported(cfg):
    """Options of cfgs/meta.yaml this build accepts as keys but does not implement must not be ignored silently."""
    crops = (cfg.get('data_cfg') or {}).get('crop_sizes') or {}
    if any(v is not None for v in crops.values()):
        raise NotImplementedError('data_cfg.crop_sizes (pad + random crop of every frame, data/vos_dataset.py:246-275) is not implemented: '
                                  'frames are fed at their native size')
