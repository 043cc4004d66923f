"""Evaluation worker logic of `src/util/evaluate.py` for the DeepLab path, on tensors.

`evaluate_sequence` restates the intended semantics of `evaluate.py:132-326` (the reference's
own loop cannot run the DeepLab model at this commit):
  per object: fine-tune on the first frame for `num_epochs.eval` iterations (`:207-281`), predict
  the following frames (`:293-314`); with online adaptation every `step` frames re-fine-tune for
  `eval_online_adapt.num_epochs` iterations on [first frame + earlier frames with their own
  thresholded predictions as ground truth] (`:170-193,227-253`), restoring the round-0 weights
  first when `reset_model_mode == 'FIRST_STEP'` (`:200-205,283-287`);
  finally merge objects: background where max prob < 0.5, else argmax + 1 (`:322-326`), the
  train frame being seeded with 2*GT (`:167-168`).
Data loading is the caller's business; the first-frame augmentation of round 0
(`random_train_transform`, `evaluate.py:215-218`, `helper_func.py:255-261`) runs on the device
(`custom_transforms.FirstFrameAugmenter`) when `data_cfg.random_train_transform` is set, or through a
caller-supplied `augment(frame, gt, batch, seed)`; benchmarks use synthetic frames.
"""
import os
import time

import numpy as np
import torch

from . import components as component_filter
from . import eval_options
from . import crf as crf_refine
from . import adapt as adapt_gate
from . import holes as hole_filler
from . import motion as mover
from . import snap as snapper
from . import tta as tta_views
from . import lucid as lucid_pass
from . import lucid_layers as layer_pass
from . import zoom as zoom_pass
from .helper_func import compute_loss, early_stopping, set_random_seeds


# frames predicted per inference launch (`evaluate_dataset` sizes its engines for it; engines sized elsewhere use what
# they have)
INFER_BATCH = int(os.environ.get('EOSVOS_INFER_BATCH', 8))


def online_adapt_schedule(num_frames, train_frame_id, step, train_batch_size):
    """Frame ranges and propagated frames per round (`evaluate.py:140-193,231-240`)."""
    rounds = []
    s = step if step else num_frames
    n_rounds = len(range(train_frame_id + 1, num_frames, step)) if step else 1
    eval_max = None
    for r in range(max(n_rounds, 1)):
        if r == 0:
            eval_min = train_frame_id + 1
            eval_max = eval_min
            prop = []
        else:
            eval_min = eval_max
            n_prop = min(step, train_batch_size)
            prop = [eval_min - j for j in range(step - n_prop + 1, step)]
        eval_max = min(eval_max + s, num_frames)
        rounds.append(dict(eval_min=eval_min, eval_max=eval_max, propagate_frames=prop))
        if eval_max == num_frames:
            break
    return rounds


def device_augment(model):
    """Round-0 batches = `batch` independent flip / scale / rotate warps of the first frame, drawn with the
    `random` state that `set_random_seeds(seed + epoch + round)` just set (evaluate.py:221-224)."""
    from .custom_transforms import FirstFrameAugmenter

    def fn(frame, gt, batch, seed):
        eng = model._ensure_engine(frame.shape[2], frame.shape[3], batch)
        images, labels, _ = FirstFrameAugmenter(eng).batch(frame[0].contiguous(), gt[0].contiguous(), batch)
        return images, labels
    return fn


def _repeat_batch(frame, gt, batch, seed):
    return frame.expand(batch, -1, -1, -1).contiguous(), gt.expand(batch, -1, -1, -1).contiguous()


PROPAGATION_IGNORE = 255.0       # the void label of the uncertainty band's targets (PASCAL's void class)


def min_prop_band(min_prop):
    """`eval_online_adapt.min_prop`: a scalar threshold (the reference, evaluate.py:231-240) -> None; a two-element list
    [lo, hi] with 0 <= lo < hi <= 1 -> (lo, hi): propagated targets are 1 where p >= hi, 0 where p < lo and void between."""
    if not isinstance(min_prop, (list, tuple)):
        return None
    ok = len(min_prop) == 2 and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in min_prop)
    if not ok or not 0.0 <= float(min_prop[0]) < float(min_prop[1]) <= 1.0:
        raise ValueError(f'eval_online_adapt.min_prop={min_prop!r}: a number, or [lo, hi] with 0 <= lo < hi <= 1')
    return float(min_prop[0]), float(min_prop[1])


def finetune_object(model, meta_optim, meta_optim_state_dict, frames, gt, cfg, augment=None, train_frame_id=0, lucid_others=None,
                    **groups):
    """One (sequence, object) work item of `evaluate.py:132-317`: fine-tune on the train frame, predict the following
    frames, with online adaptation re-fine-tune every `step` frames.  Returns (probs (N,H,W) with the train frame seeded
    as 2*GT (`:167-168`), train-loss history per round).  `groups`: the object-stage option groups of `eval_options.TABLE`, by
    keyword; `lucid_others` (M, 1, H, W), the other objects' masks at this object's train frame, goes with `layers`."""
    share, _ = eval_options.split('finetune_object', groups, merge=False)
    return _drain(finetune_object_steps(model, meta_optim, meta_optim_state_dict, frames, gt, cfg, augment, train_frame_id,
                                        **eval_options.travelling(share, lucid_others=lucid_others)))


def others_at_train_frame(gts, train_frame_ids, o):
    """The masks (M, 1, H, W) of the objects that share object o's train frame, in object order; None when there is none."""
    sel = [gts[j].float().reshape(1, *gts[j].shape[-2:]) for j in range(len(gts)) if j != o and train_frame_ids[j] == train_frame_ids[o]]
    return torch.stack(sel) if sel else None


def _others_for(layers, gts, train_frame_ids, o):
    """`others_at_train_frame` when `layers` is active, else None: an inactive `layers` computes nothing."""
    return others_at_train_frame(gts, train_frame_ids, o) if layer_pass.active(layers) else None


def _object_share(share, gts, train_frame_ids, o):
    """The object-stage share as it travels to object o's fine-tune: `layers` with the masks of the objects on o's train frame."""
    return eval_options.travelling(share, lucid_others=_others_for(share.get('layers'), gts, train_frame_ids, o))


def lucid_batches(model, augment, frame, gt, batch, lucid, layers=None, lucid_others=None):
    """The round-0 batch source of rule 12 of `lucid.py`: `fn(seed) -> (inputs, gts)` whose first batch - k samples come from
    `augment` (today's path, called for batch - k samples and not at all for 0) and whose last k = min(samples, batch) are
    synthesised.  The plate is built at the first batch, once.  A mask that is empty or fills the frame: every batch is today's.
    With `layers` active and an other object in `lucid_others` (rule L9 of `lucid_layers.py`) the samples are the layered
    ones; otherwise they are today's."""
    k = min(lucid_pass.check(lucid)['samples'], batch)
    held = []                                                       # the augmenter, built at the first batch
    layered = layer_pass.active(layers) and lucid_others is not None and len(lucid_others) > 0

    def build(eng):
        if layered:
            aug = layer_pass.LayeredAugmenter(eng, frame[0].contiguous(), gt[0].contiguous(),
                                              lucid_others.to(frame.device).float().contiguous(), lucid, layers)
            if aug.has_layers:
                return aug
        return lucid_pass.LucidAugmenter(eng, frame[0].contiguous(), gt[0].contiguous(), lucid)

    def fn(seed):
        eng = model._ensure_engine(frame.shape[2], frame.shape[3], batch)
        if not held:
            held.append(build(eng))
        aug = held[0]
        aug.engine = eng                                            # the model's live engine (its stream, its scratch)
        if not aug.has_object:
            return augment(frame, gt, batch, seed)
        plain = augment(frame, gt, batch - k, seed) if batch - k else None
        images, labels, _ = aug.batch(k)
        if plain is None:
            return images, labels
        return torch.cat([plain[0], images]), torch.cat([plain[1], labels])
    return fn


def _drain(gen):
    try:
        while True:
            next(gen)
    except StopIteration as stop:
        return stop.value


def finetune_object_steps(model, meta_optim, meta_optim_state_dict, frames, gt, cfg, augment=None, train_frame_id=0,
                          lucid_others=None, **groups):
    """`finetune_object` as a generator: it yields each time a fine-tune iteration (or a few inference frames) has been
    ENQUEUED on the model's engine and before the host waits for its loss, so that a caller holding several objects
    (one model / engine / stream each, `run_objects_in_flight`) can queue the others' work in between.  Everything
    random (`set_random_seeds` + the augmentation draws of an iteration) happens inside one resume, so the draws of an
    object do not depend on what runs beside it.  The generator's return value is `finetune_object`'s.
    The consumer of the object-stage groups of `eval_options.TABLE`; a name that is none of them raises here, at the call."""
    share, _ = eval_options.split('finetune_object_steps', groups, merge=False)
    return _object_steps(model, meta_optim, meta_optim_state_dict, frames, gt, cfg, augment, train_frame_id, lucid_others, **share)


def _object_steps(model, meta_optim, meta_optim_state_dict, frames, gt, cfg, augment, train_frame_id, lucid_others, tta=None,
                  zoom=None, lucid=None, adapt=None, layers=None):
    if augment is None and cfg['data_cfg'].get('random_train_transform'):
        augment = device_augment(model)
    augment = augment or _repeat_batch
    # test-time augmentation: the frames' probabilities (the propagated targets of the adaptation rounds included: they are the
    # frames' prediction) are the mean over the views; off = the plain inference call below
    view_set = tta_views.ViewSet(model, frames.shape[2], frames.shape[3], tta) if tta_views.active(tta) else None
    # the zoom pass follows the first pass of each inference batch (the propagated targets see the refined probabilities, as they
    # see the mean over the views); off = nothing new is called
    refiner = zoom_pass.Refiner(model, frames.shape[2], frames.shape[3], zoom, tta if view_set is not None else None) \
        if zoom_pass.active(zoom) else None
    n = frames.shape[0]
    ona = cfg['eval_online_adapt']
    band = min_prop_band(ona['min_prop'])
    # the distance gate of the adaptation rounds (`adapt.py`): a scalar min_prop t becomes the band (0, t); off = nothing new is
    # called, the two branches below as they were
    gate = adapt_gate.band_of(ona['min_prop'], band) if adapt_gate.active(adapt) else None
    step = ona['step']
    bsz = cfg['data_cfg']['batch_sizes']['train']
    es = cfg.get('train_early_stopping_cfg', {'patience': None, 'min_loss_improv': 0.001})
    loss_func = cfg.get('loss_func', 'cross_entropy')
    gt = gt.to(frames.device).float().view(1, 1, *gt.shape[-2:])
    masks = torch.zeros(n, 1, *frames.shape[-2:], device=frames.device)
    masks[train_frame_id] = 2 * gt[0]                               # evaluate.py:167-168
    # lucid synthesis: the last samples of every round-0 batch are composed from the train frame (the plate is built once per
    # object, at the first batch); off = nothing new is called, nothing is drawn
    if layers is not None:
        layer_pass.check(layers)
    lucid_batch = lucid_batches(model, augment, frames[train_frame_id:train_frame_id + 1], gt, bsz, lucid, layers, lucid_others) \
        if lucid_pass.active(lucid) else None
    hist = []
    for r, rd in enumerate(online_adapt_schedule(n, train_frame_id, step, bsz)):
        if r == 0 or ona['reset_model_mode'] == 'FULL':
            meta_optim.load_state_dict(meta_optim_state_dict)
            meta_optim.reset()
            meta_optim.eval()
        elif ona['reset_model_mode'] == 'FIRST_STEP':
            meta_optim.load_state_dict(meta_optim_state_dict)
            if model._dirty:                    # new lrs: push them without touching theta twice
                model.push_state()
            model.engine.restore()              # model.load_state_dict(model_state_dict_first_step)
            meta_optim.eval()
        num_epochs = cfg['num_epochs']['eval'] if r == 0 else ona['num_epochs']
        model.train_without_dropout()
        round_hist = []
        loss_kwargs = None
        if r > 0:
            # the adaptation batch of this round: train frame + the propagated frames whose thresholded prediction is
            # not empty (evaluate.py:231-240).  The reference rebuilds it every epoch from the same masks; once is enough.
            round_inputs, round_gts = frames[train_frame_id:train_frame_id + 1], gt
            if gate is not None:
                # distance gate: one call builds every propagated frame's targets -- the band's, and 0 wherever the pixel is far
                # from the (eroded) mask of the frame before it -- and counts its positives; one host read for the round
                if rd['propagate_frames']:
                    fs = list(rd['propagate_frames'])
                    pg, n_pos = adapt_gate.targets(model.engine, masks[fs], masks[[f - 1 for f in fs]], gate[0], gate[1], adapt,
                                                   PROPAGATION_IGNORE)
                    keep = [i for i, c in enumerate(n_pos) if c != 0]
                    if keep:
                        loss_kwargs = {'ignore': PROPAGATION_IGNORE}
                        round_inputs = torch.cat([round_inputs, frames[[fs[i] for i in keep]]])
                        round_gts = torch.cat([round_gts, pg[keep]])
            elif band is None:
                for f in rd['propagate_frames']:
                    pg = masks[f:f + 1].ge(ona['min_prop']).float()
                    if pg.sum().item() != 0:                            # evaluate.py:239
                        round_inputs = torch.cat([round_inputs, frames[f:f + 1]])
                        round_gts = torch.cat([round_gts, pg])
            elif rd['propagate_frames']:
                # uncertainty band: one launch builds every propagated frame's targets (void between lo and hi) and counts
                # its positives, one host read for the round; the train frame's ground truth is never void
                fs = list(rd['propagate_frames'])
                pg, n_pos = model.engine.propagation_targets(masks[fs], band[0], band[1], PROPAGATION_IGNORE)
                keep = [i for i, c in enumerate(n_pos) if c != 0]
                if keep:                                                # no surviving frame: no void pixel, the plain loss
                    loss_kwargs = {'ignore': PROPAGATION_IGNORE}
                    round_inputs = torch.cat([round_inputs, frames[[fs[i] for i in keep]]])
                    round_gts = torch.cat([round_gts, pg[keep]])
            round_inputs, round_gts = round_inputs.contiguous(), round_gts.contiguous()
        for epoch in range(1, num_epochs + 1):
            set_random_seeds(cfg.get('seed', 1) + epoch + r)
            if r == 0 and lucid_batch is not None:
                inputs, gts = lucid_batch(cfg.get('seed', 1) + epoch)
            elif r == 0:
                inputs, gts = augment(frames[train_frame_id:train_frame_id + 1], gt, bsz, cfg.get('seed', 1) + epoch)
            else:
                inputs, gts = round_inputs, round_gts
            outputs = model(inputs)
            train_loss = compute_loss(loss_func, outputs[-1], gts, loss_kwargs)     # a device scalar: no host wait yet
            model.zero_grad()
            meta_optim.set_train_loss(train_loss)
            meta_optim.step(train_loss)
            meta_optim.meta_model.detach_param_groups()
            yield
            round_hist.append(train_loss.item())                       # the loss before the step (evaluate.py:262-264)
            if early_stopping(round_hist, **es):
                break
        hist.append(round_hist)
        if r == 0:
            model.engine.snapshot()             # model_state_dict_first_step (evaluate.py:283-287)
        model.eval()
        # the reference predicts frame by frame (`test` batch size 1, evaluate.py:293-314); frozen normalisation makes
        # the frames of a batch independent, and at 480x854 a batch of 3 costs 1.40 ms per frame, one of 8 1.16, one 2.30
        nb = max(1, min(int(getattr(model.engine, 'max_batch', 1)), INFER_BATCH))
        if view_set is not None and rd['eval_min'] < rd['eval_max']:
            view_set.sync()                     # the view engines of other sizes take this round's weights
        for f in range(rd['eval_min'], rd['eval_max'], nb):
            g = min(f + nb, rd['eval_max'])
            if refiner is not None:
                x = frames[f:g].contiguous()
                masks[f:g] = refiner.refine(x, view_set.infer(x) if view_set is not None else model.engine.infer(x))
            elif view_set is not None:
                masks[f:g] = view_set.infer(frames[f:g].contiguous())
            else:
                masks[f:g] = model.engine.infer(frames[f:g].contiguous())
            yield
    return masks[:, 0], hist


class ObjectWorker:
    """A (model, meta_optim) pair bound to one torch stream: one fine-tune in flight."""

    def __init__(self, model, meta_optim, stream=None):
        self.model, self.meta_optim, self.stream = model, meta_optim, stream

    def on_stream(self):
        return torch.cuda.stream(self.stream) if self.stream is not None else _NullCtx()


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def object_workers(model, meta_optim, meta_optim_cfg, n, wg_budget=256):
    """`n` workers for `run_objects_in_flight`, each a spawned copy of `model` (same construction and learned state) with
    its own engine on its own NEW stream and no side stream: one hardware queue per engine.  The caller's model is not one
    of them -- its engine lives on the caller's (default) stream, and which hardware queue the next new stream shares with
    it is not under our control (`engine.warm_stream_pool`); consecutive new streams do sit on different queues.
    The objects of a multi-object sequence are independent fine-tunes (`evaluate.py:132`); three of them in flight fill
    the tails and small grids one leaves idle (+19 % iterations/s at batch 3, 480x854, `bench.py` extra).  Engines that
    share the GPU plan for `wg_budget` workgroups per launch."""
    from .meta_optim import MetaOptimizer
    ws = []
    on_gpu = model.device.type == 'cuda'
    for _ in range(n):
        m = model.spawn()
        m.side_stream = os.environ.get('EOSVOS_INFLIGHT_SIDE_STREAM', '0') == '1'      # default: one queue per engine
        ws.append(ObjectWorker(m, MetaOptimizer(m, **meta_optim_cfg), torch.cuda.Stream(model.device) if on_gpu else None))
    for w in ws:
        w.wg_budget = wg_budget
    return ws


def run_objects_in_flight(workers, meta_optim_state_dict, frames, gts, cfg, augment=None, train_frame_id=0, lucid_others=None,
                          **groups):
    """[(probs, hist)] for the objects `gts` of one sequence, up to len(workers) of them in flight together; results are
    those of `finetune_object` one after the other (same engine arithmetic at the same workgroup budget).
    `train_frame_id`: one frame for all objects, or one per object (YouTube-VOS objects that appear later).
    `groups`: the object-stage option groups of `eval_options.TABLE`, by keyword.  With `layers`, every object's lucid samples move
    the objects of `gts` that share its train frame too; `lucid_others`, one entry per object, replaces them (a caller that holds
    only some of the sequence's objects)."""
    share, _ = eval_options.split('run_objects_in_flight', groups, merge=False)
    out = [None] * len(gts)
    tfid = list(train_frame_id) if isinstance(train_frame_id, (list, tuple)) else [train_frame_id] * len(gts)
    if frames.is_cuda:
        torch.cuda.current_stream(frames.device).synchronize()      # frames / masks were produced on this stream
    pending = list(range(len(gts)))
    active = {}                                                     # worker index -> (object index, generator)
    together = min(len(gts), len(workers)) > 1
    budget = workers[0].wg_budget if together else 0   # alone on the GPU: plan for the whole chip
    for w in workers:
        if hasattr(w.model, 'set_wg_budget'):
            w.model.set_wg_budget(budget)
    while pending or active:
        for wi, w in enumerate(workers):
            if wi not in active and pending:
                oi = pending.pop(0)
                others = lucid_others[oi] if lucid_others is not None else _others_for(share.get('layers'), gts, tfid, oi)
                active[wi] = (oi, finetune_object_steps(w.model, w.meta_optim, meta_optim_state_dict, frames, gts[oi], cfg,
                                                        augment, tfid[oi], **eval_options.travelling(share, lucid_others=others)))
        for wi in sorted(active):
            oi, gen = active[wi]
            w = workers[wi]
            with w.on_stream():
                try:
                    next(gen)
                except StopIteration as stop:
                    if w.model.engine is not None:
                        w.model.engine.synchronize()
                    out[oi] = stop.value
                    del active[wi]
    return out


def merge_objects(engine, probs_all, frames=None, crf=None, keep=(), components=None, holes=None, snap=None, frame_offset=None,
                  motion=None):
    """Per-object probabilities [(N,H,W)] -> label maps (N,H,W) uint8 (`evaluate.py:322-326`).
    `crf` (`crf.py`; None or iterations 0: off, the code below as it always was): the local dense CRF refines the merge against
    `frames` (N,3,H,W), one `crf_labels` call per chunk of frames.  The frames listed in `keep` -- the train frame of EVERY
    object of the sequence, whose prediction is the seeded ground truth -- take the plain merge and stay it.
    `components` (`components.py`; None or neutral values: off, nothing new is called): after the merge and the CRF, the
    connected-component filter zeroes small / non-dominant / ungated components frame by frame; the `keep` frames pass
    unchanged and anchor the gate of the frame after them.
    `holes` (`holes.py`; None or max_area 0: off, nothing new is called): last, enclosed background islands that are small
    and were object in the previous frame's filled map are filled; the `keep` frames pass unchanged and anchor that chain.
    `snap` (`snap.py`; None or step 0: off, nothing new is called): between the CRF and the component filter, every SLIC
    superpixel of `frames` takes the label that holds its majority; the `keep` frames pass unchanged.  `frame_offset`: what the
    data set subtracted from the RGB frame (`mean_val` under `data_cfg.normalize`), for `snap.quantise`.
    `motion` (`motion.py`; None or block 0: off, nothing new is called): the gate of the component filter and `prev_overlap` of
    the hole filler see the previous frame's cleaned map warped onto the current frame by block motion of `frames`.  The
    vectors of all frames are computed once; a stage whose temporal rule is on then runs one frame per call, a stage whose
    rule is off keeps its single batched call.  Needs `frames` and at least one of the two rules.
    The chain: merge -> CRF -> snap -> components -> holes."""
    stack = torch.stack(list(probs_all), dim=1)                       # (N, n_obj, H, W)
    clean = component_filter.active(components)
    fill = hole_filler.active(holes)
    snapping = snapper.active(snap)
    if snapping and (frames is None or frames.shape[0] != stack.shape[0] or frames.shape[2:] != stack.shape[2:]):
        raise ValueError('merge_objects: snap needs the frames (N, 3, H, W) of the probabilities it snaps')
    moving = mover.active(motion)
    gated = clean and component_filter.check(components)['gate'] > 0
    overlapped = fill and hole_filler.overlap_q16(hole_filler.check(holes)['prev_overlap']) > 0
    if moving and (frames is None or frames.shape[0] != stack.shape[0] or frames.shape[2:] != stack.shape[2:]):
        raise ValueError('merge_objects: motion needs the frames (N, 3, H, W) of the probabilities it follows')
    if moving and not (gated or overlapped):
        raise ValueError('merge_objects: motion has no consumer: neither components.gate nor holes.prev_overlap is on')
    if crf_refine.active(crf):
        labels = _merge_refined(engine, stack, frames, crf, keep)
    else:
        labels = torch.stack([engine.merge_labels(stack[f].contiguous()) for f in range(stack.shape[0])])
    rgb = snapper.quantise(frames, frame_offset) if snapping or moving else None
    if snapping:
        labels = snapper.snap(engine, rgb, labels, snap, keep=keep, n_obj=stack.shape[1])
    if not moving:
        if clean:
            labels = component_filter.filter(engine, labels, components, keep=keep)
        return hole_filler.fill(engine, labels, holes, keep=keep) if fill else labels
    block = mover.check(motion)['block']
    mv = mover.vectors(engine, rgb, motion)
    if clean:
        labels = _follow(component_filter.filter, engine, labels, components, keep, mv, block) if gated else \
            component_filter.filter(engine, labels, components, keep=keep)
    if fill:
        labels = _follow(hole_filler.fill, engine, labels, holes, keep, mv, block) if overlapped else \
            hole_filler.fill(engine, labels, holes, keep=keep)
    return labels


def _follow(stage, engine, labels, params, keep, mv, block):
    """A temporal stage (`components.filter`, `holes.fill`) one frame per call in ascending order, each frame against the
    stage's output of the frame before it warped by the frame's vectors (`motion.py`, rule 8).  Frame 0 has no `prev`; a `keep`
    frame passes unchanged and is still warped for its successor."""
    keep = {int(f) for f in keep}
    out = torch.empty_like(labels)
    prev = None
    for f in range(labels.shape[0]):
        out[f:f + 1] = stage(engine, labels[f:f + 1], params, prev=prev, keep=(0,) if f in keep else ())
        if f + 1 < labels.shape[0]:
            prev = mover.warp(engine, out[f:f + 1], mv[f + 1:f + 2], block)[0]
    return out


def _merge_refined(engine, stack, frames, crf, keep):
    if frames is None or frames.shape[0] != stack.shape[0] or frames.shape[2:] != stack.shape[2:]:
        raise ValueError('merge_objects: the CRF needs the frames (N, 3, H, W) of the probabilities it refines')
    n, n_obj, h, w = stack.shape
    keep = {int(f) for f in keep}
    out = torch.empty(n, h, w, dtype=torch.uint8, device=stack.device)
    todo = [f for f in range(n) if f not in keep]
    step = crf_refine.frames_per_call(n_obj, h, w)
    for i in range(0, len(todo), step):
        fs = todo[i:i + step]
        out[fs] = crf_refine.labels(engine, frames[fs].float().contiguous(), stack[fs].contiguous(), crf)
    for f in sorted(keep):
        if 0 <= f < n:
            out[f] = engine.merge_labels(stack[f].contiguous())
    return out


def evaluate_sequence(model, meta_optim, meta_optim_state_dict, frames, object_gts, cfg, augment=None, train_frame_id=0, **groups):
    """frames (N,3,H,W) on the GPU, object_gts: list of (1,H,W) binary masks of the train frame.
    cfg keys (names of cfgs/meta.yaml): num_epochs.eval, eval_online_adapt.{step,reset_model_mode,
    num_epochs,min_prop (a threshold, or [lo, hi]: `min_prop_band`)}, data_cfg.batch_sizes.train, seed, loss_func, train_early_stopping_cfg.
    `groups`: the option groups of `eval_options.TABLE`, by keyword; the object-stage ones go to every `finetune_object`, the
    merge-stage ones to `merge_objects`, where the train frame is the `keep` frame.
    Returns (labels (N,H,W) uint8, per-object probs list, train loss history per object)."""
    share, merge_share = eval_options.split('evaluate_sequence', groups)
    probs_all, hist_all = [], []
    for o, gt in enumerate(object_gts):
        probs, hist = finetune_object(model, meta_optim, meta_optim_state_dict, frames, gt, cfg, augment, train_frame_id,
                                      **_object_share(share, object_gts, [train_frame_id] * len(object_gts), o))
        probs_all.append(probs)
        hist_all.append(hist)
    merge_kw = eval_options.travelling(merge_share, cfg)
    if not merge_kw:
        return merge_objects(model.engine, probs_all), probs_all, hist_all
    # this call site hands `frames` and `crf` over by position, the CRF set or not
    return merge_objects(model.engine, probs_all, frames, merge_kw.pop('crf', None), keep=(train_frame_id,), **merge_kw), \
        probs_all, hist_all


def prediction_paths(save_dir, dataset_name, split):
    """`{save_dir}/best_eval_preds/{name}/{split}` and the `_debug` sibling (`evaluate.py:68-90`)."""
    return (os.path.join(save_dir, 'best_eval_preds', f'{dataset_name}', f'{split}'),
            os.path.join(save_dir, 'best_eval_preds_debug', f'{dataset_name}', f'{split}'))


def save_label_png(path, labels_hw):
    """One uint8 label map per frame (`imageio.imsave(pred_path, mask_frame)`, `evaluate.py:338-342`)."""
    from PIL import Image
    Image.fromarray(np.asarray(labels_hw, dtype=np.uint8), mode='L').save(path)


def evaluate_dataset(model, meta_optim, meta_optim_state_dict, dataset, cfg, dataset_key, save_dir=None,
                     meta_iter=None, meta_epoch=None, best_mean_J=0.0, dist=None, device=None, vis_win_names=None,
                     log=None, objects_in_flight=None, **groups):
    """The evaluation worker of `src/util/evaluate.py:111-382` for the DeepLab path: every sequence of `dataset`
    (an `eosvos_amd.data` reader), every object, fine-tune / online adaptation / inference / merge; prediction PNGs
    under `{save_dir}/best_eval_preds/{name}/{split}/{seq}/{frame}.png`, J per sequence, and the
    `last_{key}_meta_iter.model` / `best_{key}_meta_iter.model` checkpoints (`:361-382`).

    With `dist` (torch.distributed, world > 1) the (sequence, object) work items are dealt round-robin over the
    ranks (they are independent fine-tunes); the only exchange is one all-reduce(sum) per sequence of the
    zero-initialised per-object probability stack (every slot is written by exactly one rank, so the sum is exact),
    after which every rank merges the same label maps and rank 0 writes files.
    `objects_in_flight` (default: EOSVOS_OBJECTS_IN_FLIGHT, else 3 on a GPU): how many of a sequence's objects this
    rank fine-tunes side by side, one engine and stream each (`run_objects_in_flight`); 1 = one after the other.
    Engines that run side by side plan every launch for half the chip (`eosvos_set_wg_budget` 256), an object alone on
    the GPU for all of it, and engines built for side-by-side work have no side stream (every stage's weight gradients
    grouped): budget and grouping change the split-K partition, i.e. the order of fp32 partial sums, so the last
    bits of a result (not its parity margins, `profiles/*parity_margins*`) depend on how many objects of the sequence
    landed on this rank.  EOSVOS_OBJECTS_IN_FLIGHT=1 gives one schedule-independent order.
    `groups`: the option groups of `eval_options.TABLE`, by keyword (`eval_options.from_cfg(cfg)` for a parsed config).  The
    object-stage ones go to every object's fine-tune (the view engines `tta` builds are released with the parked ones at the
    end); the merge-stage ones to `merge_objects`, so that the PNGs, J_seq and the J / F counts see the final label maps.  A frame
    that is the train frame of every object of its sequence is the `keep` frame of the merge.
    Returns dict(J_seq, mean_J, best_mean_J, time_per_frame, labels={seq: (N,H,W) uint8}) and the DAVIS J / F statistics
    of `eval_davis_seq` (`evaluate.py:345-359`), one entry per object in sequence order: J_obj (the per-object J means the
    reference calls J_seq), J_recall_seq, J_decay_seq, F_seq, F_recall_seq, F_decay_seq, with mean_F and
    mean_JF = (mean J_obj + mean_F) / 2.  Their counts are taken on the device from the merged label maps
    (`data.davis_counts`); J_seq, mean_J and the best-checkpoint choice stay per sequence, from `sequence_J`."""
    from .checkpoint import save_meta_checkpoint
    from .data import davis_counts, measures_from_counts, sequence_J
    share, merge_share = eval_options.split('evaluate_dataset', groups)
    rank = dist.get_rank() if dist is not None else 0
    world = dist.get_world_size() if dist is not None else 1
    ds_cfg = cfg['datasets'][dataset_key]
    preds_dir = None
    if save_dir is not None:
        preds_dir, _ = prediction_paths(save_dir, ds_cfg['name'], ds_cfg['split'])
        if rank == 0:
            for seq in dataset.seqs_names:
                os.makedirs(os.path.join(preds_dir, seq), exist_ok=True)
    set_random_seeds(cfg.get('seed', 1))                                        # evaluate.py:42
    if objects_in_flight is None:
        objects_in_flight = int(os.environ.get('EOSVOS_OBJECTS_IN_FLIGHT', 3 if torch.device(device or model.device).type == 'cuda' else 1))
    if torch.device(device or model.device).type == 'cuda' and model.max_batch < INFER_BATCH:
        # size the engine(s) for the inference batch before any object starts (a fine-tune never needs the old engine's
        # weights: every object begins with load_state_dict + reset)
        model.max_batch = INFER_BATCH
        if model.engine is not None and model.engine.max_batch < INFER_BATCH:
            model.engine.close()
            model.engine = None
            model._dirty = True
        if hasattr(model, 'close_parked_engines'):
            model.close_parked_engines()        # parked engines of the smaller max_batch would be closed on first use anyway
        model._object_workers = None
    workers = None
    if objects_in_flight > 1:
        workers = getattr(model, '_object_workers', None)
        if workers is None or len(workers) != objects_in_flight:
            workers = model._object_workers = object_workers(model, meta_optim, cfg['meta_optim_cfg'], objects_in_flight)
        else:
            # cached workers are spawned COPIES: the caller may have loaded another parent checkpoint since (one per dataset
            # key, evaluate.py:46-50) -- MetaOptimizer.load_state_dict never touches the frozen norm statistics, and with
            # `learn_model_init: False` not the weights either
            for w in workers:
                w.model.copy_state_from(model)
    J_seq, labels_out, item, eval_time, num_frames = [], {}, 0, 0.0, 0
    phases = {}                                  # seconds per phase on the calling thread (EOSVOS_EVAL_TIMING=1 drains the GPU at the boundaries)
    drain = os.environ.get('EOSVOS_EVAL_TIMING') == '1' and torch.device(device or model.device).type == 'cuda'

    def tick(name, t_start):
        if drain:
            torch.cuda.synchronize()
        phases[name] = phases.get(name, 0.0) + time.perf_counter() - t_start
        return time.perf_counter()
    # File readers (`prefetchable`) are used through shallow copies on two worker threads: sequence k + 1 is decoded while
    # sequence k is fine-tuned, and the PNGs / J of sequence k are written while k + 1 runs (PIL releases the GIL).
    # EOSVOS_EVAL_PREFETCH=0 keeps everything on the calling thread.
    import copy
    from concurrent.futures import ThreadPoolExecutor
    seqs = list(dataset.seqs_names)
    pool = None
    if getattr(dataset, 'prefetchable', False) and seqs and os.environ.get('EOSVOS_EVAL_PREFETCH', '1') != '0':
        pool = ThreadPoolExecutor(max_workers=2)
    def read(ds, sq, dev):
        """(frames, train-frame masks, train frame per object); readers without late objects report frame 0."""
        import inspect
        if 'with_frame_ids' in inspect.signature(ds.sequence_tensors).parameters:
            return ds.sequence_tensors(sq, dev, with_frame_ids=True)
        fr, gs = ds.sequence_tensors(sq, dev)
        return fr, gs, [0] * len(gs)

    def read_gt(ds, sq):
        """Ground-truth label maps of the J / F measures (none in test mode)."""
        return None if ds.test_mode else ds.label_maps(sq)

    def load(sq):
        ds = copy.copy(dataset)
        return read(ds, sq, 'cpu') + (read_gt(ds, sq),)
    budget_before = getattr(model, 'wg_budget', 0)
    ahead = pool.submit(load, seqs[0]) if pool else None
    finishing = []

    def finish(ds, sq, labels, n_obj, gt_maps, counts):
        """PNG files, J and the J / F statistics of one finished sequence (host only)."""
        if rank == 0 and preds_dir is not None:
            names = ds.frame_names(sq)
            for f in range(labels.shape[0]):
                if getattr(ds, 'all_frames', False) and not ds.has_label_file(sq, names[f]):
                    continue                                                    # evaluate.py:334-335
                save_label_png(os.path.join(preds_dir, sq, names[f] + '.png'), labels[f].numpy())
        if ds.test_mode:                                                        # evaluate.py:344-347
            return 0.0, {m: {'mean': [0.0], 'recall': [0.0], 'decay': [0.0]} for m in ('J', 'F')}
        return sequence_J(labels.numpy(), gt_maps, n_obj), measures_from_counts(counts[1:len(counts) - 1])

    for k, seq in enumerate(seqs):
        tp = time.perf_counter()
        if pool:
            frames, gts, fids, gt_maps = ahead.result()
            frames, gts = frames.to(device or model.device), [g.to(device or model.device) for g in gts]
            if k + 1 < len(seqs):
                ahead = pool.submit(load, seqs[k + 1])
        else:
            frames, gts, fids = read(dataset, seq, device or model.device)
            gt_maps = read_gt(dataset, seq)
        tp = tick('read_s', tp)
        n = frames.shape[0]
        probs = torch.zeros(len(gts), n, *frames.shape[-2:], device=frames.device)
        t0 = time.perf_counter()
        mine = []
        for obj_id in range(len(gts)):
            if item % world == rank:
                mine.append(obj_id)
            item += 1
        if workers is not None and len(mine) > 1:
            res = run_objects_in_flight(workers, meta_optim_state_dict, frames, [gts[o] for o in mine], cfg,
                                        train_frame_id=[fids[o] for o in mine],
                                        lucid_others=[_others_for(share.get('layers'), gts, fids, o) for o in mine], **share)
            for o, (p, _) in zip(mine, res):
                probs[o] = p
        else:
            if workers is not None:
                model.set_wg_budget(0)                                          # alone on the GPU
            for o in mine:
                probs[o], _ = finetune_object(model, meta_optim, meta_optim_state_dict, frames, gts[o], cfg,
                                              train_frame_id=fids[o], **_object_share(share, gts, fids, o))
        if world > 1:
            dist.all_reduce(probs)
        eval_time += time.perf_counter() - t0
        tp = tick('finetune_s', tp)
        num_frames += n * len(gts)                                              # per (object, frame), evaluate.py:320
        if model.engine is None:                                                # this rank had no item yet
            model._ensure_engine(frames.shape[2], frames.shape[3], 1)
        merge_kw = eval_options.travelling(merge_share, cfg, dataset)
        # this call site hands everything over by keyword: `keep` also beside a `holes` that is set and fills nothing, `frames`
        # only to the stages that read them
        if merge_kw or 'holes' in merge_share:
            merge_kw['keep'] = tuple(set(fids)) if len(set(fids)) == 1 else ()
        if any(k in merge_kw for k in ('crf', 'snap', 'motion')):
            merge_kw['frames'] = frames
        labels = merge_objects(model.engine, [probs[o] for o in range(len(gts))], **merge_kw)
        counts = None
        if not dataset.test_mode:                                               # J / F counts where the labels are
            gt_dev = torch.from_numpy(np.ascontiguousarray(gt_maps, dtype=np.uint8)).to(labels.device)
            counts = davis_counts(model.engine, labels, gt_dev, len(gts))
        labels = labels.cpu()
        labels_out[seq] = labels
        tp = tick('merge_s', tp)
        if pool:
            finishing.append(pool.submit(finish, copy.copy(dataset), seq, labels, len(gts), gt_maps, counts))
        else:
            finishing.append(finish(dataset, seq, labels, len(gts), gt_maps, counts))
        tp = tick('finish_s', tp)
    stats = {k: [] for k in ('J_obj', 'J_recall_seq', 'J_decay_seq', 'F_seq', 'F_recall_seq', 'F_decay_seq')}
    for seq, j in zip(seqs, finishing):
        j_seq, ev = j.result() if pool else j
        J_seq.append(j_seq)
        for key, (m, st) in zip(stats, [(m, st) for m in ('J', 'F') for st in ('mean', 'recall', 'decay')]):
            stats[key].extend(ev[m][st])                                        # evaluate.py:354-359
        if log is not None and rank == 0:
            log(f"{dataset_key}: {seq} [{J_seq[-1]}]")
    if pool:
        pool.shutdown(wait=True)
    if workers is not None and hasattr(model, 'set_wg_budget'):
        model.set_wg_budget(budget_before)
    # engines parked for the frame sizes this dataset went through (4-17 GB each, per model AND per object worker) are released;
    # the live engines stay for the next call
    for m in [model] + [w.model for w in (workers or [])]:
        if hasattr(m, 'close_parked_engines'):
            m.close_parked_engines()
    mean_J = float(np.mean(J_seq)) if J_seq else 0.0
    mean_F = float(np.mean(stats['F_seq'])) if stats['F_seq'] else 0.0
    mean_JF = (float(np.mean(stats['J_obj'])) + mean_F) / 2 if stats['J_obj'] else 0.0
    out_best = best_mean_J
    if rank == 0 and save_dir is not None and not dataset.test_mode:
        save_meta_checkpoint(os.path.join(save_dir, f'last_{dataset_key}_meta_iter.model'), meta_optim_state_dict,
                             meta_iter, meta_epoch, vis_win_names)
    if dataset.test_mode or mean_J > best_mean_J:                               # evaluate.py:368-382
        out_best = mean_J
        if rank == 0 and save_dir is not None and not dataset.test_mode:
            save_meta_checkpoint(os.path.join(save_dir, f'best_{dataset_key}_meta_iter.model'), meta_optim_state_dict,
                                 meta_iter, meta_epoch, vis_win_names)
    return {'J_seq': J_seq, 'mean_J': mean_J, 'best_mean_J': out_best, 'labels': labels_out,
            'time_per_frame': eval_time / max(num_frames, 1), 'meta_iter': meta_iter, 'phases': phases,
            'mean_F': mean_F, 'mean_JF': mean_JF, **stats}
