"""Mirror of the hot-path helpers of `src/util/helper_func.py` on the MI355X engine.

  compute_loss        `helper_func.py:28-56`   (cross_entropy = fused BCE-with-logits kernel)
  init_parent_model   `helper_func.py:339-385` (DeepLabV3Plus only)
  run_frames          `helper_func.py:67-159`  (`run_loader` for the DeepLab branch `:131-142`:
                                                sigmoid, per-sample BCE, >=0.5 accuracy)
  early_stopping      `helper_func.py:388-397`
  EpochSampler        `helper_func.py:521-545`
  set_random_seeds    `helper_func.py:515-518`
`dice` (`networks/loss_dice.py:4-40`), `cross_entropy_and_dice` (`:45-54`) and
`class_balanced_cross_entropy` (`networks/loss_ce.py:15-60`) run as fused HIP kernels too, and so does the
Lovasz hinge of `networks/loss_lovasz.py:78-111` as `lovasz_hinge` (`per_image=True`, the reference default) and
`lovasz_hinge_flat` (`per_image=False`); unknown names raise NotImplementedError as in the reference (`:55-56`).
`loss_kwargs={'ignore': v}` marks the pixels whose target equals `v` as void for every kind: the reference's keyword for the
Lovasz hinge (`networks/loss_lovasz.py:78-126`), the same rule for the others (in no sum and no count, gradient 0).
`bootstrapped_cross_entropy` (`bootstrap.py`; not in the reference) averages the BCE of the hardest fraction of each image's
pixels: the engine's fraction (0.25 by default), `bootstrapped_cross_entropy_<P>` for P percent, or `loss_kwargs={'fraction': f}`.
`boundary_f` / `cross_entropy_and_boundary_f` (`boundary.py`; not in the reference) are the soft boundary-F loss and its sum
with `cross_entropy`: the engine's window radius (by default the DAVIS tolerance of the frame size), `boundary_f_<r>` for
r pixels, or `loss_kwargs={'radius': r}`.
`surface` (`surface.py`; not in the reference) weights every pixel's error by its distance to the target's boundary, capped at
the engine's cap (by default a quarter of the frame's short side, untuned), `surface_<L>` for L pixels, or
`loss_kwargs={'cap': L}`; it is meant as a term of a sum, e.g. `dice+0.5*surface_64`.
`potts` (`potts.py`; not in the reference) is the image-aware pairwise loss: it reads the frames of the last forward and no
target (void pixels get its gradient too), on the engine's window (radius 3, dilation 2 by default, untuned), `potts_<r>` /
`potts_<r>x<d>` for another, or `loss_kwargs={'window': r}`; it is meant as a term of a sum, e.g. `cross_entropy+0.1*potts_3x2`,
and has no per-sample form (`batch_average: False`), which carries no frames.
`cldice` (`cldice.py`; not in the reference) is the topology-aware centreline loss (soft clDice): how much of each map's soft
skeleton lies inside the other map, so a cut through a thin part costs far more than the same pixels off a blob's edge; the
engine's depth (by default one erosion per 96 pixels of the frame's short side, untuned), `cldice_<k>` for k erosions, or
`loss_kwargs={'depth': k}`; it is meant as a term of a sum, e.g. `dice+0.5*cldice_5`.
A `loss_func` with a '+' or a '*' is a weighted sum of up to four of these (`loss_sum.py`), e.g. `0.5*lovasz_hinge+boundary_f_4`.
"""
import random

import numpy as np
import torch

from . import loss_sum
from . import tta as tta_views
from . import zoom as zoom_pass
from .loss_names import KEYWORDS
from .networks import DeepLabV3, DeepLabV3Plus


def compute_loss(loss_func, outputs, gts, loss_kwargs=None):
    """`compute_loss(loss_func, outputs, gts, loss_kwargs=None)`, helper_func.py:28-56.  The returned
    0-dim loss carries the engine handle so `MetaOptimizer.step(loss)` can run the backward."""
    loss_kwargs = loss_kwargs or {}
    per_image = loss_kwargs.get('per_image', True)
    # a plain name is the sum of one term here (the engine still runs it as that one kind); unknown names and bad suffixes:
    # NotImplementedError; a keyword without a term of its family, out of range or against a suffix: ValueError
    names = loss_sum.resolve_terms(loss_func, per_image, **{k: loss_kwargs.get(k) for k in KEYWORDS})[2]
    if 'class_balanced_cross_entropy' in names and not loss_kwargs.get('size_average', True):
        raise NotImplementedError('class_balanced_cross_entropy with size_average=False')
    if not per_image:
        loss_func = loss_sum.flat_spelling(loss_func)      # loss_lovasz.py:89-90: the whole batch as one set
    eng = getattr(outputs, '_eosvos_engine', None)
    if eng is None:
        raise RuntimeError('compute_loss needs logits produced by eosvos_amd.networks.DeepLabV3Plus '
                           '(there is no CPU/eager path)')
    gts = gts.contiguous().float()
    kw = {k: loss_kwargs[k] for k in ('ignore', *KEYWORDS) if loss_kwargs.get(k) is not None}
    if loss_kwargs.get('batch_average', True):
        loss = eng.loss(loss_func, gts, **kw).view(())      # also leaves dL/dlogits in the engine
        loss._eosvos_engine = eng
        return loss
    # per-sample values (run_loader metrics, helper_func.py:131-137): every loss evaluated sample by sample
    return torch.cat([eng.loss_of(loss_func, outputs[b], gts[b], **kw) for b in range(outputs.shape[0])])


def init_parent_model(architecture, encoder, train_encoder, decoder_norm_layer=None,
                      replace_batch_with_group_norms=False, batch_norm=None, roi_pool_output_sizes=None,
                      eval_augment_rpn_proposals_mode=None, box_nms_thresh=None, maskrcnn_loss=None, **datasets):
    """Same signature as the reference; returns (model, parent_states)."""
    if architecture == 'DeepLabV3':                         # helper_func.py:343-344
        model = DeepLabV3(encoder, num_classes=1, batch_norm=batch_norm, train_encoder=train_encoder)
    elif architecture == 'DeepLabV3Plus':
        model = DeepLabV3Plus(encoder, num_classes=1, batch_norm=batch_norm, train_encoder=train_encoder,
                              replace_batch_with_group_norms=replace_batch_with_group_norms)
    else:
        raise NotImplementedError(f"architecture='{architecture}': the MI355X engine implements DeepLabV3Plus and DeepLabV3")
    parent_states = {}
    for k, v in datasets.items():
        parent_states[k] = {
            'states': [torch.load(p, map_location='cpu', weights_only=False) for p in v.get('paths', [])],
            'splits': [np.loadtxt(p, dtype=str).tolist() for p in v.get('val_split_files', [])
                       if isinstance(p, str) and __import__('os').path.exists(p)],
        }
    return model, parent_states


def run_frames(model, frames, gts=None, loss_func='cross_entropy', tta=None, zoom=None):
    """Inference over frames (N,3,H,W) one at a time (batch 1, `test` batch size of the configs):
    returns (`loss_func` per frame or None, acc per frame or None, probs (N,1,H,W)) -- `run_loader`,
    helper_func.py:131-142, evaluates the configured loss with `batch_average: False`.
    `tta` ({'flip': bool, 'scales': [floats]}, `tta.py`): probs are the mean over the mirrored / rescaled views, and the
    loss is that of the averaged prediction (of its logit, log(p / (1 - p))); None or the neutral dictionary: one plain view.
    `zoom` (`zoom.py`): every frame gets a second look at a crop around the object its first pass (the plain view or the mean
    over the views) found, blended into probs inside the crop; the loss is that of the refined prediction's logit.  None or
    `max_zoom: 0`: off."""
    model.eval()
    probs, losses, accs = [], [], []
    use_tta = tta_views.active(tta)
    use_zoom = zoom_pass.active(zoom)
    view_set = refiner = None
    framed = gts is not None and isinstance(loss_func, str) and 'potts' in loss_func      # (a bad spelling fails in the engine, as before)
    for i in range(frames.shape[0]):
        x = frames[i:i + 1].contiguous()
        eng = model._ensure_engine(x.shape[2], x.shape[3], 1)
        if use_tta:
            if view_set is None or (view_set.height, view_set.width) != tuple(x.shape[2:]):
                view_set = tta_views.ViewSet(model, x.shape[2], x.shape[3], tta)
                view_set.sync()                               # the weights do not change while this function runs
            p = view_set.infer(x)
        else:
            p = eng.infer(x)
        if use_zoom:
            if refiner is None or (refiner.height, refiner.width) != tuple(x.shape[2:]):
                refiner = zoom_pass.Refiner(model, x.shape[2], x.shape[3], zoom, tta if use_tta else None)
            p = refiner.refine(x, p)
        probs.append(p)
        if gts is not None:
            logits = torch.logit(p, eps=1e-7) if use_tta or use_zoom else eng.debug_tensor('logits')[:1]
            if framed:                                        # a `potts` term reads the frame
                losses.append(eng.loss_of_framed(loss_func, logits, gts[i:i + 1].contiguous(), x))
            else:
                losses.append(eng.loss_of(loss_func, logits, gts[i:i + 1].contiguous()))
            pred = p.ge(0.5)
            accs.append(pred.eq(gts[i:i + 1].bool()).float().mean().view(1))
    probs = torch.cat(probs)
    if gts is None:
        return None, None, probs
    return torch.cat(losses).cpu(), torch.cat(accs).cpu(), probs


def early_stopping(loss_hist, patience, min_loss_improv):
    if patience is None or len(loss_hist) <= patience:
        return False
    best = min(loss_hist)
    prev_best = min(loss_hist[:-patience])
    return not abs(best - prev_best) > min_loss_improv


def set_random_seeds(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


class EpochSampler:
    """Sample `num_epochs` passes over the dataset into ONE batch (`helper_func.py:521-545`)."""

    def __init__(self, dataset, shuffle, num_epochs, sampler=None):
        if shuffle and sampler is None:
            raise NotImplementedError('shuffle=True needs an explicit sampler here')
        self.sampler = sampler if sampler is not None else range(len(dataset))
        self.num_epochs = num_epochs

    def __iter__(self):
        batch = []
        for _ in range(self.num_epochs):
            batch.extend(self.sampler)
        yield batch

    def __len__(self):
        return 1
