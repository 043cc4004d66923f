/*
 * eosvos.h -- C-ABI of the MI355X-native e-OSVOS inner-loop engine (libeosvos.so).
 *
 * The reference (dvl-tum/e-osvos) is pure Python with no FFI layer of its own; the
 * seam this library replaces is the Python duck-typed boundary between the
 * orchestration loops (src/util/evaluate.py, src/util/meta_run.py, src/train_meta.py)
 * and src/networks + src/meta_optim.  Each entry point below names the reference
 * interface it stands in for (file:line under /root/reference).  INTEGRATION.md shows
 * the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (hipMalloc / torch-ROCm `tensor.data_ptr()`)
 *    unless the parameter name ends in `_host`;
 *  - tensors crossing the boundary use the reference's layouts: images NCHW fp32,
 *    parameters OIHW fp32 flattened in `named_parameters()` order, per-neuron learning
 *    rates one float per output channel in the same tensor order;
 *  - every call returns 0 on success, non-zero on error; `eosvos_last_error()` gives
 *    the message.  No exceptions or aborts cross the ABI;
 *  - an engine is bound to one HIP device + stream and is not thread-safe (one engine
 *    per process/rank, as the reference has one model per process,
 *    src/util/helper_func.py:499-512);
 *  - work is enqueued on the engine's stream; calls that return host scalars
 *    synchronise that stream.
 */
#ifndef EOSVOS_H
#define EOSVOS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eosvos_engine eosvos_engine;

#define EOSVOS_ARCH_RESNET50 50
#define EOSVOS_ARCH_RESNET101 101
/* plain DeepLabV3 (src/networks/deeplabv3.py:10-83; init_parent_model(architecture='DeepLabV3'), helper_func.py:343-344):
 * torchvision ResNet with replace_stride_with_dilation = [False, True, True] (output stride 8), DeepLabHead =
 * ASPP[12, 24, 36] -> 3x3 conv + BatchNorm + ReLU -> 1x1 conv, logits resized x8 (align_corners = False); no decoder.
 * State-dict keys: backbone.*, classifier.0.* (ASPP), classifier.1 / classifier.2 (3x3 conv + norm), classifier.4. */
#define EOSVOS_ARCH_V3_RESNET50 1050
#define EOSVOS_ARCH_V3_RESNET101 1101
#define EOSVOS_NORM_BN_FROZEN 0 /* BatchNorm in eval mode, frozen affine (deeplabv3plus.py:148-155,259-265) */
#define EOSVOS_NORM_GN16 1      /* GroupNorm(16, C) sharing the frozen BN affine (deeplabv3plus.py:180-191) */

/* ---- library / topology (host only, no GPU needed) ------------------------------ */
const char* eosvos_version(void);
const char* eosvos_last_error(void);

/* How the fp32 contractions of the convolutions run on the matrix cores (process-wide; results agree to fp32
 * rounding):
 *   F16X3 (default): every operand TENSOR is scaled by a power of two taken from its largest finite magnitude (kept on the
 *          device by the kernels that write the tensor), every scaled fp32 value is split into two fp16 pieces
 *          (round to nearest: together they hold the value to <= 1 fp32 ulp) and the product is accumulated in fp32 from
 *          the three leading partial products on v_mfma_f32_16x16x32_f16.  Error <= the fp32 MFMA's on tensors whose
 *          elements lie within 2^16 of the largest; smaller elements lose relative precision gradually (absolute
 *          error <= 2^-40 of the tensor's maximum each), which only shows in outputs that no large element reaches.
 *   BF16X6: every fp32 operand is split exactly into three bf16 pieces and the product is accumulated in fp32 from the six
 *          leading partial products on v_mfma_f32_16x16x32_bf16 (error <= fp32 MFMA's, no scaling, any dynamic range);
 *          1.5x the LDS traffic and 2x the MFMAs of F16X3.  EOSVOS_MFMA=bf16x6.
 *   F32:   v_mfma_f32_32x32x2_f32 (1/16 of the bf16 rate on CDNA4).  EOSVOS_MFMA=f32.
 * Special values (tests/test_gpu_conv_algos.py::test_bf16x6_special_values_propagate, ::test_f16x3_special_values_and_
 * dynamic_range): a NaN operand gives NaN in every mode; a +-inf operand gives +-inf in F32 and NaN in the split modes
 * (inf - piece(inf) is NaN) -- non-finite either way, which is what the meta loop's NaN-skip (meta_run.py:209-211)
 * needs: an overflowed task shows up as a NaN loss.  NaN / inf never set an F16X3 scale (finite values only), so the
 * outputs they do not reach keep their accuracy.  Denormal operands contribute nothing in any mode; BF16X6 splits
 * finite values up to FLT_MAX exactly. */
#define EOSVOS_MATRIX_F32 0
#define EOSVOS_MATRIX_BF16X6 1
#define EOSVOS_MATRIX_F16X3 2
int eosvos_set_matrix_mode(int mode);
int eosvos_get_matrix_mode(void);
/* Pre-split operand path of the F16X3 mode (round 6, presplit_kernels.hip): weight gradients whose channel counts are multiples
 * of 256 read their operands as fp16 (hi, lo) pair tensors made by a split pass (same two pieces, same products, same fp32
 * accumulation as the on-the-fly split) on 256 x 256 tiles staged by LDS-DMA.  Process-wide switch, default on
 * (EOSVOS_PRESPLIT=0: off; on = 2: also for maps below the 4000-pixel minimum, for tests on small frames); returns the previous
 * setting.  Live engines re-plan at their next call. */
int eosvos_set_presplit(int on);
/* Launch-plan fingerprint of the engine's last forward (out2[0]) and backward (out2[1]) pass: a 64-bit FNV-1a hash over (kind,
 * conv, M, N, K, workgroups / K splits) of every matrix launch and the slab counts the update consumed.  The split plan fixes the
 * fp32 summation order; the full-length parity fixtures were cleared with ONE plan per (mode, batch), and an equally valid other
 * plan moves a 240-iteration trajectory by up to 1e-3 -- tests/test_gpu_plan_fingerprint.py fails when a
 * change of the tile / split rules alters the plan without the fixtures having been re-cleared.  (The loop it guards:
 * `/root/reference/src/util/evaluate.py:207-281`.) */
int eosvos_plan_fingerprint(eosvos_engine* e, uint64_t* out2);
/* One engine's own matrix mode (round 5): every later call on `e` plans and launches its contractions in `mode`, whatever
 * the process-wide mode is and whatever other engines run in (-1: follow the process-wide mode again, the default).  This is
 * what the range guard of the Python shim uses: a state that leaves the F16X3 envelope moves the ENGINE that holds it to
 * BF16X6, not the process (engine.py Engine.verify_matrix_mode).  Thread-safe in the sense of the rest of the ABI: the mode
 * travels with the call on the calling host thread.  eosvos_get_engine_matrix_mode returns the mode in effect for `e`. */
int eosvos_set_engine_matrix_mode(eosvos_engine* e, int mode);
int eosvos_get_engine_matrix_mode(eosvos_engine* e);

/* Workgroups one launch of this engine plans for.  0 (default): two per CU, i.e. the whole chip -- right for an
 * engine that has the GPU to itself.  Engines that run beside each other (concurrent meta tasks, one engine per task:
 * meta_run.run_tasks_concurrent) do better with half of that: every launch then splits its reduction less (fewer parked
 * partial tiles to write and re-read) and the other engines' launches fill the rest of the chip (4 tasks in flight:
 * +8 % meta tasks/s at 256).  Rounded up to a multiple of 64; values >= 512 mean 0.  Changes the summation order of
 * split reductions (results stay within the parity tolerances, not bit-identical across budgets).  Call between
 * steps, not between a backward pass and its update.  Returns the budget in effect, < 0 on error.
 * No reference counterpart (the reference runs one task per process and lets cuDNN choose). */
int eosvos_set_wg_budget(eosvos_engine* e, int workgroups);

/* An engine alone on the GPU runs its weight-gradient launches on a second (side) stream beside the data-gradient chain
 * (on = 1, the default).  Engines that run side by side -- the tasks of a meta-batch in flight on one GPU, the objects of
 * a sequence (evaluate.py:132) -- are better off with ONE queue each (on = 0): the other engines fill the chip, and the
 * fork / join events between the two streams of every engine only add bubbles.  Measured on one MI355X at 480x854
 * (tools/inflight_sweep.py, profiles/r03_inflight_sweep.txt): 4 engines at batch 1, 192 -> 264 fine-tune iterations/s;
 * 3 engines at batch 3, 95.6 -> 105.5.  Call it while the engine is idle.  The loss, every data gradient and
 * most weight gradients do not change (same kernels, same order per engine).  Two groups of weight gradients keep their
 * accuracy but take another fp32 summation order, i.e. are not bit-identical across the switch: at batch > 1 layer1's ten
 * (an engine without the stream groups them into one stage launch, which plans their K splits together; with the stream
 * they overlap the data-gradient chain one by one), and in the f16x3 mode those of the pre-split operand path (stride-16
 * maps of >= 4000 pixels), which only an engine with the stream takes.  Returns 0 / 1 = the state now in effect, -1 on
 * error. */
int eosvos_set_side_stream(eosvos_engine* e, int on);

/* Number of convolutions of DeepLabV3+ on `arch` (63 for ResNet-50); -1 on bad arch.
 * Replaces: module enumeration of networks/deeplabv3plus.py:104-155. */
int eosvos_num_convs(int arch);
/* Fill info[9] = {cin, cout, k, stride, dilation, padding, has_norm, has_bias, param_offset}
 * for conv `idx` in the reference's named_parameters() order.  param_offset is the
 * offset (in floats) of its OIHW weight inside the flat parameter vector (a bias, if
 * any, follows its weight). */
int eosvos_conv_info(int arch, int idx, int64_t* info);
/* Totals: trainable scalars (40 289 729 for R50), per-neuron lr scalars (28 658),
 * norm channels (sum of Cout over the 62 norm layers). */
int64_t eosvos_param_count(int arch);
int64_t eosvos_lr_count(int arch);
int64_t eosvos_norm_count(int arch);

/* ---- engine life cycle ----------------------------------------------------------- */
/* Replaces: init_parent_model() + model.to(device) (helper_func.py:339-385).
 * `stream` is a hipStream_t (NULL = the device's default stream). */
int eosvos_create(eosvos_engine** out, int arch, int norm_mode, int height, int width,
                  int max_batch, int device_id, void* stream);
/* Same with construction flags.  EOSVOS_CREATE_NO_SIDE_STREAM: the engine never creates its second HIP stream (an engine
 * that will run beside other engines of the process: one hardware queue each, see eosvos_set_side_stream); the
 * environment variable EOSVOS_NO_SIDE_STREAM=1 sets the same flag for every engine of the process. */
#define EOSVOS_CREATE_NO_SIDE_STREAM 1
int eosvos_create_ex(eosvos_engine** out, int arch, int norm_mode, int height, int width,
                     int max_batch, int device_id, void* stream, int flags);
int eosvos_destroy(eosvos_engine* e);
int eosvos_synchronize(eosvos_engine* e);

/* Debug aid.  With EOSVOS_DEBUG_GUARD=1 in the environment every device buffer of an engine is allocated between two
 * 256 KB guard bands holding a pattern; this call waits for the device, reports on stderr every band a kernel wrote into
 * (an out-of-bounds write) and returns the number of overwritten words (0 without the environment variable). */
int eosvos_debug_check_guards(eosvos_engine* e);

/* ---- state ------------------------------------------------------------------------ */
/* Learned model initialisation (`model_init_*`, meta_optim.py:71-78): flat OIHW. */
int eosvos_set_init(eosvos_engine* e, const float* flat_params);
/* Learned per-neuron learning rates (`log_init_lr_*`, meta_optim.py:46-67), flat. */
int eosvos_set_lr(eosvos_engine* e, const float* flat_lr);
/* Frozen BatchNorm statistics + affine, each `eosvos_norm_count` floats, norm layers in
 * module order; folded on device to a*x+b with eps (networks/deeplabv3plus.py:259-265). */
int eosvos_set_norm(eosvos_engine* e, const float* gamma, const float* beta,
                    const float* running_mean, const float* running_var, float eps);
/* theta <- learned init.  Replaces MetaOptimizer.reset() (meta_optim.py:144-155). */
int eosvos_reset(eosvos_engine* e);
/* Current fine-tuned parameters, flat OIHW (model.state_dict() of the trainables). */
int eosvos_get_params(eosvos_engine* e, float* flat_params_out);
/* Overwrite the current parameters (model.load_state_dict, evaluate.py:200-203). */
int eosvos_set_params(eosvos_engine* e, const float* flat_params);
/* FIRST_STEP reset of online adaptation (evaluate.py:200-205,283-287). */
int eosvos_snapshot_params(eosvos_engine* e);
int eosvos_restore_params(eosvos_engine* e);

/* ---- fine-tuning hot loop (evaluate.py:220-274) ----------------------------------- */
/* logits = model(images)[-1]  (deeplabv3plus.py:282-301); keeps activations for backward.
 * images: B x 3 x H x W, logits_out: B x 1 x H x W (may be NULL). */
int eosvos_forward(eosvos_engine* e, const float* images, int batch, float* logits_out);
/* The loss entry points below are forms of one evaluation.  On the last forward: eosvos_loss_bce, eosvos_loss,
 * eosvos_loss_ignore and eosvos_loss_sum, which leave dL/dlogits for eosvos_backward_step -- and leave none when they return
 * an error -- and which eosvos_finetune_step / eosvos_meta_grad* run with what eosvos_set_loss / eosvos_set_loss_sum /
 * eosvos_set_loss_ignore stored.  On caller tensors: eosvos_bce, eosvos_loss_tensors, eosvos_loss_tensors_ignore and
 * eosvos_loss_sum_tensors.  A form with a kind runs that kind's own launches and nothing else; a form with a term list
 * runs each term into its slice and then the combine launch, for one term too.
 * Fused BCE-with-logits (mean over B*H*W, helper_func.py:32-37) of the last forward and
 * its gradient.  loss_out: one device float (may be NULL). */
int eosvos_loss_bce(eosvos_engine* e, const float* masks, int batch, float* loss_out);
/* Same for the other losses of compute_loss (helper_func.py:28-56), batch_average=True:
 * EOSVOS_LOSS_DICE = `dice` (networks/loss_dice.py:4-40, the config default cfgs/meta.yaml:68),
 * EOSVOS_LOSS_BCE_DICE = `cross_entropy_and_dice` (helper_func.py:45-54). */
#define EOSVOS_LOSS_BCE 0
#define EOSVOS_LOSS_DICE 1
#define EOSVOS_LOSS_BCE_DICE 2
#define EOSVOS_LOSS_CLASS_BALANCED_BCE 3 /* `class_balanced_cross_entropy`, networks/loss_ce.py:15-60 */
/* Lovasz hinge, the Jaccard hinge (networks/loss_lovasz.py:78-111): errors e = 1 - x * (2 * (t >= .5) - 1) ranked in
 * descending order (ties by ascending pixel index), weighted by the increments of the Jaccard loss along that order.
 * EOSVOS_LOSS_LOVASZ_HINGE = `per_image=True` (the reference default): the mean over the images of the batch;
 * EOSVOS_LOSS_LOVASZ_HINGE_FLAT = `per_image=False`: the whole batch is one set.  Through eosvos_loss_tensors the n
 * elements are one set for either kind.  A non-finite logit makes the loss NaN.  The first use of either kind allocates
 * the sort scratch (16 bytes per pixel of the largest batch) once; a failed allocation is reported and leaves the
 * engine usable with the other kinds. */
#define EOSVOS_LOSS_LOVASZ_HINGE 4
#define EOSVOS_LOSS_LOVASZ_HINGE_FLAT 5
/* Bootstrapped (hard-pixel) cross-entropy of OnAVOS / PReMVOS, `bootstrapped_cross_entropy`: per set, the BCE mean over the
 * hardest fraction of the pixels only.  A set is one image of the batch for eosvos_loss* and the fused entry points; through
 * eosvos_loss_tensors* the n elements are one set.  Within a set, V = the non-void pixels, n = |V|:
 *   key    key_p = -z_p * (2 * (y_p >= .5) - 1), an exact fp32 sign flip (the Lovasz sign rule).  For hard targets BCE-with-
 *          logits is strictly increasing in the key, so the top-k keys are the top-k losses; for soft targets this is the
 *          documented ranking and the summed term is still the true BCE.  Keys are compared as order-preserving 32-bit
 *          unsigned words (negative float: all bits flipped; otherwise the top bit set); -0 counts as +0; a NaN key maps to
 *          0xFFFFFFFF, so a NaN logit at a valid pixel is selected and makes the loss NaN.
 *   k      q = round(fraction * 65536), 1 <= q <= 65536;  k = max(1, (n * q + 32768) >> 16) in 64 bits.
 *   tau    the k-th largest key;  G = #{key > tau}, T = #{key = tau}, r = k - G (1 <= r <= T).
 *          w_p = 1 where key > tau, (float)r / (float)T where key = tau (one fp32 division, exactly 1 when r = T), else 0:
 *          the tied pixels share the remaining slots, nothing depends on an index order.
 *   loss   set loss = (sum_V w_p * bce_p) / k, bce_p = max(z, 0) - z * y + log1p(exp(-|z|));  loss = the mean of the set
 *          losses over the images;  dL/dz_p = w_p * (sigmoid(z_p) - y_p) / (k * images).  A pixel with w_p = 0 and every void
 *          pixel gets exactly +0, and the logit of a void pixel never reaches the result (it may be NaN / inf).  An empty V
 *          gives set loss 0: an all-void image adds 0 to the mean.
 * Fraction 1 keeps every valid pixel: EOSVOS_LOSS_BCE up to summation order.  Limits: fraction in (0, 1]; sets of fewer than
 * 2^31 pixels; one kind, per image on the forward path (no whole-batch sibling).  The selection is an exact radix select on
 * integer histograms and the sums run in a fixed order: loss and gradient are bit-identical from run to run.  The first use
 * allocates a small scratch (about 27 KB per image of the largest batch) once; a failed allocation is reported and leaves
 * the engine usable with the other kinds.  The default fraction 0.25 is OnAVOS's and is untuned here: no J&F figure exists
 * for it, no dataset being at hand. */
#define EOSVOS_LOSS_BOOTSTRAPPED_BCE 6
/* The fraction of EOSVOS_LOSS_BOOTSTRAPPED_BCE for every evaluation on this engine (eosvos_loss, eosvos_loss_ignore,
 * eosvos_loss_tensors[_ignore], eosvos_finetune_step, eosvos_meta_grad[_ex]): in (0, 1], anything else (NaN included) is an
 * error and changes nothing.  Per engine, 0.25 on every new engine; an engine that shares another's state does not take it
 * over. */
int eosvos_set_loss_bootstrap(eosvos_engine* e, float fraction);
/* Soft boundary-F loss, `boundary_f`: the soft form of the DAVIS F measure (Bokhovkin & Burnaev, "Boundary Loss for Remote
 * Sensing Imagery Semantic Segmentation", 2019).  Not in the reference.  Per image of H x W pixels, z the logits, y the targets,
 * V the valid (non-void) pixels; every window is square, centred, clipped to the frame and ranges over valid pixels only:
 *   q = sigmoid(-z), formed with the branch on the sign of z, never as 1 - sigmoid(z);  h = 1 - y
 *   pb(i) = max_{N1(i)} q - q(i),  gb(i) = max_{N1(i)} h - h(i)     N1 the 3 x 3 window; both 0 at void pixels
 *   pe(i) = max_{Nr(i)} pb,        ge(i) = max_{Nr(i)} gb           Nr the (2r+1)^2 window; both 0 at void pixels
 *   Sp = sum_V pb + eps,  Sg = sum_V gb + eps,  P = sum_V pb ge / Sp,  R = sum_V pe gb / Sg,  BF = 2PR / (P + R + eps),
 *   eps = 1e-7;  image loss = 1 - BF, 0 (with gradient 0) for an image without a valid pixel;  loss = the mean over the images.
 * Among equal maxima the first in row-major order is the arg-max (torch's max_pool2d rule on the CPU); the gradient routes
 * through both arg-max maps and is exactly 0 at void pixels, whose logits never reach the result.  An empty target, a full
 * target or constant logits give loss exactly 1 and gradient 0; a NaN logit at a valid pixel makes the loss NaN.
 * EOSVOS_LOSS_BCE_AND_BOUNDARY_F, `cross_entropy_and_boundary_f`: EOSVOS_LOSS_BCE over the same valid pixels plus the above,
 * a plain 1:1 sum (this project's own combination).
 * The radius r is per engine (eosvos_set_loss_boundary), in [1, 16]; by default min(16, ceil(0.008 * the frame diagonal)), the
 * DAVIS boundary tolerance: 8 at 480 x 854.  It is untuned: no J&F figure exists for it.  Both kinds need the frame's shape:
 * through eosvos_loss* and the fused entry points an image is the engine's H x W; eosvos_loss_tensors* accept n == H * W only,
 * as one image.  No atomics and fixed-order sums: loss and gradient are bit-identical from run to run.  The first use allocates
 * a scratch of 34 bytes per pixel of the engine's largest batch once; a failed allocation is reported and leaves the engine
 * usable with the other kinds.
 * Kind 7 is deliberately left unassigned: the tests of the earlier kinds use it as their unknown loss kind, so it stays an
 * error. */
#define EOSVOS_LOSS_BOUNDARY_F 8
#define EOSVOS_LOSS_BCE_AND_BOUNDARY_F 9
/* The radius of the two boundary kinds for every evaluation on this engine: 1 .. 16, or 0 for the frame-size default; anything
 * else is an error and changes nothing.  Per engine, like the bootstrap fraction. */
int eosvos_set_loss_boundary(eosvos_engine* e, int radius);
/* The boundary kinds on caller tensors with an explicit shape: `batch` images of height x width (batch <= the engine's largest
 * batch, batch * height * width <= its pixels), DEVICE pointers.  radius 1 .. 16, or 0 for this shape's default; `combined`
 * selects EOSVOS_LOSS_BCE_AND_BOUNDARY_F; `ignore_on` the void label `ignore`.  The loss goes to loss_out, the gradient to
 * dlogits_out or, when that is null, to the engine's own gradient scratch (a pending eosvos_loss* gradient is then lost). */
int eosvos_boundary_f(eosvos_engine* e, const float* logits, const float* masks, int batch, int height, int width, int radius,
                      int combined, int ignore_on, float ignore, float* loss_out, float* dlogits_out);
/* Distance-weighted surface loss, `surface`: every pixel's error weighted by its distance to the target's boundary (Kervadec
 * et al., "Boundary loss for highly unbalanced segmentation", MIDL 2019).  Not in the reference.  Meant as a term beside a
 * region loss (`dice+0.5*surface_64`).  Per image of H x W pixels, z the logits, y the targets, v the void label:
 *   V = {y != v};  F = {i in V : y_i >= 0.5};  B = V \ F.  A void pixel is in neither set and never a source of a distance.
 *   1. D2_i = the least dy^2 + dx^2 to a pixel of the OTHER class (B for i in F, F for i in B), infinite if that class is
 *      empty;  c_i = min(D2_i, L^2 + 1) as int32, the capped form of eosvos_distance_sq;  c_i = 0 at a void pixel.
 *   2. d_i = L if c_i > L^2, else sqrt(float(c_i));  w_i = d_i / float(L), in (0, 1] on V: correctly rounded IEEE fp32
 *      operations, so the numpy float32 expression reproduces w bit for bit.
 *   3. p = sigmoid(z);  e_i = 1 - p_i on F, p_i on B;  image loss = sum_V w e / |V|, 0 without a valid pixel;  loss = the mean
 *      over the images.  It is Kervadec's sum p phi up to a constant that makes it >= 0, and 0 for a perfect prediction.  An empty
 *      (or full) target gives w = 1 everywhere: the mean foreground (background) probability, no special case.
 *   4. dL/dz_i = s_i w_i p_i (1 - p_i) / (|V| images), s = -1 on F and +1 on B; exactly +0 at a void pixel, whose logit never
 *      reaches the result.
 * The cap L is per engine (eosvos_set_loss_surface), a whole number of pixels in [1, 4095]; by default max(1, min(H, W) / 4)
 * (integer division), 120 at 480 x 854.  It is untuned: no J&F figure exists for it.  The kind needs the frame's shape, as the
 * boundary kinds do: through eosvos_loss* and the fused entry points an image is the engine's H x W; eosvos_loss_tensors* accept
 * n == H * W only, as one image; frames of at most 4096 pixels a side.  Five launches (the two passes of the transform, the
 * partial sums, their fixed-order reduction, the gradient), no atomics: loss and gradient are bit-identical from run to run.
 * The first use allocates a scratch of 4 bytes per pixel of the engine's largest batch (plus 2 KB per image) once; a failed
 * allocation is reported and leaves the engine usable with the other kinds. */
#define EOSVOS_LOSS_SURFACE 10
/* The cap of EOSVOS_LOSS_SURFACE for every evaluation on this engine: 1 .. 4095, or 0 for the frame-size default; anything
 * else is an error and changes nothing.  Per engine, like the boundary radius. */
int eosvos_set_loss_surface(eosvos_engine* e, int cap);
/* The surface loss on caller tensors with an explicit shape: `images` (1 .. 65535) maps of height x width, each side in
 * [1, 4096], DEVICE pointers.  cap 1 .. 4095, or 0 for this shape's default; `ignore`: null, or a HOST pointer to the void
 * label.  The loss goes to loss_out (a device float), the gradient to dlogits_out, which may be null (none is formed).  The
 * scratch (4 bytes per pixel) comes from the arena of the evaluation-stage entry points, under its 512 MB cap per call.  Bad
 * arguments return non-zero before any launch: the outputs stay untouched. */
int eosvos_surface_loss(eosvos_engine* e, const float* logits, const float* masks, int images, int height, int width, int cap,
                        const float* ignore, float* loss_out, float* dlogits_out);
/* Rules 1 and 2 alone, with the arguments and limits of eosvos_surface_loss: c_out [image][H][W] int32 and / or w_out
 * [image][H][W] fp32, DEVICE pointers; either may be null, not both. */
int eosvos_surface_weights(eosvos_engine* e, const float* masks, int images, int height, int width, int cap, const float* ignore,
                           int32_t* c_out, float* w_out);
/* Image-aware pairwise loss, `potts`: neighbouring pixels of similar colour are pulled to the same label (the relaxed Potts /
 * dense-CRF regulariser evaluated as a loss: Tang et al., "On Regularized Losses for Weakly-supervised CNN Segmentation",
 * ECCV 2018; the local-window form of Obukhov et al., "Gated CRF Loss", 2019).  Not in the reference.  Meant as a term beside a
 * supervised loss (`cross_entropy+0.1*potts`).  Per image of H x W pixels, z the logits, p = sigmoid(z), I the frame as the
 * engine received it (3 channels, any offset: only differences are used), window radius r taps, dilation d; the neighbours
 * N(i) of pixel i are the pixels i + d (dy, dx), dy, dx in [-r, r], (dy, dx) != (0, 0), inside the frame:
 *   k_ij = exp(-d^2 (dy^2 + dx^2) / (2 sigma_xy^2)) exp(-|I_i - I_j|^2 / (2 sigma_rgb^2))
 *   S_i = sum_{j in N(i)} k_ij;   M_i = sum_{j in N(i)} k_ij p_j;   E = sum_i p_i (S_i - M_i);   Z = sum_i S_i
 * Every pair counts once in each direction, so E holds p_i (1 - p_j) + p_j (1 - p_i) per pair.  Image loss = E / Z, 0 when
 * Z = 0 (a one-pixel image, kernels that underflow); loss = the mean over the images.  Window and kernel are symmetric, so
 *   dL/dz_i = (S_i - 2 M_i) p_i (1 - p_i) / (Z images).
 * THE TERM READS NO TARGET: `masks` are accepted and not read, the void label changes nothing, and void pixels receive this
 * term's gradient like every other pixel -- that is its purpose: under eval_online_adapt.min_prop = [lo, hi] the band around
 * the contour is void for every other loss, and this term is what spreads the labelled pixels into it along the frame's edges.
 * A NaN logit makes the loss NaN.
 * Limits: r in [1, 7], d in [1, 4], r d <= 16 (the CRF's, so its table size fits), the sigmas finite and > 0, sides <= 4096.
 * Engine defaults: r = 3, d = 2, sigma_xy = r d, sigma_rgb = 0.1 with colours in units of the frame's [0, 1] range --
 * Obukhov's values rescaled; they are UNTUNED and no J&F figure exists.
 * The frame is the engine's copy of the last forward's input (kept for the stem's weight gradient), so the kind is evaluated
 * on the logits of the last forward only: by eosvos_loss / eosvos_loss_ignore / eosvos_loss_sum (at most one such term) and
 * the fused entry points.  eosvos_loss_tensors* and eosvos_loss_sum_tensors carry no frames and refuse the kind; on caller
 * tensors use eosvos_potts_loss.  An evaluation on an engine that has run no forward fails and leaves no gradient.
 * Three launches (the stencil over 32 x 8 pixel tiles, which writes the unscaled gradient and one partial of E and of Z per
 * tile; the fixed-order sum of the partials; the scaling of the gradient), no atomics: loss and gradient are bit-identical
 * from run to run.  Scratch: two words per tile and one per image, from the arena of the evaluation-stage entry points. */
#define EOSVOS_LOSS_POTTS 12            /* (11 is unassigned, like 7) */
/* Window radius, dilation and sigmas of EOSVOS_LOSS_POTTS for every later evaluation on this engine; 0 for any of the four
 * selects its default (3, 2, radius * dilation, 0.1).  Out of the limits above (negative or non-finite sigmas included): an
 * error, nothing changes. */
int eosvos_set_loss_potts(eosvos_engine* e, int window, int dilation, float sigma_xy, float sigma_rgb);
/* The pairwise loss on caller tensors with their frames: `images` (1 .. 65535) maps of height x width logits, each side in
 * [1, 4096], and frames fp32 [image][3][height][width]; DEVICE pointers.  0 for window, dilation or a sigma selects the
 * default above (the engine's own settings are not used).  The loss goes to loss_out (a device float), the gradient to
 * dlogits_out, which may be null (none is formed).  The same kernel body as on the engine, which reads its padded copy of the
 * frames through another accessor: the same frames and logits give the same bits either way.  Bad arguments return non-zero
 * before any launch: the outputs stay untouched. */
int eosvos_potts_loss(eosvos_engine* e, const float* logits, const float* frames, int images, int height, int width, int window,
                      int dilation, float sigma_xy, float sigma_rgb, float* loss_out, float* dlogits_out);
/* Topology-aware centreline loss, `cldice`: the soft centreline Dice of Shit et al., "clDice -- a Novel Topology-Preserving Loss
 * Function for Tubular Structure Segmentation" (CVPR 2021).  Not in the reference.  No other kind sees connectivity: a cut
 * through a thin part removes skeleton and costs far more here than the same number of pixels shaved off a blob's edge.  Meant
 * as a term beside a region loss (`dice+0.5*cldice_5`).  Per image of H x W pixels, z the logits, y the targets in [0, 1], v
 * the void label, V = {y != v}, p = sigmoid(z).  Every window is clipped to the frame and ranges over pixels of V only; a void
 * pixel is in no window, no sum and no ranking.  For a map x (p, or y), x_0 = x, and the levels j = 0 .. k (k the depth):
 *   1. v_j(i) = the first minimum of x_j over (up, centre, down);  h_j(i) = the first minimum over (left, centre, right);
 *      x_{j+1}(i) = min(v_j, h_j);  o_j(i) = the first maximum of x_{j+1} over the 3 x 3 window in row-major order;
 *      d_j(i) = max(x_j(i) - o_j(i), 0).
 *   2. u = 1, then u = u (1 - d_j) for j = 0 .. k in ascending order, every difference and product rounded on its own;
 *      S(x) = 1 - u: the published recurrence skel + relu(delta - skel delta) in closed form.  The selections are exact, so the
 *      numpy float32 expression reproduces the x_j and S planes bit for bit.
 *   3. Tp = (sum_V S(p) y + 1) / (sum_V S(p) + 1);  Ts = (sum_V S(y) p + 1) / (sum_V S(y) + 1);  image loss =
 *      1 - 2 Tp Ts / (Tp + Ts), 0 without a valid pixel;  loss = the mean over the images.  An empty or a full target is no
 *      special case; a NaN logit at a valid pixel makes the loss NaN.
 *   4. The gradient follows the selections (torch's CPU rules for the published max_pool2d / torch.min form): a window routes to
 *      its first extremum in row-major order; min(v, h) routes to v's pixel if v < h, to h's if h < v, half to each if v = h.
 *      S(y) carries none.  With Bq = sum_V S(p) + 1, Sy = sum_V S(y) + 1, cP = -2 Ts^2 / (Tp + Ts)^2, cS = -2 Tp^2 / (Tp + Ts)^2:
 *      g_S(i) = cP (y_i - Tp) / Bq;  Gd_j(i) = [d_j(i) > 0] g_S(i) prod_{m != j} (1 - d_m(i)), the product in ascending m from 1;
 *      T_{k+1}(q) = -sum_{i in N3x3(q), arg o_k(i) = q} Gd_k(i);
 *      T_j(q) = Gd_j(q) + sum_{i in cross(q)} w_j(i -> q) T_{j+1}(i) - [j >= 1] sum_{i in N3x3(q), arg o_{j-1}(i) = q} Gd_{j-1}(i),
 *      w in {0, 1/2, 1} from the erosion's routing, both gathers in row-major order of i, the cross first;
 *      dL/dz = (T_0 + cS S(y) / Sy) p (1 - p) / images; exactly +0 at a void pixel, whose logit never reaches the result.
 * The depth k is per engine (eosvos_set_loss_cldice), a whole number in [1, 16]; by default clamp((min(H, W) + 48) / 96, 1, 16)
 * (integer division), 5 at 480 x 854.  It is untuned: no J&F figure exists for it.  The kind needs the frame's shape, as the
 * boundary kinds and the surface loss do: through eosvos_loss* and the fused entry points an image is the engine's H x W;
 * eosvos_loss_tensors* accept n == H * W only, as one image; frames of at most 4096 pixels a side.  3 k + 8 launches (p; an
 * erosion and a dilation per level for p and y together; the partial sums; their fixed-order fp64 reduction; the Gd_j; one
 * backward launch for T_{k+1} and one per level, the last writing dL/dz), no atomics: loss and gradient are bit-identical from
 * run to run.  The first use allocates a scratch of 6 (k + 1) + 24 bytes per pixel of the engine's largest batch (d_j in fp32
 * and a 16-bit routing code per level; p, S(y), two planes each for x and T) plus 40 KB per image; a deeper evaluation later
 * replaces it by a larger one.  A failed allocation is reported and leaves the engine usable with the other kinds. */
#define EOSVOS_LOSS_CLDICE 13           /* (14 and up are unknown) */
/* The depth of EOSVOS_LOSS_CLDICE for every evaluation on this engine: 1 .. 16, or 0 for the frame-size default; anything
 * else is an error and changes nothing.  Per engine, like the boundary radius. */
int eosvos_set_loss_cldice(eosvos_engine* e, int depth);
/* The centreline loss on caller tensors with an explicit shape: `images` (1 .. 65535) maps of height x width, each side in
 * [1, 4096], DEVICE pointers.  depth 1 .. 16, or 0 for this shape's default; `ignore`: null, or a HOST pointer to the void
 * label.  The loss goes to loss_out (a device float), the gradient to dlogits_out, which may be null (none is formed).  The
 * scratch comes from the arena of the evaluation-stage entry points, under its 512 MB cap per call.  Bad arguments return
 * non-zero before any launch: the outputs stay untouched. */
int eosvos_cldice_loss(eosvos_engine* e, const float* logits, const float* masks, int images, int height, int width, int depth,
                       const float* ignore, float* loss_out, float* dlogits_out);
/* Rules 1 and 2 alone, with the arguments and limits of eosvos_cldice_loss: out [image][H][W] fp32 = S of `maps` (values in
 * [0, 1]), 0 at void pixels, which are where `masks` -- null: the maps themselves -- equal the void label.  The debugging and
 * visualisation view of the selection chain. */
int eosvos_soft_skeleton(eosvos_engine* e, const float* maps, const float* masks, int images, int height, int width, int depth,
                         const float* ignore, float* out);
/* eosvos_loss_bce for any kind (the forms of one evaluation, see there). */
int eosvos_loss(eosvos_engine* e, int kind, const float* masks, int batch, float* loss_out);
/* The value of the last loss evaluated by eosvos_loss* / eosvos_finetune_step / eosvos_meta_grad*, copied to a DEVICE
 * float on the engine's stream without synchronising (several engines in flight on one GPU: concurrent meta tasks). */
int eosvos_last_loss(eosvos_engine* e, float* loss_out);
/* Loss used by the fused entry points eosvos_finetune_step / eosvos_meta_grad (`loss_func` of
 * the run config, cfgs/meta.yaml:68; default EOSVOS_LOSS_BCE = the north-star path). */
int eosvos_set_loss(eosvos_engine* e, int kind);
/* Stand-alone BCE-with-logits mean over n elements of caller tensors (compute_loss with
 * `batch_average: False` per sample, helper_func.py:36-39; run_loader metrics :131-134).
 * dlogits_out may be NULL (engine scratch is used; a pending eosvos_loss_bce gradient is
 * then invalidated). */
int eosvos_bce(eosvos_engine* e, const float* logits, const float* masks, int64_t n,
               float* loss_out, float* dlogits_out);
/* The same for any loss kind: value of `compute_loss(loss_func, ...)` on n elements of caller tensors, e.g.
 * one sample of a batch for `batch_average: False` (run_loader metrics, helper_func.py:131-137;
 * loss_dice.py:33-40, loss_ce.py:26-40).  No gradient is kept; a pending loss gradient is invalidated. */
int eosvos_loss_tensors(eosvos_engine* e, int kind, const float* logits, const float* masks, int64_t n,
                        float* loss_out);
/* ---- void pixels: an ignore label for every loss ------------------------------------------------------------------------
 * A pixel is void iff masks[p] == ignore (compared as floats); `ignore` must be finite and outside [0, 1], anything else is
 * rejected before a launch.  A void pixel is in no sum, no count and no ranking, its logit is never read into the result (it
 * may be NaN / inf) and its gradient is exactly +0.  With V the valid pixels of the set:
 *   EOSVOS_LOSS_BCE                  sum_V bce / |V|                                   (helper_func.py:32-37)
 *   EOSVOS_LOSS_DICE                 the three sums of networks/loss_dice.py:25-30 over V, smooth = 1
 *   EOSVOS_LOSS_BCE_DICE             bce_V - log(1 - dice_V)                            (helper_func.py:45-54)
 *   EOSVOS_LOSS_CLASS_BALANCED_BCE   num_labels_pos / _neg, loss_pos / _neg of networks/loss_ce.py:42-53 over V; the two
 *                                    trailing divisions stay those of the tensor's full shape (OSVOS void-pixel weighting)
 *   EOSVOS_LOSS_LOVASZ_HINGE[_FLAT]  the void pixels are removed before the ranking, per image or from the whole batch
 *                                    (`ignore=`, flatten_binary_scores, networks/loss_lovasz.py:78-126)
 * An empty V gives loss 0 and an all-zero gradient (an all-void image adds 0 to the per-image mean, loss_lovasz.py:101-103).
 * Without a void pixel in `masks` the result has the bits of eosvos_loss / eosvos_loss_tensors.
 * eosvos_loss_ignore leaves dL/dlogits for eosvos_backward_step exactly as eosvos_loss does. */
int eosvos_loss_ignore(eosvos_engine* e, int kind, const float* masks, int batch, float ignore, float* loss_out);
/* eosvos_loss_tensors with a void label (networks/loss_lovasz.py:78-126 and the loss files above): the n elements are one set;
 * no gradient is kept, a pending loss gradient is invalidated. */
int eosvos_loss_tensors_ignore(eosvos_engine* e, int kind, const float* logits, const float* masks, int64_t n,
                               float ignore, float* loss_out);
/* The fused entry points eosvos_finetune_step / eosvos_meta_grad[_ex] evaluate their loss (eosvos_set_loss) with the void label
 * `ignore` (networks/loss_lovasz.py:78-126) while `on` != 0.  Per engine, off by default; an engine that shares another's state
 * (eosvos_alias_state) does not take its setting over. */
int eosvos_set_loss_ignore(eosvos_engine* e, int on, float ignore);
/* ---- weighted sums of the kinds above (`0.5*lovasz_hinge+boundary_f`) ---------------------------------------------------
 * A sum is a list of 1 .. EOSVOS_LOSS_MAX_TERMS kinds with weights; it needs no kind id of its own.  With terms
 * i = 0 .. n-1 in the order given, L_i / d_i the loss and the gradient kind i produces alone (its own rule for what a set is,
 * its own void-pixel handling, its own limits) and w_i its weight:
 *   acc = w_0 (x) x_0;   acc = acc (+) (w_i (x) x_i)   for i = 1 .. n-1        x = the loss value, and per element the gradient
 * where every (x) and every (+) is an fp32 operation rounded on its own -- never a fused multiply-add -- so that float32
 * arithmetic on the host reproduces loss and gradient bit for bit (`loss_sum.combine_host`).  A void pixel keeps gradient +0:
 * (w (x) +0) (+) +0 = +0; a NaN loss in any term makes the sum NaN.
 * Checks, before any launch: 1 <= n_terms <= 4, every kind valid, no kind twice, not both boundary kinds (they share the
 * engine's radius), every weight finite and > 0.  The terms are evaluated by their own launches, unchanged, into a gradient
 * slice of the largest batch's H * W floats each, then one streaming launch combines them (16-byte accesses, no atomics; bit-
 * identical from run to run like its terms).  The slices and every term's own scratch are allocated when a sum is set or first
 * used; a failed allocation is reported and leaves the engine usable with single kinds.  A term fails as it fails alone, and a
 * failed term fails the sum.  The existing 1:1 kinds EOSVOS_LOSS_BCE_DICE and EOSVOS_LOSS_BCE_AND_BOUNDARY_F keep their own
 * kernels and bits; they may be terms.  The weights are untuned: no J&F figure exists for any sum. */
#define EOSVOS_LOSS_MAX_TERMS 4
/* The sum becomes the loss of eosvos_finetune_step / eosvos_meta_grad[_ex]; eosvos_set_loss returns the engine to a single
 * kind, eosvos_set_loss_ignore applies to both.  Per engine, like eosvos_set_loss. */
int eosvos_set_loss_sum(eosvos_engine* e, int n_terms, const int* kinds, const float* weights);
/* The term-list form of eosvos_loss / eosvos_loss_ignore.
 * The sum on the logits of the last forward (eosvos_loss's rules: the Lovasz hinge and the bootstrapped BCE per image, the
 * boundary kinds per frame); `ignore_on` selects the void label `ignore`.  Leaves dL/dlogits for eosvos_backward_step. */
int eosvos_loss_sum(eosvos_engine* e, int n_terms, const int* kinds, const float* weights, const float* masks, int batch,
                    int ignore_on, float ignore, float* loss_out);
/* The term-list form of eosvos_loss_tensors[_ignore].
 * The sum on n elements of caller tensors (DEVICE pointers), the n elements one set for every term as in eosvos_loss_tensors;
 * n may not exceed the largest batch's pixels, and a boundary term accepts n == H * W only.  The gradient goes to dlogits_out
 * (any 4-byte alignment) or, when that is NULL, to the engine's own scratch (a pending loss gradient is then invalidated).
 * With one term of weight 1 this is that kind's value and gradient, bit for bit. */
int eosvos_loss_sum_tensors(eosvos_engine* e, int n_terms, const int* kinds, const float* weights, const float* logits,
                            const float* masks, int64_t n, int ignore_on, float ignore, float* loss_out, float* dlogits_out);
/* The unweighted term values L_i of the last sum evaluated on this engine (eosvos_loss_sum*, or a fused entry point under
 * eosvos_set_loss_sum), copied to EOSVOS_LOSS_MAX_TERMS DEVICE floats on the engine's stream without synchronising; the
 * entries past that sum's n_terms, which goes to the HOST int n_terms_host (may be NULL), are unspecified.  An error before the
 * first sum. */
int eosvos_last_loss_terms(eosvos_engine* e, float* out, int* n_terms_host);
/* Pseudo-label targets of online adaptation with an uncertainty band (the thresholding of evaluate.py:231-240, whose void
 * label the losses above skip, networks/loss_lovasz.py:78-126): for n_frames probability maps of n_pix pixels,
 * targets_out = 1 where p >= hi, 0 where p < lo, `ignore` between (0 <= lo < hi <= 1, n_frames <= 1024).  n_pos_host (may be
 * NULL: nothing waits) receives the number of 1s of each frame after one synchronisation. */
int eosvos_propagation_targets(eosvos_engine* e, const float* probs, int n_frames, int64_t n_pix, float lo, float hi,
                               float ignore, float* targets_out, int64_t* n_pos_host);
/* autograd.grad + theta <- theta - lr (.) grad (meta_optim.py:177-214,
 * meta_model.py:78-80), using the gradient left by eosvos_loss_bce.
 * accumulate != 0 additionally adds the step's gradients into the task's sum_k g_k
 * (meta-training, see eosvos_meta_grad). */
int eosvos_backward_step(eosvos_engine* e, int accumulate);
/* forward + loss + backward + update in one call; loss_host may be NULL (no sync). */
int eosvos_finetune_step(eosvos_engine* e, const float* images, const float* masks, int batch,
                         int accumulate, float* loss_host);
/* Gradient of the last backward w.r.t. the trainables, flat OIHW (for parity tests); the
 * engine only materialises it after eosvos_keep_grads(e, 1) (one extra 161 MB write/step). */
int eosvos_keep_grads(eosvos_engine* e, int on);
int eosvos_get_grads(eosvos_engine* e, float* flat_grads_out);
/* Read-only copy of the gradient sum of the accumulating steps since eosvos_meta_task_begin (the `gsum` eosvos_meta_grad
 * multiplies with the meta frame's gradient), flat OIHW as eosvos_get_grads, zeros for the frozen tensors (for the per-link
 * tests).  Fails without eosvos_meta_task_begin; changes nothing in the engine. */
int eosvos_debug_gsum(eosvos_engine* e, float* flat_gsum_out);

/* ---- inference (helper_func.py:131-142, evaluate.py:322-326) ----------------------- */
/* probs = sigmoid(model(images)[-1]); probs_out B x 1 x H x W.  An inference forward keeps no ReLU masks: a loss +
 * backward step must follow eosvos_forward / eosvos_finetune_step, not this call (eosvos_backward_step fails otherwise). */
int eosvos_infer(eosvos_engine* e, const float* images, int batch, float* probs_out);
/* labels[p] = 0 if max_o probs[o][p] < 0.5 else argmax_o + 1.  probs: n_obj x H*W. */
int eosvos_merge_labels(eosvos_engine* e, const float* probs, int n_obj, int64_t n_pix,
                        uint8_t* labels_out);

/* ---- test-time augmentation: mirrored and rescaled views averaged in probability space ---------
 * (the test-time ensemble of the OSVOS / OnAVOS family; the reference scores one view, helper_func.py:131-142.)
 * One frame's prediction = sum over views of weight_v * sigmoid(resize_to_frame(unmirror(logits_v))), weights summing
 * to 1, so the accumulator IS the probability map (no finishing pass; eosvos_merge_labels reads it as it is).
 * Per view: eosvos_resize_frames (views of another size) -> eosvos_infer_view on the engine of that size ->
 * eosvos_tta_accumulate. */
/* Forward only, in the inference mode of eosvos_infer (no ReLU masks kept: no backward step may follow); the logits
 * stay in the engine.  mirror != 0 feeds the frame mirrored left-right: the layout pass writes source column x to
 * column W-1-x, the padded input is byte for byte that of the flipped frame and no flipped copy is made.  The launch
 * plan (eosvos_plan_fingerprint) is that of eosvos_infer. */
int eosvos_infer_view(eosvos_engine* e, const float* images, int batch, int mirror);
/* acc (batch x H x W) = (first ? 0 : acc) + weight * sigmoid(R(U(logits))) in one launch, where logits (batch x h x w)
 * are those of e_view's last forward (h, w must be e_view's frame size), U un-mirrors them when mirror != 0 and R is
 * torch.nn.functional.interpolate(mode='bilinear', align_corners=False) to H x W: source coordinate
 * max(0, (in / out) * (o + 0.5) - 0.5) in fp32, upper neighbour clamped at the edge.  h == H and w == W takes the
 * logit itself (weight 1, first 1 then gives eosvos_infer's bits).  One writer per pixel: deterministic.  Runs on
 * e_view's stream; acc is the caller's. */
int eosvos_tta_accumulate(eosvos_engine* e_view, int h, int w, int batch, int mirror, float weight, int first, float* acc,
                          int H, int W);
/* dst (B x C x h_out x w_out) = bilinear align_corners=False resize of src (B x C x h_in x w_in), the rule above (the
 * engine's resize kernel on B * C one-channel planes); any sizes >= 1, not tied to e's frame size.  The index tables
 * of a size pair are built on first use and stay with e. */
int eosvos_resize_frames(eosvos_engine* e, const float* src, int B, int C, int h_in, int w_in, int h_out, int w_out,
                         float* dst);

/* ---- data augmentation (data/custom_transforms.py:9-92,189-213; helper_func.py:255-261) --- */
/* One RandomHorizontalFlip + RandomScaleNRotate application on the device: dst = cv2.warpAffine(
 * cv2.flip(src) if flip else src, cv2.getRotationMatrix2D((W/2, H/2), rot_deg, scale), (W, H),
 * flags = INTER_NEAREST (labels, `:46-47`) | INTER_CUBIC (frames, `:48-49`)), border constant 0.
 * src/dst: channels x H x W planes (H, W of the engine).  The caller draws flip / rot / scale with the
 * reference's `random` sequence and repeats the label warp while it lost the object (`:53-78`):
 * nonzero_host (may be NULL; synchronises) receives the number of non-zero output elements.
 * OpenCV is not part of the reference tree; the algorithm restated is opencv-python 4.1
 * (requirements.txt:63) imgproc/imgwarp.cpp: inverse matrix, 10-bit fixed-point coordinates,
 * 1/32-pixel bicubic (a = -0.75) table. */
#define EOSVOS_INTER_NEAREST 0
#define EOSVOS_INTER_CUBIC 2
int eosvos_warp_affine(eosvos_engine* e, const float* src, int channels, int flip, double rot_deg,
                       double scale, int interp, float* dst, int* nonzero_host);
/* The same warp for a frame of any size (round 5): the videos of a meta-batch reach the network at their native sizes (no resize
 * in the reference's data layer), so the augmentation of a task's frames cannot be tied to one engine's frame size.  `e` lends
 * its stream and coefficient table only. */
int eosvos_warp_affine_hw(eosvos_engine* e, const float* src, int channels, int height, int width, int flip, double rot_deg,
                          double scale, int interp, float* dst, int* nonzero_host);

/* ---- DAVIS-2017 evaluation counts (evaluate.py:345-359 -> eval_davis_seq, helper_func.py:444-458) ---------------- */
/* The integer counts behind the `davis` package's region (J) and contour (F) measures, for every frame of a sequence and
 * every object o in 1..n_obj, with P = (pred == o), G = (gt == o) (label values above n_obj belong to no object):
 * counts_out[(f * n_obj + o - 1) * 6 + k], k = 0 inter |P & G|, 1 union |P | G|, 2 n_fg |bmap(P)|, 3 n_gt |bmap(G)|,
 * 4 fg_match |bmap(P) & dilate(bmap(G))|, 5 gt_match |bmap(G) & dilate(bmap(P))|.  bmap is seg2bmap (boundary pixels), dilate
 * a binary dilation by the disk dx^2 + dy^2 <= bound_pix^2 (outside the frame is 0).  Ratios and statistics are the
 * caller's (data.sequence_measures).  pred / gt: device uint8 label maps [n_frames][height][width] of any size (`e` lends
 * its stream and scratch memory only); counts_out: host memory.  Synchronises the engine's stream.  Rejected without a
 * launch: a null pointer, bound_pix outside [0, 63], n_obj outside [1, 255], width > 4096. */
int eosvos_davis_counts(eosvos_engine* e, const uint8_t* pred, const uint8_t* gt, int n_frames, int height, int width, int n_obj,
                        int bound_pix, int64_t* counts_out);

/* ---- local dense-CRF refinement of the merged label maps (stands beside src/util/evaluate.py:322-326) ----------- */
/* The reference merges the per-object probabilities by threshold + arg-max (`:322-326`, eosvos_merge_labels) and never
 * looks at the frame.  This is the appearance-aware form of that step the OSVOS family uses (OnAVOS, DeepLab v1/v2): the
 * locally connected dense CRF -- mean field with Gaussian position / colour kernels on a dilated (2r+1)^2 window, the
 * "ConvCRF" restriction of Kraehenbuehl-Koltun.  An opt-in extension; with iterations = 0 it IS eosvos_merge_labels.
 * Per frame, labels l = 0 (background), 1..n_obj, p_o = clamp(probs[o - 1], 0, 1) (the train frame holds 2 * GT):
 *   unary     m = max_o p_o; s_0 = 1 - m, s_o = p_o; s_l <- max(s_l, 1e-5); q0_l = s_l / sum_l s_l; U_l = -log q0_l
 *   window    offsets D = dilation * (dy, dx), dy, dx in [-radius, radius], (dy, dx) != (0, 0), neighbours inside the frame only
 *   kernels   k_a(p, q) = exp(-|D|^2 / (2 theta_alpha^2) - |I_p - I_q|^2 / (2 theta_beta^2))   (squared difference summed
 *             over the 3 channels; only colour differences enter, so the frames' normalisation does not matter)
 *             k_s(p, q) = exp(-|D|^2 / (2 theta_gamma^2))
 *   norms     N_a(p) = sum_q exp(-|D|^2 / (2 theta_alpha^2)), N_s(p) = sum_q k_s: position only (they differ from the interior
 *             constant only near the border), deliberately not sum_q k_a, which underflows to 0 in fp32 at a pixel unlike all
 *             its neighbours; a term whose normaliser is 0 (no neighbour inside the frame) contributes 0
 *   update    Q^0 = q0; t = 1..iterations, all of Q^{t-1} read before any of Q^t is written:
 *             msg_l(p) = w_appearance * sum_q k_a Q^{t-1}_l(q) / N_a(p) + w_smooth * sum_q k_s Q^{t-1}_l(q) / N_s(p)
 *             Q^t(p) = softmax_l(-U_l(p) + msg_l(p))        (Potts compatibility; the label-independent part cancels)
 *   decision  0 if Q^T_0 > max_o Q^T_o (strict), else the lowest o attaining the maximum.  iterations = 0 takes
 *             eosvos_merge_labels' decision (max_o probs < 0.5 ? 0 : first arg-max + 1) on probs as given, bit for bit:
 *             1 - m > m <=> m < 0.5 holds in fp32 without exception, and the clamp moves no decision on [0, 1] and 2 * GT.
 * images [n_frames][3][height][width], probs [n_frames][n_obj][height][width], labels_out [n_frames][height][width],
 * q_out (may be NULL) receives Q^T as [n_frames][n_obj + 1][height][width]; all device memory, frames of any size (`e`
 * lends its stream and scratch memory only).  Asynchronous on the engine's stream.  Launches: one to prepare (unary, Q^0),
 * one per iteration (the last one also decides); no matrix kernel, eosvos_plan_fingerprint is untouched.  One writer per
 * element and a fixed summation order: two calls give the same bits, and a frame's result does not depend on the frames
 * beside it.  Scratch: 3 * n_frames * (n_obj + 1) * height * width floats (none with iterations = 0), allocated on first
 * use, growing only, at most 512 MB per call -- a call that needs more is rejected (pass fewer frames per call); a
 * failed allocation is reported and leaves the engine usable.
 * Rejected without a launch: a null pointer (q_out excepted), height or width < 1, n_obj outside [1, 255], iterations
 * outside [0, 20], radius outside [1, 7], dilation outside [1, 4], radius * dilation > 16, a weight < 0 or non-finite,
 * a theta <= 0 or non-finite, more than 65535 frames.  The customary defaults (iterations 5, radius 5, dilation 2,
 * w_appearance 10, w_smooth 3, theta_alpha 8 px, theta_beta 0.05 on [0, 1] RGB, theta_gamma 3 px: eosvos_amd/crf.py)
 * are pydensecrf's rescaled to this normalisation and are not tuned on data. */
int eosvos_crf_labels(eosvos_engine* e, const float* images, const float* probs, int n_frames, int n_obj,
                      int height, int width, int iterations, int radius, int dilation, float w_appearance,
                      float w_smooth, float theta_alpha, float theta_beta, float theta_gamma,
                      uint8_t* labels_out, float* q_out);

/* ---- connected-component clean-up of the merged label maps (after src/util/evaluate.py:322-326 and the CRF) ------ */
/* The reference has no such step; the OSVOS family removes confident blobs on look-alikes after the fact (small components,
 * all but the dominant component, components that do not continue the previous frame's mask).  An opt-in extension.
 * labels: device uint8 maps [n_frames][height][width] of one sequence in frame order; 0 is background, every non-zero value
 * an object label (no object count is needed).
 *   components  two pixels of a frame are connected when they hold the same non-zero label and are neighbours under
 *               `connectivity`: 4 = edge neighbours, 8 = edge and corner neighbours.  Pixels with different labels never
 *               connect, frames never connect.  The id of a component is 1 + min(y * width + x) over its pixels, background
 *               has id 0: the id map is unique.
 *   filter      for frame f in ascending order, for every label o present in it:
 *     1. gate (g = `gate` in 0..63, 0 = off).  R is the FILTERED output of frame f - 1; for the first frame of the call R is
 *        `prev` (may be NULL: no R).  The gate is active for (f, o) when g > 0, R exists and R has at least one pixel equal
 *        to o.  When active, a component is a candidate only if one of its pixels p has a pixel q with R[q] == o and
 *        max(|px - qx|, |py - qy|) <= g (Chebyshev distance; outside the frame R counts as 0).  When inactive, every
 *        component of o is a candidate.
 *     2. area rules over the candidates of (f, o) only; A = a candidate's pixel count, Amax = the largest candidate count of
 *        (f, o).  The candidate is kept iff  A >= min_area,  and  A * 65536 >= rel_q16 * Amax  (64-bit integers; rel_q16 =
 *        round(min_rel_area * 65536) with min_rel_area in [0, 1], computed once by the caller),  and, if largest_only,
 *        A == Amax and among those the candidate has the smallest id.
 *     3. pixels of components that are not kept become 0, everything else is copied.
 *   keep        (HOST memory, n_frames flags, may be NULL) frames flagged there -- the train frames, whose map is the seeded
 *               ground truth -- are copied unchanged; they still serve as R of the frame after them.
 * eosvos_label_components writes the id map (device int32 [n_frames][height][width]); eosvos_filter_components writes the
 * filtered maps to `out` (device, not overlapping `labels`) and, if removed_out (HOST memory, n_frames values) is not NULL,
 * the number of pixels zeroed per frame -- it then synchronises the engine's stream; otherwise both are asynchronous on
 * the engine's stream.  `e` lends its stream and scratch memory only; frames of any size within the limits.
 * Launches (csrc/ccl_kernels.hip): union-find labelling in three (64 x 16 tiles in LDS, tile seams by atomicMin, flatten
 * + areas with one atomic per tile-local root); then with the gate per frame gate flags / largest candidate / apply, without
 * it one such pair for all frames.  No launch is cooperative and no workgroup waits for another; parent[i] <= i holds at
 * all times, so every loop walks strictly downward and ends.  Integer arithmetic only: results are exact and independent
 * of arrival order.  Scratch: 8 bytes per pixel for the id map, 17 bytes per pixel (+ 2312 per frame) for the filter,
 * allocated on first use, growing only, at most 512 MB per call -- a call that needs more is rejected (pass fewer
 * frames per call and the last filtered frame as `prev` of the next).
 * Rejected without a launch: a null pointer (prev, keep, removed_out excepted), height or width < 1 or > 4096,
 * height * width >= 2^24, connectivity not 4 or 8, gate outside [0, 63], min_area < 0, rel_q16 outside [0, 65536], more
 * than 65535 frames. */
int eosvos_label_components(eosvos_engine* e, const uint8_t* labels, int n_frames, int height, int width, int connectivity,
                            int32_t* ids_out);
int eosvos_filter_components(eosvos_engine* e, const uint8_t* labels, int n_frames, int height, int width, int connectivity,
                             int min_area, int rel_q16, int largest_only, int gate, const uint8_t* prev, const uint8_t* keep,
                             uint8_t* out, int64_t* removed_out);

/* ---- hole filling of the merged label maps (after the component filter) ------------------------------------------- */
/* The reference has no such step; the OSVOS family fills the background islands a few sub-threshold pixels leave inside an
 * object.  Real holes (a bicycle frame, the gap between legs) are in the ground truth, so a hole is filled only if it is small
 * and most of it was object in the previous frame's FILLED map -- the chain the component filter's gate uses, anchored at the
 * train frame.  An opt-in extension.
 * labels: device uint8 maps [n_frames][height][width] of one sequence in frame order; 0 is background, every non-zero value
 * an object label.
 *   1. background components  two pixels of a frame that hold 0 are connected when they are neighbours under the DUAL of
 *        `connectivity`: connectivity 8 (objects join over corners) = the background joins over edges only; connectivity 4 =
 *        the background joins over edges and corners.  Frames never connect.
 *   2. holes  a background component is a hole when none of its pixels lies on the frame border (x = 0, y = 0, x = width - 1,
 *        y = height - 1).  Its bordering labels are the non-zero labels among the neighbours (under the background's
 *        connectivity) of its pixels.  A hole with exactly one bordering label o is a candidate for o; with two or more it is
 *        left alone; it cannot have none.
 *   3. size  A = the hole's pixel count, S = the number of pixels equal to o in the frame's INPUT map.  The candidate passes
 *        iff  A <= max_area  and  A * 65536 <= rel_q16 * S  (64-bit integers; rel_q16 = round(max_rel_area * 65536) with
 *        max_rel_area in [0, 1], computed once by the caller).
 *   4. previous frame  R is the FILLED output of frame f - 1; for the first frame of the call R is `prev` (may be NULL: no R).
 *        The rule is active for a candidate of o when overlap_q16 = round(prev_overlap * 65536) > 0, R exists and R has a pixel
 *        equal to o.  When active, C = the number of the hole's pixels p with R[p] == o, and the candidate passes iff
 *        C * 65536 >= overlap_q16 * A.  When inactive, it passes.
 *   5. fill  pixels of holes that pass become o, everything else is copied.
 *   6. independence  every decision in a frame is taken on the frame's input map: holes of a frame never influence each other.
 *   7. keep  (HOST memory, n_frames flags, may be NULL) frames flagged there -- the train frames -- are copied unchanged and
 *        still serve as R of the frame after them.
 *   8. off  max_area == 0 or rel_q16 == 0: no hole can pass, every frame is copied.
 * Writes the filled maps to `out` (device, not overlapping `labels`) and, if filled_out (HOST memory, n_frames values) is not
 * NULL, the number of pixels filled per frame -- it then synchronises the engine's stream; otherwise the call is asynchronous
 * on the engine's stream.  `e` lends its stream and scratch memory only; frames of any size within the limits.
 * Launches (csrc/ccl_kernels.hip): the three union-find launches of eosvos_label_components over the zero pixels; a scan (per
 * root: border flag, smallest and largest neighbour label -- one label <=> they are equal -- and the frame's label histogram);
 * with overlap_q16 > 0 per frame in order an overlap count and the apply, without it one apply for all frames.  Integer
 * atomics only: results are exact and independent of arrival order.  No launch is cooperative, no workgroup waits for another.
 * Scratch (shared with the component filter): 24 bytes per pixel (parent, tile count, id, area, record, overlap count as
 * 32-bit words) + 1288 per frame (histogram, pixels filled, labels present) + 264, allocated on first use, growing only, at
 * most 512 MB per call -- a call that needs more is rejected (pass fewer frames per call and the last filled frame as `prev`
 * of the next).
 * Rejected without a launch: a null pointer (prev, keep, filled_out excepted), height or width < 1 or > 4096,
 * height * width >= 2^24, connectivity not 4 or 8, max_area outside [0, 2^24], rel_q16 or overlap_q16 outside [0, 65536], more
 * than 65535 frames. */
int eosvos_fill_holes(eosvos_engine* e, const uint8_t* labels, int n_frames, int height, int width, int connectivity,
                      int max_area, int rel_q16, int overlap_q16, const uint8_t* prev, const uint8_t* keep, uint8_t* out,
                      int64_t* filled_out);

/* ---- SLIC superpixels and the superpixel vote on the merged label maps (between the CRF and the component filter) ----- */
/* The reference has no such step; the OSVOS family snaps its masks to superpixels of the frame ("contour snapping"): each
 * superpixel takes the label that holds its majority, which moves a label boundary onto the image edge it belongs to.  The
 * superpixels are SLIC in its GPU form (gSLIC) restricted to integers.  An opt-in extension; the parameter values shown anywhere
 * are examples, untuned.
 * rgb: device uint8 [n_frames][3][height][width], planar (the caller quantises its frames: eosvos_amd/snap.py `quantise`);
 * labels: device uint8 maps [n_frames][height][width], 0 is background, 1..n_obj are objects.  Frames never interact.  Every
 * quantity is an integer.  S = step, T = iterations, m = compactness.
 *   1. grid  gy = ceil(height / S), gx = ceil(width / S), K = gy * gx clusters per frame; the id of cell (cy, cx) is
 *        cy * gx + cx.  Its initial centre is the pixel (min(cy * S + S / 2, height - 1), min(cx * S + S / 2, width - 1))
 *        (integer division) and that pixel's colour: a centre is five integers (y, x, R, G, B).
 *   2. assign  pixel (y, x) has home cell (y / S, x / S); its candidates are the clusters of the up to nine cells within +-1 of
 *        the home cell that exist in the grid.  D = (dR^2 + dG^2 + dB^2) * S^2 + m^2 * (dy^2 + dx^2) against the candidate's
 *        current centre; the pixel takes the smallest D, ties go to the smaller id.  D < 2^32 under the limits (colour
 *        <= 195075 * 4096; a centre is a mean of pixels of cells within +-1 of its own, so |d| < 3 S and the position gives
 *        <= 2 * 192^2 * 4096): the kernel computes it in unsigned 32 bits.
 *   3. update  per cluster n and the sums of y, x, R, G, B over its pixels (each fits 32 bits: <= (3 * 64)^2 pixels * 4095); a
 *        new centre component is (2 * sum + n) / (2 * n), integer division (round half up); a cluster with n = 0 keeps its
 *        centre.
 *   4. schedule  for t = 1..T: assign; if t < T: update.  The ids are those of the last assign.  No connectivity enforcement:
 *        a cluster may be disconnected, and the vote below is per id.
 *   5. vote  for a cluster c, cnt_c[l] = its pixels with label l <= n_obj, n_c their sum; a pixel with a label > n_obj votes
 *        nowhere and is copied unchanged.  The winner w is the label with the largest count, ties to the smaller label.  If
 *        n_c > 0 and cnt_c[w] * 65536 >= min_share_q16 * n_c (64-bit products; min_share_q16 = round(min_share * 65536) with
 *        min_share in [0, 1], computed once by the caller), every voting pixel of c becomes w; otherwise the pixels of c are
 *        copied.
 *   6. keep  (HOST memory, n_frames flags, may be NULL) frames flagged there -- the train frames -- are copied unchanged.
 * eosvos_superpixels writes the ids of rules 1-4 to ids_out (device int32 [n_frames][height][width]); asynchronous on the
 * engine's stream.  eosvos_snap_labels writes the snapped maps to `out` (device, not overlapping `labels`) and, if changed_out
 * (HOST memory, n_frames values) is not NULL, the number of pixels changed per frame -- it then synchronises the engine's
 * stream; otherwise nothing waits.  `e` lends its stream and scratch memory only; frames of any size within the limits.
 * Launches (csrc/slic_kernels.hip): one init; per iteration but the last a fused assign + accumulate (64 x 16 pixel tiles, the
 * centres of the at most 133 clusters a tile can meet and their accumulators in LDS, one global integer atomic per non-zero
 * accumulator word) and a finish (new centres, sums zeroed); the last assign writes the ids and, for the vote, counts into the
 * K x (n_obj + 1) table (privatised in LDS where the tile's slice fits in 2048 words, else one atomic per wave and distinct
 * target); then one apply per run of frames with the same keep flag.  Integer atomics only: results are exact and independent
 * of arrival order.  No launch is cooperative, no workgroup waits for another.
 * Scratch (shared with the component filter and the hole filler), 32-bit words: eosvos_superpixels 5 + 6 per cluster;
 * eosvos_snap_labels 1 per pixel (ids) + 5 + 6 + (n_obj + 1) per cluster, + 8 bytes per frame (pixels changed) + up to 8 of
 * padding; allocated on first use, growing only, at most 512 MB per call -- a call that needs more is rejected, a single frame
 * included, never truncated (pass fewer frames per call).
 * Rejected without a launch: a null pointer (keep, changed_out excepted), height or width < 1 or > 4096, step outside [4, 64],
 * iterations outside [1, 20], compactness outside [1, 64], n_obj outside [1, 255], min_share_q16 outside [0, 65536], more than
 * 65535 frames. */
int eosvos_superpixels(eosvos_engine* e, const uint8_t* rgb, int n_frames, int height, int width, int step, int iterations,
                       int compactness, int32_t* ids_out);
int eosvos_snap_labels(eosvos_engine* e, const uint8_t* rgb, const uint8_t* labels, int n_frames, int height, int width, int n_obj,
                       int step, int iterations, int compactness, int min_share_q16, const uint8_t* keep, uint8_t* out,
                       int64_t* changed_out);

/* ---- block motion on 8-bit luma and the warp of label maps by it (for the filter's gate and the hole filler's overlap) - */
/* The reference has no such step.  The gate of eosvos_filter_components and the previous-frame rule of eosvos_fill_holes read
 * the previous frame's cleaned map at the same pixel coordinates, which is right only while an object moves less than the gate
 * between two frames; the OSVOS / PReMVOS family propagates the previous mask by motion before it compares.  These two entry
 * points are that step: exhaustive block matching on 8-bit luma and a gather.  The caller passes the warped map as `prev` of
 * the two stages, one frame per call (eosvos_amd/evaluate.py `merge_objects(..., motion=)`).  An opt-in extension; the
 * parameter values shown anywhere are examples, untuned.
 * rgb: device uint8 [n_frames][3][height][width], planar, the frames of one sequence in order (the caller quantises its
 * frames: eosvos_amd/snap.py `quantise`); prev_rgb: device uint8 [3][height][width], the frame before the first, or NULL.
 * Every quantity is an integer.  B = block, R = radius.
 *   1. luma  Y = (77 R + 150 G + 29 B + 128) >> 8, a uint8.
 *   2. blocks  by = ceil(height / B), bx = ceil(width / B); block (j, i) covers rows [jB, min(jB + B, height)) and columns
 *        [iB, min(iB + B, width)), n = its pixel count: blocks at the lower and right border are smaller, and a frame smaller
 *        than one block is one partial block.
 *   3. candidates  for frame f against frame f - 1, a displacement (dy, dx) with |dy|, |dx| <= R is valid for a block when the
 *        whole block, shifted by it, lies inside the frame.  (0, 0) is always valid.
 *   4. cost  cost(d) = sum over the block of |Y_f(y, x) - Y_{f-1}(y + dy, x + dx)|, plus bias * n for d != (0, 0): the bias keeps
 *        flat regions at rest.
 *   5. choice  the valid candidate that is smallest under the lexicographic order (cost, dy^2 + dx^2, dy, dx).  It packs into
 *        one 64-bit key, cost << 26 | (dy^2 + dx^2) << 14 | (dy + 32) << 7 | (dx + 32) (cost <= 2 * 65280 < 2^17, then 12 + 7
 *        + 7 bits): a single integer min decides, in whatever order the lanes reduce.
 *   6. output  mv: device int8 [n_frames][by][bx][2], (dy, dx) per block.  Frame 0 of the call is matched against prev_rgb --
 *        that is how a sequence is chunked: pass the last frame of a call as prev_rgb of the next; with NULL it gets zeros.
 *   7. warp  out(y, x) = labels(y + dy, x + dx) with the vector of the pixel's block: the map of frame f - 1 as frame f sees
 *        it.  Rule 3 keeps every read inside the frame; a vector from elsewhere that leaves it is clamped to the border.
 * eosvos_warp_labels: labels, out: device uint8 [n_frames][height][width] (not overlapping); frame n is warped by mv[n].
 * Both are asynchronous on the engine's stream; `e` lends its stream and scratch memory only; frames of any size within the
 * limits.
 * Launches (csrc/motion_kernels.hip): one luma launch (planes with rows padded to four bytes, so a word never straddles rows);
 * one search launch: a workgroup owns 32 x 64 pixels of blocks and stages that tile of Y_f and the window of Y_{f-1} its
 * candidates reach (at most 96 rows x 132 bytes, 0 outside the frame) in LDS, each wave takes blocks in turn, a lane takes a
 * row offset dy and four adjacent dx -- the eight bytes a packed quad-SAD (v_qsad_pk_u16_u8) needs are two aligned words of a
 * window row, one instruction per four bytes of a block row, sums in four 16-bit lanes (16 * 16 * 255 = 65280); blocks cut by
 * the right border take v_alignbyte_b32 and a masked v_sad_u8 per candidate; the wave reduces the key by an integer min;
 * one warp launch.  No atomics; the result does not depend on any order.  No launch is cooperative, no workgroup waits for
 * another.
 * Scratch of eosvos_block_motion (shared with the component filter, the hole filler and the snapping): n_frames + 1 luma
 * planes of height * (width rounded up to 4) bytes; allocated on first use, growing only, at most 512 MB per call -- a call
 * that needs more is rejected, never truncated (pass fewer frames per call).  eosvos_warp_labels takes none.
 * Rejected without a launch: a null pointer (prev_rgb excepted), height or width < 1 or > 4096, block other than 8 or 16,
 * radius outside [1, 32], bias outside [0, 255], more than 65534 (warp: 65535) frames. */
int eosvos_block_motion(eosvos_engine* e, const uint8_t* rgb, const uint8_t* prev_rgb, int n_frames, int height, int width, int block,
                        int radius, int bias, int8_t* mv);
int eosvos_warp_labels(eosvos_engine* e, const uint8_t* labels, const int8_t* mv, int n_frames, int height, int width, int block,
                       uint8_t* out);

/* ---- object-centred zoom pass of the inference path: a second look at a crop around the object ------------------------ */
/* The reference scores each frame once (helper_func.py:131-142).  At output stride 16 a 30-pixel object is two cells of the
 * ASPP input; the OSVOS / PReMVOS family answers small objects with a second look at a crop around them.  These four entry
 * points are that step.  The zoomed view has the frame's own size, so it runs on the live engine (eosvos_infer_view) with the
 * fine-tuned weights in it: what is new is finding the box, cutting the view and putting the result back.  An opt-in extension
 * (eosvos_amd/zoom.py, `eval_zoom`); the parameter values shown anywhere are examples, untuned.
 * Per frame, from its first-pass probabilities p0 (height x width = H x W).  Box arithmetic is in integers only; the two zooms
 * and the margin enter as Q16, zq = round(z * 65536).
 *   1. mask box  my0, my1, mx0, mx1 = the inclusive bounds of {p0 >= threshold} (an fp32 compare), cnt = its size.
 *        cnt < min_pixels: the frame is INVALID.
 *   2. wanted extent  mh = my1 - my0 + 1, mw likewise; pad = ((max(mh, mw) * margin_q16) >> 16) + margin_px;
 *        gh = mh + 2 pad, gw = mw + 2 pad.
 *   3. box size, the frame's aspect  bh = min(H, max(gh, ceil(gw * H / W), ceil(H * 65536 / max_zoom_q16)));
 *        bw = min(W, ceil(bh * W / H)).  bh * min_zoom_q16 > H * 65536: the frame is INVALID (the object is already large, or
 *        a distant false positive has blown the box up).
 *   4. position  y0 = clamp((2 my0 + mh - bh) >> 1, 0, H - bh) with an arithmetic shift; x0 likewise: centred on the mask
 *        box, pushed inside the frame.
 *   5. record  five int32 per frame: valid, y0, x0, bh, bw.  Invalid frames carry 0, 0, 0, H, W.
 * eosvos_zoom_boxes: probs device fp32 [n_frames][H][W] -> boxes device int32 [n_frames][5]; any H, W <= 4096, not tied to e's
 * frame size.  Two launches (csrc/zoom_kernels.hip): a wave per 64-pixel row segment takes the segment's x-range from the
 * lowest and highest set bit of the ballot word and the count from its popcount, the workgroup combines in LDS and issues
 * integer atomicMax / atomicAdd on the frame's record (8 words of the engine's scratch, zeroed by the call itself on the
 * stream); then one thread per frame does steps 2-5.  No float atomics: the result does not depend on any order.  No launch
 * is cooperative, no workgroup waits for another.
 *   6. cut  view = bilinear(frame[:, y0 : y0 + bh, x0 : x0 + bw] -> H x W) with torch's align_corners=False rule applied to
 *        the slice (it clamps at the box edge), scales (float)bh / (float)H and (float)bw / (float)W as in
 *        eosvos_tta_accumulate.  An invalid frame is copied through bit for bit.
 * eosvos_zoom_crop: frames, out device fp32 [B][C][H][W] (not overlapping), one thread per output element; the box is read
 * from device memory, so nothing waits for eosvos_zoom_boxes on the host.
 *   7. score  eosvos_infer_view(e, view, B, mirror) on the live engine.
 *   8. put back  pz = sum over the views of view_weight * sigmoid(bilinear(U(logits), H x W -> bh x bw)), the sigmoid
 *        expression and the resize rule of eosvos_tta_accumulate, U un-mirroring the logits when mirror != 0; defined inside
 *        the box only.  Plain bilinear down-sampling: the logits are a x4 bilinear up-sampling of the decoder's output, so up
 *        to max_zoom 4 point sampling between them loses nothing the network produced.
 * eosvos_zoom_accumulate: reads the logits of e's last forward (H, W are e's frame size) and writes pz (device fp32
 * [batch][H][W]) inside each valid frame's box only: pz = (first ? 0 : pz) + view_weight * ...; everything else keeps its
 * bits.
 *   9. blend  inside the box out = p0 + (weight * f) * (pz - p0), fp32, in this order; outside out = p0.  The ramp is
 *        f = min(1, (d + 1) / (feather + 1)), d the smallest distance in whole pixels to a box side that is NOT on the frame
 *        border (y - y0 counts only when y0 > 0, y0 + bh - 1 - y only when y0 + bh < H, the same for x); no such side, or
 *        feather 0: f = 1.
 * eosvos_zoom_blend: in place on probs_inout (device fp32 [B][H][W]), inside valid boxes only: invalid frames and pixels
 * outside the boxes are not written, their bits stay p0's.
 * All four are asynchronous on the engine's stream and read the boxes from device memory (every consumer clamps a box into the
 * frame before it addresses anything).  The cost of never reading a box on the host: an invalid frame still pays its forward.
 * Rejected without a launch: a null pointer; n_frames, B, C, height or width < 1; height or width > 4096; more than 65535
 * frames; a batch beyond e's (accumulate); threshold outside (0, 1); min_pixels < 1; margin_q16 outside [0, 4 * 65536];
 * margin_px outside [0, 256]; max_zoom_q16 outside [65536, 4 * 65536]; min_zoom_q16 outside [65536, max_zoom_q16]; a
 * non-finite view_weight; weight outside (0, 1]; feather outside [0, 64]. */
int eosvos_zoom_boxes(eosvos_engine* e, const float* probs, int n_frames, int height, int width, float threshold, int min_pixels,
                      int margin_q16, int margin_px, int min_zoom_q16, int max_zoom_q16, int32_t* boxes);
int eosvos_zoom_crop(eosvos_engine* e, const float* frames, const int32_t* boxes, int B, int C, int height, int width, float* out);
int eosvos_zoom_accumulate(eosvos_engine* e, const int32_t* boxes, int batch, int mirror, float view_weight, int first, float* pz);
int eosvos_zoom_blend(eosvos_engine* e, const int32_t* boxes, int B, int height, int width, float weight, int feather,
                      const float* pz, float* probs_inout);

/* ---- lucid first-frame synthesis for the one-shot fine-tune: the object and its background moved independently --------- */
/* The reference's only first-frame augmentation warps the whole frame about its centre (custom_transforms.py), so in every
 * training sample the object sits in the same place relative to its background.  "Lucid data dreaming" (Khoreva et al.) cuts
 * the object out, fills the hole, moves object and background independently and composes them again.  These two entry points
 * are that step; an opt-in extension (eosvos_amd/lucid.py, `eval_lucid`), off by default.  The parameter values shown anywhere
 * are examples, UNTUNED.  frame [C][H][W] fp32, mask [H][W] fp32 (object = mask != 0), height x width = H x W.
 * Plate, the frame with the object removed (once per sequence and object):
 *   1. hole(y, x) = 1 iff a pixel with mask != 0 lies within Chebyshev distance `dilate` inside the frame; known = !hole.
 *   2. level 0 is H x W: v0 = frame where known, else 0; k0 = known.
 *   3. level l + 1 is ceil(H_l / 2) x ceil(W_l / 2): k = the OR of the up to four children (2y + i, 2x + j) inside level l;
 *        v = the sum of the known children's v in the order (0,0), (0,1), (1,0), (1,1), divided by their number, 0 if none is
 *        known.  Levels are built down to 1 x 1 whatever the data: their number depends on (H, W) only, nothing is read back.
 *   4. pull, l = top - 1 .. 0: a pixel with k_l = 0 takes the bilinear sample of the COMPLETED level l + 1 at
 *        ((y + 0.5) / 2 - 0.5, (x + 0.5) / 2 - 0.5): taps floor and floor + 1, both clamped to the level, weights 1/4 and 3/4;
 *        (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11), every operation rounded on its own.
 *        Known pixels keep their value.
 *   5. plate = v0.  Known pixels carry the frame's bits; a frame with no known pixel gives an all-zero plate.  fp32, no
 *        atomics, deterministic; every scratch element a call reads is written by it first (EOSVOS_DEBUG_FILL changes no bit).
 * eosvos_lucid_plate: asynchronous on the engine's stream, 2 + 2 (levels - 1) small launches (csrc/lucid_kernels.hip); the
 * levels above 0 live in the engine's grow-only scratch.  Any H, W <= 4096, not tied to e's frame size.
 * Compose, per sample s with `flip`, the inverse background matrix Bi and the inverse object matrix Oi (2 x 3 doubles each, built
 * and inverted on the host; X = m0 x + m1 y + m2, Y = m3 x + m4 y + m5):
 *   6. output pixel (y, x): xm = flip ? W - 1 - x : x.  Source coordinates in the 10-bit fixed point of eosvos_warp_affine, entry
 *        by entry: Xf = lrint((m1 * y + m2) * 1024) + 16 + lrint((m0 * xm) * 1024), Yf likewise from m4, m5, m3 (16 = the
 *        interpolating round_delta); X = Xf >> 5, Y = Yf >> 5 carry 5 fractional bits.  Evaluated once for Bi, once for Oi.
 *   7. coverage  A = sum over the 2 x 2 bilinear taps at the object coordinates of wy_i * wx_j * [mask(sy + i, sx + j) != 0],
 *        sy = Y >> 5, sx = X >> 5, integer weights (32 - f, f), taps outside the frame 0: an integer in [0, 1024].
 *        label = (A >= 512), alpha = A / 1024, both exact.
 *   8. Bg = the bicubic sample of the plate at the background coordinates, Ob = that of the frame at the object coordinates:
 *        the a = -0.75 table at 1/32 pixel of eosvos_warp_affine, taps (Y >> 5) - 1 .. + 2, taps outside the frame 0, the 16
 *        products value * (cy[i] * cx[j]) added tap by tap, rows first.  Ob is only sampled where A > 0.  image = Ob where
 *        A == 1024, Bg where A == 0, Bg + alpha * (Ob - Bg) otherwise, fp32, every operation rounded on its own.
 *   9. count[s] = the number of labelled pixels of sample s: an integer sum (wave reduction, one integer atomic per wave) on a
 *        record the call zeroes itself on the stream.
 * eosvos_lucid_compose: ONE launch for all n_samples <= 16 samples (one thread per output pixel, the sample in the grid's third
 * dimension).  flips [n] int32 and matrices [n][12] doubles (Bi, then Oi) are HOST arrays copied into the launch's arguments:
 * a queued launch owns everything it reads.  images [n][C][H][W], labels [n][H][W] (0.f / 1.f) on the device, not overlapping
 * the inputs.  counts_host non-null: the counts [n] are copied there and the call waits for the stream (the one host read of a
 * batch attempt); null: nothing waits.  Acceptance, redraws and the batch layout (rules 10-13) are the caller's: lucid.py.
 * Rejected without a launch: a null pointer (counts_host excepted); channels outside [1, 64]; height or width < 1 or > 4096;
 * dilate outside [0, 16]; n_samples outside [1, 16]; a non-finite matrix entry. */
int eosvos_lucid_plate(eosvos_engine* e, const float* frame, const float* mask, int channels, int height, int width, int dilate,
                       float* plate);
int eosvos_lucid_compose(eosvos_engine* e, const float* frame, const float* mask, const float* plate, int channels, int height,
                         int width, int n_samples, const int32_t* flips, const double* matrices, float* images, float* labels,
                         int32_t* counts_host);

/* ---- lucid synthesis with the sequence's other objects as moving layers ------------------------------------------------ */
/* eosvos_lucid_compose moves one object; the train frame's other annotated objects stay in the plate, move rigidly with the
 * background and never cover the target.  Lucid data dreaming proper moves every object on its own over the filled plate, with
 * a depth order: each object's net sees its neighbours as negatives in new places, sometimes in front of it.  An opt-in
 * extension (eosvos_amd/lucid_layers.py, `eval_lucid_layers`), off by default; every value shown anywhere is UNTUNED.
 * frame [C][H][W] fp32; ids [H][W] uint8: 0 = background, 1 = the target, 2 .. M + 1 = the other objects in the order given (a
 * pixel lying in several masks takes the target if it is in the target's mask, else the largest id).
 *  L1. plate     rules 1-5 above on the mask ids != 0: eosvos_lucid_plate, called unchanged.  The hole is the union of all
 *        layered objects grown by `dilate`.
 *  L2. sample    `flip` and Bi as above; a layer count L in [1, 8]; per layer k = 0 .. L - 1, BACK TO FRONT, an id id_k in
 *        [1, 255], distinct within the sample, and an inverse matrix Oi_k.  Coordinates: rule 6 entry by entry, once for Bi and
 *        once per Oi_k.
 *  L3. coverage  A_k = rule 7 with the tap predicate ids(tap) == id_k: an integer in [0, 1024].
 *  L4. image     v = Bg, the rule-8 bicubic sample of the plate at the background coordinates; then for k = 0 .. L - 1:
 *        A_k == 1024: v = Ob_k; else A_k > 0: v = v + (A_k / 1024) * (Ob_k - v); else v unchanged.  Ob_k = the rule-8 bicubic
 *        sample of the frame at layer k's coordinates.  fp32, every operation rounded on its own.  The kernel starts at the
 *        front-most layer with A == 1024 (what lies under it is overwritten) and samples Ob_k only where A_k > 0: the bits are
 *        the rule's either way.
 *  L5. visible   top = the largest k with A_k >= 512, or none.  ids_out = id_top, 0 when there is none; label = 1.f iff
 *        id_top == target_id; counts[s][k] = the number of pixels of sample s whose top is k: an integer sum (one wave
 *        reduction per layer, one integer atomic per wave and non-zero layer) on a record the call zeroes itself on the stream.
 *  L6. one layer is eosvos_lucid_compose: L = 1, id_0 = 1 and ids = (mask != 0) give its images, labels and count bit for bit
 *        (the two kernels share the coordinate, coverage and bicubic code).
 * The draws, the depth order, acceptance on the target's visible count and which objects take part (rules L7-L10) are the
 * caller's: lucid_layers.py.
 * eosvos_lucid_compose_layers: ONE launch for all n_samples <= 8 samples (one thread per output pixel, the sample in the grid's
 * third dimension).  flips [n] int32, n_layers [n] int32, layer_ids [n][8] uint8 and matrices [n][9][6] doubles (Bi, then Oi_0 ..
 * Oi_7; of both only the first n_layers[s] layer entries of a sample are read) are HOST arrays copied into the launch's
 * arguments (8 samples are 3.5 KB of HIP's 4 KB): a queued launch owns everything it reads.  images [n][C][H][W], labels
 * [n][H][W] (0.f / 1.f) and ids_out [n][H][W] (may be null) on the device, not overlapping the inputs.  counts_host non-null: the
 * counts [n][8] (0 for layers a sample does not have) are copied there and the call waits for the stream; null: nothing waits.
 * The result does not depend on what the outputs or the engine's scratch held.
 * Rejected without a launch, the outputs untouched: a null pointer (ids_out and counts_host excepted); channels outside [1, 64];
 * height or width < 1 or > 4096; n_samples outside [1, 8]; a layer count outside [1, 8]; a layer id of 0 or one repeated within
 * a sample; target_id outside [1, 255]; a non-finite entry of a matrix that is read. */
int eosvos_lucid_compose_layers(eosvos_engine* e, const float* frame, const uint8_t* ids, const float* plate, int channels,
                                int height, int width, int n_samples, const int32_t* flips, const int32_t* n_layers,
                                const uint8_t* layer_ids, const double* matrices, int target_id, float* images, float* labels,
                                uint8_t* ids_out, int32_t* counts_host);

/* ---- online adaptation: distance-gated negatives from a capped distance transform --------------------------------------- */
/* The pseudo-labels of the adaptation rounds (evaluate.py:231-240) come from the frame's own probabilities; nothing looks at
 * where the object was, so a confident blob on a look-alike becomes a positive target of every later round.  OnAVOS
 * (Voigtlaender & Leibe, 2017) gates them by distance: pixels farther than `neg_dist` from the eroded mask of the previous frame
 * are negatives whatever the network says, sure and near pixels are positives, the rest is void.  An opt-in extension
 * (eosvos_amd/adapt.py, `eval_adapt`), off by default; neg_dist 220 / erode 15 (OnAVOS's 480p values) are examples, UNTUNED.
 * Everything below is integer arithmetic; frames are [H][W] fp32 maps, H, W <= 4096.
 *   1. capped squared distance  S a set of seed pixels of a frame, L >= 1 an integer limit: D2(p) = min over q in S of
 *        dy^2 + dx^2 (pixel centres, inside the frame only), out(p) = min(D2(p), L^2 + 1); an empty S gives L^2 + 1 everywhere.
 *        int32; L <= 4095.  The definition does not depend on the algorithm.  A NaN probability is never a seed under p >= t and
 *        always one under the inverted predicate !(p >= t).
 *   2. anchor  for a propagated frame f: A = {p(f - 1) >= t_pos}, p(f - 1) the previous frame's probabilities (the train frame
 *        holds 2 * ground truth, evaluate.py:167-168); t_pos = the scalar `min_prop`, or `hi` of the band.
 *   3. erosion  erode = e > 0: E = {q in A : D2_in(q) > e^2}, D2_in = rule 1 with the frame's pixels NOT in A as seeds and
 *        L = e.  Pixels outside the frame are not background: an object cut by the border is not eroded from the border.
 *        e = 0: E = A.
 *   4. far  far(p) <=> rule 1 with seeds E and L = neg_dist gives out(p) > neg_dist^2.
 *   5. targets of f (p = the frame's own probability): the band's rule, 1 where p >= hi, 0 where p < lo, `ignore` otherwise (a
 *        NaN is void); a scalar min_prop = t is the band (0, t): nothing near is negative.  Then target = 0 where far.
 *   6. counts  n_pos[f] = the 1s after the override.  An empty E (object lost or eroded away): n_pos[f] = 0 and the frame's
 *        targets are the band rule's; the caller drops frames with n_pos = 0.
 * eosvos_distance_sq (rule 1, the public primitive): seeds = {probs >= threshold}, or its complement with invert != 0;
 * out [n_frames][H][W] int32.  2 launches (csrc/edt_kernels.hip): a column pass, one thread per column, leaves the vertical
 * distance capped at L + 1 as 16-bit words in the engine's grow-only scratch; a row pass, one workgroup per row staged in LDS,
 * takes min over k of k^2 + g^2[x +- k] and stops at k^2 >= best, which is exact.
 * eosvos_adapt_targets (rules 2-6): anchors [n_frames][H][W] holds frame i's previous-frame probabilities; 2 launches with
 * erode 0, 4 with it; the distances never reach memory (the row pass writes the eroded mask bytes, or the targets, itself).
 * Scratch: 2 bytes per pixel, 1 more with erode, 8 per frame; at most 512 MB per call (pass fewer frames).  The two counts per
 * frame are integer sums (wave reduction, one integer atomic per wave) on words the call zeroes itself on the stream; nothing
 * depends on what scratch or outputs held before.  n_pos (may be NULL: nothing waits) receives the counts after one
 * synchronisation.  Asynchronous on the engine's stream otherwise; not tied to e's frame size.
 * Rejected without a launch, the outputs untouched: a null pointer (n_pos excepted); n_frames outside [1, 65535]; height or
 * width outside [1, 4096]; limit outside [1, 4095]; neg_dist outside [1, 4095]; erode outside [0, 255]; not 0 <= lo < hi <= 1;
 * a NaN threshold; an ignore label that is not finite or lies in [0, 1]. */
int eosvos_distance_sq(eosvos_engine* e, const float* probs, int n_frames, int height, int width, float threshold, int invert,
                       int limit, int32_t* out);
int eosvos_adapt_targets(eosvos_engine* e, const float* probs, const float* anchors, int n_frames, int height, int width, float lo,
                         float hi, float anchor_thr, int erode, int neg_dist, float ignore, float* targets, int64_t* n_pos);

/* ---- learning-rate hierarchy (meta_optim.py:27-67) ------------------------------------ */
/* `lr_hierarchy_level`: how the learned lr state is stored.  NEURON (cfgs/meta.yaml:36) one
 * value per output channel; TENSOR one per trainable tensor (`log_init_lr` of shape
 * (num_param_groups,1), meta_optim.py:33-42); SINGLE one value repeated over all tensors
 * (`:27-31,157-160`); PARAM one per weight, in the parameter's OIHW layout (`:50-51`). */
#define EOSVOS_LR_NEURON 0
#define EOSVOS_LR_TENSOR 1
#define EOSVOS_LR_SINGLE 2
#define EOSVOS_LR_PARAM 3
/* number of stored lr values at a level: lr_count / #trainable tensors / 1 / param_count */
int64_t eosvos_lr_store_count(int arch, int level);
/* Load the learned lr state at `level`; use_log != 0: the state holds log(lr) and exp() is
 * applied before the step (`use_log_init_lr`, meta_optim.py:180-185).  Supersedes eosvos_set_lr
 * (which is level NEURON, use_log 0).  eosvos_meta_grad then writes d/d(state) in the same
 * layout: [0, lr_store_count) followed by param_count init gradients. */
int eosvos_set_lr_state(eosvos_engine* e, int level, int use_log, const float* store);

/* ---- meta-training task (meta_run.py:109-238) --------------------------------------- */
/* theta <- init and sum_k g_k <- 0 (meta_optim.reset(); zero_grad(), meta_run.py:121-122). */
int eosvos_meta_task_begin(eosvos_engine* e);
/* Meta frame forward/backward at theta_K and closed-form first-order BPTT
 * (bptt_loss.backward(), meta_run.py:214):  ADDS into flat_meta_grad
 *   [0, lr_count)            d/d lr[c]   = -sum_{cin,kh,kw} (sum_k g_k) * G
 *   [lr_count, +param_count) d/d init    = G                        (OIHW)
 * which is the `named_parameters()` order of MetaOptimizer (log_init_lr_* then
 * model_init_*).  meta_loss_host may be NULL. */
int eosvos_meta_grad(eosvos_engine* e, const float* images, const float* masks, int batch,
                     float* flat_meta_grad, float* meta_loss_host);
/* The same with the other BPTT schedules of meta_run.py:154-221:
 *  - `multi_step_bptt_loss` (cfgs/meta.yaml:19): the meta loss is evaluated after EVERY inner step and
 *    weighted: call after step e with weight = multi_step_bptt_loss[e-1] (`:154-177`);
 *  - `bptt_epochs` < num_epochs.train (truncated BPTT, `:187-221`): `meta_optim.reset(keep_state=True)`
 *    detaches the parameters and the state lr (meta_optim.py:145-151), so in the reference only the
 *    FIRST segment leaves gradients on the learned init / lr: call this for the first segment's meta
 *    frames only and evaluate the later ones with eosvos_forward + eosvos_loss.
 * ADDS weight * [d/d lr-state | d/d init (if INIT_GRAD)] into flat_meta_grad; NEW_SEGMENT zeroes
 * sum_k g_k afterwards (theta is kept): the next call then differentiates through the steps taken
 * since -- a segment-wise variant that keeps learning the lr in every segment. */
#define EOSVOS_META_INIT_GRAD 1
#define EOSVOS_META_NEW_SEGMENT 2
int eosvos_meta_grad_ex(eosvos_engine* e, const float* images, const float* masks, int batch,
                        float* flat_meta_grad, float* meta_loss_host, float weight, int flags);

/* ---- outer step (train_meta.py:361-373, radam.py:28-94, meta_optim.py:116-133) ------ */
/* One RAdam step on n contiguous floats that share (lr, weight_decay):
 * grad <- clamp(grad * grad_scale, +-grad_clip) (grad_clip <= 0: no clip); `step` is the
 * 1-based step count; N_sma/step_size are computed on the host exactly as radam.py:62-79. */
int eosvos_radam_step(eosvos_engine* e, float* param, const float* grad, float* exp_avg,
                      float* exp_avg_sq, int64_t n, float lr, float weight_decay, float beta1,
                      float beta2, float eps, int step, float grad_scale, float grad_clip);
/* param <- clamp(param, lo, hi)  (clamp_init_lr; pass hi = +inf for max_lr None). */
int eosvos_clamp(eosvos_engine* e, float* param, int64_t n, float lo, float hi);
/* The whole outer step of meta-training in ONE launch (replaces train_meta.py:361-373 + RAdam.step radam.py:28-94 +
 * clamp_init_lr meta_optim.py:116-133 + the upload of the new learned state into the engine):
 *   state / grad / exp_avg / exp_avg_sq: flat device vectors [lr state (n_lr) | model_init (OIHW, eosvos_param_count)];
 *   grad <- clip(grad * grad_scale, +-grad_clip) (grad_clip <= 0: none); RAdam step `step` (>= 1) with the reference's
 *   two parameter groups: lr `lr_lr`, no weight decay for the lr state; lr `init_lr`, weight decay `weight_decay` for
 *   model_init (skipped when learn_model_init == 0: the vectors then hold the lr state only); the first `frozen_lr` /
 *   `frozen_param` elements of each part take lr 0 (freeze_encoder, train_meta.py:120-121); the lr state is clamped to
 *   [lr_lo, lr_hi]; grad is zeroed; the engine's own copies are written by the same kernel: effective per-neuron lr
 *   (exp() of the state when use_log) and learned init = current weights in the engine layout (as eosvos_set_lr_state +
 *   eosvos_set_init would leave them).  NEURON hierarchy level only (the other levels go through eosvos_radam_step /
 *   eosvos_set_lr_state); the arithmetic per element is eosvos_radam_step's. */
int eosvos_outer_step(eosvos_engine* e, float* state, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n_lr,
                      int learn_model_init, int step, float lr_lr, float init_lr, float weight_decay, float beta1, float beta2,
                      float eps, float grad_scale, float grad_clip, float lr_lo, float lr_hi, int use_log,
                      int64_t frozen_lr, int64_t frozen_param);
/* Engines that run the tasks of one meta-batch side by side always hold the same learned state: `e` drops its own copy of
 * the learned init and of the per-neuron lr and reads `src`'s from now on (no upload per engine after an outer step -- one
 * eosvos_outer_step / eosvos_set_init / eosvos_set_lr on `src` serves all of them).  `src` must outlive `e`, both on one
 * device; the caller orders `e`'s stream after the stream of `src` that wrote the state. */
int eosvos_alias_state(eosvos_engine* e, eosvos_engine* src);
/* Undo eosvos_alias_state: `e` gets its own buffers back, holding the learned init / lr it has been reading (a copy of the
 * source's current state).  The library tracks the relation: destroying a source first un-aliases every engine that reads it
 * (they keep a valid copy), destroying an alias removes it from its source's list, eosvos_outer_step on the source updates
 * the lr level / log flag of its aliases. */
int eosvos_unalias_state(eosvos_engine* e);

/* ---- frozen encoder (`parent_model.train_encoder: False`, cfgs/meta.yaml:71) --------------------------------------------
 * Convs [0, conv_idx) of the reference order (eosvos_conv_info) are frozen, the rest are trained.  The reference freezes
 * the backbone except layer4 for DeepLabV3+ (networks/deeplabv3plus.py:144-146: conv_idx = first conv of layer4) and the
 * whole backbone for DeepLabV3 (networks/deeplabv3.py:53-54: conv_idx = first ASPP conv); 0 trains everything (the
 * default).  Other values are rejected.  Under a boundary:
 *  - the backward pass ends at it: no data gradient into a frozen conv's output, no weight gradient of a frozen conv, no
 *    update of its weights (they keep the value of the last eosvos_set_init / eosvos_set_params);
 *  - entries that carry model weights keep the full layout: eosvos_set_init, eosvos_get_params, eosvos_set_params,
 *    eosvos_snapshot_params / eosvos_restore_params;
 *  - entries that carry learned state keep the full layout too, and the frozen part is inert: eosvos_lr_store_count and
 *    eosvos_set_lr_state are unchanged (the lr values of frozen tensors are read by nothing), eosvos_meta_grad[_ex] adds
 *    into the trainable part only (it leaves the frozen lr / init entries of the caller's buffer as they are) and
 *    eosvos_get_grads writes zeros for the frozen tensors.  The trainable subset -- the reference's
 *    MetaOptimizer.named_parameters() (meta_optim.py:46-78, meta_model.py:29-60) -- is the SUFFIX of every part of the full
 *    layout: lr rows / tensors / elements and init elements from the first trainable conv on;
 *  - eosvos_outer_step fails (the caller keeps the RAdam moments of the subset only: eosvos_radam_step on the suffixes);
 *  - eosvos_alias_state requires both engines to have the same boundary, and an aliased engine cannot change it.
 * Call between steps (it synchronises the engine's stream); a backward pass needs a forward made under the boundary. */
int eosvos_set_trainable_from(eosvos_engine* e, int conv_idx);

/* ---- the exchange step of meta-training over RCCL (SURVEY 8b `allreduce_sum(flat, n, comm)`) ------------------------
 * Replaces the reference's hand-off of per-process gradients into shared CPU tensors (src/util/meta_run.py:237-238) +
 * the main process's sum (src/train_meta.py:361-366) by ONE in-place all-reduce(sum) of the flat meta-gradient
 * ([lr state | init], 40 318 387 floats for ResNet-50) on the engine's stream, between the tasks' gradient accumulation and
 * eosvos_outer_step.  For hosts that are not torch processes (a torch host may keep using torch.distributed, backend "nccl" =
 * RCCL: the Python shim's default): rank 0 calls eosvos_comm_unique_id and hands the 128 bytes to the other ranks by its own
 * means, every rank calls eosvos_comm_init_rank (collective: blocks until all `world_size` ranks have called; one GPU per
 * rank), then eosvos_allreduce_sum once per meta-iteration (collective, asynchronous on the engine's stream, deterministic
 * for a fixed world size and topology), eosvos_comm_destroy at the end.  RCCL is bound at the first of these calls (the
 * instance already in the process, else librccl.so.1 / $EOSVOS_RCCL_LIB); the library itself loads without it. */
typedef struct { char internal[128]; } eosvos_rccl_id; /* = ncclUniqueId */
int eosvos_comm_unique_id(eosvos_rccl_id* id);
int eosvos_comm_init_rank(void** comm, int world_size, const eosvos_rccl_id* id, int rank, int device_id);
int eosvos_comm_destroy(void* comm);
int eosvos_allreduce_sum(eosvos_engine* e, float* flat, int64_t n, void* comm);

/* ---- instrumentation ----------------------------------------------------------------- */
/* Time `reps` launches of the largest conv_igemm launch of a fine-tune iteration (decoder.last_conv.0
 * forward: the batched GEMM of its Winograd form, 16 x [tiles x 304] x [304 x 256], + its fix-up launch)
 * with HIP events on the engine stream; returns the average milliseconds in *ms_host and that launch's own
 * FLOPs in *flops_host. */
int eosvos_time_hot_kernel(eosvos_engine* e, int batch, int reps, float* ms_host,
                           double* flops_host);
/* Tuning aid: average milliseconds of `reps` launches of conv `conv_idx`'s forward (kind 0), data
 * gradient (1) or weight gradient (2) on the engine's own buffers, and its algorithmic FLOPs. */
int eosvos_bench_conv(eosvos_engine* e, int conv_idx, int kind, int batch, int reps, float* ms_host,
                      double* flops_host);
/* Calibration: time one launch of `iters` x 16 back-to-back v_mfma_f32_32x32x2_f32 per wave on
 * register operands (2 workgroups x 4 waves on every CU, no memory traffic): the fp32 matrix
 * rate this device sustains at the clock it holds, next to the 157.3 TFLOP/s nominal peak. */
int eosvos_mfma_probe(eosvos_engine* e, int iters, float* ms_host, double* flops_host);
/* Device pointer + {B,H,W,C} of a named internal NHWC activation / gradient buffer of the
 * last forward/backward ("c1","p1","blk<i>.out","cat","proj","dcat","d1","d2","lowlog",
 * "logits", "g_*" ...), for the per-stage parity tests; the ASPP image-pooling branch, read-only, as {B,1,1,C}: "vec"
 * (the mean of layer4's output over the pixels, C = 2048), "poolout" (the branch's conv + norm + ReLU of it, C = 256), "gp"
 * (the gradient of the loss w.r.t. the pre-ReLU "poolout": the pixel sum of "g_cat"[:, 1024:1280]) and "gvec" (w.r.t. "vec");
 * "ccl_scratch": the one grow-only scratch arena that every
 * evaluation-stage entry point shares, as dims4[3] 32-bit words (null before its first use);
 * "z<ci>" (decimal conv index in eosvos_num_convs order, e.g. "z0", "z17"), GroupNorm engines only: the dense
 * {B,Ho,Wo,cout} buffer of normalised conv ci that holds its raw (pre-norm) output z after a forward and, overwritten
 * in place, dL/dz after a backward.  On a frozen-BatchNorm engine, or for a conv without a norm layer (the classifier),
 * the name fails like any unknown name.
 * Plain DeepLabV3 engines have no decoder: "d1" / "g_d1" are the output of the head's 3x3 conv (classifier.1) and its
 * gradient, "lowlog" / "g_low" the classifier's, all on the ASPP map (stride 8: {B,h8,w8,256} and {B,h8,w8,1}); "dcat",
 * "d2" and their gradients are unknown names there. */
/* Measurement aid: HIP events around every launch of the matrix-core kernels, on the stream each one runs on.
 * profile_read returns, per kernel symbol (names: max_kernels x 64 chars), launches, summed duration (ms) and summed
 * executed fp32-equivalent FLOPs since profile_launches(e, 1).  bench.py's roofline (dominant kernel by time). */
int eosvos_profile_launches(eosvos_engine* e, int on);
int eosvos_profile_read(eosvos_engine* e, int max_kernels, char* names, int64_t* counts, double* ms_host,
                        double* flops_host, int* n_out_host);
/* Test aid: a host-side log of how every tiled-conv launch was planned (off by default; no device work, no synchronisation, no
 * effect on any launch).  plan_log(e, 1) clears the log and starts recording, plan_log(e, 0) stops; the first 16 launches are
 * kept.  plan_log_read copies min(launches, max_records, 16) records: the main kernel's symbol (names: max_records x 64 chars)
 * and EOSVOS_PLAN_LOG_FIELDS ints per record, in this order: kernel id, K-major gather, column-tile width, tiles, K steps of
 * one tile, deep variant (0 / 1 / 2), whole tiles per workgroup (dp_q), streamed K steps per workgroup (per), workgroups,
 * split-K chunks, tap table attached, longest-first tile order attached, fix-up pass launched, workgroups the launch
 * planned for (eosvos_set_wg_budget).  A launch taken by a streaming kernel has zeros in the plan fields.  *n_out_host: the
 * launches seen since the log was enabled (more than 16: the later ones were dropped). */
#define EOSVOS_PLAN_LOG_FIELDS 14
int eosvos_test_conv_plan_log(eosvos_engine* e, int on);
int eosvos_test_conv_plan_log_read(eosvos_engine* e, int max_records, char* names, int* fields_host, int* n_out_host);
int eosvos_debug_tensor(eosvos_engine* e, const char* name, float** ptr_out, int64_t* dims4_out);
/* Low-level op entry used by the kernel parity tests: a single NHWC convolution
 * y = relu?(a*conv(x,w)+b (+res)); w is OIHW; all dense tensors; stride/dil/pad as torch. */
int eosvos_test_conv(eosvos_engine* e, const float* x_nhwc, const float* w_oihw,
                     const float* scale, const float* bias, const float* res_nhwc, int relu,
                     int B, int H, int W, int Cin, int Cout, int k, int stride, int dil, int pad,
                     float* y_nhwc);
/* Convolution algorithm of the *_algo entry points.  AUTO plans by work size like the network does. */
#define EOSVOS_ALGO_AUTO 0
#define EOSVOS_ALGO_DIRECT 1   /* implicit GEMM (tap tables / parity-major rows / coarse-grid stride-2 gradient included) */
#define EOSVOS_ALGO_WINO_F2 2  /* Winograd F(2x2,3x3); dilated convs as d*d interleaved sub-grids */
#define EOSVOS_ALGO_WINO_F4 3  /* Winograd F(4x4,3x3) */
/* The same convolution through the production forward path with the algorithm forced (3x3 / stride 1 /
 * pad == dilation <= 8 for the Winograd forms).  torchvision Bottleneck / ASPP / decoder convs, SURVEY 2.2 K3/K4.
 * This entry, eosvos_test_conv_bwd_algo and eosvos_test_conv_views plan their launches under the workgroup budget of `e`
 * (eosvos_set_wg_budget), as the network's passes do; their weight-gradient slabs are sized for every budget. */
int eosvos_test_conv_algo(eosvos_engine* e, int algo, const float* x_nhwc, const float* w_oihw,
                          const float* scale, const float* bias, const float* res_nhwc, int relu,
                          int B, int H, int W, int Cin, int Cout, int k, int stride, int dil, int pad,
                          float* y_nhwc);
/* dx = mask?(dgrad(scale*g)), dw = scale * wgrad(g, x) through the production backward paths; `scale` (per cout,
 * the folded norm scale) and `m8` (the ReLU mask bytes of the conv input, Cin / 4 per pixel: dx of channel 4q + j = 0
 * where bit j of byte [p][q] is clear) may be NULL. */
int eosvos_test_conv_bwd_algo(eosvos_engine* e, int algo, const float* x_nhwc, const float* w_oihw,
                              const float* g_nhwc, const float* scale, const uint8_t* m8, int B, int H, int W,
                              int Cin, int Cout, int k, int stride, int dil, int pad, float* dx_nhwc,
                              float* dw_oihw);
/* dx = conv_dgrad(g), dw = conv_wgrad(g, x) for the same geometry (no norm scale), ALGO_DIRECT. */
int eosvos_test_conv_bwd(eosvos_engine* e, const float* x_nhwc, const float* w_oihw,
                         const float* g_nhwc, int B, int H, int W, int Cin, int Cout, int k,
                         int stride, int dil, int pad, float* dx_nhwc, float* dw_oihw);

/* One convolution through the production conv_fwd / conv_dgrad / conv_wgrad in the forms the network's passes use: every
 * tensor operand is a VIEW -- `p` first element (device), `ld` floats per pixel, and, when it is a channel slice of a wider
 * tensor, `key` / `ldkey`: first element and pixel pitch (= channel count) of that tensor (key NULL: the view is the tensor).
 * The f16x3 absmax slots, the mask bytes and the pair8 siblings are kept per TENSOR, i.e. per key. */
typedef struct eosvos_view {
  float* p;
  int ld;
  float* key;
  int ldkey;
} eosvos_view;
#define EOSVOS_VIEWS_FWD 1
#define EOSVOS_VIEWS_DGRAD 2
#define EOSVOS_VIEWS_WGRAD 4
typedef struct eosvos_conv_views {
  /* geometry as eosvos_test_conv_algo: x [B][H][W][Cin], y / g [B][Ho][Wo][Cout]; scale / bias (per cout) may be NULL */
  int algo, B, H, W, Cin, Cout, k, stride, dil, pad;
  const float* w_oihw;
  const float* scale;
  const float* bias;
  int passes;                 /* EOSVOS_VIEWS_*; in one call the weight gradient runs before the data gradient */
  /* forward: y = relu?(a * conv(x) + b (+ res)).  y_m8 (may be NULL): the mask bytes of the WHOLE y tensor, y.ldkey / 4 (or
   * y.ld / 4) bytes per pixel; a ReLU forward writes bit j of byte [p][q] = (channel 4q + j of the tensor > 0) for the view */
  eosvos_view x, y, res;
  int relu;
  uint8_t* y_m8;
  /* data gradient: gx = M * ((accum ? gx : 0) + add + dgrad(a * g)); M from gx_m8 (may be NULL; gx.ld / 4 bytes per pixel,
   * byte [p][q] bit j = channel 4q + j of the view) for channels >= mask_c0, 1 below */
  eosvos_view g, gx, add;
  int accum, mask_c0;
  const uint8_t* gx_m8;
  /* weight gradient of g and x: dw [Cout][Cin][k][k] = a * wgrad(g, x) */
  float* dw_oihw;
  /* out, f16x3 mode (0 in the others): the absmax slot of the destination tensor after the pass -- [0] y, [1] gx -- as the
   * maximum of its words (the bit pattern of max |value| the writers committed), and whether a consumer would trust it.  A
   * keyed SOURCE view runs under the slot of its whole tensor, which the entry fills first, as the tensor's producer would. */
  unsigned slot_bits[2];
  int slot_valid[2];
  /* the same for the whole-tensor slots the keyed SOURCE views ran under: [0] x, [1] g (0 when the view has no key) */
  unsigned src_slot_bits[2];
  int src_slot_valid[2];
  /* forward only, > 1: that many launches in ONE absmax phase, launch i reading x.p + i * Cin and writing y.p + i * Cout
   * (x and y keyed and wide enough) -- all slices of a tensor written one after the other; slot [0] is read after the last */
  int fwd_slices;
} eosvos_conv_views;
int eosvos_test_conv_views(eosvos_engine* e, eosvos_conv_views* v);
/* The ASPP branches' data gradient into d(layer4 output) on a loaded engine -- the step backward_impl runs (aspp_dgrad: the
 * K-concatenated launch, or four accumulating conv_dgrad calls when it declines or force_fallback is set):
 * g_l4 = M * (g_l4 + sum_i dgrad_i(a_i * g_cat[..., 256 i : 256 i + 256])).  g_cat [B][h16][w16][1280], l4_m8 [B][h16][w16][Cin / 4]
 * mask bytes of the layer4 output, g_l4 [B][h16][w16][Cin] in / out (device).  merged_ran: which path ran; slot_bits /
 * slot_valid: g_l4's f16x3 absmax slot as in eosvos_conv_views. */
int eosvos_test_aspp_dgrad(eosvos_engine* e, int batch, const float* g_cat, const uint8_t* l4_m8, float* g_l4_inout,
                           int force_fallback, int* merged_ran, unsigned* slot_bits, int* slot_valid);

/* Op-level entries of the other kernels (misc_kernels.hip) for the parity tests: the production launchers with the engine's
 * own geometry, on caller DEVICE tensors (NHWC, `ld*` = floats per pixel, so a channel slice of a wider buffer works), on the
 * engine's stream; they synchronise before returning.
 *
 * GroupNorm(16, C) with frozen affine, torch.nn.GroupNorm (deeplabv3plus.py:180-191).  bwd = 0: y = relu?(group_norm(z) *
 * gamma + beta (+ res)), stats [B][16][2] = {mean, rstd} out, m8 (may be NULL; needs relu): bit j of byte [p][q] = (y of
 * channel 4q + j > 0), row pitch ldm8 bytes.  bwd = 1: z <- dL/dz of that forward without the ReLU / residual, given
 * g = dL/d(group_norm output) and the forward's stats (y, beta, res, m8 unused). */
int eosvos_test_groupnorm(eosvos_engine* e, int bwd, float* z, int ldz, const float* g, int ldg, const float* gamma,
                          const float* beta, const float* res, int ldres, int relu, int B, int P, int C, float eps, float* y,
                          int ldy, float* stats, uint8_t* m8, int ldm8);
/* F.max_pool2d(x, 3, 2, 1) of the stem (torchvision resnet maxpool), dense NHWC x [B][H][W][C] -> y [B][Ho][Wo][C] with the
 * argmax bytes idx (tap | 0x80 when the maximum is > 0).  gy, gx (both or neither): gx = max_pool2d backward(gy) * (x > 0)
 * (x being the ReLU output that was pooled). */
int eosvos_test_maxpool(eosvos_engine* e, const float* x, int B, int H, int W, int C, float* y, uint8_t* idx, const float* gy,
                        float* gx);
/* F.interpolate(mode='bilinear', align_corners) from hin x win to hout x wout (deeplabv3plus.py:144, :161): x -> y when both are
 * given, and gx = backward(gy) when gy / gx are given, zero in channel 4q + j where bit j of the ReLU mask byte m8[p][q] is
 * clear (m8 may be NULL; row pitch ldm8 bytes; needs C % 4 == 0). */
int eosvos_test_resize(eosvos_engine* e, int align_corners, int hin, int win, int hout, int wout, int B, int C, const float* x,
                       int ldx, float* y, int ldy, const float* gy, int ldgy, float* gx, int ldgx, const uint8_t* m8, int ldm8);
/* The ASPP image-pooling branch (ASPPPooling, deeplabv3plus.py:100-112): v = mean over P pixels of x [B][P][K], pool =
 * relu(a * (w v) + bias) (a = bias = NULL: w v without affine, the GroupNorm engine's form), broadcast to y [B][P][N] (+ the ReLU
 * mask bytes m8 when not NULL).  With gy: gpool = sum over pixels of gy [B][P][N] (already ReLU-masked, as the consumer's data
 * gradient leaves it), gv = a * w^T gpool, dw [N][K] = a * gpool^T v (the slab after the update's scaling), gx [B][P][K] = gv / P at every pixel. */
int eosvos_test_aspp_pool(eosvos_engine* e, int B, int P, int K, int N, const float* w, const float* a, const float* bias,
                          const float* x, int ldx, float* v, float* pool, float* y, int ldy, uint8_t* m8, int ldm8,
                          const float* gy, int ldgy, float* gpool, float* gv, float* dw, float* gx, int ldgx);
/* The 1-channel classifier (Conv2d(256, 1, 1) with bias, deeplabv3plus.py:163): y [P] = x [P][C] . w + bias.  With g: gx =
 * g w^T * (x > 0) (x is a ReLU output) and dw [C + 1] = {sum_p g x, sum_p g} after the reduction of the per-chunk slabs. */
int eosvos_test_head(eosvos_engine* e, const float* x, const float* w, const float* bias, int64_t P, int C, float* y,
                     const float* g, float* gx, float* dw);

/* Op-level entry of the pre-split operand path (round 6; e-osvos_amd/csrc/presplit_kernels.hip): the weight gradient of one
 * convolution -- dL/dW of `/root/reference/src/networks/deeplabv3plus.py:32-53`'s convs as autograd computes it -- from operands
 * stored as fp16 (hi, lo) pairs under one power-of-two scale per tensor.  Stand-alone (no engine); device pointers.
 * g [B][Ho][Wo][Cout], x [B][Hi][Wi][Cin] fp32 NHWC; ws [splits][Cout][k*k][Cin]; g2 / x2: scratch of the operands' byte size;
 * amax: 32 * 2048 zeroed 32-bit words; sc: 4 floats; zero: 2048 zero bytes.  which: 0 = absmax -> scale (`margin` spare bits)
 * -> split passes -> pre-split kernel; 1 = pre-split kernel only; 2 = the register-staged f16x3 kernel on the fp32 operands;
 * 3 = split passes only; 4 = pre-split kernel without a producer scale (its in-kernel path that stages from the fp32 tensors).  Cout, Cin multiples of 256 for which 0 / 1 / 4.  splits: K chunks (one slab each);
 * groups: workgroups per tile that share them (0: one per chunk) -- the result does not depend on it. */
int eosvos_test_wgrad_presplit(const float* g, const float* x, float* ws, void* g2, void* x2, unsigned* amax, float* sc,
                               const void* zero, int B, int Ho, int Wo, int Cout, int Hi, int Wi, int Cin, int k, int stride,
                               int pad, int dil, int splits, int groups, int margin, int which, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EOSVOS_H */
