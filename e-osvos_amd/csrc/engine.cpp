// Host side of libeosvos.so: the DeepLabV3+/ResNet graph of the e-OSVOS inner loop as an
// explicit forward / backward / fused-update program over the gfx950 kernels of
// conv_kernels.hip and misc_kernels.hip, behind the C-ABI of include/eosvos.h.
//
// Reference semantics (files under /root/reference/src):
//   forward   networks/deeplabv3plus.py:32-53,84-93,282-301 (+ torchvision ResNet/ASPP)
//   norm      BatchNorm in eval mode with frozen affine (deeplabv3plus.py:148-155,259-265)
//             == per-channel a*x+b, fused into every conv epilogue; GroupNorm(16) mode (:180-191)
//   convs     implicit GEMM; the heavy 3x3 / stride-1 layers in the Winograd F(4x4,3x3) / F(2x2,3x3) domain
//   loss      helper_func.py:32-37 (BCEWithLogits, mean)
//   step      meta_optim/meta_optim.py:177-214 + meta_model.py:78-80
//   meta-grad util/meta_run.py:109-238 (first-order BPTT, closed form of SURVEY 3.3)
//   outer     train_meta.py:361-373, util/radam.py:28-94
//
// Data layout in HBM: activations NHWC fp32 (channels contiguous = GEMM K of the gathered
// operand), weights W[cout][kh*kw][cin] per conv inside one flat arena that keeps the
// reference's tensor order and offsets (only the two inner axes are permuted), concat
// buffers are written in place by their producers (channel-slice views), gradients of
// activations hold dL/d(pre-ReLU) so the ReLU mask and the frozen-norm scale never need
// their own pass.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/eosvos.h"
#include "kernels.h"
#include "scratch_layout.h"
#include "tensor_views.h"

using namespace eosvos;

static thread_local std::string g_err;
static int fail(const std::string& m) {
  g_err = m;
  return 1;
}
#define HIPOK(expr)                                                                      \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess)                                                                \
      return fail(std::string(#expr) + ": " + hipGetErrorString(_e) + " @" + std::to_string(__LINE__)); \
  } while (0)

namespace {

struct ConvL {
  int cin, cout, k, stride, dil, pad;
  bool norm, bias;
  int64_t poff;   // offset of the weight in the flat parameter arena (bias follows)
  int64_t lroff;  // offset of its per-neuron lr (bias lr follows)
  int64_t noff;   // offset of its norm channels
  int T() const { return k * k; }
  int64_t wsize() const { return (int64_t)cout * cin * k * k; }
};
struct Block {
  int c1, c2, c3, ds;  // conv indices, ds = -1 if none
};
struct Topo {
  std::vector<ConvL> convs;
  std::vector<Block> blocks;
  std::vector<int> stage;  // per conv: ResNet layer 0..3 of a bottleneck conv, -1 otherwise
  int layer1_last_block;  // index of the block whose output is the low-level feature
  int aspp[4], pool, project, dec1, dec_a, dec_b, last;
  int head3 = -1;          // plain DeepLabV3 (networks/deeplabv3.py): the 3x3 conv of DeepLabHead; dec1 / dec_a / dec_b = -1
  bool v3 = false;
  int64_t nparam, nlr, nnorm;
};

bool build_topo(int arch, Topo& t) {
  int nb[4];
  // EOSVOS_ARCH_V3_*: plain DeepLabV3 (src/networks/deeplabv3.py:10-83): torchvision ResNet with
  // replace_stride_with_dilation = [False, True, True] and NO stride surgery -> output stride 8 (layer3 dilation 1, 2, 2..,
  // layer4 dilation 2, 4, 4), DeepLabHead = ASPP[12, 24, 36] -> 3x3 conv + norm + ReLU -> 1x1 conv (+ bias), logits resized x8
  const bool v3 = arch == EOSVOS_ARCH_V3_RESNET50 || arch == EOSVOS_ARCH_V3_RESNET101;
  const int base = v3 ? arch - 1000 : arch;
  if (base == EOSVOS_ARCH_RESNET50) { nb[0] = 3; nb[1] = 4; nb[2] = 6; nb[3] = 3; }
  else if (base == EOSVOS_ARCH_RESNET101) { nb[0] = 3; nb[1] = 4; nb[2] = 23; nb[3] = 3; }
  else return false;
  t.v3 = v3;
  t.head3 = -1;
  t.convs.clear();
  t.blocks.clear();
  auto add = [&](int cin, int cout, int k, int s, int d, int p, bool norm, bool bias) {
    ConvL c{cin, cout, k, s, d, p, norm, bias, 0, 0, 0};
    t.convs.push_back(c);
    return (int)t.convs.size() - 1;
  };
  add(3, 64, 7, 2, 1, 3, true, false);
  int inpl = 64;
  const int widths[4] = {64, 128, 256, 512};
  for (int li = 0; li < 4; ++li) {
    const int w = widths[li];
    for (int bi = 0; bi < nb[li]; ++bi) {
      const bool first = bi == 0;
      const int s1 = (!v3 && li == 2 && first) ? 2 : 1;   // reference surgery (DeepLabV3+ only): layer3[0].conv1 stride 2
      const int s2 = (li == 1 && first) ? 2 : 1;   // layer2[0].conv2 stride 2
      int d = 1;
      if (v3) {                                    // torchvision dilation rule: the first block keeps the previous dilation
        if (li == 2) d = bi == 0 ? 1 : 2;
        if (li == 3) d = bi == 0 ? 2 : 4;
      } else if (li == 3) d = bi == 0 ? 2 : (bi == nb[3] - 1 ? 8 : 4);
      Block b;
      b.c1 = add(inpl, w, 1, s1, 1, 0, true, false);
      b.c2 = add(w, w, 3, s2, d, d, true, false);
      b.c3 = add(w, 4 * w, 1, 1, 1, 0, true, false);
      b.ds = first ? add(inpl, 4 * w, 1, s1 * s2, 1, 0, true, false) : -1;
      t.blocks.push_back(b);
      t.stage.resize(t.convs.size(), -1);
      for (int ci : {b.c1, b.c2, b.c3, b.ds}) if (ci >= 0) t.stage[ci] = li;
      inpl = 4 * w;
    }
    if (li == 0) t.layer1_last_block = (int)t.blocks.size() - 1;
  }
  t.aspp[0] = add(2048, 256, 1, 1, 1, 0, true, false);
  const int rates[3] = {v3 ? 12 : 6, v3 ? 24 : 12, v3 ? 36 : 18};
  for (int i = 0; i < 3; ++i) t.aspp[i + 1] = add(2048, 256, 3, 1, rates[i], rates[i], true, false);
  t.pool = add(2048, 256, 1, 1, 1, 0, true, false);
  t.project = add(1280, 256, 1, 1, 1, 0, true, false);
  if (v3) {
    t.dec1 = t.dec_a = t.dec_b = -1;
    t.head3 = add(256, 256, 3, 1, 1, 1, true, false);
  } else {
    t.dec1 = add(256, 48, 1, 1, 1, 0, true, false);
    t.dec_a = add(304, 256, 3, 1, 1, 1, true, false);
    t.dec_b = add(256, 256, 3, 1, 1, 1, true, false);
  }
  t.last = add(256, 1, 1, 1, 1, 0, false, true);
  t.stage.resize(t.convs.size(), -1);
  int64_t po = 0, lo = 0, no = 0;
  for (auto& c : t.convs) {
    c.poff = po; c.lroff = lo; c.noff = no;
    po += c.wsize() + (c.bias ? c.cout : 0);
    lo += c.cout + (c.bias ? 1 : 0);
    if (c.norm) no += c.cout;
  }
  t.nparam = po; t.nlr = lo; t.nnorm = no;
  return true;
}

inline int conv_out(int i, int k, int s, int d, int p) { return (i + 2 * p - d * (k - 1) - 1) / s + 1; }

struct HostResize {
  std::vector<int> i0, i1, lo, hi;
  std::vector<float> lam;
};
// PyTorch upsample_bilinear2d source-index rule (ATen UpSample.h area_pixel_compute_*), fp32.
HostResize make_resize(int in, int out, bool align_corners) {
  HostResize r;
  r.i0.resize(out); r.i1.resize(out); r.lam.resize(out);
  r.lo.assign(in, out); r.hi.assign(in, -1);
  float scale;
  if (align_corners) scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  else scale = (float)in / (float)out;
  for (int d = 0; d < out; ++d) {
    float src;
    if (align_corners) src = scale * (float)d;
    else {
      src = scale * ((float)d + 0.5f) - 0.5f;
      if (src < 0.f) src = 0.f;
    }
    int i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    const int i1 = i0 + ((i0 < in - 1) ? 1 : 0);
    r.i0[d] = i0; r.i1[d] = i1; r.lam[d] = src - (float)i0;
    for (int i : {i0, i1}) {
      if (d < r.lo[i]) r.lo[i] = d;
      if (d > r.hi[i]) r.hi[i] = d;
    }
  }
  return r;
}

// One loss, as every loss entry point hands it down.  Without `combine` it is kinds[0] alone, whose own launches write the
// gradient and the value where they are wanted.  With it, each of the n terms goes to its gradient slice and value slot and
// one launch combines them by the weights (include/eosvos.h at eosvos_set_loss_sum), for one term too.
struct LossSpec {
  int n = 1;                            // as the caller gave it; loss_spec_ok checks it before anything reads kinds / weights
  int kinds[EOSVOS_LOSS_MAX_TERMS] = {EOSVOS_LOSS_BCE, 0, 0, 0};
  float weights[EOSVOS_LOSS_MAX_TERMS] = {1.f, 0.f, 0.f, 0.f};
  bool combine = false;
  bool null_terms = false;              // a sum whose caller passed no kinds or no weights
  static LossSpec single(int kind) {
    LossSpec s;
    s.kinds[0] = kind;
    return s;
  }
  static LossSpec sum(int n_terms, const int* kinds, const float* weights) {
    LossSpec s;
    s.n = n_terms;
    s.combine = true;
    s.null_terms = !kinds || !weights;
    for (int i = 0; !s.null_terms && i < n_terms && i < EOSVOS_LOSS_MAX_TERMS; ++i) { s.kinds[i] = kinds[i]; s.weights[i] = weights[i]; }
    return s;
  }
};

}  // namespace

struct eosvos_engine {
  Topo t;
  int arch, H, W, maxB, dev;
  hipStream_t s;
  hipStream_t s2 = nullptr;            // side stream: weight-gradient kernels run beside the dgrad chain
  std::vector<hipEvent_t> ev;          // one fork event per conv + a join event
  bool side_used = false;
  std::vector<std::function<void(hipStream_t)>> side_q;   // weight-gradient launches waiting for the next fork (see side_flush)
  int h2, w2, h4, w4, h8, w8, h16, w16;
  std::vector<void*> allocs;

  // parameters / state
  float *Wp = nullptr, *Winit = nullptr, *Wsnap = nullptr, *lr = nullptr, *na = nullptr, *nb = nullptr;
  float *gsum = nullptr, *gout = nullptr, *stage = nullptr;
  bool keep_grads = false;
  LossSpec fused;                       // loss of the fused entry points (eosvos_set_loss / eosvos_set_loss_sum)
  bool loss_ignore_on = false;          // eosvos_set_loss_ignore: the fused entry points evaluate their loss with a void label
  float loss_ignore = 0.f;
  int* prop_count = nullptr;            // eosvos_propagation_targets: per-frame positive counts
  float* lovasz_scratch = nullptr;      // sort buffers of the Lovasz hinge kinds, allocated when one is first selected or used
  float* bootstrap_scratch = nullptr;   // histograms, state and partials of the bootstrapped BCE, allocated like lovasz_scratch
  int bootstrap_q = 16384;              // eosvos_set_loss_bootstrap: round(fraction * 65536), default 0.25
  float* boundary_scratch = nullptr;    // per-pixel maps and partials of the boundary-F kinds, allocated like lovasz_scratch
  int boundary_radius = 0;              // eosvos_set_loss_boundary: 1 .. 16, 0 = the frame-size default
  float* surface_scratch = nullptr;     // distance words and partials of the surface loss, allocated like lovasz_scratch
  int surface_cap = 0;                  // eosvos_set_loss_surface: 1 .. 4095, 0 = the frame-size default
  // the centreline loss's planes, per-level increments and routing codes, allocated like lovasz_scratch for the depth in use
  // (cldice_levels_held levels; a deeper evaluation gives the buffer back and takes a larger one)
  float* cldice_scratch = nullptr;
  int cldice_levels_held = 0;
  int cldice_depth = 0;                 // eosvos_set_loss_cldice: 1 .. 16, 0 = the frame-size default
  // eosvos_set_loss_potts: the pairwise loss's window radius, dilation and sigmas, 0 = the default (3, 2, radius * dilation, 0.1);
  // it has no buffer of its own: its partials live in the scratch arena, its frames are xpad
  int potts_window = 0, potts_dilation = 0;
  float potts_sigma_xy = 0.f, potts_sigma_rgb = 0.f;
  // weighted sums of kinds (eosvos_set_loss_sum / eosvos_loss_sum*): a gradient slice of maxB * H * W floats per term, allocated
  // when a sum first needs that many terms; sum_vals: the terms' values as evaluated [0, 4) and of the last whole sum [4, 8)
  float* sum_slice[EOSVOS_LOSS_MAX_TERMS] = {nullptr, nullptr, nullptr, nullptr};
  float* sum_vals = nullptr;
  int sum_last_terms = 0;               // number of terms of the last evaluated sum, 0 = none yet
  int* aug_tab = nullptr;               // eosvos_warp_affine: adelta[W] bdelta[W] X0[H] Y0[H], then the nonzero counter
  float* aug_ctab = nullptr;            // bicubic coefficients at 1/32 pixel: [32][4]
  // the call scratch of every evaluation-stage entry point (scratch_for, scratch_layout.h; grow-only, freed by destroy).  One
  // buffer serves them all: a call uses it only for launches it enqueues itself on `s`, and either ends with a synchronised
  // read-back or leaves nothing behind, so the stream orders one call's use before the next one's
  void* scratch = nullptr;
  size_t scratch_cap = 0;
  // learned-lr storage level (meta_optim.py:27-67): the update consumes `lr` (per neuron) or `lr_elem`
  int lr_level = EOSVOS_LR_NEURON, lr_log = 0;
  float *lr_elem = nullptr, *glr_tmp = nullptr, *ptmp = nullptr;
  int *row_tensor = nullptr, *tensor_row0 = nullptr, *all_row0 = nullptr;
  int ntensors = 0;
  // activations (phase 0) and their gradients (phase 1, g_*): records of `ts` (tensor_views.h), each made once by
  // eosvos_create_ex with its geometry; its mask bytes, absmax slot and fp16-pair sibling hang off the record
  TensorSet ts;
  float* xpad;
  Tensor *c1, *p1, *g_c1, *g_p1, *cat, *g_cat, *proj, *g_proj, *dcat, *g_dcat, *d1, *g_d1, *d2, *g_d2;
  uint8_t* p1idx;
  struct BlkBuf { Tensor *xin, *t1, *t2, *out, *dsb, *g_xin, *g_t1, *g_t2, *g_out; };   // dsb: null without a projection shortcut
  std::vector<BlkBuf> bb;
  float *vec, *gvec, *poolout, *gp, *colscratch, *lowlog, *g_low, *logits, *dlogits, *loss_dev, *bce_partial;
  float *ws_conv, *ws_wg, *ws_conv2 = nullptr;
  // Winograd F(2x2,3x3) / F(4x4,3x3) path: per conv the transformed input planes V (made by the forward pass, reused by the
  // weight gradient) and transformed weights U; one shared buffer for the output-domain planes (forward: M, backward: dV)
  struct WinoRec {
    float *V = nullptr, *U = nullptr;   // V null: no buffers were reserved for the conv
    float* Us = nullptr;                // a[cout] * U (data gradient), made with U
    float* dM = nullptr;                // A dY A^T: made once per backward, read by wgrad and dgrad
    int v_batch = 0;                    // batch size V was computed for (0 = stale)
    int dm_batch = 0;                   // batch size dM is valid for (0 = stale)
    bool us_valid = false;              // U / Us match the current weights (set when they are made, cleared by every weight change)
  };
  std::vector<WinoRec> wino;            // per conv
  hipEvent_t ev_wino_w = nullptr;                 // the side stream has made the transformed weights of this forward
  bool wino_w_wait = false;
  float *wino_m = nullptr, *wino_dv = nullptr;    // forward M planes; data-gradient dV planes (transient)
  int64_t wino_m_n = 0;
  int norm_mode = 0;                  // EOSVOS_NORM_BN_FROZEN / EOSVOS_NORM_GN16
  std::vector<Tensor*> zbuf;          // GN: raw conv outputs (then, in backward, their gradients: phase 1), dense [B*Ho*Wo][cout]
  std::vector<float*> gn_stats;       // GN: per conv {mean, rstd} per (image, group)
  float *gn_sums = nullptr, *gn_partial = nullptr;
  struct TapTab { int* prefix; int* mask; long total; int* order; };
  std::map<long, TapTab> tap_tabs;    // (conv, fwd/dgrad, batch) -> compacted K-step table of a dilated conv
  // Grouped weight gradients: the convs of ResNet layer1..3 only queue their arguments; when the stage's data-gradient
  // chain is queued, flush_wgrad_group computes all of them: one launch per tile shape of the register-staged kernel and
  // one of the pre-split kernel (`presplit` entries carry `p`; `covered`: this iteration's producers wrote both siblings)
  struct WgPending { int ci; WgradArgs a; bool presplit; WgradPArgs p; bool covered; };
  std::vector<WgPending> wg_pending;
  // dtab: WgradArgs[] of bm x bn register-staged tiles in dtab[0], or WgradPArgs[] of 256 x 256 pre-split tiles in
  // dtab[parity of the iteration] (the scale words alternate)
  struct WgGroupLaunch { const void* dtab[2] = {nullptr, nullptr}; int* dmap = nullptr; int nwg = 0, bm = 0, bn = 0; double flops = 0; int first_ci = -1; };
  struct WgGroupPlan {
    std::vector<int> splits;                         // K splits (= slabs) of every queued conv (fixed membership: the update tables are built once)
    size_t npresplit = 0;                            // pre-split members among them
    std::vector<WgGroupLaunch> launches;             // the register-staged members: one launch per tile shape
    std::map<std::string, WgGroupLaunch> presplit;   // covered subset of the pre-split members -> their one launch
  };
  std::map<long, WgGroupPlan> wg_plans;           // (stage, batch, budget, side stream) -> split counts and device tables
  bool wg_group_on = true;
  std::vector<int> conv_hin, conv_win;            // per conv: input map size (grouped-plan slab sizing)
  std::vector<int64_t> ws_off;       // per conv: offset of its weight-gradient slabs in ws_wg
  std::vector<int> upd_splits;       // per conv: slabs written by the current backward pass
  std::vector<UpdEntry*> upd_tab;    // per batch size: device copy of the update table
  std::vector<int> upd_blocks;
  int64_t ws_conv_n = 0, ws_wg_n = 0;
  ResizeTab up_h, up_w, fin_h, fin_w;  // decoder upsample (align_corners) and final resize
  std::map<std::pair<int, int>, ResizeTab> frame_tabs;      // eosvos_resize_frames: (in, out) -> align_corners=False table
  int lastB = 0;
  bool have_loss_grad = false;
  int force_algo = 0;                 // EOSVOS_ALGO_*: 0 = plan by work size; the op-level parity tests force one path
  int wg_budget = 0;                  // eosvos_set_wg_budget: workgroups a launch plans for (0 = the whole chip)
  // K-concatenated data gradient of the four ASPP branches (ConvArgs::nseg): device tables per batch size
  struct MultiTab { int* prefix; unsigned char* taplist; ConvTap* taps; long total; };
  std::map<int, MultiTab> aspp_multi;
  OuterEnt* outer_tab = nullptr;      // eosvos_outer_step: device table of the trainable tensors
  int outer_blocks = 0;
  // eosvos_alias_state: this engine reads `alias_src`'s learned init / per-neuron lr (own_* keep its own buffers for
  // eosvos_unalias_state and for the day the source goes first); `aliased_by` = the engines that read THIS engine's
  eosvos_engine* alias_src = nullptr;
  float *own_Winit = nullptr, *own_lr = nullptr;
  std::vector<eosvos_engine*> aliased_by;
  // eosvos_set_trainable_from: convs [0, train_from) are frozen (parent_model.train_encoder False).  The backward pass ends at
  // the boundary, their weights are never updated, and their gradients are neither summed (gsum) nor exported (gout).
  int train_from = 0;
  int64_t tf_poff = 0, tf_lroff = 0;  // arena / per-neuron lr offset of the first trainable conv
  int tf_tensor = 0;                  // trainable tensors before it
  long* tf_toff = nullptr;            // export table of the trainable tensors, offsets relative to tf_poff (export_params)
  // pre-split operand path (presplit_kernels.hip, round 6): the fp16-pair siblings of the tensors (Tensor::pair)
  long pair_iter = 0;                            // training forwards so far (parity selects the producers' scale word)
  unsigned char* pair_zero = nullptr;             // 4 KB of zeros: K rows past the last contributing pixel
  float* pair_sc_pool = nullptr;
  int pair_sc_used = 0;
  // launch-plan fingerprint (eosvos_plan_fingerprint): FNV-1a over (kind, conv, M, N, K, workgroups / K splits) of every matrix
  // launch of the last forward [0] / backward [1] and the slab counts the update consumed -- the split plan fixes the fp32
  // summation order, i.e. which rounding a long trajectory accumulates (tests/test_gpu_plan_fingerprint.py)
  uint64_t plan_fp[2] = {0, 0};
  bool presplit_inflight = false;     // EOSVOS_TUNE_PRESPLIT_INFLIGHT=1 when the engine was built: the pre-split path also without a side stream
  int mode = -1;                      // eosvos_set_engine_matrix_mode: this engine's own matrix mode (-1: follow the process-wide one)
  int plan_mode = -1;                 // matrix mode the cached launch plans (wg_plans, upd_tab) were built for, see plans_match_mode()

  // f16x3 matrix mode: absmax slots (bit patterns of max|x|), kind-major [AM_KINDS][nconv]; see amax_get()
  unsigned* amax = nullptr;
  struct AmaxRec { const void* ptr = nullptr; long epoch = -1, zero_epoch = -1; };
  std::vector<AmaxRec> amax_rec;
  long fwd_epoch = 0, bwd_epoch = 0;
  bool w_amax_valid = false;         // W slots match the current weights
  long us_zero_epoch = -1;           // forward epoch whose start zeroed the U / US slots of the stale Winograd weights
  long* mt_rbase = nullptr; int* mt_rlen = nullptr; long* mt_toff = nullptr; int2* mt_tit = nullptr; int mt_nent = 0;   // ensure_meta_tabs
  long* amax_w_off = nullptr;        // device tables of launch_absmax_segments over the parameter arena
  int* amax_w_n = nullptr;
  std::vector<char> ks_amax_valid;   // KS slots match the current norm scales
  // tensor slots (Tensor::slot): absmax accumulated by the kernels that WRITE a tensor (conv epilogue, fix-up, Winograd
  // output transforms); phase 0 = activations of this forward, phase 1 = gradients of this backward
  bool fwd_masks = true;             // false during eosvos_infer: no backward pass will read the masks of this forward
  bool masks_valid = false;          // the mask bytes belong to the activations of the last forward
  int64_t max_alloc_floats = 0;      // largest single allocation (every conv operand is one of them)
  // EOSVOS_DEBUG_GUARD=1: every buffer sits between two 256 KB guard bands filled with a pattern;
  // eosvos_debug_check_guards reports bands a kernel wrote into (out-of-bounds writes)
  static constexpr int64_t GUARD = 65536;
  std::vector<std::pair<unsigned*, int64_t>> guarded;
  float* falloc(int64_t n) {
    void* p = nullptr;
    if (n < 1) n = 1;
    if (n > max_alloc_floats) max_alloc_floats = n;
    static const bool guard = getenv("EOSVOS_DEBUG_GUARD") != nullptr;
    if (guard) {
      const int64_t nn = (n + 63) / 64 * 64;
      if (hipMalloc(&p, (size_t)(nn + 2 * GUARD) * sizeof(float)) != hipSuccess) return nullptr;
      (void)hipMemsetD32((hipDeviceptr_t)p, 0xDEADBEEF, (size_t)(nn + 2 * GUARD));
      (void)hipDeviceSynchronize();
      allocs.push_back(p);
      guarded.push_back({(unsigned*)p, n});
      return (float*)p + GUARD;
    }
    if (hipMalloc(&p, (size_t)n * sizeof(float)) != hipSuccess) return nullptr;
    // EOSVOS_DEBUG_FILL=<hex word>: every buffer starts out filled with that word instead of whatever the allocator hands
    // back (zero pages in a fresh process, a closed engine's data later) -- exposes reads of memory nothing wrote
    static const char* fill = getenv("EOSVOS_DEBUG_FILL");
    if (fill) { (void)hipMemsetD32((hipDeviceptr_t)p, (int)strtoul(fill, nullptr, 16), (size_t)n); (void)hipDeviceSynchronize(); }
    allocs.push_back(p);
    return (float*)p;
  }
  // a buffer of falloc given back before the engine closes
  void ffree(float* q) {
    if (!q) return;
    void* p = q;
    for (auto it = guarded.begin(); it != guarded.end(); ++it)
      if ((float*)it->first + GUARD == q) { p = it->first; guarded.erase(it); break; }
    const auto it = std::find(allocs.begin(), allocs.end(), p);
    if (it != allocs.end()) allocs.erase(it);
    (void)hipFree(p);
  }
  float* W_(int ci) { return Wp + t.convs[ci].poff; }
  bool gn() const { return norm_mode == EOSVOS_NORM_GN16; }
  // BN: folded scale a (multiplies conv outputs / gradients); GN: none (gamma is applied by the GN kernels)
  const float* A_(int ci) const { return (t.convs[ci].norm && !gn()) ? na + t.convs[ci].noff : nullptr; }
  const float* G_(int ci) const { return na + t.convs[ci].noff; }   // GN: gamma
  const float* B_(int ci) const { return t.convs[ci].norm ? nb + t.convs[ci].noff : nullptr; }
};

namespace {

// the weights changed: the scaled Winograd weights a[cout] * U of the last forward are stale
void wino_weights_changed(eosvos_engine* e) {
  for (auto& w : e->wino) w.us_valid = false;
  e->w_amax_valid = false;
}

// ---- f16x3 mode: per-tensor absmax slots ---------------------------------------------------------------------------
// The fp16 split needs a power-of-two scale per operand tensor (conv_kernels.hip, h3_scale); the kernels read it from a
// device word that holds the bit pattern of max|x|.  Slots, per conv: X input activation (made by the forward pass, reused
// by the weight gradient), V its Winograd-domain planes, G gradient w.r.t. the conv output (shared by the data and the
// weight gradient), DM its Winograd-domain planes, W weights, U / US Winograd-domain weights, KS the frozen-norm scale
// that the data gradient multiplies into G while staging.  X / V live for one forward epoch, G / DM for one backward
// epoch; W / U / US / KS until the weights / norm change.
bool trace_on();
enum { AM_X = 0, AM_V = 1, AM_G = 2, AM_DM = 3, AM_W = 4, AM_U = 5, AM_US = 6, AM_KS = 7, AM_KINDS = 8 };
// Arena: AMAX_SUB rows of AMAX_ROW words; slot s = column s of every row (kernels.h, amax_block_commit / amax_read).
// Columns: [X | V | forward tensors][G | DM | backward tensors][W | U | US | KS] -- each phase's slots are one column
// range, zeroed by one 2-D memset when the phase begins.
inline size_t amax_col(const eosvos_engine* e, int kind, int ci) {
  const size_t nc = e->t.convs.size(), T = TSLOTS;
  if (kind <= AM_V) return (size_t)kind * nc + ci;
  if (kind <= AM_DM) return 2 * nc + T + (size_t)(kind - AM_G) * nc + ci;
  return 4 * nc + 2 * T + (size_t)(kind - AM_W) * nc + ci;
}
inline size_t amax_tcol(const eosvos_engine* e, int phase, int idx) {
  return (phase == 0 ? 2 : 4) * e->t.convs.size() + (size_t)phase * TSLOTS + idx;
}
// zero the slots [first, first + count) (all their words)
inline void amax_zero(unsigned* first, size_t count, hipStream_t st) { launch_amax_zero(first, (int)count, st); }
inline bool h3_mode() { return conv_mfma_mode() == 2; }
// An engine with a matrix mode of its own (the range guard's fallback concerns the engine whose state tripped it, not the
// process): every C-ABI call that plans or launches contractions runs under that mode on the calling thread.
struct ModeScope {
  int prev;
  bool on;
  explicit ModeScope(const eosvos_engine* e) : prev(conv_thread_mfma_mode()), on(e && e->mode >= 0) { if (on) conv_set_thread_mfma_mode(e->mode); }
  ~ModeScope() { if (on) conv_set_thread_mfma_mode(prev); }
  ModeScope(const ModeScope&) = delete;
  ModeScope& operator=(const ModeScope&) = delete;
};
int amax_init(eosvos_engine* e) {
  if (e->amax) return 0;
  const size_t n = (size_t)AM_KINDS * e->t.convs.size() + 2 * TSLOTS;
  if (n > AMAX_ROW) return 1;
  e->amax = (unsigned*)e->falloc((int64_t)AMAX_SUB * AMAX_ROW);
  if (!e->amax) return 1;
  (void)hipMemsetAsync(e->amax, 0, (size_t)AMAX_SUB * AMAX_ROW * 4, e->s);
  e->amax_rec.assign((size_t)AM_KINDS * e->t.convs.size(), eosvos_engine::AmaxRec());
  e->ks_amax_valid.assign(e->t.convs.size(), 0);
  return 0;
}
inline unsigned* amax_slot(eosvos_engine* e, int kind, int ci) { return e->amax + amax_col(e, kind, ci); }
// host-side record of slot (kind, ci)
inline eosvos_engine::AmaxRec& amax_rec_of(eosvos_engine* e, int kind, int ci) { return e->amax_rec[(size_t)kind * e->t.convs.size() + ci]; }
// the tensor's slot; nullptr when the phase's table is full
unsigned* tslot(eosvos_engine* e, Tensor& t) {
  const int idx = e->ts.slot_of(t);
  return idx < 0 ? nullptr : e->amax + amax_tcol(e, t.phase, idx);
}
// a kernel is about to write (part of) the tensor: until a writer that covers it whole reports the fused sibling write
// (pair_covered), the sibling is stale
inline void pair_uncover(Tensor& t) { t.pair.covered = false; }
// A kernel with the fused absmax is about to write the view.  What it must be handed: the tensor's absmax slot (f16x3 mode)
// and, for a writer that applies the ReLU, where the mask bytes go (none for a mask that no backward pass of this engine
// reads: inference, frozen region).
struct Written { unsigned* slot; uint8_t* mask; int ldmask; };
Written twrite_fused(eosvos_engine* e, const View& v) {
  pair_uncover(*v.t);
  Written w{nullptr, e->fwd_masks ? v.mask_to_write() : nullptr, v.ldmask()};
  if (!h3_mode() || amax_init(e)) return w;
  w.slot = tslot(e, *v.t);
  if (w.slot && v.whole()) v.t->valid = true;
  return w;
}
// a kernel WITHOUT the fused absmax writes into the tensor
void twrite_plain(Tensor& t) {
  pair_uncover(t);
  if (h3_mode()) t.valid = false;
}
// every writer of the tensor since the phase began went into its slot (the caller has checked that)
void tmark_valid(Tensor& t) {
  if (t.slot >= 0) t.valid = true;
}
// consumer: the tensor's slot if it can be trusted
const unsigned* tlookup(eosvos_engine* e, const Tensor& t) {
  return t.slot >= 0 && t.valid ? e->amax + amax_tcol(e, t.phase, t.slot) : nullptr;
}
// a new forward (phase 0) / backward (phase 1) epoch: its slots are zeroed in one memset
void amax_new_phase(eosvos_engine* e, int phase) {
  if (!h3_mode() || amax_init(e)) return;
  const size_t nc = e->t.convs.size();
  long& ep = phase == 0 ? e->fwd_epoch : e->bwd_epoch;
  ++ep;
  const int k0 = phase == 0 ? AM_X : AM_G;
  amax_zero(amax_slot(e, k0, 0), 2 * nc + TSLOTS, e->s);     // the two kinds + the phase's tensor slots
  for (size_t i = k0 * nc; i < (k0 + 2) * nc; ++i) e->amax_rec[i].zero_epoch = ep;
  e->ts.new_phase(phase);
}
// absmax of the [rows x C] view at `ptr` into slot (kind, ci) -- computed once per epoch and view
const unsigned* amax_get(eosvos_engine* e, int kind, int ci, const float* ptr, long rows, int C, int ld, hipStream_t st) {
  if (amax_init(e)) return nullptr;
  const long ep = (kind == AM_X || kind == AM_V) ? e->fwd_epoch : e->bwd_epoch;
  unsigned* slot = amax_slot(e, kind, ci);
  auto& r = amax_rec_of(e, kind, ci);
  if (r.epoch == ep && r.ptr == ptr) return slot;
  if (trace_on()) fprintf(stderr, "EOSVOS_AMAX kind=%d conv=%d rows=%ld C=%d ld=%d memset=%d\n", kind, ci, rows, C, ld, (int)(r.zero_epoch != ep));
  if (r.zero_epoch != ep) amax_zero(slot, 1, st);      // not covered by the epoch's bulk zeroing, or used since
  launch_absmax(ptr, rows, C, ld, slot, st);
  r.epoch = ep; r.zero_epoch = -1; r.ptr = ptr;
  return slot;
}
// slot (kind, ci) is about to be filled by the kernel that writes the tensor at `ptr` (V, DM: the Winograd transforms)
unsigned* amax_fused_slot(eosvos_engine* e, int kind, int ci, const float* ptr, hipStream_t st) {
  if (!h3_mode() || amax_init(e)) return nullptr;
  const long ep = (kind == AM_X || kind == AM_V) ? e->fwd_epoch : e->bwd_epoch;
  unsigned* slot = amax_slot(e, kind, ci);
  auto& r = amax_rec_of(e, kind, ci);
  if (r.zero_epoch != ep) amax_zero(slot, 1, st);
  r.epoch = ep; r.zero_epoch = -1; r.ptr = ptr;
  return slot;
}
// a slot that lives until the weights / the norm change (W, U, US, KS): the caller tracks validity
const unsigned* amax_make(eosvos_engine* e, int kind, int ci, const float* ptr, long rows, int C, int ld, hipStream_t st) {
  if (amax_init(e)) return nullptr;
  unsigned* slot = amax_slot(e, kind, ci);
  amax_zero(slot, 1, st);
  launch_absmax(ptr, rows, C, ld, slot, st);
  return slot;
}
// W slots of every conv (one pass over the parameter arena), on stream st
void amax_weights(eosvos_engine* e, hipStream_t st) {
  if (e->w_amax_valid || amax_init(e)) return;
  const size_t nc = e->t.convs.size();
  if (!e->amax_w_off) {
    std::vector<long> off(nc);
    std::vector<int> n(nc);
    for (size_t ci = 0; ci < nc; ++ci) {
      const ConvL& c = e->t.convs[ci];
      off[ci] = (long)c.poff;
      n[ci] = ((c.cin & 3) || (c.poff & 3)) ? 0 : (int)c.wsize();      // the stem (cin 3) has its own kernels
    }
    e->amax_w_off = (long*)e->falloc((int64_t)nc * 2);
    e->amax_w_n = (int*)e->falloc((int64_t)nc);
    if (!e->amax_w_off || !e->amax_w_n) return;
    (void)hipMemcpy(e->amax_w_off, off.data(), nc * sizeof(long), hipMemcpyHostToDevice);
    (void)hipMemcpy(e->amax_w_n, n.data(), nc * sizeof(int), hipMemcpyHostToDevice);
  }
  amax_zero(amax_slot(e, AM_W, 0), nc, st);
  launch_absmax_segments(e->Wp, e->amax_w_off, e->amax_w_n, (int)nc, amax_slot(e, AM_W, 0), st);
  e->w_amax_valid = true;
}
const unsigned* amax_ks(eosvos_engine* e, int ci, hipStream_t st) {
  if (amax_init(e) || !e->A_(ci)) return nullptr;
  if (!e->ks_amax_valid[ci]) {
    amax_make(e, AM_KS, ci, e->A_(ci), 1, e->t.convs[ci].cout, e->t.convs[ci].cout, st);
    e->ks_amax_valid[ci] = 1;
  }
  return amax_slot(e, AM_KS, ci);
}
// Winograd-domain weights are about to be (re)made on stream st: zeroes the U and US slots (adjacent kinds), which the
// transform kernel then fills; returns the U slot (US = U slot + nconv), nullptr outside the f16x3 mode
unsigned* amax_wino_weights(eosvos_engine* e, int ci, hipStream_t st) {
  if (!h3_mode() || amax_init(e)) return nullptr;
  unsigned* u = amax_slot(e, AM_U, ci);
  if (e->us_zero_epoch != e->fwd_epoch) {          // else: forward_impl zeroed every U / US slot of this epoch at once
    amax_zero(u, 1, st);
    amax_zero(amax_slot(e, AM_US, ci), 1, st);
  }
  return u;
}

int upload_resize(eosvos_engine* e, const HostResize& h, int in, int out, ResizeTab& tab) {
  int* ib = (int*)e->falloc(2 * out + 2 * in);
  float* lam = e->falloc(out);
  if (!ib || !lam) return fail("hipMalloc resize table");
  HIPOK(hipMemcpy(ib, h.i0.data(), out * 4, hipMemcpyHostToDevice));
  HIPOK(hipMemcpy(ib + out, h.i1.data(), out * 4, hipMemcpyHostToDevice));
  HIPOK(hipMemcpy(ib + 2 * out, h.lo.data(), in * 4, hipMemcpyHostToDevice));
  HIPOK(hipMemcpy(ib + 2 * out + in, h.hi.data(), in * 4, hipMemcpyHostToDevice));
  HIPOK(hipMemcpy(lam, h.lam.data(), out * 4, hipMemcpyHostToDevice));
  tab.in = in; tab.out = out; tab.i0 = ib; tab.i1 = ib + out; tab.lo = ib + 2 * out; tab.hi = ib + 2 * out + in;
  tab.lam = lam;
  return 0;
}

// ---- conv helpers -----------------------------------------------------------------------------
// Dilated 3x3 convs on the stride-16 map: drop the (tile, tap) K steps whose tap falls into the
// padding for every pixel of the tile.  Tables are built once per (conv, pass, batch).
void attach_tap_table(eosvos_engine* e, int ci, int kind, int B, ConvArgs& a) {
  const ConvL& c = e->t.convs[ci];
  const bool dilated = c.k == 3 && c.dil >= 2 && a.upshift == 0;
  const bool s2_dgrad = c.k == 3 && kind == 1 && a.upshift == 1 && !a.dst_up;    // 2.25 of 9 taps per pixel on average
  if (!dilated && !s2_dgrad) return;
  const int bn = conv_bn(a);
  const long tiles = (long)((a.M + 127) / 128) * ((a.N + bn - 1) / bn);
  if (tiles > 1024) return;                       // keep the partial-tile slab count bounded
  const long key = ((long)ci * 2 + kind) * 64 + B;
  auto it = e->tap_tabs.find(key);
  if (it == e->tap_tabs.end()) {
    std::vector<int> prefix, mask;
    ConvArgs probe = a;
    probe.par = s2_dgrad ? 1 : 0;
    const long total = conv_build_tap_table(probe, prefix, mask);
    eosvos_engine::TapTab tt{nullptr, nullptr, total, nullptr};
    tt.prefix = (int*)e->falloc((int64_t)prefix.size());
    tt.mask = (int*)e->falloc((int64_t)mask.size());
    tt.order = (int*)e->falloc((int64_t)mask.size());
    if (!tt.prefix || !tt.mask || !tt.order) return;
    // tiles by descending K steps: the whole-tile plan deals them out longest first (conv_plan, launches with >= budget tiles)
    std::vector<int> order(mask.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return prefix[x + 1] - prefix[x] > prefix[y + 1] - prefix[y]; });
    if (hipMemcpy(tt.prefix, prefix.data(), prefix.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return;
    if (hipMemcpy(tt.mask, mask.data(), mask.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return;
    if (hipMemcpy(tt.order, order.data(), order.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return;
    it = e->tap_tabs.emplace(key, tt).first;
  }
  if (it->second.total >= tiles * (long)c.T() * ((a.Kc + 31) / 32)) return;   // nothing to skip
  a.tprefix = it->second.prefix; a.tmask = it->second.mask; a.total_units = it->second.total; a.torder = it->second.order;
  a.par = s2_dgrad ? 1 : 0;
}

// EOSVOS_TRACE=1: one stderr line per MFMA launch (joined with rocprofv3's kernel trace by
// tools/layer_report.py to get per-layer TFLOP/s)
bool trace_on() {
  static int on = -1;
  if (on < 0) { const char* v = getenv("EOSVOS_TRACE"); on = (v && v[0] == '1') ? 1 : 0; }
  return on == 1;
}
// `frac`: share of the nominal M*N*K multiply-accumulates the launch executes (filter taps that fall into the padding
// are skipped by the tap tables / contributing-pixel rectangles): flops = executed, not 9-tap-equivalent
thread_local eosvos_engine* tl_plan_engine = nullptr;
thread_local int tl_plan_phase = 0;
inline void plan_mix(uint64_t v) {
  if (!tl_plan_engine) return;
  uint64_t& h = tl_plan_engine->plan_fp[tl_plan_phase];
  for (int i = 0; i < 8; ++i) { h ^= (v >> (8 * i)) & 0xffu; h *= 0x100000001b3ull; }
}
inline void plan_begin(eosvos_engine* e, int phase) { tl_plan_engine = e; tl_plan_phase = phase; e->plan_fp[phase] = 0xcbf29ce484222325ull; }
// One forward_impl / backward_impl records into its engine's fingerprint and nothing else does: the scope clears the
// thread's recording engine on every exit (error returns included), so later launches -- a scratch engine of a test entry
// point, eosvos_bench_conv -- neither mix into a live engine's plan nor write into a destroyed one.
struct PlanScope {
  PlanScope(eosvos_engine* e, int phase) { plan_begin(e, phase); }
  ~PlanScope() { tl_plan_engine = nullptr; }
  PlanScope(const PlanScope&) = delete;
  PlanScope& operator=(const PlanScope&) = delete;
};
// the line alone, not mixed into the plan fingerprint: launches that cover several convs and sum their flops themselves (grouped
// weight gradients: conv = the first member, M x N = the tile, splits = workgroups; the merged ASPP data gradient)
void trace_line(const char* kind, int ci, long M, long N, long K, int splits, double flops) {
  if (trace_on()) fprintf(stderr, "EOSVOS_TRACE %s conv=%d M=%ld N=%ld K=%ld splits=%d flops=%.0f\n", kind, ci, M, N, K, splits, flops);
}
void trace(const char* kind, int ci, long M, long N, long K, int splits, double frac = 1.0) {
  plan_mix((uint64_t)(unsigned char)kind[0] | ((uint64_t)(unsigned char)kind[1] << 8) | ((uint64_t)strlen(kind) << 16));
  plan_mix((uint64_t)ci); plan_mix((uint64_t)M); plan_mix((uint64_t)N); plan_mix((uint64_t)K); plan_mix((uint64_t)splits);
  trace_line(kind, ci, M, N, K, splits, 2.0 * M * N * K * frac);
}
// ---- pre-split operand path ---------------------------------------------------------------------------------------------
// Weight gradients whose channel counts are multiples of 256 (layer3, layer4, ASPP) run on wgrad_p_kernel (presplit_kernels.hip)
// in the f16x3 mode: 1.3-1.7x the register-staged kernel per launch (profiles/r06_wgrad_p_probe.txt).  EOSVOS_PRESPLIT=0: off.
int g_presplit = -1;               // process-wide switch (eosvos_set_presplit); -1: not read from the environment yet
bool presplit_switch() {
  if (g_presplit < 0) g_presplit = (getenv("EOSVOS_PRESPLIT") && atoi(getenv("EOSVOS_PRESPLIT")) == 0) ? 0 : 1;
  return g_presplit != 0;
}
// Only engines WITH a side stream take the path (or every engine under EOSVOS_TUNE_PRESPLIT_INFLIGHT=1, read when the engine is
// built: single-stream profiling).  An engine without one runs beside other engines (the objects of a sequence, the tasks of a
// meta-batch in flight: eosvos_set_side_stream): a 256 x 256 workgroup owns its CU, and several engines' one-per-CU launches
// block each other -- measured end to end on a two-object 70-frame sequence with the objects in flight
// (profiles/r06_eval_sequence_time.txt): e-OSVOS-50 0.505 -> 0.617 s per object with the path, e-OSVOS-100-OnA 1.85 -> 1.95.
bool presplit_enabled(const eosvos_engine* e) {
  return presplit_switch() && h3_mode() && e->force_algo == 0 && (e->s2 || e->presplit_inflight);
}
bool presplit_wgrad_shape(const ConvL& c, int P, int ldg, int ldx) {
  // (minimum pixel count: at batch 1 -- 1620 pixels on the stride-16 map, 50 K steps for 256 x 256 tiles -- the path is 4 % slower
  // than the register-staged kernels, profiles/r06_ab_log.txt; batch 3 = 4860 pixels)
  const int minp = g_presplit == 2 ? 1 : 4000;          // eosvos_set_presplit(2): every eligible shape (tests on small maps)
  // (stride 1 only: the inputs of the strided convs are the large maps of the previous stage, whose producers -- the streaming
  // kernels -- write no siblings: a split pass over 40-80 MB per step costs more than the kernel gains)
  return c.cout % 256 == 0 && c.cin % 256 == 0 && c.stride == 1 && ldg % 8 == 0 && ldx % 8 == 0 && P >= minp;
}
constexpr int PAIR_SC_POOL = 3072;
// the tensor's sibling ([rows][C] floats), allocated on first use; nullptr: out of memory
PairBuf* pair_buf(eosvos_engine* e, Tensor& t, long rows) {
  PairBuf& pb = t.pair;
  const int64_t need = (int64_t)rows * t.C;
  if (!e->pair_zero) {
    e->pair_zero = (unsigned char*)e->falloc(1024);
    e->pair_sc_pool = e->falloc(PAIR_SC_POOL);
    if (!e->pair_zero || !e->pair_sc_pool) return nullptr;
    (void)hipMemsetAsync(e->pair_zero, 0, 4096, e->s);
    (void)hipMemsetAsync(e->pair_sc_pool, 0, PAIR_SC_POOL * 4, e->s);
  }
  if (pb.floats < need) {
    // (the scale words first: a sibling is committed, and with that handed out by later calls, only together with them)
    if (!pb.sc && e->pair_sc_used + 3 > PAIR_SC_POOL) return nullptr;
    pb.p = (unsigned char*)e->falloc(need);
    if (!pb.p) { pb.floats = 0; return nullptr; }
    if (!pb.sc) {
      pb.sc = e->pair_sc_pool + e->pair_sc_used;
      e->pair_sc_used += 3;
    }
    pb.floats = need; pb.covered = false; pb.fresh = true;
  }
  return &pb;
}
// conv epilogue / fix-up about to write the whole tensor through the view y (the launch's arguments are filled): hand it the
// sibling if one is wanted
void pair_attach(eosvos_engine* e, const View& y, ConvArgs& a) {
  a.y2 = nullptr; a.y2_sc = nullptr; a.y2_done = 0;
  if (!presplit_enabled(e) || e->gn() || !y.whole() || a.dst_up || a.par || a.plane_rows) return;
  if (y.t->phase == 0 && !e->fwd_masks) return;                  // inference forward: no backward pass will read it
  const PairBuf& pb = y.t->pair;
  if (!pb.want || pb.fresh || !pb.p || (a.ldy & 7) || (a.N & 7)) return;
  if ((int64_t)a.M * a.ldy > pb.floats) return;
  a.y2 = y.sibling();
  a.y2_sc = pb.sc + 1 + (e->pair_iter & 1);
  if (trace_on()) fprintf(stderr, "EOSVOS_PAIR attach phase=%d M=%d N=%d ldy=%d\n", y.t->phase, a.M, a.N, a.ldy);
}
// after the launch: it wrote the sibling too
void pair_covered(eosvos_engine* e, Tensor& t, const ConvArgs& a) {
  if (!a.y2 || !a.y2_done) return;
  t.pair.covered = true;
  t.pair.cover_iter = e->pair_iter;
}
// a new trajectory (reset / new state / another batch size): the producers' scales of the previous one are forgotten; the
// first iteration runs on the register-staged kernels (which leave fresh scales), the pre-split path resumes with the second
// -- results do not depend on what the engine ran before
void pair_reset(eosvos_engine* e) {
  if (!e->pair_sc_pool) return;
  (void)hipMemsetAsync(e->pair_sc_pool, 0, PAIR_SC_POOL * 4, e->s);
  for (Tensor& t : e->ts.all) { t.pair.covered = false; t.pair.fresh = true; }
}
// Winograd F(2x2,3x3) / F(4x4,3x3) path (forward, data gradient, weight gradient) of 3x3 / stride 1 convs: 2.25x / 4x fewer MACs,
// paid for with HBM-bound transform passes.  Always on for the decoder's two convs on the stride-4 map (27 % of a
// batch-3 iteration's FLOPs); for the dilated / undilated conv2 of layer3 / layer4 only when the launch is large
// enough for the extra passes to pay (EOSVOS_WINO_MINWORK multiply-accumulates per Winograd position).
struct WinoGeom { int th, tw, d, tm, np; long ntile, prow; };
// F(4x4,3x3) (36 positions, 2.25 MACs per output) for undilated convs on maps of >= 64 x 64 outputs -- the decoder --
// where 4x4 tiles waste little at the border; F(2x2,3x3) (16 positions, 4 MACs per output) otherwise.
#define EOSVOS_WINO_F4_MINDIM 64
bool wino_f4(const eosvos_engine* e, const ConvL& c, int Ho, int Wo) {
  if (e->force_algo == EOSVOS_ALGO_WINO_F2) return false;
  if (e->force_algo == EOSVOS_ALGO_WINO_F4) return true;
  // large undilated maps (the decoder), or dilated convs whose sub-grids tile well with 4x4
  if (c.dil == 1) return Ho >= EOSVOS_WINO_F4_MINDIM && Wo >= EOSVOS_WINO_F4_MINDIM;
  return c.dil == 2 || c.dil == 4 || c.dil == 8;
}
WinoGeom wino_geom(const eosvos_engine* e, const ConvL& c, int B, int Ho, int Wo) {
  WinoGeom g;
  g.d = c.dil;
  g.tm = wino_f4(e, c, Ho, Wo) ? 4 : 2;
  g.np = (g.tm + 2) * (g.tm + 2);
  g.th = ((Ho + g.d - 1) / g.d + g.tm - 1) / g.tm;       // output tiles per sub-grid of a dilated conv
  g.tw = ((Wo + g.d - 1) / g.d + g.tm - 1) / g.tm;
  g.ntile = (long)B * g.d * g.d * g.th * g.tw;
  g.prow = (g.ntile + 127) / 128 * 128;                  // plane rows padded to the GEMM tile
  return g;
}
#define EOSVOS_WINO_MINWORK 100000000LL                // measured: layer4 conv2 and the d = 6 ASPP conv gain, layer2/3 conv2 do not
bool wino_shape(const ConvL& c) {
  return c.k == 3 && c.stride == 1 && c.pad == c.dil && c.dil >= 1 && c.dil <= 8 && (c.cin & 3) == 0 && (c.cout & 3) == 0;
}
bool wino_on(const eosvos_engine* e, int ci, int B, int Ho, int Wo) {
  const ConvL& c = e->t.convs[ci];
  if (e->force_algo == EOSVOS_ALGO_DIRECT) return false;
  if (!wino_shape(c)) return false;
  if (e->force_algo == EOSVOS_ALGO_WINO_F2 || e->force_algo == EOSVOS_ALGO_WINO_F4) return e->wino[ci].V != nullptr;
  if (ci == e->t.dec_a || ci == e->t.dec_b) return true;
  if (!e->wino[ci].V) return false;            // no buffers were reserved for it
  // f16x3 mode: the matrix kernels are 1.3-1.5x faster, the HBM-bound transforms are not -- layer4's conv2 and the d = 6 ASPP
  // conv no longer gain (same box, batch 1: 5.62 -> 5.45 ms without them, batch 3: 9.97 -> 9.93); the decoder keeps its F(4,3)
  if (conv_mfma_mode() == 2) return false;
  return (long long)B * Ho * Wo / 4 * c.cin * c.cout >= EOSVOS_WINO_MINWORK;      // MACs of one F(2,3) position
}
// The batched plane GEMM of a Winograd pass: rows = np planes x prow tiles of x, one [cout][cin] weight matrix per plane.
// Forward (kmajor 0): V x U -> M planes, K = cin, N = cout; data gradient (kmajor 1): dM x Us -> dV planes, K = cout, N = cin
ConvArgs wino_plane_gemm(const eosvos_engine* e, const ConvL& c, const WinoGeom& wg, const float* x, const float* w, float* y,
                         float* ws, int kmajor) {
  const int K = kmajor ? c.cout : c.cin, N = kmajor ? c.cin : c.cout;
  ConvArgs m;
  memset(&m, 0, sizeof(m));
  m.wg_budget = e->wg_budget;
  m.x = x; m.w = w; m.y = y; m.ws = ws; m.nplanes = wg.np;
  m.B = 1; m.Hi = 1; m.Wi = (int)(wg.np * wg.prow); m.ldx = K; m.Kc = K;
  m.Ho = 1; m.Wo = m.Wi; m.N = N; m.ldy = N; m.KH = m.KW = 1; m.mul = 1;
  m.M = m.Wi; m.wN = c.cout; m.wK = c.cin; m.kmajor = kmajor; m.plane_rows = (int)wg.prow; m.w_plane = (long)c.cout * c.cin;
  return m;
}
// U = G w G^T and Us = a[cout] * U (the data gradient's copy) of conv ci: remade on stream st when the weights changed
// since they were last made
void wino_ensure_weights(eosvos_engine* e, int ci, int tm, hipStream_t st) {
  auto& w = e->wino[ci];
  if (w.us_valid) return;
  const ConvL& c = e->t.convs[ci];
  unsigned* us = amax_wino_weights(e, ci, st);
  launch_wino_weight(tm, e->W_(ci), c.cout, c.cin, e->A_(ci), w.U, w.Us, st, us, us ? us + e->t.convs.size() : nullptr);
  w.us_valid = true;
}
// The optional operands and the flags of conv_fwd / conv_dgrad (as ConvArgs holds them: one set for both passes), named at
// the call: conv_fwd(e, ci, x, y, B, Opt().relu().add(res)), conv_dgrad(e, ci, g, gx, B, Opt().accum().mask(x, 256)).
struct Opt {
  View add_;                       // forward: the residual; data gradient: a gradient added in front of the mask
  bool relu_ = false, side_ = false, accum_ = false;
  const Tensor* mask_ = nullptr;
  int mask_c0_ = 0;
  Opt& add(const View& v) { add_ = v; return *this; }
  Opt& relu(bool on = true) { relu_ = on; return *this; }
  // launch on the side stream with its own stream-K workspace (forward branches that do not depend on each other:
  // downsample convs, decoder.conv1)
  Opt& side(bool on = true) { side_ = on; return *this; }
  Opt& accum(bool on = true) { accum_ = on; return *this; }
  // zero where the ReLU mask of `x` (the forward activation gx is the gradient of: same layout) is clear, in channels >= c0
  Opt& mask(const Tensor* x, int c0 = 0) { mask_ = x; mask_c0_ = c0; return *this; }
};
// y = conv ci of x (the map size is x's tensor's)
void conv_fwd(eosvos_engine* e, int ci, const View& xv, const View& yv, int B, const Opt& o = Opt()) {
  const float *x = xv.ptr(), *res = o.add_.ptr();
  float* y = yv.ptr();
  const int ldx = xv.ld(), ldy = yv.ld(), ldres = o.add_.ld(), Hi = xv.t->H, Wi = xv.t->W;
  const bool relu = o.relu_, side = o.side_;
  const ConvL& c = e->t.convs[ci];
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.wg_budget = e->wg_budget;
  hipStream_t st = side ? e->s2 : e->s;
  const Written yw = twrite_fused(e, yv);
  a.x = x; a.w = e->W_(ci); a.y = y; a.ws = side ? e->ws_conv2 : e->ws_conv;
  a.B = B; a.Hi = Hi; a.Wi = Wi; a.ldx = ldx; a.Kc = c.cin;
  a.Ho = conv_out(Hi, c.k, c.stride, c.dil, c.pad); a.Wo = conv_out(Wi, c.k, c.stride, c.dil, c.pad);
  a.N = c.cout; a.ldy = ldy; a.KH = a.KW = c.k;
  a.mul = c.stride; a.off0 = -c.pad; a.kstep = c.dil; a.upshift = 0;
  a.M = B * a.Ho * a.Wo; a.wN = c.cout; a.wK = c.cin; a.kmajor = 0;
  const bool gn = e->gn() && c.norm;
  if (!side && wino_on(e, ci, B, a.Ho, a.Wo)) {
    // Winograd forward: U = G w G^T, V = B^T d B (kept for the weight gradient), 16 GEMMs [tiles x cin] x [cin x cout]
    // as one batched launch (2.25x fewer MACs than the 9-tap form), y = epilogue(A^T M A)
    const WinoGeom wg = wino_geom(e, c, B, a.Ho, a.Wo);
    const int th = wg.th, tw = wg.tw;
    const long prow = wg.prow;
    // U = G w G^T (and a[cout] * U for the data gradient) only when the weights changed since it was last made; a
    // forward with a side stream has already queued all of them there (forward_impl), beside layer1..3
    if (e->wino_w_wait) { (void)hipStreamWaitEvent(st, e->ev_wino_w, 0); e->wino_w_wait = false; }
    wino_ensure_weights(e, ci, wg.tm, st);
    auto& w = e->wino[ci];
    unsigned* vslot = amax_fused_slot(e, AM_V, ci, w.V, st);   // the input transform accumulates max|V| itself
    launch_wino_input(wg.tm, x, ldx, c.cin, B, Hi, Wi, th, tw, wg.d, prow, w.V, st, vslot);
    w.v_batch = B;
    ConvArgs m = wino_plane_gemm(e, c, wg, w.V, w.U, e->wino_m, a.ws, 0);
    if (vslot) { m.amax_x = vslot; m.amax_w = amax_slot(e, AM_U, ci); }
    // the output transform writes y (directly, or the raw conv output of the GroupNorm mode)
    // (GroupNorm mode: the output transform writes the raw conv output; y and its absmax come from the GroupNorm apply pass)
    trace("fwd", ci, m.M, m.N, c.cin, conv_plan(m));
    launch_conv(m, st);
    launch_wino_output(wg.tm, e->wino_m, prow, c.cout, B, a.Ho, a.Wo, th, tw, wg.d, gn ? nullptr : e->A_(ci), gn ? nullptr : e->B_(ci),
                       (!gn && relu) ? 1 : 0, gn ? e->zbuf[ci]->p : y, gn ? c.cout : ldy, st, gn ? nullptr : yw.slot,
                       gn ? nullptr : yw.mask, yw.ldmask);
    if (gn)
      launch_gn_forward(e->zbuf[ci]->p, c.cout, e->G_(ci), e->nb + c.noff, res, ldres, y, ldy, e->gn_stats[ci], e->gn_partial, B,
                        a.Ho * a.Wo, c.cout, 1e-5f, relu ? 1 : 0, st, yw.slot, relu ? yw.mask : nullptr, yw.ldmask);
    return;
  }
  if (gn) {                       // raw conv output -> GroupNorm kernels (statistics are data dependent)
    a.y = e->zbuf[ci]->p; a.ldy = c.cout;
  } else {
    a.scale = e->A_(ci); a.bias = e->B_(ci);
    a.res = res; a.ldres = ldres; a.relu = relu ? 1 : 0;
    if (relu && yw.mask) { a.mask8_out = yw.mask; a.ldm8_out = yw.ldmask; }
  }
  attach_tap_table(e, ci, 0, B, a);
  if (h3_mode() && !amax_init(e)) {
    amax_weights(e, st);
    a.amax_x = tlookup(e, *xv.t);
    if (!a.amax_x) a.amax_x = amax_get(e, AM_X, ci, x, (long)B * Hi * Wi, c.cin, ldx, st);
    a.amax_w = amax_slot(e, AM_W, ci);
    if (!gn) a.amax_y = yw.slot;      // GroupNorm mode: y (and its absmax) is written by the apply pass
  }
  if (!gn && !side) pair_attach(e, yv, a);
  trace("fwd", ci, a.M, a.N, (long)c.T() * c.cin, conv_plan(a), conv_exec_frac(a));
  launch_conv(a, st);
  pair_covered(e, *yv.t, a);
  if (gn)
    launch_gn_forward(e->zbuf[ci]->p, c.cout, e->G_(ci), e->nb + c.noff, res, ldres, y, ldy, e->gn_stats[ci], e->gn_partial, B,
                      a.Ho * a.Wo, c.cout, 1e-5f, relu ? 1 : 0, st, yw.slot, relu ? yw.mask : nullptr, yw.ldmask);
}
// A data-gradient GEMM whose N leaves a tail of <= 64 columns over whole 128-wide column tiles, e.g. the decoder's 304
// input channels: 2 column tiles of 128 + a 64-wide launch instead of 3 x 128 (the 128-wide kernel would spend a third of
// its MFMAs on 80 padding columns)
bool dgrad_has_tail(const ConvArgs& a) { return a.N > 128 && a.N % 128 > 0 && a.N % 128 <= 64; }
void launch_dgrad_tail_split(eosvos_engine* e, int ci, ConvArgs a, long K) {
  const int tail = a.N % 128;
  ConvArgs b = a;
  a.N -= tail;
  trace("dgrad", ci, a.M, a.N, K, conv_plan(a));
  launch_conv(a, e->s);
  b.N = tail; b.w += a.N; b.y += a.N;
  if (b.mask8) { b.mask8 += a.N / 4; b.mask_c0 = b.mask_c0 > a.N ? b.mask_c0 - a.N : 0; }      // (the Winograd plane GEMM has neither)
  if (b.res) b.res += a.N;
  trace("dgrad", ci, b.M, b.N, K, conv_plan(b));
  launch_conv(b, e->s);
}
// gx[B,Hin,Win,cin] (+)= dgrad of conv ci applied to g[B,Ho,Wo,cout] (+ add) (the map size is gx's tensor's).  The mask
// tensor must have mask bytes (Tensor::mask); a masked gradient without them is an error, never an unmasked result.
int conv_dgrad(eosvos_engine* e, int ci, View gv, const View& gxv, int B, const Opt& o = Opt()) {
  const uint8_t* mask8 = o.mask_ ? o.mask_->mask : nullptr;
  if (o.mask_ && !mask8) return fail("internal: a masked data gradient of conv " + std::to_string(ci) + " has no ReLU mask bytes");
  const ConvL& c = e->t.convs[ci];
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.wg_budget = e->wg_budget;
  if (e->gn() && c.norm) gv = View(e->zbuf[ci]);   // gradient w.r.t. the raw conv output (conv_wgrad made it)
  const float *g = gv.ptr(), *add = o.add_.ptr();
  float* gx = gxv.ptr();
  const int ldg = gv.ld(), ldgx = gxv.ld(), ldadd = o.add_.ld(), Hin = gxv.t->H, Win = gxv.t->W;
  unsigned* const gxs = twrite_fused(e, gxv).slot;
  a.x = g; a.w = e->W_(ci); a.y = gx; a.ws = e->ws_conv;
  a.B = B; a.Hi = conv_out(Hin, c.k, c.stride, c.dil, c.pad); a.Wi = conv_out(Win, c.k, c.stride, c.dil, c.pad);
  a.ldx = ldg; a.Kc = c.cout;
  a.Ho = Hin; a.Wo = Win; a.N = c.cin; a.ldy = ldgx; a.KH = a.KW = c.k;
  a.mul = 1; a.off0 = c.pad; a.kstep = -c.dil; a.upshift = c.stride == 2 ? 1 : 0;
  a.M = B * Hin * Win; a.wN = c.cout; a.wK = c.cin; a.kmajor = 1;
  a.kscale = e->A_(ci);
  a.mask8 = mask8; a.ldm8 = gxv.ldmask(); a.mask_c0 = o.mask_c0_; a.accum = o.accum_ ? 1 : 0;
  a.res = add; a.ldres = ldadd;
  const bool wino_dg = !add && wino_on(e, ci, B, Hin, Win);
  if (h3_mode() && !wino_dg && !amax_init(e)) {
    amax_weights(e, e->s);
    a.amax_x = tlookup(e, *gv.t);
    if (!a.amax_x) a.amax_x = amax_get(e, AM_G, ci, g, (long)B * a.Hi * a.Wi, c.cout, ldg, e->s);
    a.amax_w = amax_slot(e, AM_W, ci);
    a.amax_ks = amax_ks(e, ci, e->s);
    a.amax_y = gxs;
  }
  if (wino_dg) {
    // Winograd data gradient: dV[p] = dM[p] (a[cout] U[p]), 16 / 36 GEMMs [tiles x cout] x [cout x cin] in one batched
    // launch, then dX = mask(B dV B^T) gathered per 2x2 / 4x4 pixel block
    const WinoGeom wg = wino_geom(e, c, B, Hin, Win);
    const int th = wg.th, tw = wg.tw;
    const long prow = wg.prow;
    auto& w = e->wino[ci];
    if (w.dm_batch != B) {
      unsigned* dms = amax_fused_slot(e, AM_DM, ci, w.dM, e->s);
      launch_wino_grad(wg.tm, g, ldg, c.cout, B, Hin, Win, th, tw, wg.d, prow, w.dM, e->s, dms);
    }
    w.dm_batch = 0;
    wino_ensure_weights(e, ci, wg.tm, e->s);         // no forward since the weights changed: rebuild a[cout] * U
    ConvArgs m = wino_plane_gemm(e, c, wg, w.dM, w.Us, e->wino_dv, e->ws_conv, 1);
    if (h3_mode() && !amax_init(e)) {
      m.amax_x = amax_get(e, AM_DM, ci, w.dM, (long)wg.np * prow, c.cout, c.cout, e->s);   // made by the transform
      m.amax_w = amax_slot(e, AM_US, ci);
    }
    if (dgrad_has_tail(m)) {
      launch_dgrad_tail_split(e, ci, m, c.cout);
    } else {
      trace("dgrad", ci, m.M, m.N, c.cout, conv_plan(m));
      launch_conv(m, e->s);
    }
    launch_wino_dgrad_output(wg.tm, e->wino_dv, prow, c.cin, B, Hin, Win, th, tw, wg.d, mask8, a.ldm8, a.mask_c0, a.accum, gx, ldgx, e->s, gxs);
    return 0;
  }
  if (c.k == 1 && c.stride == 2 && !add) {
    // only the even pixels of the finer grid receive a contribution: run the GEMM on the
    // coarse grid (4x less MFMA work) and scatter; untouched pixels are zero (or keep their sum)
    if (!a.accum) (void)hipMemsetAsync(gx, 0, (size_t)B * Hin * Win * ldgx * sizeof(float), e->s);
    a.Ho = a.Hi; a.Wo = a.Wi; a.mul = 1; a.off0 = 0; a.kstep = 0; a.upshift = 0;
    a.M = B * a.Ho * a.Wo; a.dst_up = 1; a.Hf = Hin; a.Wf = Win;
  }
  if (dgrad_has_tail(a) && !a.dst_up && !(c.k == 3 && c.dil >= 2)) {
    launch_dgrad_tail_split(e, ci, a, (long)c.T() * c.cout);
    return 0;
  }
  attach_tap_table(e, ci, 1, B, a);
  pair_attach(e, gxv, a);
  trace("dgrad", ci, a.M, a.N, (long)c.T() * c.cout, conv_plan(a), conv_exec_frac(a));
  launch_conv(a, e->s);
  pair_covered(e, *gxv.t, a);
  return 0;
}
// Weight-gradient launches are queued and forked onto the side stream a few layers at a time: every
// hipEventRecord / hipStreamWaitEvent pair costs the main stream a ~6 us bubble (measured: 57 gaps per batch-1
// step with one fork per layer), and a weight gradient only needs tensors that stay valid until the end of the
// backward pass, so it can start a few layers late.
// Measured: at batch 1 (launch-bound layers) forking every 4 layers gains 1.8 %; at batch 3 the later start of the
// weight gradients costs more than the bubbles (+1.7 %), so there every layer forks at once.
#define EOSVOS_SIDE_BATCH 4
// Workgroup budget of the pre-split weight gradients.  Beside the data-gradient chain (engines with a side stream) they plan for
// THREE QUARTERS of the chip: a 256 x 256 workgroup owns its CU (128 KB of LDS: no conv workgroup fits beside it), so a launch that
// covers every CU makes the main stream's next data gradient wait for whole weight-gradient workgroups to finish, and one that
// covers too few runs long after the chain has ended.  Measured at batch 3, three interleaved rounds (profiles/r06_ab_log.txt):
// 100 % 8.89 ms, 88 % 8.75, 75 % 8.67, 63 % 8.65, 50 % 8.75, 25 % 9.37; the register-staged kernels 8.83.
int wgp_budget(const eosvos_engine* e) {
  constexpr int share = 75;          // percent
  int b = conv_wg_budget_of(e->wg_budget);
  if (e->s2) b = conv_clamp_wg_budget(std::max(64, b * share / 100 / 64 * 64));
  return b;
}
int pair_margin(int phase) {
  static const int margin_x = getenv("EOSVOS_TUNE_PAIR_MARGIN_X") ? atoi(getenv("EOSVOS_TUNE_PAIR_MARGIN_X")) : 2;
  static const int margin_g = getenv("EOSVOS_TUNE_PAIR_MARGIN_G") ? atoi(getenv("EOSVOS_TUNE_PAIR_MARGIN_G")) : 3;
  return phase == 0 ? margin_x : margin_g;
}
// consumer side: the sibling of the view's tensor is wanted from now on; true when this iteration's producers wrote it
bool pair_operand(eosvos_engine* e, const View& v, long rows, PairBuf*& pb) {
  // sized for the engine's largest batch: the sibling never moves (the grouped launches' device tables hold its address)
  const long rows_alloc = e->lastB > 0 ? rows / e->lastB * e->maxB : rows;
  pb = pair_buf(e, *v.t, std::max(rows, rows_alloc));
  if (!pb || v.c0 < 0 || v.c0 + (rows - 1) * (int64_t)v.ld() + v.C > pb->floats || (v.c0 & 7)) { pb = nullptr; return false; }
  pb->want = true;
  const bool cov = pb->covered && pb->cover_iter == e->pair_iter && !pb->fresh;
  if (trace_on())
    fprintf(stderr, "EOSVOS_PAIR operand phase=%d rows=%ld C=%d ld=%d covered=%d fresh=%d\n", v.t->phase, rows, v.C, v.ld(), (int)cov, (int)pb->fresh);
  return cov;
}
void side_flush(eosvos_engine* e) {
  if (e->side_q.empty()) return;
  (void)hipEventRecord(e->ev[0], e->s);            // everything the queued launches read is complete here
  (void)hipStreamWaitEvent(e->s2, e->ev[0], 0);
  for (auto& f : e->side_q) f(e->s2);
  e->side_q.clear();
  e->side_used = true;
}
// a weight-gradient launch: queued for the next fork onto the side stream (side_flush) when the engine has one, else at
// once on the main stream
template <class F>
void side_enqueue(eosvos_engine* e, F&& launch) {
  if (e->s2) e->side_q.emplace_back(std::forward<F>(launch));
  else launch(e->s);
}
// ---- grouped weight gradients ------------------------------------------------------------------------
// K splits of weight gradients that share ONE launch of equal tiles: the launch should fill the chip with workgroups of
// about equal K length.  tau = (sum of tiles x K steps) / workgroups the launch plans for; an item with `steps` K steps
// of 32 pixels is cut into ceil(steps / tau) splits (>= 4 steps each, at most 512).
struct KItem { long tiles, steps; };
std::vector<int> plan_equal_k(const std::vector<KItem>& items, long resident) {
  auto splits_of = [](const KItem& it, long tau) {
    const long sp = (it.steps + tau - 1) / tau;
    return sp > it.steps / 4 ? std::max<long>(1, it.steps / 4) : sp;
  };
  long work = 0;
  for (const auto& it : items) work += it.tiles * it.steps;
  // smallest tau whose workgroups all fit one resident round (a launch a little over one round would run its
  // last workgroups alone: measured 556 workgroups at 113 TFLOP/s against 864 = 1.7 rounds at 163)
  long tau = std::max<long>(4, (work + resident - 1) / resident);
  auto count = [&](long t) {
    long n = 0;
    for (const auto& it : items) n += it.tiles * splits_of(it, t);
    return n;
  };
  while (count(tau) > resident && tau < (1L << 20)) tau += std::max<long>(1, tau / 32);
  // (the cap of 512 plays no part in the search: an item cut more often is by itself more than a resident round, <= 512)
  std::vector<int> splits;
  for (const auto& it : items) splits.push_back((int)std::min<long>(splits_of(it, tau), 512));
  return splits;
}
// the register-staged kernels: one launch, hence one plan, per tile shape wgrad_group_tile(cout) x wgrad_group_tile(cin)
struct WgGroupItem { int ci, P, cout, cin, T; };
long wgrad_group_tiles(const WgGroupItem& it) {
  const int bm = wgrad_group_tile(it.cout), bn = wgrad_group_tile(it.cin);
  return (long)((it.cout + bm - 1) / bm) * ((it.cin + bn - 1) / bn) * it.T;
}
std::vector<int> plan_wgrad_splits(const std::vector<WgGroupItem>& items, int wg_budget) {
  std::vector<int> splits(items.size(), 1);
  for (int bm : {128, 64})
    for (int bn : {128, 64}) {
      std::vector<KItem> shape;
      std::vector<size_t> at;                      // shape[j] is items[at[j]]
      for (size_t k = 0; k < items.size(); ++k) {
        if (wgrad_group_tile(items[k].cout) != bm || wgrad_group_tile(items[k].cin) != bn) continue;
        shape.push_back({wgrad_group_tiles(items[k]), (items[k].P + 31) / 32});
        at.push_back(k);
      }
      const std::vector<int> sp = plan_equal_k(shape, conv_wg_budget_of(wg_budget));
      for (size_t j = 0; j < at.size(); ++j) splits[at[j]] = sp[j];
    }
  return splits;
}
bool wgrad_groupable(const eosvos_engine* e, int ci, int B) {
  // Measured at batch 3 (profiles/r03_ab_wgrad_group.txt): grouping layer3 (30 / 14 splits per conv -> 2, 578 -> 57 MB of
  // slabs) leaves the two-stream step time unchanged; grouping layer2 / layer1 as well makes it 1 % LONGER although the
  // summed kernel time drops by 0.3 ms -- their grouped launches start only after the stage's data-gradient chain and
  // the last one runs with nothing beside it.  Round 3's default with a side stream: layer3 only.  Re-measured in round 4
  // (streaming kernels in layer1 / layer2, whole-tile plans: profiles/r04_ab_log.txt): layer2 + layer3 at batch 3 (8.88 ->
  // 8.82 ms; with layer1 as well 8.91), every stage at batch 1 (4.65 -> 4.60 ms; layer2 + layer3 4.62).
  // An engine WITHOUT a side stream (it runs beside other engines, eosvos_set_side_stream) has no such overlap to lose:
  // every stage is grouped (4 tasks in flight at batch 1: 41.0 -> 41.9 meta-tasks/s).
  const int min_stage = e->s2 && B != 1 ? 1 : 0;
  return e->wg_group_on && conv_mfma_mode() >= 1 && e->force_algo == 0 && ci < (int)e->t.stage.size() &&
         e->t.stage[ci] >= min_stage && e->t.stage[ci] <= 2 && !e->conv_hin.empty();
}
// device copy of a host table of a grouped launch (its entries, its (entry, workgroup) map)
template <class T>
int upload_table(eosvos_engine* e, const std::vector<T>& tab, T*& dev) {
  dev = (T*)e->falloc((int64_t)(tab.size() * sizeof(T) + 3) / 4);
  if (!dev) return fail("hipMalloc grouped weight-gradient tables");
  HIPOK(hipMemcpy(dev, tab.data(), tab.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
// Launch the queued weight gradients (all of one stage) -- on the side stream when there is one.
// The register-staged members run as one launch per tile shape, planned for the engine's workgroup budget.
// The pre-split members: K splits are planned over ALL eligible convs of the stage (fixed membership: the update tables are
// built once) so that the 256 x 256 workgroups fit one resident round (one per CU of wgp_budget's share) at equal K length.
// The convs whose operand siblings were written this iteration run as ONE launch; the others (first iteration of a
// trajectory) on the register-staged kernel with the same split counts.
int flush_wgrad_group(eosvos_engine* e, int stage, int B) {
  auto& Q = e->wg_pending;
  if (Q.empty()) { side_flush(e); return 0; }
  const long key = (((long)stage * 64 + B) * 1024 + e->wg_budget) * 2 + (e->s2 ? 1 : 0);
  auto it = e->wg_plans.find(key);
  if (it == e->wg_plans.end()) {
    eosvos_engine::WgGroupPlan plan;
    std::vector<WgGroupItem> items;
    std::vector<KItem> pitems;
    std::vector<size_t> at, pat;                   // items[j] is Q[at[j]], pitems[j] is Q[pat[j]]
    for (size_t k = 0; k < Q.size(); ++k) {
      const WgradArgs& a = Q[k].a;
      const int P = a.B * a.Ho * a.Wo;
      if (Q[k].presplit) { pitems.push_back({wgrad_p_tiles(Q[k].p), (P + 31) / 32}); pat.push_back(k); }
      else { items.push_back({Q[k].ci, P, a.Cout, a.Cin, a.KH * a.KW}); at.push_back(k); }
    }
    const std::vector<int> sp = plan_wgrad_splits(items, e->wg_budget);
    const std::vector<int> psp = plan_equal_k(pitems, wgrad_p_resident(wgp_budget(e)));
    plan.splits.assign(Q.size(), 1);
    plan.npresplit = pat.size();
    for (size_t j = 0; j < at.size(); ++j) plan.splits[at[j]] = sp[j];
    for (size_t j = 0; j < pat.size(); ++j) plan.splits[pat[j]] = psp[j];
    for (int bm : {128, 64})
      for (int bn : {128, 64}) {
        eosvos_engine::WgGroupLaunch L;
        std::vector<WgradArgs> tab;
        std::vector<int> map;
        for (size_t j = 0; j < items.size(); ++j) {
          const auto& im = items[j];
          if (wgrad_group_tile(im.cout) != bm || wgrad_group_tile(im.cin) != bn) continue;
          WgradArgs a = Q[at[j]].a;
          a.splits = sp[j];
          // workgroups of an entry in launch_wgrad's order: split-major, the taps of a (cout, cin) tile pair adjacent
          for (int w = 0; w < wgrad_group_tiles(im) * a.splits; ++w) { map.push_back((int)tab.size()); map.push_back(w); }
          L.flops += 2.0 * im.cout * im.cin * im.T * (double)im.P * wgrad_exec_frac(a);
          if (L.first_ci < 0) L.first_ci = im.ci;
          tab.push_back(a);
        }
        if (tab.empty()) continue;
        WgradArgs* dtab = nullptr;
        if (upload_table(e, tab, dtab) || upload_table(e, map, L.dmap)) return 1;
        L.dtab[0] = dtab; L.nwg = (int)(map.size() / 2); L.bm = bm; L.bn = bn;
        plan.launches.push_back(L);
      }
    it = e->wg_plans.emplace(key, plan).first;
  }
  eosvos_engine::WgGroupPlan& plan = it->second;
  std::string covered;             // which pre-split members' siblings were written this iteration (ResNet-101's layer3: 69 members)
  int first_p = -1;
  for (const auto& q : Q)
    if (q.presplit) { covered += q.covered ? '1' : '0'; if (first_p < 0) first_p = q.ci; }
  if (plan.splits.size() != Q.size() || plan.npresplit != covered.size()) return fail("internal: grouped weight-gradient plan does not match the queue");
  if (covered.find('1') != std::string::npos) {
    const int par = (int)(e->pair_iter & 1);
    auto pl = plan.presplit.find(covered);
    if (pl == plan.presplit.end()) {
      eosvos_engine::WgGroupLaunch L;
      std::vector<WgradPArgs> tab;
      std::vector<int> map;
      for (size_t k = 0; k < Q.size(); ++k) {
        if (!Q[k].presplit || !Q[k].covered) continue;
        WgradPArgs a = Q[k].p;
        a.splits = a.groups = plan.splits[k];            // one K chunk per workgroup
        for (int w = 0; w < wgrad_p_tiles(a) * a.groups; ++w) { map.push_back((int)tab.size()); map.push_back(w); }
        L.flops += 2.0 * a.Cout * a.Cin * a.KH * a.KW * (double)a.B * a.Ho * a.Wo * wgrad_exec_frac(Q[k].a);
        tab.push_back(a);
      }
      for (int q = 0; q < 2; ++q) {
        WgradPArgs* dtab = nullptr;
        if (upload_table(e, tab, dtab)) return 1;
        L.dtab[par ^ q] = dtab;
        for (auto& a : tab) {        // the other parity: the producers' word and the next iteration's word trade places
          const float* pg = a.scp_g; const float* px = a.scp_x;
          a.scp_g = a.scn_g; a.scp_x = a.scn_x;
          a.scn_g = const_cast<float*>(pg); a.scn_x = const_cast<float*>(px);
        }
      }
      if (upload_table(e, map, L.dmap)) return 1;
      L.nwg = (int)(map.size() / 2); L.bm = L.bn = 256; L.first_ci = first_p;
      pl = plan.presplit.emplace(covered, L).first;
    }
    const eosvos_engine::WgGroupLaunch L = pl->second;
    trace_line("wgrad", L.first_ci, L.bm, L.bn, 0, L.nwg, L.flops);
    side_enqueue(e, [L, par](hipStream_t ws) { launch_wgrad_p_group((const WgradPArgs*)L.dtab[par], L.dmap, L.nwg, L.flops, ws); });
  }
  for (size_t k = 0; k < Q.size(); ++k) {
    e->upd_splits[Q[k].ci] = plan.splits[k];
    if (!Q[k].presplit || Q[k].covered) continue;
    WgradArgs a = Q[k].a;            // siblings not written: the register-staged kernel, which leaves the scales for the next iteration
    a.splits = plan.splits[k];
    trace("wgrad", Q[k].ci, a.Cout, (long)a.Cin * a.KH * a.KW, (long)a.B * a.Ho * a.Wo, a.splits, wgrad_exec_frac(a));
    side_enqueue(e, [a](hipStream_t ws) { launch_wgrad(a, ws); });
  }
  for (const eosvos_engine::WgGroupLaunch& L : plan.launches) {
    trace_line("wgrad", L.first_ci, L.bm, L.bn, 0, L.nwg, L.flops);
    side_enqueue(e, [L](hipStream_t ws) { launch_wgrad_group((const WgradArgs*)L.dtab[0], L.dmap, L.nwg, L.bm, L.bn, L.flops, ws); });
  }
  Q.clear();
  side_flush(e);
  return 0;
}
// ---- one conv's weight gradient -------------------------------------------------------------------------
// wgrad_wino / wgrad_direct enqueue on the main stream what the operands need first (transform, absmax passes), fill the
// arguments, record the slab count in upd_splits and return the launch for conv_wgrad to place.
using WgLaunch = std::function<void(hipStream_t)>;
// Winograd domain: dM = A dY A^T feeds this weight gradient (side stream) and the data gradient (main stream)
WgLaunch wgrad_wino(eosvos_engine* e, int ci, const View& gv, const View& xv, int B, int Ho, int Wo) {
  const ConvL& c = e->t.convs[ci];
  const WinoGeom wg = wino_geom(e, c, B, Ho, Wo);
  auto& w = e->wino[ci];
  float* const dM = w.dM;
  unsigned* dms = amax_fused_slot(e, AM_DM, ci, dM, e->s);
  launch_wino_grad(wg.tm, gv.ptr(), gv.ld(), c.cout, B, Ho, Wo, wg.th, wg.tw, wg.d, wg.prow, dM, e->s, dms);
  w.dm_batch = B;
  const long ntile = wg.ntile, prow = wg.prow;
  float* V = w.V;
  const bool need_v = w.v_batch != B;       // else: V comes from the forward pass
  const float* x = xv.ptr();
  const int ldx = xv.ld(), Hin = xv.t->H, Win = xv.t->W;
  float* final_slab = e->ws_wg + e->ws_off[ci];
  WgradArgs a;
  memset(&a, 0, sizeof(a));
  a.g = dM; a.x = V; a.ws = final_slab + c.wsize();
  a.B = 1; a.Ho = 1; a.Wo = (int)ntile; a.ldg = c.cout; a.Cout = c.cout; a.Hi = 1; a.Wi = (int)ntile; a.ldx = c.cin; a.Cin = c.cin;
  a.KH = a.KW = wg.tm + 2; a.stride = 1; a.pad = 0; a.dil = 0;  // the "taps" are the Winograd positions, no pixel shift
  a.g_tap_stride = prow * c.cout; a.x_tap_stride = prow * c.cin;
  // the 16 / 36 planes already give hundreds of tiles, and every K split parks a full Winograd-domain slab that the finish
  // kernel re-reads: plan the splits for half the workgroup budget (tools/budget_sweep.py: decoder conv at batch 3 247 -> 198 us,
  // batch 1 90 -> 72 us)
  const int wbud = conv_wg_budget_of(e->wg_budget) / 2;
  a.splits = wgrad_pick_splits((int)ntile, c.cout, c.cin, wg.np, wbud);
  trace("wgrad", ci, c.cout, (long)c.cin * wg.np, ntile, a.splits);
  const int cin = c.cin, cout = c.cout;
  const bool h3 = h3_mode() && !amax_init(e);
  if (h3) {
    a.amax_g = amax_get(e, AM_DM, ci, dM, (long)wg.np * prow, c.cout, c.cout, e->s);
    a.amax_x = amax_slot(e, AM_V, ci);
    if (!need_v && amax_rec_of(e, AM_V, ci).epoch != e->fwd_epoch)      // V of a forward in another mode
      a.amax_x = amax_get(e, AM_V, ci, V, (long)wg.np * prow, c.cin, c.cin, e->s);
  }
  unsigned* vslot = h3 ? amax_slot(e, AM_V, ci) : nullptr;
  e->upd_splits[ci] = 1;           // the finish kernel sums the Winograd-domain slabs into ONE 9-tap slab
  return [=](hipStream_t ws) {
    if (need_v) {
      if (h3) amax_zero(vslot, 1, ws);
      launch_wino_input(wg.tm, x, ldx, cin, B, Hin, Win, wg.th, wg.tw, wg.d, prow, V, ws, vslot);
    }
    launch_wgrad(a, ws);
    launch_wino_wgrad_finish(wg.tm, a.ws, a.splits, cout, cin, final_slab, ws);
  };
}
// Pre-split operand path: 256 x 256 tiles on the pair8 siblings of g and x when this iteration's producers wrote both
// (`covered`); otherwise the register-staged kernel with the same K splits, which leaves the scales for the next iteration's
// producers (a.scn_*).  false: the conv does not take the path.
bool wgrad_presplit_args(eosvos_engine* e, const ConvL& c, const View& gv, const View& xv, WgradArgs& a, WgradPArgs& pa, bool& covered) {
  if (!presplit_enabled(e) || e->gn() || !a.amax_g || !a.amax_x || !presplit_wgrad_shape(c, a.B * a.Ho * a.Wo, a.ldg, a.ldx)) return false;
  const long rows_g = (long)a.B * a.Ho * a.Wo, rows_x = (long)a.B * a.Hi * a.Wi;
  PairBuf *xb = nullptr, *gb = nullptr;
  const bool covx = pair_operand(e, xv, rows_x, xb);
  const bool covg = pair_operand(e, gv, rows_g, gb);
  if (!xb || !gb) return false;
  const int par = (int)(e->pair_iter & 1);
  memset(&pa, 0, sizeof(pa));
  pa.g2 = gv.sibling(); pa.x2 = xv.sibling(); pa.ws = a.ws;
  pa.B = a.B; pa.Ho = a.Ho; pa.Wo = a.Wo; pa.ldg = a.ldg; pa.Cout = c.cout; pa.Hi = a.Hi; pa.Wi = a.Wi; pa.ldx = a.ldx; pa.Cin = c.cin;
  pa.KH = pa.KW = c.k; pa.stride = c.stride; pa.pad = c.pad; pa.dil = c.dil;
  pa.zero = e->pair_zero;
  pa.scp_g = gb->sc + 1 + par; pa.scp_x = xb->sc + 1 + par;
  pa.scn_g = gb->sc + 1 + (par ^ 1); pa.scn_x = xb->sc + 1 + (par ^ 1);
  pa.slot_g = a.amax_g; pa.slot_x = a.amax_x;
  pa.margin_g = pair_margin(1); pa.margin_x = pair_margin(0);
  pa.g = a.g; pa.x = a.x;
  a.scn_g = pa.scn_g; a.scn_x = pa.scn_x; a.margin_g = pa.margin_g; a.margin_x = pa.margin_x;
  xb->fresh = false; gb->fresh = false;        // from the next iteration on their producers have a scale to write with
  covered = covx && covg;
  return true;
}
// direct form; an empty launch: queued for the stage's grouped launch (flush_wgrad_group records the slab count)
WgLaunch wgrad_direct(eosvos_engine* e, int ci, const View& gv, const View& xv, int B, int Ho, int Wo) {
  const ConvL& c = e->t.convs[ci];
  const float *g = gv.ptr(), *x = xv.ptr();
  const int ldg = gv.ld(), ldx = xv.ld(), Hin = xv.t->H, Win = xv.t->W;
  WgradArgs a;
  memset(&a, 0, sizeof(a));
  a.g = g; a.x = x; a.ws = e->ws_wg + e->ws_off[ci];
  a.B = B; a.Ho = Ho; a.Wo = Wo;
  a.ldg = ldg; a.Cout = c.cout; a.Hi = Hin; a.Wi = Win; a.ldx = ldx; a.Cin = c.cin;
  a.KH = a.KW = c.k; a.stride = c.stride; a.pad = c.pad; a.dil = c.dil;
  if (h3_mode() && !amax_init(e)) {
    a.amax_g = tlookup(e, *gv.t);
    if (!a.amax_g) a.amax_g = amax_get(e, AM_G, ci, g, (long)B * Ho * Wo, c.cout, ldg, e->s);
    // the input activation: the slot of its tensor or of this conv's view from the forward pass, else it is made now
    a.amax_x = tlookup(e, *xv.t);
    if (!a.amax_x) {
      unsigned* xs = amax_slot(e, AM_X, ci);
      auto& r = amax_rec_of(e, AM_X, ci);
      a.amax_x = (r.epoch == e->fwd_epoch && r.ptr == x) ? xs : amax_get(e, AM_X, ci, x, (long)B * Hin * Win, c.cin, ldx, e->s);
    }
  }
  WgradPArgs pa{};
  bool covered = false;
  const bool presplit = wgrad_presplit_args(e, c, gv, xv, a, pa, covered);
  if (wgrad_groupable(e, ci, B)) {
    e->wg_pending.push_back({ci, a, presplit, pa, covered});
    return nullptr;
  }
  // Pre-split: K chunks (= slabs) and workgroups per tile: one chunk per workgroup, as many as fill the launch's share of the chip
  // (wgrad_p_pick_splits).  The kernel can also walk several chunks per workgroup (WgradPArgs::groups < splits: any K partition
  // with any number of workgroups, bit-identical slabs -- tests/test_gpu_presplit.py).
  if (presplit) pa.splits = pa.groups = a.splits = wgrad_p_pick_splits(B * Ho * Wo, c.cout, c.cin, c.T(), wgp_budget(e));
  else a.splits = wgrad_pick_splits(B * Ho * Wo, c.cout, c.cin, c.T(), e->wg_budget);
  e->upd_splits[ci] = a.splits;
  const bool on_pairs = presplit && covered;
  trace(on_pairs ? "wgrad_p" : "wgrad", ci, c.cout, (long)c.cin * c.T(), (long)B * Ho * Wo, a.splits, wgrad_exec_frac(a));
  if (on_pairs) return [pa](hipStream_t ws) { launch_wgrad_p(pa, ws); };
  return [a](hipStream_t ws) { launch_wgrad(a, ws); };
}
// slabs of dW into ws_wg (their number: upd_splits[ci]; of a conv queued for its stage's grouped launch: set by flush_wgrad_group)
// (g: gradient w.r.t. the conv's output; x: its input activation, whose tensor gives the map size)
void conv_wgrad(eosvos_engine* e, int ci, View gv, const View& xv, int B) {
  const ConvL& c = e->t.convs[ci];
  const int Ho = conv_out(xv.t->H, c.k, c.stride, c.dil, c.pad), Wo = conv_out(xv.t->W, c.k, c.stride, c.dil, c.pad);
  if (e->gn() && c.norm) {        // dz = GroupNorm backward of G_u, written over the stored raw output
    // (round 5: the apply pass reduces max|dz| itself -- the consumers below, weight and data gradient, read the slot)
    launch_gn_backward(e->zbuf[ci]->p, c.cout, gv.ptr(), gv.ld(), e->G_(ci), e->gn_stats[ci], e->gn_partial, B, Ho * Wo, c.cout,
                       e->s, twrite_fused(e, e->zbuf[ci]).slot);
    gv = View(e->zbuf[ci]);
  }
  WgLaunch go = wino_on(e, ci, B, Ho, Wo) ? wgrad_wino(e, ci, gv, xv, B, Ho, Wo) : wgrad_direct(e, ci, gv, xv, B, Ho, Wo);
  if (!go) return;
  side_enqueue(e, std::move(go));
  if (e->s2 && (int)e->side_q.size() >= (B == 1 ? EOSVOS_SIDE_BATCH : 1)) side_flush(e);
}
// one launch: sum every layer's slabs, norm scale, theta <- theta - lr*g, optional gsum/gout
// part 0: convs [split, nconv) = layer4 + ASPP + decoder (90 % of the parameters), whose backward
// finishes first; part 1: convs [0, split).  With a side stream part 0 is launched there as soon
// as layer4's backward is queued and hides under the layer3..1 backward.  With a trainable boundary
// (eosvos_set_trainable_from) part 0 is convs [train_from, nconv) and part 1 is never launched.
int flush_updates(eosvos_engine* e, int B, bool update, bool accumulate, int part, hipStream_t stream) {
  const Topo& t = e->t;
  const int split = e->train_from > 0 ? e->train_from : t.blocks[t.blocks.size() - 3].c1;   // first conv of layer4
  const int lo = part == 0 ? split : 0, hi = part == 0 ? (int)t.convs.size() : split;
  const int slot = 2 * B + part;
  if (!e->upd_tab[slot]) {
    std::vector<UpdEntry> tab(hi - lo);
    int blk = 0;
    // most slabs first: those workgroups run the longest dependent chains and must not form the tail
    std::vector<int> order(hi - lo);
    for (int i = 0; i < hi - lo; ++i) order[i] = lo + i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return e->upd_splits[x] > e->upd_splits[y]; });
    for (int k = 0; k < hi - lo; ++k) {
      const int ci = order[k];
      const ConvL& c = t.convs[ci];
      UpdEntry& u = tab[k];
      u.w_off = c.poff; u.ws_off = e->ws_off[ci];
      u.n = (int)(c.wsize() + (c.bias ? c.cout : 0)); u.slab = u.n;
      u.splits = e->upd_splits[ci]; u.rowlen = c.T() * c.cin;
      u.lr_off = (int)c.lroff; u.norm_off = (c.norm && !e->gn()) ? (int)c.noff : -1; u.blk0 = blk;
      u.amax_idx = ((c.cin & 3) || (u.n & 3)) ? -1 : ci;      // tensors the matrix kernels read (not the stem, not conv + bias)
      blk += (u.n + 1024 * UPD_CHUNKS - 1) / (1024 * UPD_CHUNKS);
    }
    UpdEntry* d = (UpdEntry*)e->falloc((int64_t)(tab.size() * sizeof(UpdEntry) + 3) / 4);
    if (!d) return fail("hipMalloc update table");
    HIPOK(hipMemcpy(d, tab.data(), tab.size() * sizeof(UpdEntry), hipMemcpyHostToDevice));
    e->upd_tab[slot] = d; e->upd_blocks[slot] = blk;
  }
  // f16x3: the update kernel refreshes max|w| of the tensors it rewrites (their slots are zeroed first, on the same
  // stream), so the W slots stay valid across the update.  The slots of the other part are not touched: the rest of
  // the backward pass (main stream) reads only those.
  unsigned* amax_w = nullptr;
  if (update) {
    for (int ci = 0; ci < (int)e->wino.size(); ++ci)
      if (e->train_from == 0 || ci >= lo) e->wino[ci].us_valid = false;     // a frozen conv keeps its transformed weights
    if (h3_mode() && !amax_init(e) && e->w_amax_valid) {
      amax_w = amax_slot(e, AM_W, 0);
      amax_zero(amax_w + lo, (size_t)(hi - lo), stream);
    } else {
      e->w_amax_valid = false;
    }
  }
  launch_sgd_update_all(e->upd_tab[slot], hi - lo, e->upd_blocks[slot], e->Wp, e->ws_wg, e->na,
                        update ? e->lr : nullptr, (update && e->lr_level == EOSVOS_LR_PARAM) ? e->lr_elem : nullptr,
                        accumulate ? e->gsum : nullptr, e->keep_grads ? e->gout : nullptr, stream, amax_w);
  return 0;
}

// The four ASPP branches' data gradients into d(layer4 output) as ONE K-concatenated launch (ConvArgs::nseg): K = 256 (1x1)
// + 3 x 9 taps x 256 (dilated 3x3, taps that fall into the padding for a whole tile skipped), no accumulate
// read-modify-write between the branches, one fix-up pass.  Returns false when this engine / mode has to run them one by
// one (GroupNorm mode: the gradients w.r.t. the raw conv outputs live in separate buffers; fp32-MFMA mode: no such kernel).
bool aspp_dgrad_merged(eosvos_engine* e, int B, Tensor* g_l4, const Tensor* l4) {
  const Topo& t = e->t;
  if (e->gn() || !conv_multi_supported() || e->force_algo != 0) return false;
  for (int i = 0; i < 4; ++i) {
    const ConvL& c = t.convs[t.aspp[i]];
    if (c.cout != 256 || c.cin != t.convs[t.aspp[0]].cin || c.stride != 1 || t.aspp[i] != t.aspp[0] + i) return false;
    if (wino_on(e, t.aspp[i], B, e->h16, e->w16)) return false;
  }
  const ConvL& c0 = t.convs[t.aspp[0]];
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.wg_budget = e->wg_budget;
  a.x = e->g_cat->p; a.w = e->W_(t.aspp[0]); a.y = g_l4->p; a.ws = e->ws_conv;
  a.B = B; a.Hi = e->h16; a.Wi = e->w16; a.ldx = e->g_cat->C; a.Kc = 256;
  a.Ho = e->h16; a.Wo = e->w16; a.N = c0.cin; a.ldy = c0.cin; a.KH = a.KW = 1;
  a.mul = 1; a.off0 = 0; a.kstep = 0; a.upshift = 0;
  a.M = B * e->h16 * e->w16; a.wN = 256; a.wK = c0.cin; a.kmajor = 1;
  a.kscale = e->A_(t.aspp[0]);
  a.mask8 = l4->mask; a.ldm8 = View(g_l4).ldmask(); a.mask_c0 = 0; a.accum = 1;
  if (!a.mask8) return false;                      // (conv_dgrad reports the missing mask bytes)
  a.nseg = 4;
  a.w_floats = 0;
  ConvSegHost segs[4];
  for (int i = 0; i < 4; ++i) {
    const ConvL& c = t.convs[t.aspp[i]];
    segs[i] = ConvSegHost{c.k, c.dil, c.pad, 256 * i, (long)(c.poff - c0.poff), (int)(c.noff - c0.noff)};
    a.w_floats = (long)(c.poff - c0.poff) + c.wsize();
  }
  auto it = e->aspp_multi.find(B);
  if (it == e->aspp_multi.end()) {
    std::vector<int> prefix;
    std::vector<unsigned char> taplist;
    std::vector<ConvTap> taps;
    const long total = conv_build_multi_table(a, segs, 4, prefix, taplist, taps);
    eosvos_engine::MultiTab mt{nullptr, nullptr, nullptr, total};
    mt.prefix = (int*)e->falloc((int64_t)prefix.size());
    mt.taplist = (unsigned char*)e->falloc((int64_t)(taplist.size() + 3) / 4);
    mt.taps = (ConvTap*)e->falloc((int64_t)(taps.size() * sizeof(ConvTap) + 3) / 4);
    if (!mt.prefix || !mt.taplist || !mt.taps) return false;
    if (hipMemcpy(mt.prefix, prefix.data(), prefix.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
    if (hipMemcpy(mt.taplist, taplist.data(), taplist.size(), hipMemcpyHostToDevice) != hipSuccess) return false;
    if (hipMemcpy(mt.taps, taps.data(), taps.size() * sizeof(ConvTap), hipMemcpyHostToDevice) != hipSuccess) return false;
    it = e->aspp_multi.emplace(B, mt).first;
  }
  a.tprefix = it->second.prefix; a.taplist = it->second.taplist; a.taps = it->second.taps; a.total_units = it->second.total;
  if (h3_mode()) {
    if (amax_init(e)) return false;
    amax_weights(e, e->s);
    a.amax_x = tlookup(e, *e->g_cat);
    if (!a.amax_x) a.amax_x = amax_get(e, AM_G, t.aspp[0], e->g_cat->p, (long)B * e->h16 * e->w16, e->g_cat->C, e->g_cat->C, e->s);
    for (int i = 0; i < 4; ++i) {
      a.seg_amax_w[i] = amax_slot(e, AM_W, t.aspp[i]);
      a.seg_amax_ks[i] = amax_ks(e, t.aspp[i], e->s);
    }
    a.amax_y = twrite_fused(e, g_l4).slot;         // every element of g_l4 is rewritten (accumulating the pooling branch's broadcast)
  }
  if (trace_on())
    trace_line("dgrad", t.aspp[0], a.M, a.N, (long)(a.total_units * 32 / (((a.M + 127) / 128) * ((a.N + 127) / 128))), conv_plan(a),
               2.0 * 128 * 128 * 32 * (double)a.total_units);
  pair_attach(e, g_l4, a);
  launch_conv(a, e->s);
  pair_covered(e, *g_l4, a);
  return true;
}

// g_l4 (holding the pooling branch's broadcast) += the four ASPP branches' data gradients, masked with the ReLU mask of l4: the
// K-concatenated launch, or -- where it declines, or `force_fallback` (parity tests) -- one accumulating conv_dgrad per branch,
// the mask applied by the last.  *merged (may be null): which of the two ran.
int aspp_dgrad(eosvos_engine* e, int B, Tensor* g_l4, const Tensor* l4, bool force_fallback, bool* merged) {
  const Topo& t = e->t;
  const bool m = !force_fallback && aspp_dgrad_merged(e, B, g_l4, l4);
  if (merged) *merged = m;
  if (m) return 0;
  for (int i = 0; i < 4; ++i)
    if (conv_dgrad(e, t.aspp[i], View(e->g_cat, 256 * i, 256), g_l4, B, Opt().accum().mask(i == 3 ? l4 : nullptr))) return 1;
  return 0;
}

// The grouped weight-gradient tables (WgradArgs with or without absmax slots, split counts) and the update tables (slab
// counts per conv) depend on the process-wide matrix mode: a mode switch on a live engine drops them.
void plans_match_mode(eosvos_engine* e) {
  const int mode = conv_mfma_mode() | (presplit_switch() ? 16 * g_presplit : 0);      // the pre-split switch changes split counts like a mode does
  if (e->plan_mode == mode) return;
  e->plan_mode = mode;
  e->wg_plans.clear();                             // (the device tables stay allocated until the engine goes: a few KB per switch)
  for (auto& tab : e->upd_tab) tab = nullptr;
  for (auto& w : e->wino) w.v_batch = w.dm_batch = 0;      // Winograd selection differs per mode: V / dM of the other mode are stale
}

int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
// slab sizing: the K splits of a weight gradient depend on the matrix mode (tile rules), which may change after create
int wgrad_max_splits(int P, int Cout, int Cin, int T, int wg_budget) {
  int m = 1;
  for (int mode = 0; mode <= 2; ++mode) m = std::max(m, wgrad_pick_splits(P, Cout, Cin, T, wg_budget, mode));
  if (Cout % 256 == 0 && Cin % 256 == 0) m = std::max(m, wgrad_p_pick_splits(P, Cout, Cin, T, wg_budget));    // pre-split path (also covers its grouped plans: fewer splits)
  return m;
}

}  // namespace

extern "C" {

const char* eosvos_version(void) { return "eosvos-mi355x 0.8 (gfx950, fp32 implicit GEMM on the fp16 matrix cores: 2-way split, 3 partial products on v_mfma_f32_16x16x32_f16, weight gradients of the stride-16 layers on pre-split fp16-pair operands by LDS-DMA; bf16x6 and fp32-MFMA modes selectable)"; }
const char* eosvos_last_error(void) { return g_err.c_str(); }

int eosvos_set_matrix_mode(int mode) {
  if (mode != EOSVOS_MATRIX_F32 && mode != EOSVOS_MATRIX_BF16X6 && mode != EOSVOS_MATRIX_F16X3) return fail("unknown matrix mode");
  conv_set_mfma_mode(mode);
  return 0;
}
int eosvos_get_matrix_mode(void) { return conv_mfma_mode(); }
int eosvos_plan_fingerprint(eosvos_engine* e, uint64_t* out2) {
  if (!e || !out2) return fail("null argument");
  out2[0] = e->plan_fp[0]; out2[1] = e->plan_fp[1];
  return 0;
}
int eosvos_set_presplit(int on) {
  const int prev = presplit_switch() ? g_presplit : 0;
  g_presplit = on == 2 ? 2 : (on ? 1 : 0);
  return prev;
}
int eosvos_set_engine_matrix_mode(eosvos_engine* e, int mode) {
  if (!e) return fail("null engine");
  if (mode != -1 && mode != EOSVOS_MATRIX_F32 && mode != EOSVOS_MATRIX_BF16X6 && mode != EOSVOS_MATRIX_F16X3) return fail("unknown matrix mode");
  e->mode = mode;
  return 0;
}
int eosvos_get_engine_matrix_mode(eosvos_engine* e) {
  if (!e) { fail("null engine"); return -1; }
  return e->mode >= 0 ? e->mode : conv_mfma_mode();
}
int eosvos_set_wg_budget(eosvos_engine* e, int workgroups) {
  if (!e) { fail("null engine"); return -1; }
  if (workgroups < 0) { fail("workgroup budget must be >= 0"); return -1; }
  const int b = conv_clamp_wg_budget(workgroups);
  if (b == e->wg_budget) return b;
  e->wg_budget = b;
  for (auto& tab : e->upd_tab) tab = nullptr;      // the update tables carry the split counts of the old budget
  return e->wg_budget;
}

static hipError_t create_side_stream(hipStream_t* out) {
  int plo = 0, phi = 0;
  const hipError_t rc = hipDeviceGetStreamPriorityRange(&plo, &phi);       // plo = least, phi = greatest priority
  if (rc != hipSuccess) return rc;
  return hipStreamCreateWithPriority(out, hipStreamNonBlocking, plo);
}
int eosvos_set_side_stream(eosvos_engine* e, int on) {
  if (!e) { fail("null engine"); return -1; }
  if (hipSetDevice(e->dev) != hipSuccess) { fail("hipSetDevice"); return -1; }
  if (!on && e->s2) {
    // The stream is DESTROYED, not parked: an idle second stream per engine still costs the engines that run side by side
    // a quarter of their throughput once every stream has a hardware queue of its own (six queues or more; measured
    // 41 -> 29 meta-tasks/s with four engines, profiles/r03_hw_queue_sweep.txt).
    (void)hipStreamSynchronize(e->s);
    (void)hipStreamSynchronize(e->s2);
    (void)hipStreamDestroy(e->s2);
    e->s2 = nullptr;
    e->side_used = false;
    e->side_q.clear();
    e->wino_w_wait = false;
    for (auto& tab : e->upd_tab) tab = nullptr;      // which stages group their weight gradients (hence the split counts) changes
  } else if (on && !e->s2 && e->ws_conv2) {          // (engines built under EOSVOS_NO_SIDE_STREAM=1 have no side workspace)
    (void)hipStreamSynchronize(e->s);
    if (create_side_stream(&e->s2) != hipSuccess) { e->s2 = nullptr; fail("hipStreamCreate"); return -1; }
    for (auto& tab : e->upd_tab) tab = nullptr;
  }
  return e->s2 ? 1 : 0;
}

int eosvos_num_convs(int arch) {
  Topo t;
  if (!build_topo(arch, t)) return -1;
  return (int)t.convs.size();
}
int eosvos_conv_info(int arch, int idx, int64_t* info) {
  Topo t;
  if (!build_topo(arch, t)) return fail("bad arch");
  if (idx < 0 || idx >= (int)t.convs.size() || !info) return fail("bad conv index");
  const ConvL& c = t.convs[idx];
  info[0] = c.cin; info[1] = c.cout; info[2] = c.k; info[3] = c.stride; info[4] = c.dil; info[5] = c.pad;
  info[6] = c.norm; info[7] = c.bias; info[8] = c.poff;
  return 0;
}
int64_t eosvos_param_count(int arch) { Topo t; return build_topo(arch, t) ? t.nparam : -1; }
int64_t eosvos_lr_count(int arch) { Topo t; return build_topo(arch, t) ? t.nlr : -1; }
int64_t eosvos_norm_count(int arch) { Topo t; return build_topo(arch, t) ? t.nnorm : -1; }

int eosvos_create(eosvos_engine** out, int arch, int norm_mode, int height, int width, int max_batch,
                  int device_id, void* stream) {
  return eosvos_create_ex(out, arch, norm_mode, height, width, max_batch, device_id, stream, 0);
}
int eosvos_create_ex(eosvos_engine** out, int arch, int norm_mode, int height, int width, int max_batch,
                     int device_id, void* stream, int flags) {
  if (!out) return fail("null out");
  if (flags & ~EOSVOS_CREATE_NO_SIDE_STREAM) return fail("unknown construction flag");
  if (norm_mode != EOSVOS_NORM_BN_FROZEN && norm_mode != EOSVOS_NORM_GN16) return fail("unknown norm mode");
  if (height < 32 || width < 32 || max_batch < 1) return fail("bad geometry");
  {
    // The conv kernels address every operand through a buffer descriptor of at most 2^31 - 1 bytes with 32-bit byte
    // offsets (conv_kernels.hip make_rsrc): beyond that the hardware range check would zero-fill instead of failing.
    // The largest operands are the Winograd-domain planes of the decoder (36 x tiles x 304 floats) and the stem output.
    const int64_t h2 = conv_out(height, 7, 2, 1, 3), w2 = conv_out(width, 7, 2, 1, 3);
    const int64_t h4 = conv_out((int)h2, 3, 2, 1, 1), w4 = conv_out((int)w2, 3, 2, 1, 1);
    const int64_t tiles = ((int64_t)max_batch * ((h4 + 3) / 4) * ((w4 + 3) / 4) + 127) / 128 * 128;
    const int64_t worst = std::max<int64_t>({36 * tiles * 304, (int64_t)max_batch * h4 * w4 * 304, (int64_t)max_batch * h2 * w2 * 64,
                                            (int64_t)max_batch * (height + 6) * (width + 6) * 3});
    if (worst * 4 > 0x7fffffffLL)
      return fail("frame size x max_batch too large: a conv operand of " + std::to_string(worst * 4) +
                  " bytes exceeds the 2 GiB buffer-descriptor range of the kernels (reduce max_batch or the frame size)");
  }
  eosvos_engine* e = new eosvos_engine();
  if (!build_topo(arch, e->t)) { delete e; return fail("bad arch"); }
  e->norm_mode = norm_mode;
  e->arch = arch; e->H = height; e->W = width; e->maxB = max_batch; e->dev = device_id;
  e->s = (hipStream_t)stream;
  HIPOK(hipSetDevice(device_id));
  const Topo& t = e->t;
  const int B = max_batch, H = height, W = width;
  e->h2 = conv_out(H, 7, 2, 1, 3); e->w2 = conv_out(W, 7, 2, 1, 3);
  e->h4 = conv_out(e->h2, 3, 2, 1, 1); e->w4 = conv_out(e->w2, 3, 2, 1, 1);
  e->h8 = conv_out(e->h4, 3, 2, 1, 1); e->w8 = conv_out(e->w4, 3, 2, 1, 1);
  // (h16, w16) = the map ASPP runs on: stride 16 for DeepLabV3+, the stride-8 map for plain DeepLabV3
  if (t.v3) { e->h16 = e->h8; e->w16 = e->w8; }
  else { e->h16 = conv_out(e->h8, 1, 2, 1, 0); e->w16 = conv_out(e->w8, 1, 2, 1, 0); }
  if (t.v3 && e->gn()) { delete e; return fail("plain DeepLabV3 has no GroupNorm variant (networks/deeplabv3.py)"); }

#define ALLOC(ptr, n)                                                  \
  do {                                                                 \
    ptr = e->falloc((int64_t)(n));                                     \
    if (!ptr) { eosvos_destroy(e); return fail("hipMalloc " #ptr); }  \
  } while (0)
  ALLOC(e->Wp, t.nparam); ALLOC(e->Winit, t.nparam); ALLOC(e->Wsnap, t.nparam);
  ALLOC(e->gout, t.nparam); ALLOC(e->stage, t.nparam);
  ALLOC(e->lr, t.nlr); ALLOC(e->na, t.nnorm); ALLOC(e->nb, t.nnorm);
  ALLOC(e->xpad, (int64_t)B * (H + 6) * (W + 6) * 3 + 8);      // + 8: the matrix-core stem reads whole 8-float slots (odd x odd frames: 3 floats past the last row)
  HIPOK(hipMemset(e->xpad, 0, ((size_t)B * (H + 6) * (W + 6) * 3 + 8) * 4));      // the tail too: nothing ever writes it
  HIPOK(hipMemset(e->Wp, 0, (size_t)t.nparam * 4));
  HIPOK(hipMemset(e->Winit, 0, (size_t)t.nparam * 4));
  HIPOK(hipMemset(e->lr, 0, (size_t)t.nlr * 4));
  // a tensor of the engine, [B][h][w][c]; `masked`: with ReLU mask bytes (an activation that a data gradient masks with; in
  // the GroupNorm mode the apply pass that writes y = relu(gn(z) (+ res)) writes them), one byte per 4 floats
  auto new_tensor = [&](int h, int w, int c, int phase, bool masked) {
    Tensor* x = e->ts.add(nullptr, h, w, c, phase);
    x->p = e->falloc(x->floats(B));
    if (x->p && masked) x->mask = (uint8_t*)e->falloc((x->floats(B) / 4 + 3) / 4);
    return x;
  };
#define TENSOR(ptr, h, w, c, phase, masked)                                                 \
  do {                                                                                      \
    ptr = new_tensor(h, w, c, phase, masked);                                               \
    if (!ptr->p) { eosvos_destroy(e); return fail("hipMalloc " #ptr); }                     \
    if (masked && !ptr->mask) { eosvos_destroy(e); return fail("hipMalloc ReLU mask bytes"); } \
  } while (0)
  const int64_t n4 = (int64_t)B * e->h4 * e->w4;
  TENSOR(e->c1, e->h2, e->w2, 64, 0, false); TENSOR(e->g_c1, e->h2, e->w2, 64, 1, false);
  TENSOR(e->p1, e->h4, e->w4, 64, 0, false); TENSOR(e->g_p1, e->h4, e->w4, 64, 1, false);
  { float* t8; ALLOC(t8, (e->p1->floats(B) + 3) / 4); e->p1idx = (uint8_t*)t8; }

  int64_t wsc = conv_ws_floats(), wsw = 0;
  e->zbuf.assign(t.convs.size(), nullptr);
  e->gn_stats.assign(t.convs.size(), nullptr);
  if (e->gn()) {
    e->gn_sums = e->falloc((int64_t)B * 32);
    e->gn_partial = e->falloc((int64_t)gn_partial_floats(B));
    e->zbuf[0] = new_tensor(e->h2, e->w2, 64, 1, false);
    e->gn_stats[0] = e->falloc((int64_t)B * 32);
    e->zbuf[t.pool] = new_tensor(1, 1, 256, 1, false);
    e->gn_stats[t.pool] = e->falloc((int64_t)B * 32);
  }
  e->ws_off.assign(t.convs.size(), 0);
  e->upd_splits.assign(t.convs.size(), 1);
  e->upd_tab.assign(2 * B + 2, nullptr);
  e->upd_blocks.assign(2 * B + 2, 0);
  std::vector<int64_t> slabs(t.convs.size(), 0);   // floats of slab space per conv (max over batch sizes)
  e->conv_hin.assign(t.convs.size(), 0);
  e->conv_win.assign(t.convs.size(), 0);
  e->wino.assign(t.convs.size(), eosvos_engine::WinoRec());
  auto track = [&](int ci, int Hin, int Win) {
    const ConvL& c = t.convs[ci];
    e->conv_hin[ci] = Hin; e->conv_win[ci] = Win;
    const int Ho = conv_out(Hin, c.k, c.stride, c.dil, c.pad), Wo = conv_out(Win, c.k, c.stride, c.dil, c.pad);
    for (int b = 1; b <= B; ++b)
      for (int wb = 0; wb <= 512; wb += 64)          // every budget eosvos_set_wg_budget accepts
        slabs[ci] = max64(slabs[ci], (int64_t)wgrad_max_splits(b * Ho * Wo, c.cout, c.cin, c.T(), wb) * c.wsize());
    const bool reserve = wino_shape(c) && (ci == t.dec_a || ci == t.dec_b ||
                                           (long long)B * Ho * Wo / 4 * c.cin * c.cout >= EOSVOS_WINO_MINWORK);
    if (reserve) {                     // [final 9-tap slab][Winograd-domain slabs: splits x cout x 16 x cin]
      for (int b = 1; b <= B; ++b) {
        const WinoGeom gb = wino_geom(e, c, b, Ho, Wo);
        for (int wb = 0; wb <= 512; wb += 64)
          slabs[ci] = max64(slabs[ci], c.wsize() + (int64_t)wgrad_max_splits((int)gb.ntile, c.cout, c.cin, gb.np, wb) * c.cout * gb.np * c.cin);
      }
      const WinoGeom gm = wino_geom(e, c, B, Ho, Wo);
      const int64_t prow = gm.prow, np = gm.np;
      auto& w = e->wino[ci];
      w.V = e->falloc(np * prow * c.cin);
      w.U = e->falloc(np * c.cout * c.cin);
      w.Us = e->falloc(np * c.cout * c.cin);
      w.dM = e->falloc(np * prow * c.cout);
      e->wino_m_n = max64(e->wino_m_n, np * prow * max64(c.cout, c.cin));
    }
    if (e->gn() && c.norm) {
      e->zbuf[ci] = new_tensor(Ho, Wo, c.cout, 1, false);
      e->gn_stats[ci] = e->falloc((int64_t)B * 32);
    }
  };
  // bottleneck buffers
  eosvos_engine::BlkBuf bf;
  bf.out = e->p1; bf.g_out = e->g_p1;
  for (size_t i = 0; i < t.blocks.size(); ++i) {
    const Block& b = t.blocks[i];
    const ConvL &c1 = t.convs[b.c1], &c2 = t.convs[b.c2], &c3 = t.convs[b.c3];
    bf.xin = bf.out; bf.g_xin = bf.g_out;
    const int Hm = conv_out(bf.xin->H, 1, c1.stride, 1, 0), Wm = conv_out(bf.xin->W, 1, c1.stride, 1, 0);
    const int Ho = conv_out(Hm, 3, c2.stride, c2.dil, c2.pad), Wo = conv_out(Wm, 3, c2.stride, c2.dil, c2.pad);
    TENSOR(bf.t1, Hm, Wm, c1.cout, 0, true); TENSOR(bf.g_t1, Hm, Wm, c1.cout, 1, false);
    TENSOR(bf.t2, Ho, Wo, c2.cout, 0, true); TENSOR(bf.g_t2, Ho, Wo, c2.cout, 1, false);
    TENSOR(bf.out, Ho, Wo, c3.cout, 0, true); TENSOR(bf.g_out, Ho, Wo, c3.cout, 1, false);
    bf.dsb = nullptr;
    if (b.ds >= 0) TENSOR(bf.dsb, Ho, Wo, c3.cout, 0, false);
    track(b.c1, bf.xin->H, bf.xin->W); track(b.c2, Hm, Wm); track(b.c3, Ho, Wo);
    if (b.ds >= 0) track(b.ds, bf.xin->H, bf.xin->W);
    e->bb.push_back(bf);
  }
  if (bf.out->H != e->h16 || bf.out->W != e->w16) { eosvos_destroy(e); return fail("internal: stride-16 geometry mismatch"); }
  TENSOR(e->cat, e->h16, e->w16, 1280, 0, true); TENSOR(e->g_cat, e->h16, e->w16, 1280, 1, false);   // 4 ASPP branches + the pooling branch
  ALLOC(e->vec, (int64_t)B * 2048); ALLOC(e->gvec, (int64_t)B * 2048);
  ALLOC(e->poolout, (int64_t)B * 256); ALLOC(e->gp, (int64_t)B * 256);
  ALLOC(e->colscratch, (int64_t)B * 64 * 2048);      // COLSUM_CHUNKS partial sums
  TENSOR(e->proj, e->h16, e->w16, 256, 0, true); TENSOR(e->g_proj, e->h16, e->w16, 256, 1, false);
  TENSOR(e->dcat, e->h4, e->w4, 304, 0, true); TENSOR(e->g_dcat, e->h4, e->w4, 304, 1, false);       // upsampled projection (256) + decoder.conv1 (48)
  TENSOR(e->d1, e->h4, e->w4, 256, 0, true); TENSOR(e->g_d1, e->h4, e->w4, 256, 1, false);
  TENSOR(e->d2, e->h4, e->w4, 256, 0, false); TENSOR(e->g_d2, e->h4, e->w4, 256, 1, false);
  ALLOC(e->lowlog, n4); ALLOC(e->g_low, n4);
  ALLOC(e->logits, (int64_t)B * H * W); ALLOC(e->dlogits, (int64_t)B * H * W);
  ALLOC(e->loss_dev, 4); ALLOC(e->bce_partial, LOSS_PARTIAL_FLOATS);
#undef TENSOR
  for (int i = 0; i < 4; ++i) track(t.aspp[i], e->h16, e->w16);
  track(t.project, e->h16, e->w16);
  if (t.v3) {
    track(t.head3, e->h16, e->w16);
  } else {
    track(t.dec1, e->h4, e->w4);
    track(t.dec_a, e->h4, e->w4); track(t.dec_b, e->h4, e->w4);
  }
  for (int b = 1; b <= B; ++b) {
    slabs[0] = max64(slabs[0], (int64_t)stem_wgrad_chunks(b, e->h2, e->w2) * 64 * 147);
    slabs[t.last] = max64(slabs[t.last], (int64_t)last_bwd_chunks((int64_t)b * e->h4 * e->w4) * 257);
  }
  slabs[t.pool] = (int64_t)256 * 2048;
  // grouped weight gradients of layer1..3 (flush_wgrad_group): their split counts come from the stage plan
  for (int st = 0; st <= 2; ++st)
    for (int b = 1; b <= B; ++b)
      for (int wb = 0; wb <= 512; wb += 64) {
        std::vector<WgGroupItem> items;
        for (size_t ci = 0; ci < t.convs.size(); ++ci) {
          if (t.stage[ci] != st) continue;
          const ConvL& c = t.convs[ci];
          const int Ho = conv_out(e->conv_hin[ci], c.k, c.stride, c.dil, c.pad), Wo = conv_out(e->conv_win[ci], c.k, c.stride, c.dil, c.pad);
          items.push_back({(int)ci, b * Ho * Wo, c.cout, c.cin, c.T()});
        }
        const std::vector<int> sp = plan_wgrad_splits(items, wb);
        for (size_t k = 0; k < items.size(); ++k)
          slabs[items[k].ci] = max64(slabs[items[k].ci], (int64_t)sp[k] * t.convs[items[k].ci].wsize());
      }
  for (size_t ci = 0; ci < t.convs.size(); ++ci) {
    e->ws_off[ci] = wsw;
    wsw += (slabs[ci] + 3) / 4 * 4;
  }
  ALLOC(e->ws_conv, wsc); ALLOC(e->ws_wg, wsw);
  if (e->wino_m_n > 0) { ALLOC(e->wino_m, e->wino_m_n); ALLOC(e->wino_dv, e->wino_m_n); }
  e->ws_conv_n = wsc; e->ws_wg_n = wsw;
#undef ALLOC
  if (!t.v3) {       // decoder upsample of the ASPP output onto the stride-4 map
    if (upload_resize(e, make_resize(e->h16, e->h4, true), e->h16, e->h4, e->up_h)) { eosvos_destroy(e); return 1; }
    if (upload_resize(e, make_resize(e->w16, e->w4, true), e->w16, e->w4, e->up_w)) { eosvos_destroy(e); return 1; }
  }
  // final resize of the 1-channel logits: from the stride-4 decoder map (DeepLabV3+) or straight from the ASPP map (V3)
  const int hl = t.v3 ? e->h16 : e->h4, wl = t.v3 ? e->w16 : e->w4;
  if (upload_resize(e, make_resize(hl, H, false), hl, H, e->fin_h)) { eosvos_destroy(e); return 1; }
  if (upload_resize(e, make_resize(wl, W, false), wl, W, e->fin_w)) { eosvos_destroy(e); return 1; }
  {
    const char* pi = getenv("EOSVOS_TUNE_PRESPLIT_INFLIGHT");
    e->presplit_inflight = pi && pi[0] == '1';
    const char* v = getenv("EOSVOS_NO_SIDE_STREAM");
    if (!(v && v[0] == '1') && !(flags & EOSVOS_CREATE_NO_SIDE_STREAM)) {
      // The side stream (weight gradients, early update, independent forward branches) yields to the main stream, whose
      // forward / data-gradient chain is the critical path: least stream priority.  Scheduling only -- results are bit-identical.
      // Round 5, three interleaved rounds: batch 3 8.81 -> 8.77 ms, batch 1 4.48 -> 4.47 (round 1 had found no gain with the
      // fp32-MFMA kernels).
      HIPOK(create_side_stream(&e->s2));
      e->ev.resize(t.convs.size() + 2);
      for (auto& evt : e->ev) HIPOK(hipEventCreateWithFlags(&evt, hipEventDisableTiming));
      HIPOK(hipEventCreateWithFlags(&e->ev_wino_w, hipEventDisableTiming));
      e->ws_conv2 = e->falloc(conv_ws_floats());
      if (!e->ws_conv2) { eosvos_destroy(e); return fail("hipMalloc side workspace"); }
    }
  }
  if (e->max_alloc_floats * 4 > 0x7fffffffLL && e->max_alloc_floats != wsw && e->max_alloc_floats != wsc) {
    // belt and braces for topologies / sizes the estimate above does not cover (slab arenas are plain pointers)
    const int64_t bytes = e->max_alloc_floats * 4;
    eosvos_destroy(e);
    return fail("internal buffer of " + std::to_string(bytes) + " bytes exceeds the 2 GiB buffer-descriptor range");
  }
  // identity norm until eosvos_set_norm
  launch_fill(e->na, t.nnorm, 1.f, e->s);
  launch_fill(e->nb, t.nnorm, 0.f, e->s);
  HIPOK(hipStreamSynchronize(e->s));
  *out = e;
  return 0;
}

static int unalias_impl(eosvos_engine* e);
int eosvos_destroy(eosvos_engine* e) {
  if (!e) return 0;
  if (tl_plan_engine == e) tl_plan_engine = nullptr;      // (PlanScope already clears it; this thread only)
  // engines that read this engine's learned state get their own copy back before its memory goes; an alias leaves its source's list
  while (!e->aliased_by.empty()) (void)unalias_impl(e->aliased_by.back());
  if (e->alias_src) {
    auto& v = e->alias_src->aliased_by;
    v.erase(std::remove(v.begin(), v.end(), e), v.end());
    e->alias_src = nullptr;
  }
  (void)hipStreamSynchronize(e->s);
  if (e->s2) { (void)hipStreamSynchronize(e->s2); (void)hipStreamDestroy(e->s2); }
  for (auto& evt : e->ev) (void)hipEventDestroy(evt);
  if (e->ev_wino_w) (void)hipEventDestroy(e->ev_wino_w);
  for (void* p : e->allocs) (void)hipFree(p);
  if (e->scratch) (void)hipFree(e->scratch);
  delete e;
  return 0;
}
// debug: returns the number of guard words that no longer hold the pattern and prints where (stderr)
int eosvos_debug_check_guards(eosvos_engine* e) {
  if (!e) return -1;
  (void)hipDeviceSynchronize();
  int bad = 0;
  for (size_t i = 0; i < e->guarded.size(); ++i) {
    unsigned* base = e->guarded[i].first;
    const int64_t n = e->guarded[i].second, nn = (n + 63) / 64 * 64;
    for (int side = 0; side < 2; ++side) {
      // side 1 starts at the first float past the n requested ones (the rounding pad belongs to the band)
      const unsigned* g = side == 0 ? base : base + eosvos_engine::GUARD + n;
      const int64_t cnt = side == 0 ? eosvos_engine::GUARD : eosvos_engine::GUARD + (nn - n);
      std::vector<unsigned> hh((size_t)cnt);
      if (hipMemcpy(hh.data(), g, (size_t)cnt * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
      int64_t first = -1, last = -1, c = 0;
      for (int64_t k = 0; k < cnt; ++k)
        if (hh[k] != 0xDEADBEEFu) { if (first < 0) first = k; last = k; ++c; }
      if (c) {
        fprintf(stderr, "[guard] allocation #%zu (%lld floats): %lld words overwritten %s it, offsets %lld..%lld (floats %s)\n", i,
                (long long)n, (long long)c, side ? "after" : "before", (long long)first, (long long)last,
                side ? "past the end" : "from the band start; the buffer begins at 65536");
        bad += (int)c;
      }
    }
  }
  return bad;
}
int eosvos_synchronize(eosvos_engine* e) {
  if (!e) return fail("null engine");
  HIPOK(hipStreamSynchronize(e->s));
  return 0;
}

// flat OIHW -> engine arena (dst), through the permute kernel per conv
static void import_params(eosvos_engine* e, const float* flat, float* dst) {
  for (const ConvL& c : e->t.convs) {
    launch_oihw_to_ohwi(flat + c.poff, dst + c.poff, c.cout, c.cin, c.T(), e->s);
    if (c.bias) (void)hipMemcpyAsync(dst + c.poff + c.wsize(), flat + c.poff + c.wsize(), c.cout * 4, hipMemcpyDeviceToDevice, e->s);
  }
}
// device tables of the one-launch forms (meta path): per lr row its element range in the arena, per tensor its offset / shape
static int ensure_meta_tabs(eosvos_engine* e) {
  if (e->mt_rbase) return 0;
  const Topo& t = e->t;
  std::vector<long> rbase((size_t)t.nlr), toff;
  std::vector<int> rlen((size_t)t.nlr);
  std::vector<int2> tit;
  for (const ConvL& c : t.convs) {
    const long rowlen = (long)c.T() * c.cin;
    for (int r = 0; r < c.cout; ++r) { rbase[c.lroff + r] = (long)c.poff + r * rowlen; rlen[c.lroff + r] = (int)rowlen; }
    toff.push_back((long)c.poff); tit.push_back(make_int2(c.cin, c.T()));
    if (c.bias) {
      for (int r = 0; r < c.cout; ++r) { rbase[c.lroff + c.cout + r] = (long)c.poff + c.wsize() + r; rlen[c.lroff + c.cout + r] = 1; }
      toff.push_back((long)c.poff + c.wsize()); tit.push_back(make_int2(1, 1));
    }
  }
  if (toff.size() > 160) return fail("internal: more than 160 trainable tensors");
  e->mt_nent = (int)toff.size();
  e->mt_rbase = (long*)e->falloc((int64_t)t.nlr * 2);
  e->mt_rlen = (int*)e->falloc(t.nlr);
  e->mt_toff = (long*)e->falloc((int64_t)toff.size() * 2);
  e->mt_tit = (int2*)e->falloc((int64_t)tit.size() * 2);
  if (!e->mt_rbase || !e->mt_rlen || !e->mt_toff || !e->mt_tit) return fail("hipMalloc meta tables");
  HIPOK(hipMemcpy(e->mt_rbase, rbase.data(), rbase.size() * sizeof(long), hipMemcpyHostToDevice));
  HIPOK(hipMemcpy(e->mt_rlen, rlen.data(), rlen.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPOK(hipMemcpy(e->mt_toff, toff.data(), toff.size() * sizeof(long), hipMemcpyHostToDevice));
  HIPOK(hipMemcpy(e->mt_tit, tit.data(), tit.size() * sizeof(int2), hipMemcpyHostToDevice));
  return 0;
}
// trainable_only: the tensors of convs [train_from, nconv) only (the frozen prefix of `flat` is not touched)
static void export_params(eosvos_engine* e, const float* src, float* flat, float alpha, int add, bool trainable_only = false) {
  const bool sub = trainable_only && e->train_from > 0;
  if (!ensure_meta_tabs(e)) {                         // one launch for the whole arena (64 before)
    if (sub)
      launch_ohwi_to_oihw_all(src + e->tf_poff, flat + e->tf_poff, e->tf_toff, e->mt_tit + e->tf_tensor, e->mt_nent - e->tf_tensor,
                              e->t.nparam - e->tf_poff, alpha, add, e->s);
    else
      launch_ohwi_to_oihw_all(src, flat, e->mt_toff, e->mt_tit, e->mt_nent, e->t.nparam, alpha, add, e->s);
    return;
  }
  for (const ConvL& c : e->t.convs) {
    if (sub && c.poff < e->tf_poff) continue;
    launch_ohwi_to_oihw(src + c.poff, flat + c.poff, c.cout, c.cin, c.T(), alpha, add, e->s);
    if (c.bias) launch_ohwi_to_oihw(src + c.poff + c.wsize(), flat + c.poff + c.wsize(), c.cout, 1, 1, alpha, add, e->s);
  }
}

int eosvos_set_init(eosvos_engine* e, const float* flat_params) {
  ModeScope mode_scope(e);
  if (!e || !flat_params) return fail("null argument");
  wino_weights_changed(e);
  pair_reset(e);
  import_params(e, flat_params, e->Winit);
  HIPOK(hipMemcpyAsync(e->Wp, e->Winit, (size_t)e->t.nparam * 4, hipMemcpyDeviceToDevice, e->s));
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_set_lr(eosvos_engine* e, const float* flat_lr) {
  ModeScope mode_scope(e);
  if (!e || !flat_lr) return fail("null argument");
  HIPOK(hipMemcpyAsync(e->lr, flat_lr, (size_t)e->t.nlr * 4, hipMemcpyDeviceToDevice, e->s));
  e->lr_level = EOSVOS_LR_NEURON; e->lr_log = 0;
  return 0;
}
static int64_t lr_store_count(const Topo& t, int level) {
  int ntens = 0;
  for (const ConvL& c : t.convs) ntens += c.bias ? 2 : 1;
  switch (level) {
    case EOSVOS_LR_NEURON: return t.nlr;
    case EOSVOS_LR_TENSOR: return ntens;
    case EOSVOS_LR_SINGLE: return 1;
    case EOSVOS_LR_PARAM: return t.nparam;
  }
  return -1;
}
int64_t eosvos_lr_store_count(int arch, int level) {
  Topo t;
  if (!build_topo(arch, t)) return -1;
  return lr_store_count(t, level);
}
static int ensure_lr_maps(eosvos_engine* e) {
  if (e->row_tensor) return 0;
  const Topo& t = e->t;
  std::vector<int> rt((size_t)t.nlr), r0;
  int ti = 0;
  for (const ConvL& c : t.convs) {      // trainable tensors in named_parameters() order: weight [, bias]
    r0.push_back((int)c.lroff);
    for (int r = 0; r < c.cout; ++r) rt[c.lroff + r] = ti;
    ++ti;
    if (c.bias) {
      r0.push_back((int)c.lroff + c.cout);
      for (int r = 0; r < c.cout; ++r) rt[c.lroff + c.cout + r] = ti;
      ++ti;
    }
  }
  r0.push_back((int)t.nlr);
  e->ntensors = ti;
  e->row_tensor = (int*)e->falloc(t.nlr);
  e->tensor_row0 = (int*)e->falloc(ti + 1);
  e->all_row0 = (int*)e->falloc(2);
  e->glr_tmp = e->falloc(t.nlr);
  if (!e->row_tensor || !e->tensor_row0 || !e->all_row0 || !e->glr_tmp) return fail("hipMalloc lr maps");
  const int all[2] = {0, (int)t.nlr};
  HIPOK(hipMemcpy(e->row_tensor, rt.data(), rt.size() * 4, hipMemcpyHostToDevice));
  HIPOK(hipMemcpy(e->tensor_row0, r0.data(), r0.size() * 4, hipMemcpyHostToDevice));
  HIPOK(hipMemcpy(e->all_row0, all, 8, hipMemcpyHostToDevice));
  return 0;
}
int eosvos_set_lr_state(eosvos_engine* e, int level, int use_log, const float* store) {
  ModeScope mode_scope(e);
  if (!e || !store) return fail("null argument");
  if (lr_store_count(e->t, level) < 0) return fail("unknown lr hierarchy level");
  if (ensure_lr_maps(e)) return 1;
  if (level == EOSVOS_LR_PARAM) {
    if (!e->lr_elem) {
      e->lr_elem = e->falloc(e->t.nparam);
      e->ptmp = e->falloc(e->t.nparam);
      if (!e->lr_elem || !e->ptmp) return fail("hipMalloc per-parameter lr");
    }
    import_params(e, store, e->lr_elem);
    if (use_log) launch_exp_inplace(e->lr_elem, e->t.nparam, e->s);
  } else {
    launch_lr_expand(store, e->row_tensor, e->lr, (int)e->t.nlr, level, use_log, e->s);
  }
  HIPOK(hipGetLastError());
  e->lr_level = level; e->lr_log = use_log ? 1 : 0;
  return 0;
}
int eosvos_set_norm(eosvos_engine* e, const float* gamma, const float* beta, const float* mean,
                    const float* var, float eps) {
  ModeScope mode_scope(e);
  if (!e || !gamma || !beta || !mean || !var) return fail("null argument");
  wino_weights_changed(e);
  std::fill(e->ks_amax_valid.begin(), e->ks_amax_valid.end(), 0);
  if (e->gn()) {                  // GroupNorm shares the (frozen) affine only (deeplabv3plus.py:186-188)
    HIPOK(hipMemcpyAsync(e->na, gamma, (size_t)e->t.nnorm * 4, hipMemcpyDeviceToDevice, e->s));
    HIPOK(hipMemcpyAsync(e->nb, beta, (size_t)e->t.nnorm * 4, hipMemcpyDeviceToDevice, e->s));
    return 0;
  }
  launch_fold_norm(gamma, beta, mean, var, eps, e->na, e->nb, e->t.nnorm, e->s);
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_reset(eosvos_engine* e) {
  ModeScope mode_scope(e);
  if (!e) return fail("null engine");
  wino_weights_changed(e);
  pair_reset(e);
  HIPOK(hipMemcpyAsync(e->Wp, e->Winit, (size_t)e->t.nparam * 4, hipMemcpyDeviceToDevice, e->s));
  return 0;
}
int eosvos_get_params(eosvos_engine* e, float* out) {
  ModeScope mode_scope(e);
  if (!e || !out) return fail("null argument");
  export_params(e, e->Wp, out, 1.f, 0);
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_set_params(eosvos_engine* e, const float* flat) {
  ModeScope mode_scope(e);
  if (!e || !flat) return fail("null argument");
  wino_weights_changed(e);
  pair_reset(e);
  import_params(e, flat, e->Wp);
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_snapshot_params(eosvos_engine* e) {
  ModeScope mode_scope(e);
  if (!e) return fail("null engine");
  HIPOK(hipMemcpyAsync(e->Wsnap, e->Wp, (size_t)e->t.nparam * 4, hipMemcpyDeviceToDevice, e->s));
  return 0;
}
int eosvos_restore_params(eosvos_engine* e) {
  ModeScope mode_scope(e);
  if (!e) return fail("null engine");
  wino_weights_changed(e);
  pair_reset(e);
  HIPOK(hipMemcpyAsync(e->Wp, e->Wsnap, (size_t)e->t.nparam * 4, hipMemcpyDeviceToDevice, e->s));
  return 0;
}

// ---- forward ------------------------------------------------------------------------------------
static int forward_impl(eosvos_engine* e, const float* images, int B, bool mirror = false) {
  const Topo& t = e->t;
  hipStream_t s = e->s;
  if (B != e->lastB) pair_reset(e);          // another batch size: a new trajectory for the pre-split producers' scales
  if (e->fwd_masks) ++e->pair_iter;          // training forward: the iteration the pre-split siblings belong to
  plans_match_mode(e);
  PlanScope plan_scope(e, 0);
  amax_new_phase(e, 0);
  if (h3_mode() && amax_init(e)) return fail("f16x3 matrix mode: no room for the absmax slots of this topology");
  if (h3_mode()) {
    amax_weights(e, s);
    bool stale = false, fresh = false;
    for (const auto& w : e->wino)
      if (w.V) { stale |= !w.us_valid; fresh |= w.us_valid; }
    if (stale && !fresh) {                          // every Winograd-domain weight is remade by this forward
      amax_zero(amax_slot(e, AM_U, 0), 2 * t.convs.size(), s);
      e->us_zero_epoch = e->fwd_epoch;
    }
  }
  // f16x3 mode: the stem runs on the fp16 matrix cores too (the frame's absmax comes from the layout pass)
  unsigned* ax = h3_mode() ? amax_fused_slot(e, AM_X, 0, e->xpad, s) : nullptr;
  launch_nchw_to_nhwc_pad(images, e->xpad, B, 3, e->H, e->W, 3, s, ax, mirror ? 1 : 0);
  auto stem_fwd = [&](const float* a, const float* b, float* y) {
    if (ax) launch_stem_fwd_h3(e->xpad, e->W_(0), a, b, y, B, e->H, e->W, e->h2, e->w2, ax, s);
    else launch_stem_fwd(e->xpad, e->W_(0), a, b, y, B, e->H, e->W, e->h2, e->w2, s);
  };
  if (e->gn()) {
    stem_fwd(nullptr, nullptr, e->zbuf[0]->p);
    launch_gn_forward(e->zbuf[0]->p, 64, e->G_(0), e->nb, nullptr, 0, e->c1->p, 64, e->gn_stats[0], e->gn_partial, B, e->h2 * e->w2, 64,
                      1e-5f, 1, s);
  } else {
    stem_fwd(e->A_(0), e->B_(0), e->c1->p);
  }
  launch_maxpool_fwd(e->c1->p, e->p1->p, e->p1idx, B, e->h2, e->w2, 64, e->h4, e->w4, s, twrite_fused(e, e->p1).slot);
  // independent forward branches go to the side stream (frozen-BN mode; the GroupNorm kernels share scratch)
  const bool fside = e->s2 != nullptr && !e->gn();
  auto fork = [&](int ci) {      // the side stream continues from this point of the main stream
    (void)hipEventRecord(e->ev[ci], s);
    (void)hipStreamWaitEvent(e->s2, e->ev[ci], 0);
  };
  if (fside && e->ev_wino_w && e->force_algo == 0) {
    // Winograd-domain weights depend on the weights only: all of them are made on the side stream now, beside the stem
    // and layer1..3, instead of in front of each Winograd conv on the critical path
    bool any = false;
    for (int ci = 0; ci < (int)e->wino.size(); ++ci) {      // (ascending: the order fixes the side stream's launch sequence)
      if (!e->wino[ci].V || e->wino[ci].us_valid || ci >= (int)e->conv_hin.size() || !e->conv_hin[ci]) continue;
      const ConvL& c = t.convs[ci];
      const int Ho = conv_out(e->conv_hin[ci], c.k, c.stride, c.dil, c.pad), Wo = conv_out(e->conv_win[ci], c.k, c.stride, c.dil, c.pad);
      if (!wino_on(e, ci, B, Ho, Wo)) continue;
      if (!any) { fork(0); any = true; }
      wino_ensure_weights(e, ci, wino_geom(e, c, B, Ho, Wo).tm, e->s2);
    }
    if (any) { (void)hipEventRecord(e->ev_wino_w, e->s2); e->wino_w_wait = true; }
  }
  const View dcat_low(e->dcat, 256, 48);      // decoder.conv1's slice of the decoder concat, behind the upsampled projection
  for (size_t i = 0; i < t.blocks.size(); ++i) {
    const Block& b = t.blocks[i];
    auto& f = e->bb[i];
    if (b.ds >= 0) {               // the projection shortcut only needs the block input: beside conv1 / conv2
      if (fside) fork(b.ds);
      conv_fwd(e, b.ds, f.xin, f.dsb, B, Opt().side(fside));
      if (fside) (void)hipEventRecord(e->ev[b.c3], e->s2);
    }
    conv_fwd(e, b.c1, f.xin, f.t1, B, Opt().relu());
    conv_fwd(e, b.c2, f.t1, f.t2, B, Opt().relu());
    if (b.ds >= 0 && fside) (void)hipStreamWaitEvent(s, e->ev[b.c3], 0);
    conv_fwd(e, b.c3, f.t2, f.out, B, Opt().relu().add(b.ds >= 0 ? f.dsb : f.xin));
    if ((int)i == t.layer1_last_block && fside && !t.v3) {
      // decoder.conv1 reads the layer1 feature only: it runs beside layer2..4 + ASPP
      fork(t.dec1);
      conv_fwd(e, t.dec1, f.out, dcat_low, B, Opt().relu().side());
      (void)hipEventRecord(e->ev[t.dec_a], e->s2);
    }
  }
  Tensor* const l4 = e->bb.back().out;
  const int P16 = e->h16 * e->w16;
  // The image-pooling branch (column sums, GEMV, broadcast, absmax: five small latency-bound launches) reads layer4's output
  // only: with a side stream it runs there, beside the four ASPP convs, and joins in front of the projection.
  hipStream_t ps = fside ? e->s2 : s;
  if (fside) fork(t.pool);
  auto pool_branch = [&]() {
    launch_colsum(l4->p, l4->C, e->vec, B, P16, 2048, 1.0f / (float)P16, e->colscratch, ps);
    if (e->gn()) {
      launch_gemv_fwd(e->W_(t.pool), e->vec, nullptr, nullptr, e->zbuf[t.pool]->p, B, 256, 2048, ps);
      launch_gn_forward(e->zbuf[t.pool]->p, 256, e->G_(t.pool), e->nb + t.convs[t.pool].noff, nullptr, 0, e->poolout, 256,
                        e->gn_stats[t.pool], e->gn_partial, B, 1, 256, 1e-5f, 1, ps);
    } else {
      launch_gemv_fwd(e->W_(t.pool), e->vec, e->A_(t.pool), e->B_(t.pool), e->poolout, B, 256, 2048, ps);
    }
    const View cat_pool(e->cat, 1024, 256);      // the pooling branch's slice of the ASPP concat, behind the four conv branches
    launch_bcast_pixels(e->poolout, cat_pool.ptr(), cat_pool.ld(), B, P16, 256, 1.f, ps, e->fwd_masks ? cat_pool.mask_to_write() : nullptr,
                        cat_pool.ldmask());
  };
  if (fside) pool_branch();
  for (int i = 0; i < 4; ++i)
    conv_fwd(e, t.aspp[i], l4, View(e->cat, 256 * i, 256), B, Opt().relu());
  if (!fside) pool_branch();
  if (h3_mode() && !amax_init(e)) {
    // cat = 4 conv outputs (their epilogues fed the tensor's slot) + the broadcast pooling branch (its B x 256 values here)
    if (unsigned* cs = tslot(e, *e->cat)) { launch_absmax(e->poolout, 1, B * 256, B * 256, cs, ps); tmark_valid(*e->cat); }
  }
  if (fside) { (void)hipEventRecord(e->ev[t.pool], e->s2); (void)hipStreamWaitEvent(s, e->ev[t.pool], 0); }
  conv_fwd(e, t.project, e->cat, e->proj, B, Opt().relu());
  const ConvL& lc = t.convs[t.last];
  if (t.v3) {
    // DeepLabHead after ASPP: 3x3 conv + norm + ReLU, 1x1 classifier, logits resized from the ASPP map (deeplabv3.py:13)
    conv_fwd(e, t.head3, e->proj, e->d1, B, Opt().relu());
    launch_last_fwd(e->d1->p, e->W_(t.last), e->W_(t.last) + lc.wsize(), e->lowlog, (int64_t)B * e->h16 * e->w16, 256, s);
  } else {
    if (fside) (void)hipStreamWaitEvent(s, e->ev[t.dec_a], 0);
    else conv_fwd(e, t.dec1, e->bb[t.layer1_last_block].out, dcat_low, B, Opt().relu());
    launch_resize_fwd(e->proj->p, e->proj->C, e->dcat->p, e->dcat->C, B, 256, e->up_h, e->up_w, s);
    conv_fwd(e, t.dec_a, e->dcat, e->d1, B, Opt().relu());
    conv_fwd(e, t.dec_b, e->d1, e->d2, B, Opt().relu());
    launch_last_fwd(e->d2->p, e->W_(t.last), e->W_(t.last) + lc.wsize(), e->lowlog, (int64_t)B * e->h4 * e->w4, 256, s);
  }
  launch_resize_fwd(e->lowlog, 1, e->logits, 1, B, 1, e->fin_h, e->fin_w, s);
  e->lastB = B;
  e->have_loss_grad = false;
  e->masks_valid = e->fwd_masks;
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(std::string("forward launch: ") + hipGetErrorString(err));
  return 0;
}

// ---- backward + fused update ----------------------------------------------------------------------
static int backward_impl(eosvos_engine* e, bool update, bool accumulate) {
  e->side_q.clear();              // nothing may be left over from a call that failed half way
  e->wg_pending.clear();
  const Topo& t = e->t;
  hipStream_t s = e->s;
  const int B = e->lastB;
  if (B < 1 || !e->have_loss_grad) return fail("backward without forward + loss");
  if (accumulate && !e->gsum) return fail("accumulate without eosvos_meta_task_begin");
  if (!e->masks_valid)
    return fail("backward after eosvos_infer: an inference forward keeps no ReLU masks (run eosvos_forward / eosvos_finetune_step)");
  plans_match_mode(e);
  PlanScope plan_scope(e, 1);
  const int64_t P4 = (int64_t)B * e->h4 * e->w4;
  const int P16 = e->h16 * e->w16;
  // trainable boundary (eosvos_set_trainable_from): no data gradient flows into a frozen conv's output, no frozen conv's
  // weight gradient is made; `l4_frozen`: the whole backbone is frozen, the pass ends at the ASPP
  const bool frozen = e->train_from > 0;
  const bool l4_frozen = frozen && e->train_from > t.blocks.back().c3;
  amax_new_phase(e, 1);
  // final resize
  launch_resize_bwd(e->dlogits, 1, e->g_low, 1, nullptr, 0, B, 1, e->fin_h, e->fin_w, s);
  if (t.v3) {
    // classifier conv (Cout = 1) and the head's 3x3 conv, both on the ASPP map; the projection output is ReLU-masked
    const int64_t PA = (int64_t)B * e->h16 * e->w16;
    const int chunks = last_bwd_chunks(PA);
    launch_last_bwd(e->d1->p, e->W_(t.last), e->g_low, e->g_d1->p, e->ws_wg + e->ws_off[t.last], PA, 256, chunks, s);
    twrite_plain(*e->g_d1);
    e->upd_splits[t.last] = chunks;
    conv_wgrad(e, t.head3, e->g_d1, e->proj, B);
    if (conv_dgrad(e, t.head3, e->g_d1, e->g_proj, B, Opt().mask(e->proj))) return 1;
  } else {
  // classifier conv (Cout = 1)
  {
    const int chunks = last_bwd_chunks(P4);
    launch_last_bwd(e->d2->p, e->W_(t.last), e->g_low, e->g_d2->p, e->ws_wg + e->ws_off[t.last], P4, 256, chunks, s);
    twrite_plain(*e->g_d2);
    e->upd_splits[t.last] = chunks;
  }
  // decoder 3x3 convs
  {
    conv_wgrad(e, t.dec_b, e->g_d2, e->d1, B);
    if (conv_dgrad(e, t.dec_b, e->g_d2, e->g_d1, B, Opt().mask(e->d1))) return 1;
    conv_wgrad(e, t.dec_a, e->g_d1, e->dcat, B);
    // channels [0,256) of dcat are the (unclamped) upsampled ASPP output: no ReLU mask there
    if (conv_dgrad(e, t.dec_a, e->g_d1, e->g_dcat, B, Opt().mask(e->dcat, 256))) return 1;
  }
  // decoder.conv1 on the low-level feature: raw gradient into g_out of layer1's last block
  {
    const auto& low = e->bb[t.layer1_last_block];
    const View g_dcat_low(e->g_dcat, 256, 48);
    conv_wgrad(e, t.dec1, g_dcat_low, low.out, B);
    if (!frozen && conv_dgrad(e, t.dec1, g_dcat_low, low.g_out, B)) return 1;
  }
  // decoder upsample backward (+ ReLU mask of the projection output)
  const View proj(e->proj);
  if (!proj.mask()) return fail("internal: the projection output has no ReLU mask bytes");
  launch_resize_bwd(e->g_dcat->p, e->g_dcat->C, e->g_proj->p, e->g_proj->C, proj.mask(), proj.ldmask(), B, 256, e->up_h, e->up_w, s,
                    twrite_fused(e, e->g_proj).slot);
  }
  // ASPP projection
  {
    conv_wgrad(e, t.project, e->g_proj, e->cat, B);
    if (conv_dgrad(e, t.project, e->g_proj, e->g_cat, B, Opt().mask(e->cat))) return 1;
  }
  Tensor* const g_l4 = e->bb.back().g_out;
  Tensor* const l4 = e->bb.back().out;
  // image-pooling branch: gp = sum_p g_cat[:,1024:1280]; g_l4 starts as the broadcast of its input gradient
  {
    const View g_cat_pool(e->g_cat, 1024, 256);
    launch_colsum(g_cat_pool.ptr(), g_cat_pool.ld(), e->gp, B, P16, 256, 1.f, e->colscratch, s);
    const float* gpz = e->gp;
    if (e->gn()) {
      launch_gn_backward(e->zbuf[t.pool]->p, 256, e->gp, 256, e->G_(t.pool), e->gn_stats[t.pool], e->gn_partial, B, 1, 256, s);
      gpz = e->zbuf[t.pool]->p;
    }
    // (frozen backbone: the weight gradient only, no input gradient)
    launch_gemv_bwd(e->W_(t.pool), e->vec, gpz, e->A_(t.pool), l4_frozen ? nullptr : e->gvec, e->ws_wg + e->ws_off[t.pool], B, 256,
                    2048, s);
    if (!l4_frozen) {
      launch_bcast_pixels(e->gvec, g_l4->p, g_l4->C, B, P16, 2048, 1.0f / (float)P16, s);
      twrite_plain(*g_l4);
    }
    e->upd_splits[t.pool] = 1;
  }
  {
    for (int i = 0; i < 4; ++i) conv_wgrad(e, t.aspp[i], View(e->g_cat, 256 * i, 256), l4, B);
    if (!l4_frozen && aspp_dgrad(e, B, g_l4, l4, false, nullptr)) return 1;
  }
  // layer4, ASPP and decoder are done: update them now (on the side stream if there is one)
  auto flush_part0 = [&]() -> int {
    if (e->s2) {
      side_flush(e);
      (void)hipEventRecord(e->ev[t.convs.size()], e->s);      // their dgrads were the last readers of W
      (void)hipStreamWaitEvent(e->s2, e->ev[t.convs.size()], 0);
      if (flush_updates(e, B, update, accumulate, 0, e->s2)) return 1;
      e->side_used = true;
    } else if (flush_updates(e, B, update, accumulate, 0, e->s)) return 1;
    return 0;
  };
  if (l4_frozen && flush_part0()) return 1;
  // bottlenecks, last to first.  g_out of each block = dL/d(pre-ReLU block output).
  const int first_l4_block = (int)t.blocks.size() - 3;
  for (int i = l4_frozen ? -1 : (int)t.blocks.size() - 1; i >= 0; --i) {
    if (i == first_l4_block - 1) {
      if (flush_part0()) return 1;
      if (frozen) break;                 // layer1..3 and the stem are frozen
    }
    const Block& b = t.blocks[i];
    auto& f = e->bb[i];
    conv_wgrad(e, b.c3, f.g_out, f.t2, B);
    if (conv_dgrad(e, b.c3, f.g_out, f.g_t2, B, Opt().mask(f.t2))) return 1;
    conv_wgrad(e, b.c2, f.g_t2, f.t1, B);
    if (conv_dgrad(e, b.c2, f.g_t2, f.g_t1, B, Opt().mask(f.t1))) return 1;
    // gradient w.r.t. the block input: conv1 path + identity / downsample path
    const bool is_first_block = i == 0;
    // the low-level feature already holds decoder.conv1's contribution
    bool have = !t.v3 && (i == t.layer1_last_block + 1);
    const Tensor* inmask = is_first_block ? nullptr : f.xin;   // p1 is a max-pool output: masked in maxpool_bwd
    // (the block's input is a frozen conv's output: weight gradients only)
    const bool in_frozen = frozen && b.c1 == e->train_from;
    if (b.ds >= 0) {
      conv_wgrad(e, b.ds, f.g_out, f.xin, B);
      if (!in_frozen && conv_dgrad(e, b.ds, f.g_out, f.g_xin, B, Opt().accum(have))) return 1;
      conv_wgrad(e, b.c1, f.g_t1, f.xin, B);
      if (!in_frozen && conv_dgrad(e, b.c1, f.g_t1, f.g_xin, B, Opt().accum().mask(inmask))) return 1;
    } else {
      // identity path: g_xin = mask * (dgrad_conv1(g_t1) + g_out)
      if (have) return fail("internal: identity block after the low-level tap is unsupported");
      conv_wgrad(e, b.c1, f.g_t1, f.xin, B);
      if (conv_dgrad(e, b.c1, f.g_t1, f.g_xin, B, Opt().mask(inmask).add(f.g_out))) return 1;
    }
    // first block of a ResNet layer: its data-gradient chain is queued, every operand of the stage's weight gradients
    // is final -> one grouped launch per tile shape
    if (b.ds >= 0 && flush_wgrad_group(e, t.stage[b.c1], B)) return 1;
  }
  // stem
  if (!frozen) {
  // f16x3 mode (frozen norm): the stem's weight gradient on the fp16 matrix cores; the absmax of its gradient operand comes
  // from the pooling backward, the frame's from this iteration's forward (slot (X, conv 0))
  const auto& xrec = amax_rec_of(e, AM_X, 0);
  const bool stem_h3 = h3_mode() && e->amax && xrec.epoch == e->fwd_epoch && xrec.ptr == e->xpad;
  // (GroupNorm mode, round 5: the gradient operand is dz of the stem's GroupNorm, whose apply pass reduces its absmax)
  unsigned* ag = stem_h3 ? amax_fused_slot(e, AM_G, 0, e->gn() ? e->zbuf[0]->p : e->g_c1->p, s) : nullptr;
  launch_maxpool_bwd(e->g_p1->p, e->p1idx, e->g_c1->p, B, e->h2, e->w2, 64, e->h4, e->w4, s, e->gn() ? nullptr : ag);
  {
    const int chunks = stem_wgrad_chunks(B, e->h2, e->w2);
    const float* gc1 = e->g_c1->p;
    if (e->gn()) {
      launch_gn_backward(e->zbuf[0]->p, 64, e->g_c1->p, 64, e->G_(0), e->gn_stats[0], e->gn_partial, B, e->h2 * e->w2, 64, s, ag);
      gc1 = e->zbuf[0]->p;
    }
    if (ag) launch_stem_wgrad_h3(e->xpad, gc1, e->ws_wg + e->ws_off[0], B, e->H, e->W, e->h2, e->w2, chunks, ag, amax_slot(e, AM_X, 0), s);
    else launch_stem_wgrad(e->xpad, gc1, e->ws_wg + e->ws_off[0], B, e->H, e->W, e->h2, e->w2, chunks, s);
    e->upd_splits[0] = chunks;
  }
  }
  if (e->s2) side_flush(e);
  if (e->s2 && e->side_used) {           // join: the update reads every slab
    (void)hipEventRecord(e->ev.back(), e->s2);
    (void)hipStreamWaitEvent(e->s, e->ev.back(), 0);
    e->side_used = false;
  }
  if (!frozen && flush_updates(e, B, update, accumulate, 1, e->s)) return 1;
  for (size_t ci = 0; ci < e->upd_splits.size(); ++ci) plan_mix((uint64_t)e->upd_splits[ci]);     // slabs per conv (incl. grouped launches)
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(std::string("backward launch: ") + hipGetErrorString(err));
  return 0;
}

int eosvos_forward(eosvos_engine* e, const float* images, int batch, float* logits_out) {
  ModeScope mode_scope(e);
  if (!e || !images) return fail("null argument");
  if (batch < 1 || batch > e->maxB) return fail("batch out of range");
  if (forward_impl(e, images, batch)) return 1;
  if (logits_out)
    HIPOK(hipMemcpyAsync(logits_out, e->logits, (size_t)batch * e->H * e->W * 4, hipMemcpyDeviceToDevice, e->s));
  return 0;
}
static int scratch_for(eosvos_engine* e, const char* who, const ScratchLayout& L, int n_frames, bool capped);   // the arena, below
namespace {
inline bool lovasz_kind(int kind) { return kind == EOSVOS_LOSS_LOVASZ_HINGE || kind == EOSVOS_LOSS_LOVASZ_HINGE_FLAT; }
inline bool bootstrap_kind(int kind) { return kind == EOSVOS_LOSS_BOOTSTRAPPED_BCE; }
inline bool boundary_kind(int kind) { return kind == EOSVOS_LOSS_BOUNDARY_F || kind == EOSVOS_LOSS_BCE_AND_BOUNDARY_F; }
inline bool surface_kind(int kind) { return kind == EOSVOS_LOSS_SURFACE; }
inline bool cldice_kind(int kind) { return kind == EOSVOS_LOSS_CLDICE; }
inline bool frame_shape_kind(int kind) { return boundary_kind(kind) || surface_kind(kind) || cldice_kind(kind); }   // an image is the engine's H x W
inline bool potts_kind(int kind) { return kind == EOSVOS_LOSS_POTTS; }                         // ... and reads the last forward's frames
// (7 and 11 are unassigned on purpose, see include/eosvos.h; 14 and up are unknown)
inline bool loss_kind_ok(int kind) {
  return (kind >= EOSVOS_LOSS_BCE && kind <= EOSVOS_LOSS_BOOTSTRAPPED_BCE) || frame_shape_kind(kind) || potts_kind(kind);
}
// a void label (null: none) is a finite value no target can take; 0 when it is one
int ignore_check(const float* v) {
  if (v && !(std::isfinite(*v) && (*v < 0.f || *v > 1.f))) return fail("the ignore label must be finite and outside [0, 1]");
  return 0;
}
constexpr int PROP_MAX_FRAMES = 1024;
// clamp((min(H, W) + 48) / 96, 1, 16): one erosion per 96 pixels of the frame's short side, 5 at 480 x 854.  Untuned.
inline int cldice_default_depth(int H, int W) { return std::min(CLDICE_MAX_DEPTH, std::max(1, (std::min(H, W) + 48) / 96)); }
inline int cldice_depth_of(const eosvos_engine* e) { return e->cldice_depth ? e->cldice_depth : cldice_default_depth(e->H, e->W); }
// The scratch some kinds need beside the gradient, sized for the engine's largest batch and allocated when such a kind is
// first selected or used: the Lovasz kinds' sort buffers, the bootstrapped BCE's histograms, state and partials (for maxB
// sets; their size does not depend on the number of pixels), the boundary-F kinds' per-pixel maps and partials, the surface
// loss's distance words (4 bytes per pixel of the largest batch) and partials, the centreline loss's planes and levels
// (6 (depth + 1) + 24 bytes per pixel of the largest batch, for the depth in use when it is allocated: loss_eval).
const struct {
  bool (*uses)(int kind);
  float* eosvos_engine::*buf;
  int64_t (*floats)(const eosvos_engine*);
  int64_t (*pixels)(const eosvos_engine*);      // what `limit` bounds
  int64_t limit;
  const char *too_many, *no_memory;
} LOSS_SCRATCH[] = {
    {lovasz_kind, &eosvos_engine::lovasz_scratch,
     [](const eosvos_engine* e) { return (int64_t)lovasz_scratch_floats((int64_t)e->maxB * e->H * e->W, e->maxB); },
     [](const eosvos_engine* e) { return (int64_t)e->maxB * e->H * e->W; }, (int64_t)1 << 30,
     "lovasz hinge: too many pixels for 32-bit sort values", "lovasz hinge: out of device memory for the sort scratch"},
    {bootstrap_kind, &eosvos_engine::bootstrap_scratch,
     [](const eosvos_engine* e) { return (int64_t)bootstrap_scratch_floats(e->maxB); },
     [](const eosvos_engine* e) { return (int64_t)e->maxB * e->H * e->W; }, (int64_t)1 << 31,
     "bootstrapped cross-entropy: a set must have fewer than 2^31 pixels",
     "bootstrapped cross-entropy: out of device memory for the selection scratch"},
    {boundary_kind, &eosvos_engine::boundary_scratch,
     [](const eosvos_engine* e) { return (int64_t)boundary_scratch_floats((int64_t)e->maxB * e->H * e->W, e->maxB); },
     [](const eosvos_engine* e) { return (int64_t)e->H * e->W; }, (int64_t)1 << 31,
     "boundary_f: an image must have fewer than 2^31 pixels", "boundary_f: out of device memory for the boundary maps"},
    {surface_kind, &eosvos_engine::surface_scratch,
     [](const eosvos_engine* e) { return (int64_t)surface_scratch_floats((int64_t)e->maxB * e->H * e->W, e->maxB); },
     [](const eosvos_engine* e) { return (int64_t)std::max(e->H, e->W); }, (int64_t)4097,
     "surface: frames larger than 4096 pixels a side are not supported", "surface: out of device memory for the distance words"},
    {cldice_kind, &eosvos_engine::cldice_scratch,
     [](const eosvos_engine* e) { return (int64_t)cldice_scratch_floats((int64_t)e->maxB * e->H * e->W, e->maxB, cldice_depth_of(e)); },
     [](const eosvos_engine* e) { return (int64_t)std::max(e->H, e->W); }, (int64_t)4097,
     "cldice: frames larger than 4096 pixels a side are not supported", "cldice: out of device memory for the skeleton levels"},
};
// the scratch of `kind`, if it needs one: called wherever a kind is about to be used or is selected; 0 on success
int loss_scratch_ensure(eosvos_engine* e, int kind) {
  for (const auto& s : LOSS_SCRATCH) {
    if (!s.uses(kind) || e->*s.buf) continue;
    if (s.pixels(e) >= s.limit) return fail(s.too_many);
    e->*s.buf = e->falloc(s.floats(e));
    if (!(e->*s.buf)) {
      (void)hipGetLastError();              // the failed hipMalloc must not surface in a later call's launch check
      return fail(s.no_memory);
    }
    if (cldice_kind(kind)) e->cldice_levels_held = cldice_depth_of(e) + 1;
  }
  return 0;
}
// min(16, ceil(0.008 * the frame diagonal)): the DAVIS boundary tolerance (data.davis_bound_pix) as the window radius
inline int boundary_default_radius(int H, int W) {
  const int r = (int)std::ceil(0.008 * std::sqrt((double)H * H + (double)W * W));
  return r < 1 ? 1 : r > 16 ? 16 : r;
}
// `images` maps of H x W (the scratch ensured by the caller); the combined kind evaluates the cross-entropy first and the
// boundary launches add to it
void boundary_eval(eosvos_engine* e, bool combined, const float* logits, const float* masks, int H, int W, int images, int radius,
                   const float* ignore, float* dlogits, float* loss) {
  if (combined) launch_loss(EOSVOS_LOSS_BCE, logits, masks, dlogits, loss, e->bce_partial, (int64_t)H * W * images, ignore, e->s);
  launch_boundary_f(logits, masks, dlogits, loss, e->boundary_scratch, H, W, images, radius ? radius : boundary_default_radius(H, W),
                    combined ? 1 : 0, ignore, e->s);
}
// max(1, min(H, W) / 4), at most 4095: a quarter of the frame's short side.  Untuned.
inline int surface_default_cap(int H, int W) { return std::min(4095, std::max(1, std::min(H, W) / 4)); }
// The pairwise loss's window and sigmas with 0 read as the default (radius 3, dilation 2, sigma_xy = radius * dilation,
// sigma_rgb 0.1; untuned), checked against the CRF's limits; 0 on success
struct PottsParams { int r, d; float sigma_xy, sigma_rgb; };
int potts_params(const char* who, int window, int dilation, float sigma_xy, float sigma_rgb, PottsParams* out) {
  const std::string w(who);
  if (window < 0 || window > 7) return fail(w + ": the window radius must be 1 .. 7, or 0 for the default");
  if (dilation < 0 || dilation > 4) return fail(w + ": the dilation must be 1 .. 4, or 0 for the default");
  const int r = window ? window : 3, d = dilation ? dilation : 2;
  if (r * d > 16) return fail(w + ": window radius * dilation must be at most 16");
  if (!(std::isfinite(sigma_xy) && sigma_xy >= 0.f)) return fail(w + ": sigma_xy must be finite and > 0, or 0 for the default");
  if (!(std::isfinite(sigma_rgb) && sigma_rgb >= 0.f)) return fail(w + ": sigma_rgb must be finite and > 0, or 0 for the default");
  if (out) *out = {r, d, sigma_xy > 0.f ? sigma_xy : (float)(r * d), sigma_rgb > 0.f ? sigma_rgb : 0.1f};
  return 0;
}
// the pairwise loss of `images` maps of H x W logits against `frames` (launch_potts's two layouts), its partials in the arena
int potts_eval(eosvos_engine* e, const char* who, const PottsParams& q, const float* logits, const float* frames, int pad, int H, int W,
               int images, float* dlogits, float* loss) {
  const PottsLayout L((size_t)potts_scratch_floats(H, W, images));
  if (scratch_for(e, who, L, images, true)) return 1;
  launch_potts(logits, frames, pad, dlogits, loss, (float*)((char*)e->scratch + L.partial.at), H, W, images, q.r, q.d, q.sigma_xy,
               q.sigma_rgb, e->s);
  return 0;
}
// Loss `kind` (checked by the caller) of `images` maps of n_per_image pixels -- the Lovasz kinds: per map, or with `flat` over
// all of them as one set -- with its gradient, into the device pointers loss / dlogits.  `ignore`: the void label, or null.
int loss_eval(eosvos_engine* e, int kind, const float* logits, const float* masks, int64_t n_per_image, int images, int flat,
              const float* ignore, float* dlogits, float* loss) {
  if (boundary_kind(kind) && n_per_image != (int64_t)e->H * e->W)      // needs the frame's shape: an image is the engine's H x W
    return fail("boundary_f: the loss needs the frame's shape, so n must be the engine's H * W (one image); use eosvos_boundary_f for another shape");
  if (surface_kind(kind) && n_per_image != (int64_t)e->H * e->W)
    return fail("surface: the loss needs the frame's shape, so n must be the engine's H * W (one image); use eosvos_surface_loss for another shape");
  if (cldice_kind(kind)) {
    if (n_per_image != (int64_t)e->H * e->W)
      return fail("cldice: the loss needs the frame's shape, so n must be the engine's H * W (one image); use eosvos_cldice_loss for another shape");
    if (e->cldice_scratch && cldice_depth_of(e) + 1 > e->cldice_levels_held) {     // deeper than the buffer holds: a larger one
      HIPOK(hipStreamSynchronize(e->s));                                           // earlier launches may still read the old one
      e->ffree(e->cldice_scratch);
      e->cldice_scratch = nullptr;
      e->cldice_levels_held = 0;
    }
  }
  if (potts_kind(kind)) {                // on the logits of the last forward only: its frames are the engine's copy of that forward's
    PottsParams q;
    if (logits != e->logits || e->lastB < 1 || images > e->lastB || n_per_image != (int64_t)e->H * e->W)
      return fail("potts: the loss reads the frames of the last forward; use eosvos_potts_loss (Engine.potts_loss) for caller tensors");
    if (potts_params("potts", e->potts_window, e->potts_dilation, e->potts_sigma_xy, e->potts_sigma_rgb, &q)) return 1;
    if (potts_eval(e, "potts", q, logits, e->xpad, 3, e->H, e->W, images, dlogits, loss)) return 1;
    HIPOK(hipGetLastError());
    return 0;
  }
  if (loss_scratch_ensure(e, kind)) return 1;
  if (lovasz_kind(kind)) {
    launch_lovasz(logits, masks, dlogits, loss, e->lovasz_scratch, n_per_image, images, flat, ignore, e->s);
  } else if (bootstrap_kind(kind)) {                          // per image, or (`flat`: caller tensors) all elements one set
    if (n_per_image * (flat ? images : 1) >= ((int64_t)1 << 31)) return fail("bootstrapped cross-entropy: a set must have fewer than 2^31 pixels");
    launch_bootstrap_bce(logits, masks, dlogits, loss, e->bootstrap_scratch, flat ? n_per_image * images : n_per_image,
                         flat ? 1 : images, e->bootstrap_q, ignore, e->s);
  } else if (boundary_kind(kind)) {
    boundary_eval(e, kind == EOSVOS_LOSS_BCE_AND_BOUNDARY_F, logits, masks, e->H, e->W, images, e->boundary_radius, ignore, dlogits, loss);
  } else if (surface_kind(kind)) {
    launch_surface(logits, masks, dlogits, loss, e->surface_scratch, e->H, e->W, images,
                   e->surface_cap ? e->surface_cap : surface_default_cap(e->H, e->W), ignore, e->s);
  } else if (cldice_kind(kind)) {
    launch_cldice(logits, masks, dlogits, loss, e->cldice_scratch, e->H, e->W, images, cldice_depth_of(e), ignore, e->s);
  } else {
    launch_loss(kind, logits, masks, dlogits, loss, e->bce_partial, n_per_image * images, ignore, e->s);
  }
  HIPOK(hipGetLastError());
  return 0;
}
// 0 when the spec names a loss: one known kind, or the term list of a sum (include/eosvos.h at eosvos_set_loss_sum)
int loss_spec_ok(const LossSpec& spec) {
  if (!spec.combine) return loss_kind_ok(spec.kinds[0]) ? 0 : fail("unknown loss kind");
  if (spec.n < 1 || spec.n > EOSVOS_LOSS_MAX_TERMS) return fail("a loss sum has 1 .. 4 terms");
  if (spec.null_terms) return fail("null argument");
  int boundary = 0;
  for (int i = 0; i < spec.n; ++i) {
    if (!loss_kind_ok(spec.kinds[i])) return fail("unknown loss kind");
    if (!(std::isfinite(spec.weights[i]) && spec.weights[i] > 0.f)) return fail("the weights of a loss sum must be finite and > 0");
    for (int j = 0; j < i; ++j)
      if (spec.kinds[j] == spec.kinds[i]) return fail("a loss sum names a kind twice");
    boundary += boundary_kind(spec.kinds[i]) ? 1 : 0;
  }
  if (boundary > 1) return fail("a loss sum takes one boundary kind: the two share the engine's radius");
  return 0;
}
// all a (checked) spec needs beside the launches' arguments: every kind's own scratch and, where it combines, the value
// slots and one gradient slice per term; 0 on success
int loss_spec_ensure(eosvos_engine* e, const LossSpec& spec) {
  for (int i = 0; i < spec.n; ++i)
    if (loss_scratch_ensure(e, spec.kinds[i])) return 1;
  if (!spec.combine) return 0;
  if (!e->sum_vals) {
    e->sum_vals = e->falloc(2 * EOSVOS_LOSS_MAX_TERMS);
    if (e->sum_vals && hipMemsetAsync(e->sum_vals, 0, sizeof(float) * 2 * EOSVOS_LOSS_MAX_TERMS, e->s) != hipSuccess) e->sum_vals = nullptr;
  }
  for (int i = 0; e->sum_vals && i < spec.n; ++i) {
    if (!e->sum_slice[i]) e->sum_slice[i] = e->falloc((int64_t)e->maxB * e->H * e->W);
    if (!e->sum_slice[i]) break;
  }
  if (!e->sum_vals || !e->sum_slice[spec.n - 1]) {
    (void)hipGetLastError();              // as loss_scratch_ensure
    return fail("loss sum: out of device memory for the terms' gradients");
  }
  return 0;
}
// The (checked) spec on `images` maps of n_per_image pixels, into the device pointers loss / dlogits.  `one_set`: caller
// tensors, every kind takes the elements as one set; otherwise only the flat Lovasz kind does.  One kind: its own launches and
// nothing else.  A sum: each term by the same launches into its slice and value slot, then the one that combines them; the
// slices bound n.
int loss_spec_eval(eosvos_engine* e, const LossSpec& spec, const float* logits, const float* masks, int64_t n_per_image, int images,
                   bool one_set, const float* ignore, float* dlogits, float* loss) {
  const auto flat = [&](int kind) { return one_set || kind == EOSVOS_LOSS_LOVASZ_HINGE_FLAT; };
  if (!spec.combine) return loss_eval(e, spec.kinds[0], logits, masks, n_per_image, images, flat(spec.kinds[0]), ignore, dlogits, loss);
  const int64_t n = n_per_image * images;
  if (n > (int64_t)e->maxB * e->H * e->W) return fail("n exceeds the engine's scratch");
  if (loss_spec_ensure(e, spec)) return 1;
  for (int i = 0; i < spec.n; ++i)
    if (loss_eval(e, spec.kinds[i], logits, masks, n_per_image, images, flat(spec.kinds[i]), ignore, e->sum_slice[i], e->sum_vals + i))
      return 1;
  launch_loss_sum(spec.n, e->sum_slice, spec.weights, e->sum_vals, dlogits, loss, e->sum_vals + EOSVOS_LOSS_MAX_TERMS, n, e->s);
  HIPOK(hipGetLastError());
  e->sum_last_terms = spec.n;
  return 0;
}
inline bool spec_has_potts(const LossSpec& spec) {
  for (int i = 0; i < spec.n && i < EOSVOS_LOSS_MAX_TERMS; ++i)
    if (potts_kind(spec.kinds[i])) return true;
  return false;
}
// on the logits of the last forward: leaves dL/dlogits for eosvos_backward_step, and none after a failed evaluation
int loss_on_forward(eosvos_engine* e, const LossSpec& spec, const float* masks, int batch, const float* ignore, float* loss_out) {
  if (!e || !masks) return fail("null argument");
  if (loss_spec_ok(spec) || ignore_check(ignore)) return 1;
  if (e->lastB < 1 && spec_has_potts(spec)) {
    e->have_loss_grad = false;
    return fail("potts: the loss reads the frames of the last forward, and there has been none on this engine");
  }
  if (batch != e->lastB) return fail("loss batch differs from the last forward");
  e->have_loss_grad = false;
  if (loss_spec_eval(e, spec, e->logits, masks, (int64_t)e->H * e->W, batch, false, ignore, e->dlogits, e->loss_dev)) return 1;
  e->have_loss_grad = true;
  if (loss_out) HIPOK(hipMemcpyAsync(loss_out, e->loss_dev, 4, hipMemcpyDeviceToDevice, e->s));
  return 0;
}
// where an evaluation on caller tensors puts its gradient: the caller's buffer, or the engine's own dlogits scratch, which
// invalidates a pending eosvos_loss* gradient
float* grad_target(eosvos_engine* e, float* dlogits_out) {
  if (!dlogits_out) e->have_loss_grad = false;
  return dlogits_out ? dlogits_out : e->dlogits;
}
// on caller tensors, the n elements one set.  The engine's dlogits scratch bounds n; a single kind with a caller buffer has no
// bound, a sum always that of its slices.
int loss_on_tensors(eosvos_engine* e, const LossSpec& spec, const float* logits, const float* masks, int64_t n, const float* ignore,
                    float* loss_out, float* dlogits_out) {
  if (!e || !logits || !masks || !loss_out || n < 1) return fail("bad argument");
  if (loss_spec_ok(spec) || ignore_check(ignore)) return 1;
  if (spec_has_potts(spec))              // no frames travel with caller tensors through these entry points
    return fail("potts: the loss needs the frames; on caller tensors use eosvos_potts_loss (Engine.potts_loss), which takes them");
  if (!spec.combine && !dlogits_out && n > (int64_t)e->maxB * e->H * e->W) return fail("n exceeds the engine's scratch");
  return loss_spec_eval(e, spec, logits, masks, n, 1, true, ignore, grad_target(e, dlogits_out), loss_out);
}
// the loss of the fused entry points
inline int fused_loss(eosvos_engine* e, const float* masks, int batch) {
  return loss_on_forward(e, e->fused, masks, batch, e->loss_ignore_on ? &e->loss_ignore : nullptr, nullptr);
}
int set_fused_loss(eosvos_engine* e, const LossSpec& spec) {
  if (!e) return fail("null engine");
  if (loss_spec_ok(spec) || loss_spec_ensure(e, spec)) return 1;
  e->fused = spec;
  return 0;
}
}  // namespace

// ---- the loss entry points: forms of loss_on_forward / loss_on_tensors, each building its LossSpec ----
int eosvos_loss_bce(eosvos_engine* e, const float* masks, int batch, float* loss_out) {
  ModeScope mode_scope(e);
  return loss_on_forward(e, LossSpec::single(EOSVOS_LOSS_BCE), masks, batch, nullptr, loss_out);
}
int eosvos_loss(eosvos_engine* e, int kind, const float* masks, int batch, float* loss_out) {
  ModeScope mode_scope(e);
  return loss_on_forward(e, LossSpec::single(kind), masks, batch, nullptr, loss_out);
}
int eosvos_loss_ignore(eosvos_engine* e, int kind, const float* masks, int batch, float ignore, float* loss_out) {
  ModeScope mode_scope(e);
  return loss_on_forward(e, LossSpec::single(kind), masks, batch, &ignore, loss_out);
}
int eosvos_loss_sum(eosvos_engine* e, int n_terms, const int* kinds, const float* weights, const float* masks, int batch,
                    int ignore_on, float ignore, float* loss_out) {
  ModeScope mode_scope(e);
  return loss_on_forward(e, LossSpec::sum(n_terms, kinds, weights), masks, batch, ignore_on ? &ignore : nullptr, loss_out);
}
int eosvos_bce(eosvos_engine* e, const float* logits, const float* masks, int64_t n, float* loss_out,
               float* dlogits_out) {
  ModeScope mode_scope(e);
  return loss_on_tensors(e, LossSpec::single(EOSVOS_LOSS_BCE), logits, masks, n, nullptr, loss_out, dlogits_out);
}
int eosvos_loss_tensors(eosvos_engine* e, int kind, const float* logits, const float* masks, int64_t n, float* loss_out) {
  ModeScope mode_scope(e);
  return loss_on_tensors(e, LossSpec::single(kind), logits, masks, n, nullptr, loss_out, nullptr);
}
int eosvos_loss_tensors_ignore(eosvos_engine* e, int kind, const float* logits, const float* masks, int64_t n, float ignore,
                               float* loss_out) {
  ModeScope mode_scope(e);
  return loss_on_tensors(e, LossSpec::single(kind), logits, masks, n, &ignore, loss_out, nullptr);
}
int eosvos_loss_sum_tensors(eosvos_engine* e, int n_terms, const int* kinds, const float* weights, const float* logits,
                            const float* masks, int64_t n, int ignore_on, float ignore, float* loss_out, float* dlogits_out) {
  ModeScope mode_scope(e);
  return loss_on_tensors(e, LossSpec::sum(n_terms, kinds, weights), logits, masks, n, ignore_on ? &ignore : nullptr, loss_out,
                         dlogits_out);
}
int eosvos_set_loss(eosvos_engine* e, int kind) { return set_fused_loss(e, LossSpec::single(kind)); }
int eosvos_set_loss_sum(eosvos_engine* e, int n_terms, const int* kinds, const float* weights) {
  return set_fused_loss(e, LossSpec::sum(n_terms, kinds, weights));
}
int eosvos_set_loss_ignore(eosvos_engine* e, int on, float ignore) {
  if (!e) return fail("null engine");
  if (on && ignore_check(&ignore)) return 1;
  e->loss_ignore_on = on != 0;
  e->loss_ignore = on ? ignore : 0.f;
  return 0;
}
int eosvos_last_loss(eosvos_engine* e, float* loss_out) {
  if (!e || !loss_out) return fail("null argument");
  HIPOK(hipMemcpyAsync(loss_out, e->loss_dev, 4, hipMemcpyDeviceToDevice, e->s));
  return 0;
}
int eosvos_last_loss_terms(eosvos_engine* e, float* out, int* n_terms_host) {
  if (!e || !out) return fail("null argument");
  if (!e->sum_last_terms) return fail("eosvos_last_loss_terms: no loss sum has been evaluated on this engine");
  HIPOK(hipMemcpyAsync(out, e->sum_vals + EOSVOS_LOSS_MAX_TERMS, sizeof(float) * EOSVOS_LOSS_MAX_TERMS, hipMemcpyDeviceToDevice, e->s));
  if (n_terms_host) *n_terms_host = e->sum_last_terms;
  return 0;
}
int eosvos_set_loss_bootstrap(eosvos_engine* e, float fraction) {
  if (!e) return fail("null engine");
  if (!(fraction > 0.f && fraction <= 1.f)) return fail("the bootstrap fraction must be in (0, 1]");      // (NaN fails both)
  const long q = lround((double)fraction * 65536.0);
  e->bootstrap_q = (int)(q < 1 ? 1 : q > 65536 ? 65536 : q);
  return 0;
}
int eosvos_set_loss_boundary(eosvos_engine* e, int radius) {
  if (!e) return fail("null engine");
  if (radius < 0 || radius > 16) return fail("the boundary radius must be 1 .. 16, or 0 for the frame-size default");
  e->boundary_radius = radius;
  return 0;
}
int eosvos_boundary_f(eosvos_engine* e, const float* logits, const float* masks, int batch, int height, int width, int radius,
                      int combined, int ignore_on, float ignore, float* loss_out, float* dlogits_out) {
  ModeScope mode_scope(e);
  if (!e || !logits || !masks || !loss_out) return fail("null argument");
  if (batch < 1 || batch > e->maxB || height < 1 || width < 1) return fail("eosvos_boundary_f: bad geometry");
  if ((int64_t)batch * height * width > (int64_t)e->maxB * e->H * e->W) return fail("eosvos_boundary_f: more pixels than the engine's scratch holds");
  if (radius < 0 || radius > 16) return fail("the boundary radius must be 1 .. 16, or 0 for the frame-size default");
  if (ignore_on && ignore_check(&ignore)) return 1;
  float* const dlogits = grad_target(e, dlogits_out);
  if (loss_scratch_ensure(e, EOSVOS_LOSS_BOUNDARY_F)) return 1;
  boundary_eval(e, combined != 0, logits, masks, height, width, batch, radius, ignore_on ? &ignore : nullptr, dlogits, loss_out);
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_propagation_targets(eosvos_engine* e, const float* probs, int n_frames, int64_t n_pix, float lo, float hi,
                               float ignore, float* targets_out, int64_t* n_pos_host) {
  if (!e || !probs || !targets_out) return fail("null argument");
  if (n_frames < 1 || n_frames > PROP_MAX_FRAMES || n_pix < 1 || n_pix >= ((int64_t)1 << 31))
    return fail("eosvos_propagation_targets: 1 .. 1024 frames of 1 .. 2^31 - 1 pixels");
  if (!(lo >= 0.f && lo < hi && hi <= 1.f)) return fail("eosvos_propagation_targets: needs 0 <= lo < hi <= 1");
  if (ignore_check(&ignore)) return 1;
  if (!e->prop_count) {
    e->prop_count = (int*)e->falloc(PROP_MAX_FRAMES);
    if (!e->prop_count) {
      (void)hipGetLastError();
      return fail("hipMalloc propagation counters");
    }
  }
  HIPOK(hipMemsetAsync(e->prop_count, 0, sizeof(int) * n_frames, e->s));
  launch_propagation_targets(probs, targets_out, e->prop_count, n_frames, n_pix, lo, hi, ignore, e->s);
  HIPOK(hipGetLastError());
  if (n_pos_host) {
    std::vector<int> host(n_frames);
    HIPOK(hipMemcpyAsync(host.data(), e->prop_count, sizeof(int) * n_frames, hipMemcpyDeviceToHost, e->s));
    HIPOK(hipStreamSynchronize(e->s));
    for (int f = 0; f < n_frames; ++f) n_pos_host[f] = host[f];
  }
  return 0;
}
int eosvos_backward_step(eosvos_engine* e, int accumulate) {
  ModeScope mode_scope(e);
  if (!e) return fail("null engine");
  return backward_impl(e, true, accumulate != 0);
}
int eosvos_finetune_step(eosvos_engine* e, const float* images, const float* masks, int batch, int accumulate,
                         float* loss_host) {
  ModeScope mode_scope(e);
  if (eosvos_forward(e, images, batch, nullptr)) return 1;
  if (fused_loss(e, masks, batch)) return 1;
  if (backward_impl(e, true, accumulate != 0)) return 1;
  if (loss_host) {
    HIPOK(hipMemcpyAsync(loss_host, e->loss_dev, 4, hipMemcpyDeviceToHost, e->s));
    HIPOK(hipStreamSynchronize(e->s));
  }
  return 0;
}
int eosvos_get_grads(eosvos_engine* e, float* out) {
  ModeScope mode_scope(e);
  if (!e || !out) return fail("null argument");
  if (!e->keep_grads) return fail("gradients are only kept after eosvos_keep_grads(e, 1)");
  if (e->train_from > 0) HIPOK(hipMemsetAsync(out, 0, (size_t)e->tf_poff * 4, e->s));     // frozen tensors: zero gradient
  export_params(e, e->gout, out, 1.f, 0, true);
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_debug_gsum(eosvos_engine* e, float* out) {
  ModeScope mode_scope(e);
  if (!e || !out) return fail("null argument");
  if (!e->gsum) return fail("eosvos_debug_gsum without eosvos_meta_task_begin");
  if (e->train_from > 0) HIPOK(hipMemsetAsync(out, 0, (size_t)e->tf_poff * 4, e->s));     // frozen tensors: nothing is summed
  export_params(e, e->gsum, out, 1.f, 0, true);
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_keep_grads(eosvos_engine* e, int on) {
  if (!e) return fail("null engine");
  e->keep_grads = on != 0;
  return 0;
}

int eosvos_infer(eosvos_engine* e, const float* images, int batch, float* probs_out) {
  ModeScope mode_scope(e);
  if (!e || !images || !probs_out) return fail("null argument");
  if (batch < 1 || batch > e->maxB) return fail("batch out of range");
  e->fwd_masks = false;                 // inference: nothing will differentiate through this forward
  const int rc = forward_impl(e, images, batch);
  e->fwd_masks = true;
  if (rc) return 1;
  launch_sigmoid(e->logits, probs_out, (int64_t)batch * e->H * e->W, e->s);
  HIPOK(hipGetLastError());
  return 0;
}
// ---- test-time augmentation: mirrored / rescaled views averaged in probability space ------------
int eosvos_infer_view(eosvos_engine* e, const float* images, int batch, int mirror) {
  ModeScope mode_scope(e);
  if (!e || !images) return fail("null argument");
  if (batch < 1 || batch > e->maxB) return fail("batch out of range");
  e->fwd_masks = false;                 // inference, as eosvos_infer
  const int rc = forward_impl(e, images, batch, mirror != 0);
  e->fwd_masks = true;
  return rc ? 1 : 0;
}
int eosvos_tta_accumulate(eosvos_engine* e_view, int h, int w, int batch, int mirror, float weight, int first, float* acc,
                          int H, int W) {
  if (!e_view || !acc) return fail("null argument");
  if (batch < 1 || batch > e_view->maxB) return fail("batch out of range");
  if (h < 1 || w < 1 || H < 1 || W < 1) return fail("eosvos_tta_accumulate: sizes must be >= 1");
  if (h != e_view->H || w != e_view->W) return fail("eosvos_tta_accumulate: h x w is not the frame size of the view's engine");
  if (!(weight == weight) || weight - weight != 0.f) return fail("eosvos_tta_accumulate: the weight must be finite");
  launch_tta_accumulate(e_view->logits, acc, batch, h, w, H, W, mirror != 0, weight, first != 0, e_view->s);
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_resize_frames(eosvos_engine* e, const float* src, int B, int C, int h_in, int w_in, int h_out, int w_out, float* dst) {
  if (!e || !src || !dst) return fail("null argument");
  if (B < 1 || C < 1) return fail("batch out of range");
  if (h_in < 1 || w_in < 1 || h_out < 1 || w_out < 1) return fail("eosvos_resize_frames: sizes must be >= 1");
  if ((int64_t)B * C > 0x7fffffff) return fail("eosvos_resize_frames: too many planes");
  // the tables of a (in, out) pair stay with the engine: the frames of a sequence all take the same ones
  auto tab = [&](int in, int out) -> const ResizeTab* {
    auto it = e->frame_tabs.find({in, out});
    if (it == e->frame_tabs.end()) {
      ResizeTab t;
      if (upload_resize(e, make_resize(in, out, false), in, out, t)) return nullptr;
      it = e->frame_tabs.emplace(std::make_pair(in, out), t).first;
    }
    return &it->second;
  };
  const ResizeTab* th = tab(h_in, h_out);
  const ResizeTab* tw = th ? tab(w_in, w_out) : nullptr;
  if (!th || !tw) return 1;
  launch_resize_fwd(src, 1, dst, 1, B * C, 1, *th, *tw, e->s);      // NCHW planes = B * C one-channel images
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_merge_labels(eosvos_engine* e, const float* probs, int n_obj, int64_t n_pix, uint8_t* labels) {
  if (!e || !probs || !labels || n_obj < 1) return fail("bad argument");
  launch_merge_labels(probs, n_obj, n_pix, labels, e->s);
  HIPOK(hipGetLastError());
  return 0;
}

// ---- data augmentation on the device (custom_transforms.py:9-92,189-213) --------------------------
int eosvos_warp_affine(eosvos_engine* e, const float* src, int channels, int flip, double rot_deg, double scale,
                       int interp, float* dst, int* nonzero_host) {
  if (!e) return fail("bad argument");
  return eosvos_warp_affine_hw(e, src, channels, e->H, e->W, flip, rot_deg, scale, interp, dst, nonzero_host);
}
// the warp's counter and the cubic coefficient table, allocated on first use (eosvos_warp_affine_hw, eosvos_lucid_compose)
static int aug_tables(eosvos_engine* e) {
  if (!e->aug_tab) {
    e->aug_tab = (int*)e->falloc(4);            // the non-zero counter of label warps
    e->aug_ctab = e->falloc(128);
    if (!e->aug_tab || !e->aug_ctab) return fail("hipMalloc augmentation tables");
    float ct[128];
    for (int i = 0; i < 32; ++i) {        // interpolateCubic(i/32), A = -0.75, float arithmetic as OpenCV's table
      const float A = -0.75f, x = i * (1.f / 32);
      float* c = ct + i * 4;
      c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
      c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
      c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
      c[3] = 1.f - c[0] - c[1] - c[2];
    }
    HIPOK(hipMemcpy(e->aug_ctab, ct, sizeof(ct), hipMemcpyHostToDevice));
  }
  return 0;
}
int eosvos_warp_affine_hw(eosvos_engine* e, const float* src, int channels, int height, int width, int flip, double rot_deg,
                          double scale, int interp, float* dst, int* nonzero_host) {
  ModeScope mode_scope(e);
  if (!e || !src || !dst || channels < 1 || height < 1 || width < 1) return fail("bad argument");
  if (interp != EOSVOS_INTER_NEAREST && interp != EOSVOS_INTER_CUBIC) return fail("unknown interpolation");
  const int H = height, W = width;
  if (aug_tables(e)) return 1;
  // cv2.getRotationMatrix2D((w/2, h/2), rot, sc): center is a Point2f
  const double ang = rot_deg * (3.1415926535897932384626433832795 / 180.0);
  const double alpha = cos(ang) * scale, beta = sin(ang) * scale;
  const double cx = (double)(float)(W / 2.0), cy = (double)(float)(H / 2.0);
  double M[6] = {alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy};
  // cv::warpAffine without WARP_INVERSE_MAP inverts the matrix, then walks dst pixels in fixed point
  double D = M[0] * M[4] - M[1] * M[3];
  D = D != 0 ? 1. / D : 0;
  const double A11 = M[4] * D, A22 = M[0] * D;
  M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
  const double b1 = -M[0] * M[2] - M[1] * M[5], b2 = -M[3] * M[2] - M[4] * M[5];
  M[2] = b1; M[5] = b2;
  const int AB_SCALE = 1 << 10;
  const int round_delta = interp == EOSVOS_INTER_NEAREST ? AB_SCALE / 2 : AB_SCALE / 32 / 2;
  // the fixed-point tables are evaluated in the kernel from M and round_delta (travelling by value): a queued launch
  // owns everything it reads, so calls can follow each other without a host wait
  int* counter = e->aug_tab;
  if (nonzero_host) HIPOK(hipMemsetAsync(counter, 0, sizeof(int), e->s));
  launch_warp_affine(src, dst, channels, H, W, M, round_delta, e->aug_ctab, interp == EOSVOS_INTER_CUBIC, flip != 0,
                     nonzero_host ? counter : nullptr, e->s);
  HIPOK(hipGetLastError());
  if (nonzero_host) {
    HIPOK(hipMemcpyAsync(nonzero_host, counter, sizeof(int), hipMemcpyDeviceToHost, e->s));
    HIPOK(hipStreamSynchronize(e->s));
  }
  return 0;
}

// ---- what the evaluation-stage entry points below share: the scratch arena, the geometry check, keep runs, the count read ----
// Makes e->scratch hold `need` bytes; with `capped`, a call may ask for 512 MB at most.  Grow-only.
static int scratch_grow(eosvos_engine* e, const char* who, size_t need, int n_frames, bool capped = true) {
  const std::string w(who);
  if (capped && need > ((size_t)512 << 20))
    return fail(w + ": " + std::to_string(need >> 20) + " MB of scratch for " + std::to_string(n_frames) +
                " frames exceeds the 512 MB cap of one call: pass fewer frames per call");
  if (need > e->scratch_cap) {
    HIPOK(hipStreamSynchronize(e->s));                              // earlier calls' launches may still read the old buffer
    if (e->scratch) HIPOK(hipFree(e->scratch));
    e->scratch = nullptr;
    e->scratch_cap = 0;
    if (hipMalloc(&e->scratch, need) != hipSuccess) {
      (void)hipGetLastError();                                      // the failed allocation is reported here, not by a later call
      e->scratch = nullptr;
      return fail(w + ": hipMalloc of " + std::to_string(need >> 20) + " MB of scratch failed");
    }
    e->scratch_cap = need;
    static const char* fill = getenv("EOSVOS_DEBUG_FILL");          // as falloc: the buffer starts out as that word
    if (fill) { (void)hipMemsetD32((hipDeviceptr_t)e->scratch, (int)strtoul(fill, nullptr, 16), need / 4); (void)hipDeviceSynchronize(); }
  }
  return 0;
}
// ... for a stage's layout, with the range that stage needs cleared set to 0 on the stream
static int scratch_for(eosvos_engine* e, const char* who, const ScratchLayout& L, int n_frames, bool capped = true) {
  if (scratch_grow(e, who, L.need(), n_frames, capped)) return 1;
  if (L.clear_bytes) HIPOK(hipMemsetAsync((char*)e->scratch + L.clear_at, 0, L.clear_bytes, e->s));
  return 0;
}
// frames in [min_frames, max_frames] and sides in [1, max_side]; a limit of 0 is not checked
static int frames_check(const char* who, int n_frames, int height, int width, int max_frames = 65535, int max_side = 4096, int min_frames = 0) {
  const std::string w(who);
  if (n_frames < min_frames || height < 1 || width < 1) return fail(w + ": bad frame geometry");
  if (max_side && (height > max_side || width > max_side))
    return fail(w + ": frames larger than " + std::to_string(max_side) + " pixels a side are not supported");
  if (max_frames && n_frames > max_frames) return fail(w + ": at most " + std::to_string(max_frames) + " frames per call");
  return 0;
}
extern "C++" {
template <class T> static T* scratch_at(eosvos_engine* e, ScratchAt<T> r) { return (T*)((char*)e->scratch + r.at); }
// launch(f, frames, flag) for every run of frames with the same `keep` flag: one frame per run where a frame reads the result
// of the frame before it (`chained`), one run of kept frames with `all`
template <class F> static int keep_runs(const uint8_t* keep, int n_frames, bool all, bool chained, F launch) {
  for (int f = 0, g; f < n_frames; f = g) {
    const int flag = all || (keep && keep[f]);
    for (g = f + 1; !chained && g < n_frames && (all || (keep && keep[g]) == flag); ++g) {}
    launch(f, g - f, flag);
    HIPOK(hipGetLastError());
  }
  return 0;
}
// a call's one host read: its n counters at `at`, widened where the device keeps narrower ones; without `host`, no wait
template <class D, class H> static int read_counts(eosvos_engine* e, ScratchAt<D> at, size_t n, H* host) {
  if (!host) return 0;
  std::vector<D> dev(n);
  HIPOK(hipMemcpyAsync(dev.data(), scratch_at(e, at), n * sizeof(D), hipMemcpyDeviceToHost, e->s));
  HIPOK(hipStreamSynchronize(e->s));
  std::copy(dev.begin(), dev.end(), host);
  return 0;
}
}

// ---- DAVIS-2017 evaluation counts (evaluate.py:345-359, helper_func.py:444-458) -------------------------------------
int eosvos_davis_counts(eosvos_engine* e, const uint8_t* pred, const uint8_t* gt, int n_frames, int height, int width, int n_obj,
                        int bound_pix, int64_t* counts_out) {
  if (!e || !pred || !gt || !counts_out) return fail("davis_counts: null argument");
  if (frames_check("davis_counts", n_frames, height, width, 0, 0)) return 1;
  if (width > 64 * 64) return fail("davis_counts: frames wider than 4096 pixels are not supported");
  if (n_obj < 1 || n_obj > 255) return fail("davis_counts: n_obj must be in [1, 255]");
  if (bound_pix < 0 || bound_pix > 63) return fail("davis_counts: the dilation radius must be in [0, 63] pixels");
  if (n_frames == 0) return 0;
  const DavisCountsLayout L(n_frames, n_obj, height, width);
  if (scratch_for(e, "davis_counts", L, n_frames, false)) return 1;   // no cap: the maps are chunked here, the counts are small
  const size_t plane = (size_t)height * width;
  for (size_t f0 = 0; f0 < (size_t)n_frames; f0 += L.chunk) {
    const int nf = (int)std::min<size_t>(L.chunk, (size_t)n_frames - f0);
    launch_davis_counts(pred + f0 * plane, gt + f0 * plane, nf, height, width, n_obj, bound_pix, scratch_at(e, L.pred_map),
                        scratch_at(e, L.gt_map), scratch_at(e, L.counts) + f0 * n_obj * 6, e->s);
    HIPOK(hipGetLastError());
  }
  return read_counts(e, L.counts, (size_t)n_frames * n_obj * 6, counts_out);
}

// ---- local dense-CRF refinement of the merged label maps (beside evaluate.py:322-326) -------------------------------
int eosvos_crf_labels(eosvos_engine* e, const float* images, const float* probs, int n_frames, int n_obj, int height, int width,
                      int iterations, int radius, int dilation, float w_appearance, float w_smooth, float theta_alpha,
                      float theta_beta, float theta_gamma, uint8_t* labels_out, float* q_out) {
  if (!e || !images || !probs || !labels_out) return fail("crf_labels: null argument");
  if (frames_check("crf_labels", n_frames, height, width, 65535, 0)) return 1;
  if (n_obj < 1 || n_obj > 255) return fail("crf_labels: n_obj must be in [1, 255]");
  if (iterations < 0 || iterations > 20) return fail("crf_labels: iterations must be in [0, 20]");
  if (radius < 1 || radius > 7) return fail("crf_labels: radius must be in [1, 7]");
  if (dilation < 1 || dilation > 4) return fail("crf_labels: dilation must be in [1, 4]");
  if (radius * dilation > 16) return fail("crf_labels: radius * dilation must be at most 16");
  if (!std::isfinite(w_appearance) || !std::isfinite(w_smooth) || w_appearance < 0.f || w_smooth < 0.f)
    return fail("crf_labels: the weights must be finite and >= 0");
  if (!std::isfinite(theta_alpha) || !std::isfinite(theta_beta) || !std::isfinite(theta_gamma) || theta_alpha <= 0.f ||
      theta_beta <= 0.f || theta_gamma <= 0.f)
    return fail("crf_labels: every theta must be finite and > 0");
  if (n_frames == 0) return 0;
  const int n_lab = n_obj + 1;
  const int64_t n_pix = (int64_t)height * width;
  if (iterations == 0) {                // the plain merge; Q^0 only on request, straight into q_out
    launch_crf_prepare(probs, n_frames, n_obj, n_pix, q_out, nullptr, labels_out, e->s);
    HIPOK(hipGetLastError());
    return 0;
  }
  const CrfLabelsLayout L((size_t)n_frames * n_lab * n_pix);
  if (scratch_for(e, "crf_labels", L, n_frames)) return 1;
  float* unary = scratch_at(e, L.unary);
  float* q[2] = {scratch_at(e, L.q[0]), scratch_at(e, L.q[1])};
  CrfTables tab;
  crf_fill_tables(tab, radius, dilation, theta_alpha, theta_gamma);
  launch_crf_prepare(probs, n_frames, n_obj, n_pix, q[0], unary, nullptr, e->s);
  HIPOK(hipGetLastError());
  for (int t = 0; t < iterations; ++t) {
    const bool last = t + 1 == iterations;
    launch_crf_iteration(images, unary, q[t & 1], last && q_out ? q_out : q[(t + 1) & 1], last ? labels_out : nullptr, n_frames,
                         n_lab, height, width, radius, dilation, w_appearance, w_smooth, theta_beta, tab, e->s);
    HIPOK(hipGetLastError());
  }
  return 0;
}

// ---- connected-component clean-up of the merged label maps (after evaluate.py:322-326 and the CRF) --------------------
// argument checks shared by the two entry points; `who` names the entry point in the message
static int ccl_check(const char* who, int n_frames, int height, int width, int connectivity) {
  const std::string w(who);
  if (frames_check(who, n_frames, height, width)) return 1;
  if ((int64_t)height * width >= ((int64_t)1 << 24)) return fail(w + ": frames of 2^24 pixels or more are not supported");
  if (connectivity != 4 && connectivity != 8) return fail(w + ": connectivity must be 4 or 8");
  return 0;
}

int eosvos_label_components(eosvos_engine* e, const uint8_t* labels, int n_frames, int height, int width, int connectivity,
                            int32_t* ids_out) {
  if (!e || !labels || !ids_out) return fail("label_components: null argument");
  if (ccl_check("label_components", n_frames, height, width, connectivity)) return 1;
  if (n_frames == 0) return 0;
  const LabelComponentsLayout L((size_t)n_frames * height * width);
  if (scratch_for(e, "label_components", L, n_frames)) return 1;
  launch_ccl_label(labels, n_frames, height, width, connectivity, scratch_at(e, L.parent), scratch_at(e, L.tarea), ids_out,
                   nullptr, e->s);
  HIPOK(hipGetLastError());
  return 0;
}

int eosvos_filter_components(eosvos_engine* e, const uint8_t* labels, int n_frames, int height, int width, int connectivity,
                             int min_area, int rel_q16, int largest_only, int gate, const uint8_t* prev, const uint8_t* keep,
                             uint8_t* out, int64_t* removed_out) {
  if (!e || !labels || !out) return fail("filter_components: null argument");
  if (ccl_check("filter_components", n_frames, height, width, connectivity)) return 1;
  if (gate < 0 || gate > 63) return fail("filter_components: gate must be in [0, 63] pixels");
  if (min_area < 0) return fail("filter_components: min_area must be >= 0");
  if (rel_q16 < 0 || rel_q16 > 65536) return fail("filter_components: rel_q16 must be in [0, 65536]");
  if (n_frames == 0) return 0;
  const size_t P = (size_t)height * width, np = (size_t)n_frames * P;
  const FilterComponentsLayout L(n_frames, np);
  if (scratch_for(e, "filter_components", L, n_frames)) return 1;
  int *ids = scratch_at(e, L.ids), *area = scratch_at(e, L.area);
  unsigned long long *best = scratch_at(e, L.best), *removed = scratch_at(e, L.removed);
  uint8_t *cand = scratch_at(e, L.cand), *pres = scratch_at(e, L.pres);
  launch_ccl_label(labels, n_frames, height, width, connectivity, scratch_at(e, L.parent), scratch_at(e, L.tarea), ids, area,
                   e->s);
  HIPOK(hipGetLastError());
  const bool chained = gate > 0;          // frame by frame: the gate of a frame reads the filtered frame before it
  if (chained && prev) launch_ccl_presence(prev, (int)P, pres, e->s);
  if (keep_runs(keep, n_frames, false, chained, [&](int f, int frames, int flag) {
        const uint8_t* R = !chained ? nullptr : f == 0 ? prev : out + (size_t)(f - 1) * P;
        const uint8_t* pres_f = R ? pres + (size_t)f * 256 : nullptr;
        if (R && !flag) launch_ccl_gate(labels + f * P, R, pres_f, ids + f * P, height, width, gate, cand + f * P, e->s);
        launch_ccl_filter(labels + f * P, ids + f * P, area + f * P, pres_f, cand + f * P, flag, frames, (int)P, min_area,
                          (unsigned)rel_q16, largest_only != 0, best + (size_t)f * 256, out + f * P, pres + (size_t)(f + 1) * 256,
                          removed + f, e->s);
      }))
    return 1;
  return read_counts(e, L.removed, n_frames, removed_out);
}

// ---- hole filling of the merged label maps (after the component filter) ------------------------------------------------
int eosvos_fill_holes(eosvos_engine* e, const uint8_t* labels, int n_frames, int height, int width, int connectivity,
                      int max_area, int rel_q16, int overlap_q16, const uint8_t* prev, const uint8_t* keep, uint8_t* out,
                      int64_t* filled_out) {
  if (!e || !labels || !out) return fail("fill_holes: null argument");
  if (ccl_check("fill_holes", n_frames, height, width, connectivity)) return 1;
  if (max_area < 0 || max_area > (1 << 24)) return fail("fill_holes: max_area must be in [0, 2^24]");
  if (rel_q16 < 0 || rel_q16 > 65536) return fail("fill_holes: rel_q16 must be in [0, 65536]");
  if (overlap_q16 < 0 || overlap_q16 > 65536) return fail("fill_holes: overlap_q16 must be in [0, 65536]");
  if (n_frames == 0) return 0;
  const size_t P = (size_t)height * width, np = (size_t)n_frames * P;
  const FillHolesLayout L(n_frames, np);
  if (scratch_for(e, "fill_holes", L, n_frames)) return 1;
  int *ids = scratch_at(e, L.ids), *area = scratch_at(e, L.area);
  unsigned *rec = scratch_at(e, L.rec), *cnt = scratch_at(e, L.cnt), *hist = scratch_at(e, L.hist);
  unsigned long long* filled = scratch_at(e, L.filled);
  uint8_t* pres = scratch_at(e, L.pres);
  const bool off = max_area == 0 || rel_q16 == 0;                  // no hole can pass the size rule: every frame is copied
  if (!off) {
    launch_ccl_label_zero(labels, n_frames, height, width, connectivity == 8 ? 4 : 8, scratch_at(e, L.parent),
                          scratch_at(e, L.tarea), ids, area, e->s);
    launch_hole_scan(labels, ids, n_frames, height, width, connectivity, rec, hist, e->s);
    HIPOK(hipGetLastError());
  }
  const bool chained = !off && overlap_q16 > 0;   // frame by frame: the rule of a frame reads the filled frame before it
  if (chained && prev) launch_ccl_presence(prev, (int)P, pres, e->s);
  if (keep_runs(keep, n_frames, off, chained, [&](int f, int frames, int flag) {
        const uint8_t* R = !chained ? nullptr : f == 0 ? prev : out + (size_t)(f - 1) * P;
        const uint8_t* pres_f = R ? pres + (size_t)f * 256 : nullptr;
        if (R && !flag)
          launch_hole_overlap(labels + f * P, R, pres_f, ids + f * P, area + f * P, rec + f * P, hist + (size_t)f * 256, (int)P,
                              max_area, (unsigned)rel_q16, cnt + f * P, e->s);
        launch_hole_apply(labels + f * P, ids + f * P, area + f * P, rec + f * P, hist + (size_t)f * 256, cnt + f * P, pres_f, flag,
                          frames, (int)P, max_area, (unsigned)rel_q16, chained ? (unsigned)overlap_q16 : 0u, out + f * P,
                          pres + (size_t)(f + 1) * 256, filled + f, e->s);
      }))
    return 1;
  return read_counts(e, L.filled, n_frames, filled_out);
}

// ---- SLIC superpixels and the superpixel vote on the merged label maps (between the CRF and the component filter) ----------
// argument checks shared by the two entry points; `who` names the entry point in the message
static int slic_check(const char* who, int n_frames, int height, int width, int step, int iterations, int compactness) {
  const std::string w(who);
  if (frames_check(who, n_frames, height, width)) return 1;
  if (step < 4 || step > 64) return fail(w + ": step must be in [4, 64]");
  if (iterations < 1 || iterations > 20) return fail(w + ": iterations must be in [1, 20]");
  if (compactness < 1 || compactness > 64) return fail(w + ": compactness must be in [1, 64]");
  return 0;
}

// rules 1-4: init, (iterations - 1) x (assign + update), the last assign (with `labels` it also counts the votes)
static void slic_run(const uint8_t* rgb, const uint8_t* labels, int n_frames, int height, int width, int step, int iterations,
                     int compactness, int n_obj, int* centres, unsigned* sums, int* ids, unsigned* votes, hipStream_t s) {
  launch_slic_init(rgb, n_frames, height, width, step, centres, s);
  for (int t = 1; t < iterations; ++t) launch_slic_iterate(rgb, n_frames, height, width, step, compactness, centres, sums, s);
  launch_slic_last(rgb, labels, n_frames, height, width, step, compactness, n_obj, centres, ids, votes, s);
}

int eosvos_superpixels(eosvos_engine* e, const uint8_t* rgb, int n_frames, int height, int width, int step, int iterations,
                       int compactness, int32_t* ids_out) {
  if (!e || !rgb || !ids_out) return fail("superpixels: null argument");
  if (slic_check("superpixels", n_frames, height, width, step, iterations, compactness)) return 1;
  if (n_frames == 0) return 0;
  const SuperpixelsLayout L(n_frames * slic_clusters(height, width, step));
  if (scratch_for(e, "superpixels", L, n_frames)) return 1;
  slic_run(rgb, nullptr, n_frames, height, width, step, iterations, compactness, 0, scratch_at(e, L.centres),
           scratch_at(e, L.sums), ids_out, nullptr, e->s);
  HIPOK(hipGetLastError());
  return 0;
}

int eosvos_snap_labels(eosvos_engine* e, const uint8_t* rgb, const uint8_t* labels, int n_frames, int height, int width, int n_obj,
                       int step, int iterations, int compactness, int min_share_q16, const uint8_t* keep, uint8_t* out,
                       int64_t* changed_out) {
  if (!e || !rgb || !labels || !out) return fail("snap_labels: null argument");
  if (slic_check("snap_labels", n_frames, height, width, step, iterations, compactness)) return 1;
  if (n_obj < 1 || n_obj > 255) return fail("snap_labels: n_obj must be in [1, 255]");
  if (min_share_q16 < 0 || min_share_q16 > 65536) return fail("snap_labels: min_share_q16 must be in [0, 65536]");
  if (n_frames == 0) return 0;
  const size_t P = (size_t)height * width, K = slic_clusters(height, width, step), nl = (size_t)n_obj + 1;
  const SnapLabelsLayout L(n_frames, n_frames * P, n_frames * K, nl);
  if (scratch_for(e, "snap_labels", L, n_frames)) return 1;
  int* ids = scratch_at(e, L.ids);
  unsigned* votes = scratch_at(e, L.votes);
  unsigned long long* changed = scratch_at(e, L.changed);
  slic_run(rgb, labels, n_frames, height, width, step, iterations, compactness, n_obj, scratch_at(e, L.centres),
           scratch_at(e, L.sums), ids, votes, e->s);
  HIPOK(hipGetLastError());
  if (keep_runs(keep, n_frames, false, false, [&](int f, int frames, int flag) {
        launch_slic_apply(labels + f * P, ids + f * P, votes + f * K * nl, flag, frames, height, width, step, n_obj,
                          (unsigned)min_share_q16, out + f * P, changed + f, e->s);
      }))
    return 1;
  return read_counts(e, L.changed, n_frames, changed_out);
}

// ---- block motion on 8-bit luma and the warp of label maps by it (for the temporal rules of the filter and the hole filler) --
int eosvos_block_motion(eosvos_engine* e, const uint8_t* rgb, const uint8_t* prev_rgb, int n_frames, int height, int width, int block,
                        int radius, int bias, int8_t* mv) {
  if (!e || !rgb || !mv) return fail("block_motion: null argument");
  if (frames_check("block_motion", n_frames, height, width, 65534)) return 1;   // one plane more than frames: `prev_rgb`'s
  if (block != 8 && block != 16) return fail("block_motion: block must be 8 or 16");
  if (radius < 1 || radius > 32) return fail("block_motion: radius must be in [1, 32]");
  if (bias < 0 || bias > 255) return fail("block_motion: bias must be in [0, 255]");
  if (n_frames == 0) return 0;
  const BlockMotionLayout L(n_frames, height, width);
  if (scratch_for(e, "block_motion", L, n_frames)) return 1;
  unsigned* luma = scratch_at(e, L.luma);
  const int first = prev_rgb ? 0 : 1;
  const size_t per_frame = (size_t)((height + block - 1) / block) * ((width + block - 1) / block) * 2;
  if (first) HIPOK(hipMemsetAsync(mv, 0, per_frame, e->s));          // no frame before the first: zeros
  launch_motion_luma(rgb, prev_rgb, n_frames, height, width, luma, e->s);
  HIPOK(hipGetLastError());
  launch_motion_search(luma, first, n_frames, height, width, block, radius, bias, mv, e->s);
  HIPOK(hipGetLastError());
  return 0;
}

int eosvos_warp_labels(eosvos_engine* e, const uint8_t* labels, const int8_t* mv, int n_frames, int height, int width, int block,
                       uint8_t* out) {
  if (!e || !labels || !mv || !out) return fail("warp_labels: null argument");
  if (frames_check("warp_labels", n_frames, height, width)) return 1;
  if (block != 8 && block != 16) return fail("warp_labels: block must be 8 or 16");
  if (n_frames == 0) return 0;
  launch_motion_warp(labels, mv, n_frames, height, width, block, out, e->s);
  HIPOK(hipGetLastError());
  return 0;
}

// ---- object-centred zoom pass of the inference path: box, cut, put back, blend (eosvos_amd/zoom.py) -----------------------
static bool finite_f(float v) { return v == v && v - v == 0.f; }
int eosvos_zoom_boxes(eosvos_engine* e, const float* probs, int n_frames, int height, int width, float threshold, int min_pixels,
                      int margin_q16, int margin_px, int min_zoom_q16, int max_zoom_q16, int32_t* boxes) {
  if (!e || !probs || !boxes) return fail("zoom_boxes: null argument");
  if (frames_check("zoom_boxes", n_frames, height, width, 65535, 4096, 1)) return 1;
  if (!finite_f(threshold) || !(threshold > 0.f && threshold < 1.f)) return fail("zoom_boxes: threshold must be in (0, 1)");
  if (min_pixels < 1) return fail("zoom_boxes: min_pixels must be >= 1");
  if (margin_q16 < 0 || margin_q16 > 4 * 65536) return fail("zoom_boxes: margin must be in [0, 4] (Q16)");
  if (margin_px < 0 || margin_px > 256) return fail("zoom_boxes: margin_px must be in [0, 256]");
  if (max_zoom_q16 < 65536 || max_zoom_q16 > 4 * 65536) return fail("zoom_boxes: max_zoom must be in [1, 4] (Q16)");
  if (min_zoom_q16 < 65536 || min_zoom_q16 > max_zoom_q16) return fail("zoom_boxes: min_zoom must be in [1, max_zoom] (Q16)");
  // one record of 8 words per frame; zeroed here, on the stream, whatever the buffer held
  const size_t need = (size_t)n_frames * 8 * sizeof(int);
  if (scratch_grow(e, "zoom_boxes", need, n_frames)) return 1;
  int* rec = (int*)e->scratch;
  HIPOK(hipMemsetAsync(rec, 0, need, e->s));
  launch_zoom_boxes(probs, n_frames, height, width, threshold, min_pixels, margin_q16, margin_px, min_zoom_q16, max_zoom_q16, rec,
                    boxes, e->s);
  HIPOK(hipGetLastError());
  return 0;
}

int eosvos_zoom_crop(eosvos_engine* e, const float* frames, const int32_t* boxes, int B, int C, int height, int width, float* out) {
  if (!e || !frames || !boxes || !out) return fail("zoom_crop: null argument");
  if (B < 1 || C < 1) return fail("zoom_crop: batch out of range");
  if (frames_check("zoom_crop", B, height, width, 0)) return 1;
  if ((int64_t)B * C > 0x7fffffff) return fail("zoom_crop: too many planes");
  launch_zoom_crop(frames, boxes, B, C, height, width, out, e->s);
  HIPOK(hipGetLastError());
  return 0;
}

int eosvos_zoom_accumulate(eosvos_engine* e, const int32_t* boxes, int batch, int mirror, float view_weight, int first, float* pz) {
  if (!e || !boxes || !pz) return fail("zoom_accumulate: null argument");
  if (batch < 1 || batch > e->maxB) return fail("zoom_accumulate: batch out of range");
  if (!finite_f(view_weight)) return fail("zoom_accumulate: the weight must be finite");
  launch_zoom_accumulate(e->logits, boxes, batch, e->H, e->W, mirror != 0, view_weight, first != 0, pz, e->s);
  HIPOK(hipGetLastError());
  return 0;
}

int eosvos_zoom_blend(eosvos_engine* e, const int32_t* boxes, int B, int height, int width, float weight, int feather, const float* pz,
                      float* probs_inout) {
  if (!e || !boxes || !pz || !probs_inout) return fail("zoom_blend: null argument");
  if (B < 1) return fail("zoom_blend: batch out of range");
  if (frames_check("zoom_blend", B, height, width, 0)) return 1;
  if (!finite_f(weight) || !(weight > 0.f && weight <= 1.f)) return fail("zoom_blend: weight must be in (0, 1]");
  if (feather < 0 || feather > 64) return fail("zoom_blend: feather must be in [0, 64]");
  launch_zoom_blend(boxes, B, height, width, weight, feather, pz, probs_inout, e->s);
  HIPOK(hipGetLastError());
  return 0;
}

// ---- lucid first-frame synthesis for the fine-tune: the background plate and the composed samples (eosvos_amd/lucid.py) ----
static int lucid_check(const char* who, int channels, int height, int width) {
  const std::string w(who);
  if (channels < 1 || channels > 64) return fail(w + ": channels must be in [1, 64]");
  return frames_check(who, 1, height, width, 0);
}
int eosvos_lucid_plate(eosvos_engine* e, const float* frame, const float* mask, int channels, int height, int width, int dilate,
                       float* plate) {
  if (!e || !frame || !mask || !plate) return fail("lucid_plate: null argument");
  if (lucid_check("lucid_plate", channels, height, width)) return 1;
  if (dilate < 0 || dilate > 16) return fail("lucid_plate: dilate must be in [0, 16]");
  size_t floats, bytes;
  lucid_scratch(channels, height, width, &floats, &bytes);
  if (scratch_grow(e, "lucid_plate", (floats * sizeof(float) + bytes + 3) / 4 * 4, 1)) return 1;
  float* vbuf = (float*)e->scratch;
  launch_lucid_plate(frame, mask, channels, height, width, dilate, plate, vbuf, (uint8_t*)(vbuf + floats), e->s);
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_lucid_compose(eosvos_engine* e, const float* frame, const float* mask, const float* plate, int channels, int height,
                         int width, int n_samples, const int32_t* flips, const double* matrices, float* images, float* labels,
                         int32_t* counts_host) {
  if (!e || !frame || !mask || !plate || !flips || !matrices || !images || !labels) return fail("lucid_compose: null argument");
  if (lucid_check("lucid_compose", channels, height, width)) return 1;
  if (n_samples < 1 || n_samples > LUCID_MAX_SAMPLES)
    return fail("lucid_compose: between 1 and " + std::to_string(LUCID_MAX_SAMPLES) + " samples per call");
  for (int i = 0; i < n_samples * 12; ++i)
    if (!std::isfinite(matrices[i])) return fail("lucid_compose: the matrices must be finite");
  if (aug_tables(e)) return 1;
  if (scratch_grow(e, "lucid_compose", LUCID_MAX_SAMPLES * sizeof(int), n_samples)) return 1;
  int* counts = (int*)e->scratch;
  HIPOK(hipMemsetAsync(counts, 0, (size_t)n_samples * sizeof(int), e->s));
  launch_lucid_compose(frame, mask, plate, channels, height, width, n_samples, flips, matrices, e->aug_ctab, images, labels, counts,
                       e->s);
  HIPOK(hipGetLastError());
  return read_counts(e, ScratchAt<int>{0}, n_samples, counts_host);            // the batch attempt's one host read
}
int eosvos_lucid_compose_layers(eosvos_engine* e, const float* frame, const uint8_t* ids, const float* plate, int channels,
                                int height, int width, int n_samples, const int32_t* flips, const int32_t* n_layers,
                                const uint8_t* layer_ids, const double* matrices, int target_id, float* images, float* labels,
                                uint8_t* ids_out, int32_t* counts_host) {
  if (!e || !frame || !ids || !plate || !flips || !n_layers || !layer_ids || !matrices || !images || !labels)
    return fail("lucid_compose_layers: null argument");
  if (lucid_check("lucid_compose_layers", channels, height, width)) return 1;
  if (n_samples < 1 || n_samples > LUCID_LAYERS_MAX_SAMPLES)
    return fail("lucid_compose_layers: between 1 and " + std::to_string(LUCID_LAYERS_MAX_SAMPLES) + " samples per call");
  if (target_id < 1 || target_id > 255) return fail("lucid_compose_layers: target_id must be in [1, 255]");
  for (int i = 0; i < n_samples; ++i) {
    const int nl = n_layers[i];
    if (nl < 1 || nl > LUCID_MAX_LAYERS)
      return fail("lucid_compose_layers: between 1 and " + std::to_string(LUCID_MAX_LAYERS) + " layers per sample");
    const uint8_t* id = layer_ids + (size_t)i * LUCID_MAX_LAYERS;
    for (int k = 0; k < nl; ++k) {
      if (id[k] == 0) return fail("lucid_compose_layers: a layer id must be in [1, 255]");
      for (int j = 0; j < k; ++j)
        if (id[j] == id[k]) return fail("lucid_compose_layers: the layer ids of a sample must be distinct");
    }
    const double* m = matrices + (size_t)i * (1 + LUCID_MAX_LAYERS) * 6;       // Bi and the nl layer matrices are read
    for (int j = 0; j < (1 + nl) * 6; ++j)
      if (!std::isfinite(m[j])) return fail("lucid_compose_layers: the matrices must be finite");
  }
  if (aug_tables(e)) return 1;
  const LucidLayersLayout L(n_samples);
  if (scratch_for(e, "lucid_compose_layers", L, n_samples)) return 1;
  launch_lucid_layers(frame, ids, plate, channels, height, width, n_samples, flips, n_layers, layer_ids, matrices, target_id,
                      e->aug_ctab, images, labels, ids_out, scratch_at(e, L.counts), e->s);
  HIPOK(hipGetLastError());
  return read_counts(e, L.counts, (size_t)n_samples * LUCID_MAX_LAYERS, counts_host);   // the batch attempt's one host read
}

// ---- online adaptation: the capped distance transform and the distance-gated targets (OnAVOS; evaluate.py:231-240) ------
static int edt_check(const char* who, int n_frames, int height, int width) {
  const std::string w(who);
  if (n_frames < 1 || n_frames > 65535) return fail(w + ": between 1 and 65535 frames per call");
  if (frames_check(who, n_frames, height, width)) return fail(w + ": frames of 1 .. 4096 pixels a side");   // this stage's wording
  return 0;
}
int eosvos_distance_sq(eosvos_engine* e, const float* probs, int n_frames, int height, int width, float threshold, int invert,
                       int limit, int32_t* out) {
  if (!e || !probs || !out) return fail("distance_sq: null argument");
  if (edt_check("distance_sq", n_frames, height, width)) return 1;
  if (limit < 1 || limit > 4095) return fail("distance_sq: limit must be in [1, 4095]");
  if (std::isnan(threshold)) return fail("distance_sq: the threshold is NaN");
  const DistanceSqLayout L((size_t)n_frames * height * width);
  if (scratch_for(e, "distance_sq", L, n_frames)) return 1;
  launch_edt_distance(probs, n_frames, height, width, threshold, invert != 0, limit, scratch_at(e, L.g), out, e->s);
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_adapt_targets(eosvos_engine* e, const float* probs, const float* anchors, int n_frames, int height, int width, float lo,
                         float hi, float anchor_thr, int erode, int neg_dist, float ignore, float* targets, int64_t* n_pos) {
  if (!e || !probs || !anchors || !targets) return fail("adapt_targets: null argument");
  if (edt_check("adapt_targets", n_frames, height, width)) return 1;
  if (neg_dist < 1 || neg_dist > 4095) return fail("adapt_targets: neg_dist must be in [1, 4095]");
  if (erode < 0 || erode > 255) return fail("adapt_targets: erode must be in [0, 255]");
  if (!(lo >= 0.f && lo < hi && hi <= 1.f)) return fail("adapt_targets: needs 0 <= lo < hi <= 1");
  if (std::isnan(anchor_thr)) return fail("adapt_targets: the anchor threshold is NaN");
  if (ignore_check(&ignore)) return 1;
  const AdaptTargetsLayout L(n_frames, (size_t)n_frames * height * width, erode > 0);
  if (scratch_for(e, "adapt_targets", L, n_frames)) return 1;
  launch_edt_targets(probs, anchors, n_frames, height, width, lo, hi, anchor_thr, erode, neg_dist, ignore, scratch_at(e, L.g),
                     scratch_at(e, L.eroded), scratch_at(e, L.count_e), scratch_at(e, L.n_pos), targets, e->s);
  HIPOK(hipGetLastError());
  return read_counts(e, L.n_pos, n_frames, n_pos);             // the round's one host read (32-bit counters on the device)
}

// ---- the surface loss on caller tensors of any frame shape, and its distance / weight maps -------------------------------
static int surface_check(const char* who, int images, int height, int width, int cap, const float* ignore) {
  const std::string w(who);
  if (images < 1 || images > 65535) return fail(w + ": between 1 and 65535 images per call");
  if (height < 1 || height > 4096 || width < 1 || width > 4096) return fail(w + ": frames of 1 .. 4096 pixels a side");
  if (cap < 0 || cap > 4095) return fail(w + ": the cap must be 1 .. 4095, or 0 for the frame-size default");
  return ignore_check(ignore);
}
int eosvos_set_loss_surface(eosvos_engine* e, int cap) {
  if (!e) return fail("null engine");
  if (cap < 0 || cap > 4095) return fail("the surface cap must be 1 .. 4095, or 0 for the frame-size default");
  e->surface_cap = cap;
  return 0;
}
int eosvos_surface_loss(eosvos_engine* e, const float* logits, const float* masks, int images, int height, int width, int cap,
                        const float* ignore, float* loss_out, float* dlogits_out) {
  if (!e || !logits || !masks || !loss_out) return fail("surface_loss: null argument");
  if (surface_check("surface_loss", images, height, width, cap, ignore)) return 1;
  const SurfaceLayout L(images, (size_t)images * height * width, 2 * SURFACE_BLOCKS + 1);
  if (scratch_for(e, "surface_loss", L, images)) return 1;
  const int l = cap ? cap : surface_default_cap(height, width);
  launch_surface_distance(masks, images, height, width, l, ignore, scratch_at(e, L.g), (int32_t*)scratch_at(e, L.g), e->s);
  launch_surface_loss(logits, masks, (const int32_t*)scratch_at(e, L.g), dlogits_out, loss_out, scratch_at(e, L.partial), height, width,
                      images, l, ignore, e->s);
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_surface_weights(eosvos_engine* e, const float* masks, int images, int height, int width, int cap, const float* ignore,
                           int32_t* c_out, float* w_out) {
  if (!e || !masks || (!c_out && !w_out)) return fail("surface_weights: null argument");
  if (surface_check("surface_weights", images, height, width, cap, ignore)) return 1;
  const size_t np = (size_t)images * height * width;
  const SurfaceLayout L(images, np, 0);
  if (scratch_for(e, "surface_weights", L, images)) return 1;
  const int l = cap ? cap : surface_default_cap(height, width);
  int32_t* const c = c_out ? c_out : (int32_t*)scratch_at(e, L.g);
  launch_surface_distance(masks, images, height, width, l, ignore, scratch_at(e, L.g), c, e->s);
  if (w_out) launch_surface_weights(c, w_out, (int64_t)np, l, e->s);
  HIPOK(hipGetLastError());
  return 0;
}

// ---- the centreline loss: its depth on the engine, the loss and the soft skeleton on caller tensors of any frame shape -------
static int cldice_check(const char* who, int images, int height, int width, int depth, const float* ignore) {
  const std::string w(who);
  if (images < 1 || images > 65535) return fail(w + ": between 1 and 65535 images per call");
  if (height < 1 || height > 4096 || width < 1 || width > 4096) return fail(w + ": frames of 1 .. 4096 pixels a side");
  if (depth < 0 || depth > CLDICE_MAX_DEPTH) return fail(w + ": the depth must be 1 .. 16, or 0 for the frame-size default");
  return ignore_check(ignore);
}
int eosvos_set_loss_cldice(eosvos_engine* e, int depth) {
  if (!e) return fail("null engine");
  if (depth < 0 || depth > CLDICE_MAX_DEPTH) return fail("the cldice depth must be 1 .. 16, or 0 for the frame-size default");
  e->cldice_depth = depth;
  return 0;
}
int eosvos_cldice_loss(eosvos_engine* e, const float* logits, const float* masks, int images, int height, int width, int depth,
                       const float* ignore, float* loss_out, float* dlogits_out) {
  if (!e || !logits || !masks || !loss_out) return fail("cldice_loss: null argument");
  if (cldice_check("cldice_loss", images, height, width, depth, ignore)) return 1;
  const int k = depth ? depth : cldice_default_depth(height, width);
  const CldiceLayout L((size_t)cldice_scratch_floats((int64_t)images * height * width, images, k));
  if (scratch_for(e, "cldice_loss", L, images)) return 1;
  launch_cldice(logits, masks, dlogits_out, loss_out, (float*)scratch_at(e, L.words), height, width, images, k, ignore, e->s);
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_soft_skeleton(eosvos_engine* e, const float* maps, const float* masks, int images, int height, int width, int depth,
                         const float* ignore, float* out) {
  if (!e || !maps || !out) return fail("soft_skeleton: null argument");
  if (cldice_check("soft_skeleton", images, height, width, depth, ignore)) return 1;
  const int k = depth ? depth : cldice_default_depth(height, width);
  const CldiceLayout L((size_t)cldice_skeleton_scratch_floats((int64_t)images * height * width));
  if (scratch_for(e, "soft_skeleton", L, images)) return 1;
  launch_cldice_skeleton(maps, masks, out, (float*)scratch_at(e, L.words), height, width, images, k, ignore, e->s);
  HIPOK(hipGetLastError());
  return 0;
}

// ---- the pairwise (Potts) loss: its parameters on the engine, and the loss on caller tensors with their frames --------------
int eosvos_set_loss_potts(eosvos_engine* e, int window, int dilation, float sigma_xy, float sigma_rgb) {
  if (!e) return fail("null engine");
  if (potts_params("set_loss_potts", window, dilation, sigma_xy, sigma_rgb, nullptr)) return 1;
  e->potts_window = window;
  e->potts_dilation = dilation;
  e->potts_sigma_xy = sigma_xy;
  e->potts_sigma_rgb = sigma_rgb;
  return 0;
}
int eosvos_potts_loss(eosvos_engine* e, const float* logits, const float* frames, int images, int height, int width, int window,
                      int dilation, float sigma_xy, float sigma_rgb, float* loss_out, float* dlogits_out) {
  if (!e || !logits || !frames || !loss_out) return fail("potts_loss: null argument");
  if (images < 1 || images > 65535) return fail("potts_loss: between 1 and 65535 images per call");
  if (height < 1 || height > 4096 || width < 1 || width > 4096) return fail("potts_loss: frames of 1 .. 4096 pixels a side");
  PottsParams q;
  if (potts_params("potts_loss", window, dilation, sigma_xy, sigma_rgb, &q)) return 1;
  if (potts_eval(e, "potts_loss", q, logits, frames, 0, height, width, images, dlogits_out, loss_out)) return 1;
  HIPOK(hipGetLastError());
  return 0;
}

int eosvos_meta_task_begin(eosvos_engine* e) {
  ModeScope mode_scope(e);
  if (!e) return fail("null engine");
  if (!e->gsum) {
    e->gsum = e->falloc(e->t.nparam);
    if (!e->gsum) return fail("hipMalloc gsum");
  }
  HIPOK(hipMemsetAsync(e->gsum + e->tf_poff, 0, (size_t)(e->t.nparam - e->tf_poff) * 4, e->s));   // (frozen part: never written)
  return eosvos_reset(e);
}
int eosvos_meta_grad(eosvos_engine* e, const float* images, const float* masks, int batch, float* flat_meta_grad,
                     float* meta_loss_host) {
  ModeScope mode_scope(e);
  return eosvos_meta_grad_ex(e, images, masks, batch, flat_meta_grad, meta_loss_host, 1.f, EOSVOS_META_INIT_GRAD);
}
int eosvos_meta_grad_ex(eosvos_engine* e, const float* images, const float* masks, int batch, float* flat_meta_grad,
                        float* meta_loss_host, float weight, int flags) {
  ModeScope mode_scope(e);
  if (!e || !images || !masks || !flat_meta_grad) return fail("null argument");
  if (!e->gsum) return fail("eosvos_meta_grad without eosvos_meta_task_begin");
  if (eosvos_forward(e, images, batch, nullptr)) return 1;
  if (fused_loss(e, masks, batch)) return 1;
  const bool keep = e->keep_grads;
  e->keep_grads = true;
  const int rc = backward_impl(e, false, false);
  e->keep_grads = keep;
  if (rc) return 1;
  const Topo& t = e->t;
  const int64_t nstore = lr_store_count(t, e->lr_level);
  // trainable boundary: only the trainable convs' rows / elements are made (the frozen ones of the caller's buffer are left as
  // they are: zero for a zeroed buffer); gsum / gout hold nothing for the frozen convs
  const int64_t p0 = e->tf_poff, r0 = e->tf_lroff;
  if (e->lr_level == EOSVOS_LR_PARAM) {
    launch_meta_lr_grad_elem(e->gsum + p0, e->gout + p0, e->lr_log ? e->lr_elem + p0 : nullptr, e->ptmp + p0, t.nparam - p0, e->s);
    export_params(e, e->ptmp, flat_meta_grad, weight, 1, true);
  } else {
    // per-neuron d/d lr first (into the caller's buffer directly when that is the stored level)
    const bool direct = e->lr_level == EOSVOS_LR_NEURON && !e->lr_log;
    float* gl = direct ? flat_meta_grad : e->glr_tmp;
    if (!direct) {
      if (ensure_lr_maps(e)) return 1;
      HIPOK(hipMemsetAsync(e->glr_tmp, 0, (size_t)t.nlr * 4, e->s));
    }
    if (!ensure_meta_tabs(e)) {                       // every tensor's rows in one launch (64 before)
      launch_meta_lr_grad_all(e->gsum, e->gout, gl + r0, e->mt_rbase + r0, e->mt_rlen + r0, (int)(t.nlr - r0), weight, e->s);
    } else {
      for (const ConvL& c : t.convs) {
        if (c.poff < p0) continue;
        launch_meta_lr_grad(e->gsum + c.poff, e->gout + c.poff, gl + c.lroff, c.cout, (int64_t)c.T() * c.cin, weight, e->s);
        if (c.bias)
          launch_meta_lr_grad(e->gsum + c.poff + c.wsize(), e->gout + c.poff + c.wsize(), gl + c.lroff + c.cout,
                              c.cout, 1, weight, e->s);
      }
    }
    if (e->lr_level == EOSVOS_LR_NEURON) {
      if (!direct) launch_lr_grad_neuron(gl + r0, e->lr + r0, flat_meta_grad + r0, (int)(t.nlr - r0), e->lr_log, e->s);
    } else if (e->lr_level == EOSVOS_LR_TENSOR) {
      launch_lr_grad_reduce(gl, e->lr, e->tensor_row0, flat_meta_grad, e->ntensors, e->lr_log, e->s);
    } else {
      launch_lr_grad_reduce(gl, e->lr, e->all_row0, flat_meta_grad, 1, e->lr_log, e->s);
    }
  }
  if (flags & EOSVOS_META_INIT_GRAD) export_params(e, e->gout, flat_meta_grad + nstore, weight, 1, true);
  // truncated BPTT: the next segment starts from detached parameters (meta_optim.reset(keep_state=True))
  if (flags & EOSVOS_META_NEW_SEGMENT) HIPOK(hipMemsetAsync(e->gsum + p0, 0, (size_t)(t.nparam - p0) * 4, e->s));
  HIPOK(hipGetLastError());
  if (meta_loss_host) {
    HIPOK(hipMemcpyAsync(meta_loss_host, e->loss_dev, 4, hipMemcpyDeviceToHost, e->s));
    HIPOK(hipStreamSynchronize(e->s));
  }
  return 0;
}

int eosvos_radam_step(eosvos_engine* e, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                      int64_t n, float lr, float weight_decay, float beta1, float beta2, float eps, int step,
                      float grad_scale, float grad_clip) {
  ModeScope mode_scope(e);
  if (!e || !param || !grad || !exp_avg || !exp_avg_sq || step < 1) return fail("bad argument");
  // radam.py:62-79 in double, as the reference's Python floats
  const double b1 = beta1, b2 = beta2;
  const double beta2_t = pow(b2, (double)step);
  const double n_sma_max = 2.0 / (1.0 - b2) - 1.0;
  const double n_sma = n_sma_max - 2.0 * step * beta2_t / (1.0 - beta2_t);
  double step_size;
  int use_denom = 0;
  if (n_sma >= 5.0) {
    step_size = sqrt((1.0 - beta2_t) * (n_sma - 4.0) / (n_sma_max - 4.0) * (n_sma - 2.0) / n_sma * n_sma_max /
                     (n_sma_max - 2.0)) / (1.0 - pow(b1, (double)step));
    use_denom = 1;
  } else {
    step_size = 1.0 / (1.0 - pow(b1, (double)step));
  }
  launch_radam(param, grad, exp_avg, exp_avg_sq, n, lr, weight_decay, beta1, beta2, eps, (float)step_size,
               use_denom, grad_scale, grad_clip, e->s);
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_outer_step(eosvos_engine* e, float* state, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n_lr,
                      int learn_model_init, int step, float lr_lr, float init_lr, float weight_decay, float beta1, float beta2,
                      float eps, float grad_scale, float grad_clip, float lr_lo, float lr_hi, int use_log,
                      int64_t frozen_lr, int64_t frozen_param) {
  ModeScope mode_scope(e);
  if (!e || !state || !grad || !exp_avg || !exp_avg_sq || step < 1) return fail("bad argument");
  const Topo& t = e->t;
  if (n_lr != t.nlr) return fail("eosvos_outer_step handles the NEURON lr hierarchy level only (n_lr must be eosvos_lr_count)");
  if (e->train_from > 0)
    return fail("eosvos_outer_step: not with a trainable boundary (the learned state is the trainable subset: eosvos_radam_step)");
  if (!e->outer_tab) {
    std::vector<OuterEnt> tab;
    int blk = 0;
    for (const ConvL& c : t.convs) {
      OuterEnt o;
      o.off = c.poff; o.O = c.cout; o.I = c.cin; o.T = c.T();
      o.n = (int)(c.wsize() + (c.bias ? c.cout : 0)); o.blk0 = blk;
      blk += (o.n + 1023) / 1024;
      tab.push_back(o);
    }
    if (tab.size() > 256) return fail("eosvos_outer_step: more than 256 trainable tensors");
    e->outer_tab = (OuterEnt*)e->falloc((int64_t)(tab.size() * sizeof(OuterEnt) + 3) / 4);
    if (!e->outer_tab) return fail("hipMalloc outer-step table");
    HIPOK(hipMemcpy(e->outer_tab, tab.data(), tab.size() * sizeof(OuterEnt), hipMemcpyHostToDevice));
    e->outer_blocks = blk;
  }
  // radam.py:62-79 in double, as the reference's Python floats (same as eosvos_radam_step)
  const double b1 = beta1, b2 = beta2;
  const double beta2_t = pow(b2, (double)step);
  const double n_sma_max = 2.0 / (1.0 - b2) - 1.0;
  const double n_sma = n_sma_max - 2.0 * step * beta2_t / (1.0 - beta2_t);
  OuterHyper h;
  memset(&h, 0, sizeof(h));
  if (n_sma >= 5.0) {
    h.step_size = (float)(sqrt((1.0 - beta2_t) * (n_sma - 4.0) / (n_sma_max - 4.0) * (n_sma - 2.0) / n_sma * n_sma_max /
                               (n_sma_max - 2.0)) / (1.0 - pow(b1, (double)step)));
    h.use_denom = 1;
  } else {
    h.step_size = (float)(1.0 / (1.0 - pow(b1, (double)step)));
  }
  h.n_lr = n_lr; h.frozen_lr = frozen_lr; h.frozen_param = frozen_param;
  h.lr_lr = lr_lr; h.init_lr = init_lr; h.wd = weight_decay; h.beta1 = beta1; h.beta2 = beta2; h.eps = eps;
  h.grad_scale = grad_scale; h.grad_clip = grad_clip; h.lr_lo = lr_lo; h.lr_hi = lr_hi; h.use_log = use_log ? 1 : 0;
  const int lr_blocks = (int)((n_lr + 1023) / 1024);
  if (learn_model_init) wino_weights_changed(e);
  launch_outer_step(e->outer_tab, (int)t.convs.size(), lr_blocks, lr_blocks + (learn_model_init ? e->outer_blocks : 0), state, grad,
                    exp_avg, exp_avg_sq, e->Winit, e->Wp, e->lr, h, e->s);
  e->lr_level = EOSVOS_LR_NEURON; e->lr_log = use_log ? 1 : 0;
  for (eosvos_engine* a : e->aliased_by) { a->lr_level = e->lr_level; a->lr_log = e->lr_log; }      // they read the state just written
  HIPOK(hipGetLastError());
  return 0;
}
// give `e` its own learned init / lr buffers back, holding what it has been reading (its source's current values)
static int unalias_impl(eosvos_engine* e) {
  eosvos_engine* src = e->alias_src;
  if (!src) return 0;
  (void)hipStreamSynchronize(src->s);
  (void)hipStreamSynchronize(e->s);
  // The alias is detached whether or not the copies succeed (a device in an error state must not leave the engine pointing into
  // memory its source is about to free, nor make eosvos_destroy of the source loop over an alias that never leaves its list);
  // a failed copy is reported, the engine's own buffers then hold whatever they held before.
  const bool copied = hipMemcpy(e->own_Winit, src->Winit, (size_t)e->t.nparam * 4, hipMemcpyDeviceToDevice) == hipSuccess &&
                      hipMemcpy(e->own_lr, src->lr, (size_t)e->t.nlr * 4, hipMemcpyDeviceToDevice) == hipSuccess;
  e->Winit = e->own_Winit; e->lr = e->own_lr;
  e->lr_level = src->lr_level; e->lr_log = src->lr_log;
  src->aliased_by.erase(std::remove(src->aliased_by.begin(), src->aliased_by.end(), e), src->aliased_by.end());
  e->alias_src = nullptr;
  if (!copied) return fail("eosvos_unalias_state: copy of the learned state failed (the alias was detached; the engine's own copy is stale)");
  return 0;
}
int eosvos_alias_state(eosvos_engine* e, eosvos_engine* src) {
  ModeScope mode_scope(e);
  if (!e || !src) return fail("null engine");
  if (e == src) return 0;
  if (e->dev != src->dev || e->arch != src->arch) return fail("eosvos_alias_state: engines of different devices / architectures");
  if (e->train_from != src->train_from) return fail("eosvos_alias_state: engines with different trainable boundaries");
  if (src->alias_src) return fail("eosvos_alias_state: the source engine is itself an alias (alias its source instead)");
  if (!e->aliased_by.empty()) return fail("eosvos_alias_state: other engines read this engine's state");
  if (e->alias_src == src) return 0;
  if (e->alias_src && unalias_impl(e)) return 1;
  HIPOK(hipStreamSynchronize(e->s));
  e->own_Winit = e->Winit; e->own_lr = e->lr;
  e->Winit = src->Winit;              // (e's own buffers stay in its allocation list: eosvos_unalias_state / the source's destroy)
  e->lr = src->lr;
  e->lr_level = src->lr_level; e->lr_log = src->lr_log;
  e->alias_src = src;
  src->aliased_by.push_back(e);
  return 0;
}
int eosvos_unalias_state(eosvos_engine* e) {
  ModeScope mode_scope(e);
  if (!e) return fail("null engine");
  return unalias_impl(e);
}

int eosvos_set_trainable_from(eosvos_engine* e, int conv_idx) {
  if (!e) return fail("null engine");
  const Topo& t = e->t;
  const int l4 = t.blocks[t.blocks.size() - 3].c1;
  if (conv_idx != 0 && conv_idx != l4 && conv_idx != t.aspp[0])
    return fail("eosvos_set_trainable_from: the boundary must be 0, the first conv of layer4 or the first ASPP conv");
  if (conv_idx == e->train_from) return 0;
  if (e->alias_src || !e->aliased_by.empty())
    return fail("eosvos_set_trainable_from: not on an engine that shares its learned state (eosvos_alias_state)");
  int tens = 0;
  for (int ci = 0; ci < conv_idx; ++ci) tens += t.convs[ci].bias ? 2 : 1;
  const ConvL& c0 = t.convs[conv_idx];
  if (conv_idx > 0) {                       // export table of the trainable tensors (offsets relative to the first of them)
    std::vector<long> toff;
    for (size_t ci = conv_idx; ci < t.convs.size(); ++ci) {
      const ConvL& c = t.convs[ci];
      toff.push_back((long)(c.poff - c0.poff));
      if (c.bias) toff.push_back((long)(c.poff + c.wsize() - c0.poff));
    }
    long* d = (long*)e->falloc((int64_t)toff.size() * 2);
    if (!d) return fail("hipMalloc trainable export table");
    HIPOK(hipMemcpy(d, toff.data(), toff.size() * sizeof(long), hipMemcpyHostToDevice));
    e->tf_toff = d;
  }
  HIPOK(hipStreamSynchronize(e->s));        // launches queued under the old boundary finish before the tables change
  e->train_from = conv_idx;
  e->tf_poff = conv_idx > 0 ? c0.poff : 0;
  e->tf_lroff = conv_idx > 0 ? c0.lroff : 0;
  e->tf_tensor = conv_idx > 0 ? tens : 0;
  for (auto& tab : e->upd_tab) tab = nullptr;       // the update's part 0 covers another conv range
  if (e->gsum) HIPOK(hipMemsetAsync(e->gsum, 0, (size_t)t.nparam * 4, e->s));
  // ReLU masks that only a frozen conv's data gradient reads: the activations of the frozen blocks
  for (size_t i = 0; i < t.blocks.size(); ++i) {
    const bool frozen = t.blocks[i].c1 < conv_idx;
    e->bb[i].t1->mask_frozen = e->bb[i].t2->mask_frozen = e->bb[i].out->mask_frozen = frozen;
  }
  e->masks_valid = false;                   // a backward pass needs a forward made under this boundary
  return 0;
}

// ---- RCCL: the one exchange of the meta-training path ------------------------------------------------------------------
// The library has no link-time dependency on RCCL (it loads on a box without it): the first collective call binds the
// RCCL already in the process (a torch host has loaded its own) or else loads librccl.so.1 / EOSVOS_RCCL_LIB.
namespace {
struct Rccl {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, eosvos_rccl_id, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok() const { return GetUniqueId && CommInitRank && CommDestroy && AllReduce; }
};
Rccl g_rccl;
int rccl_load() {
  if (g_rccl.ok()) return 0;
  const char* env = getenv("EOSVOS_RCCL_LIB");
  void* h = nullptr;
  if (env && env[0]) h = dlopen(env, RTLD_NOW | RTLD_GLOBAL);
  const char* names[] = {"librccl.so", "librccl.so.1"};
  for (int pass = 0; pass < 2 && !h; ++pass)          // pass 0: an instance the process already has (RTLD_NOLOAD), pass 1: load one
    for (const char* n : names) {
      h = dlopen(n, pass == 0 ? (RTLD_NOW | RTLD_NOLOAD) : (RTLD_NOW | RTLD_GLOBAL));
      if (h) break;
    }
  if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!h) return fail(std::string("RCCL not found (librccl.so / librccl.so.1 / EOSVOS_RCCL_LIB): ") + (dlerror() ? dlerror() : ""));
  g_rccl.lib = h;
  g_rccl.GetUniqueId = (int (*)(void*))dlsym(h, "ncclGetUniqueId");
  g_rccl.CommInitRank = (int (*)(void**, int, eosvos_rccl_id, int))dlsym(h, "ncclCommInitRank");
  g_rccl.CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
  g_rccl.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclAllReduce");
  g_rccl.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
  if (!g_rccl.ok()) return fail("RCCL library lacks ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllReduce");
  return 0;
}
int rccl_fail(const char* what, int rc) {
  return fail(std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error") + " (" + std::to_string(rc) + ")");
}
}  // namespace
int eosvos_comm_unique_id(eosvos_rccl_id* id) {
  if (!id) return fail("null argument");
  if (rccl_load()) return 1;
  const int rc = g_rccl.GetUniqueId(id);
  return rc ? rccl_fail("ncclGetUniqueId", rc) : 0;
}
int eosvos_comm_init_rank(void** comm, int world_size, const eosvos_rccl_id* id, int rank, int device_id) {
  if (!comm || !id || world_size < 1 || rank < 0 || rank >= world_size) return fail("bad argument");
  if (rccl_load()) return 1;
  HIPOK(hipSetDevice(device_id));
  const int rc = g_rccl.CommInitRank(comm, world_size, *id, rank);
  return rc ? rccl_fail("ncclCommInitRank", rc) : 0;
}
int eosvos_comm_destroy(void* comm) {
  if (!comm) return 0;
  if (rccl_load()) return 1;
  const int rc = g_rccl.CommDestroy(comm);
  return rc ? rccl_fail("ncclCommDestroy", rc) : 0;
}
int eosvos_allreduce_sum(eosvos_engine* e, float* flat, int64_t n, void* comm) {
  if (!e || !flat || !comm || n < 1) return fail("bad argument");
  if (rccl_load()) return 1;
  const int rc = g_rccl.AllReduce(flat, flat, (size_t)n, 7 /* ncclFloat32 */, 0 /* ncclSum */, comm, e->s);
  return rc ? rccl_fail("ncclAllReduce", rc) : 0;
}
int eosvos_clamp(eosvos_engine* e, float* param, int64_t n, float lo, float hi) {
  ModeScope mode_scope(e);
  if (!e || !param) return fail("null argument");
  launch_clamp(param, n, lo, hi, e->s);
  HIPOK(hipGetLastError());
  return 0;
}

int eosvos_profile_launches(eosvos_engine* e, int on) {
  if (!e) return fail("null engine");
  HIPOK(hipStreamSynchronize(e->s));
  if (e->s2) HIPOK(hipStreamSynchronize(e->s2));
  conv_prof_enable(on);
  return 0;
}
int eosvos_profile_read(eosvos_engine* e, int max_kernels, char* names, int64_t* counts, double* ms, double* flops,
                        int* n_out) {
  if (!e || !names || !counts || !ms || !flops || !n_out || max_kernels < 1) return fail("bad argument");
  HIPOK(hipStreamSynchronize(e->s));
  if (e->s2) HIPOK(hipStreamSynchronize(e->s2));
  std::vector<const char*> nm(max_kernels);
  std::vector<long> c(max_kernels);
  const int n = conv_prof_read(max_kernels, nm.data(), c.data(), ms, flops);
  for (int i = 0; i < n; ++i) {
    strncpy(names + 64 * i, nm[i], 63);
    names[64 * i + 63] = 0;
    counts[i] = c[i];
  }
  *n_out = n;
  return 0;
}

int eosvos_test_conv_plan_log(eosvos_engine* e, int on) {
  if (!e) return fail("null engine");
  conv_plan_log_enable(on);
  return 0;
}
int eosvos_test_conv_plan_log_read(eosvos_engine* e, int max_records, char* names, int* fields, int* n_out) {
  if (!e || !names || !fields || !n_out || max_records < 1) return fail("bad argument");
  static_assert(kConvPlanLogFields == EOSVOS_PLAN_LOG_FIELDS, "include/eosvos.h lists the fields of ConvPlanRec");
  std::vector<ConvPlanRec> recs(max_records);
  std::vector<const char*> nm(max_records);
  const int seen = conv_plan_log_read(recs.data(), nm.data(), max_records);
  const int n = std::min(seen, std::min(max_records, kConvPlanLogCap));
  for (int i = 0; i < n; ++i) {
    strncpy(names + 64 * i, nm[i], 63);
    names[64 * i + 63] = 0;
    memcpy(fields + (size_t)i * kConvPlanLogFields, &recs[i], sizeof(ConvPlanRec));
  }
  *n_out = seen;
  return 0;
}

int eosvos_time_hot_kernel(eosvos_engine* e, int batch, int reps, float* ms_host, double* flops_host) {
  ModeScope mode_scope(e);
  if (!e || !ms_host || !flops_host || batch < 1 || batch > e->maxB || reps < 1) return fail("bad argument");
  const Topo& t = e->t;
  if (t.dec_a < 0) return fail("eosvos_time_hot_kernel times the DeepLabV3+ decoder conv; this topology has none");
  hipEvent_t a, b;
  HIPOK(hipEventCreate(&a));
  HIPOK(hipEventCreate(&b));
  conv_fwd(e, t.dec_a, e->dcat, e->d1, batch, Opt().relu());   // warm (and fills V / U)
  const ConvL& c = t.convs[t.dec_a];
  if (wino_on(e, t.dec_a, batch, e->h4, e->w4)) {
    // the step runs this layer in the Winograd domain: time its batched GEMM launch (+ fix-up), the largest
    // conv_igemm launch of an iteration, against the GEMM's own FLOPs
    const WinoGeom wg = wino_geom(e, c, batch, e->h4, e->w4);
    const long ntile = wg.ntile;
    ConvArgs m = wino_plane_gemm(e, c, wg, e->wino[t.dec_a].V, e->wino[t.dec_a].U, e->wino_m, e->ws_conv, 0);
    HIPOK(hipEventRecord(a, e->s));
    for (int i = 0; i < reps; ++i) { ConvArgs k = m; launch_conv(k, e->s); }
    HIPOK(hipEventRecord(b, e->s));
    *flops_host = 2.0 * wg.np * (double)ntile * c.cout * c.cin;
  } else {
    HIPOK(hipEventRecord(a, e->s));
    for (int i = 0; i < reps; ++i) conv_fwd(e, t.dec_a, e->dcat, e->d1, batch, Opt().relu());
    HIPOK(hipEventRecord(b, e->s));
    *flops_host = 2.0 * (double)batch * e->h4 * e->w4 * (double)c.cout * c.cin * 9.0;
  }
  HIPOK(hipEventSynchronize(b));
  float ms = 0.f;
  HIPOK(hipEventElapsedTime(&ms, a, b));
  *ms_host = ms / reps;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return 0;
}

// Time one layer's forward (kind 0), data-gradient (1) or weight-gradient (2) launch in place,
// on the engine's own buffers (tuning aid; outputs are overwritten with whatever the buffers hold).
int eosvos_bench_conv(eosvos_engine* e, int ci, int kind, int batch, int reps, float* ms_host, double* flops_host) {
  ModeScope mode_scope(e);
  if (!e || !ms_host || !flops_host || batch < 1 || batch > e->maxB || reps < 1) return fail("bad argument");
  const Topo& t = e->t;
  if (ci < 1 || ci >= (int)t.convs.size()) return fail("conv index out of range");
  const ConvL& c = t.convs[ci];
  Tensor *x = nullptr, *gx = nullptr;      // the conv's input and its gradient
  View y, g;                               // its output and the gradient w.r.t. it
  for (size_t i = 0; i < t.blocks.size() && !x; ++i) {
    const Block& b = t.blocks[i];
    auto& f = e->bb[i];
    if (ci == b.c1) { x = f.xin; gx = f.g_xin; y = f.t1; g = f.g_t1; }
    else if (ci == b.c2) { x = f.t1; gx = f.g_t1; y = f.t2; g = f.g_t2; }
    else if (ci == b.c3) { x = f.t2; gx = f.g_t2; y = f.out; g = f.g_out; }
    else if (ci == b.ds) { x = f.xin; gx = f.g_xin; y = f.dsb; g = f.g_out; }
  }
  if (!x) {
    if (ci == t.dec_a) { x = e->dcat; gx = e->g_dcat; y = e->d1; g = e->g_d1; }
    else if (ci == t.dec_b) { x = e->d1; gx = e->g_d1; y = e->d2; g = e->g_d2; }
    else if (ci == t.project) { x = e->cat; gx = e->g_cat; y = e->proj; g = e->g_proj; }
    else {
      for (int i = 0; i < 4; ++i)
        if (ci == t.aspp[i]) { x = e->bb.back().out; gx = e->bb.back().g_out; y = View(e->cat, 256 * i, 256); g = View(e->g_cat, 256 * i, 256); }
    }
  }
  if (!x) return fail("conv not benchable");
  const int Ho = conv_out(x->H, c.k, c.stride, c.dil, c.pad), Wo = conv_out(x->W, c.k, c.stride, c.dil, c.pad);
  auto run = [&]() {
    if (kind == 0) conv_fwd(e, ci, x, y, batch, Opt().relu());
    else if (kind == 1) (void)conv_dgrad(e, ci, g, gx, batch, Opt().mask(x->mask ? x : nullptr));   // (p1 has no bytes)
    else conv_wgrad(e, ci, g, x, batch);
  };
  hipEvent_t a, b;
  HIPOK(hipEventCreate(&a));
  HIPOK(hipEventCreate(&b));
  hipStream_t side = e->s2;
  e->s2 = nullptr;                 // time everything on the main stream
  const bool group_was = e->wg_group_on;
  e->wg_group_on = false;          // one layer at a time: its own launch
  const int splits_was = e->upd_splits[ci];      // (conv_wgrad records the slab count of that launch)
  run();
  HIPOK(hipEventRecord(a, e->s));
  for (int i = 0; i < reps; ++i) run();
  HIPOK(hipEventRecord(b, e->s));
  HIPOK(hipEventSynchronize(b));
  e->s2 = side;
  e->wg_group_on = group_was;
  e->upd_splits[ci] = splits_was;
  float ms = 0.f;
  HIPOK(hipEventElapsedTime(&ms, a, b));
  *ms_host = ms / reps;
  *flops_host = 2.0 * batch * Ho * Wo * (double)c.cout * c.cin * c.T();
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return 0;
}

int eosvos_mfma_probe(eosvos_engine* e, int iters, float* ms_host, double* flops_host) {
  ModeScope mode_scope(e);
  if (!e || !ms_host || !flops_host || iters < 1) return fail("bad argument");
  hipEvent_t a, b;
  HIPOK(hipEventCreate(&a));
  HIPOK(hipEventCreate(&b));
  launch_mfma_probe(e->loss_dev, iters, e->s);   // warm
  HIPOK(hipEventRecord(a, e->s));
  const double fl = launch_mfma_probe(e->loss_dev, iters, e->s);
  HIPOK(hipEventRecord(b, e->s));
  HIPOK(hipEventSynchronize(b));
  float ms = 0.f;
  HIPOK(hipEventElapsedTime(&ms, a, b));
  *ms_host = ms;
  *flops_host = fl;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return 0;
}
int eosvos_debug_tensor(eosvos_engine* e, const char* name, float** ptr, int64_t* dims4) {
  if (!e || !name || !ptr || !dims4) return fail("null argument");
  const int B = e->lastB > 0 ? e->lastB : 1;
  const std::string n(name);
  auto set = [&](float* p, int h, int w, int c) { *ptr = p; dims4[0] = B; dims4[1] = h; dims4[2] = w; dims4[3] = c; return 0; };
  auto tensor = [&](const Tensor* x) { return set(x->p, x->H, x->W, x->C); };
  // folded frozen-norm scale / shift (a = gamma / sqrt(var + eps), b = beta - mean * a), all norm layers concatenated
  if (n == "norm_a" || n == "norm_b") { *ptr = n == "norm_a" ? e->na : e->nb; dims4[0] = dims4[1] = dims4[2] = 1; dims4[3] = e->t.nnorm; return 0; }
  // the grow-only scratch of the label-map and adaptation stages, as 32-bit words (null and 0 words before its first use)
  if (n == "ccl_scratch") { *ptr = (float*)e->scratch; dims4[0] = dims4[1] = dims4[2] = 1; dims4[3] = (int64_t)(e->scratch_cap / 4); return 0; }
  const std::pair<const char*, Tensor*> named[] = {{"c1", e->c1}, {"p1", e->p1}, {"g_c1", e->g_c1}, {"g_p1", e->g_p1}, {"cat", e->cat},
      {"g_cat", e->g_cat}, {"proj", e->proj}, {"g_proj", e->g_proj}, {"dcat", e->dcat}, {"g_dcat", e->g_dcat}, {"d1", e->d1}, {"d2", e->d2},
      {"g_d1", e->g_d1}, {"g_d2", e->g_d2}};
  // plain DeepLabV3 has no decoder: its head (t.head3) writes "d1" / "g_d1" and the classifier "lowlog" / "g_low" on the ASPP
  // map (e->h16 x e->w16 = its stride-8 map), dense from the start of buffers that are sized for the stride-4 map
  const int hl = e->t.v3 ? e->h16 : e->h4, wl = e->t.v3 ? e->w16 : e->w4;
  if (e->t.v3 && (n == "d1" || n == "g_d1")) return set(n == "d1" ? e->d1->p : e->g_d1->p, hl, wl, 256);
  if (e->t.v3 && (n == "dcat" || n == "g_dcat" || n == "d2" || n == "g_d2")) return fail("unknown debug tensor " + n + " (plain DeepLabV3 has no decoder)");
  for (const auto& kv : named)
    if (n == kv.first) return tensor(kv.second);
  // image-pooling branch of the ASPP: one vector per image
  if (n == "vec") return set(e->vec, 1, 1, 2048);
  if (n == "gvec") return set(e->gvec, 1, 1, 2048);
  if (n == "poolout") return set(e->poolout, 1, 1, 256);
  if (n == "gp") return set(e->gp, 1, 1, 256);
  if (n == "lowlog") return set(e->lowlog, hl, wl, 1);
  if (n == "g_low") return set(e->g_low, hl, wl, 1);
  if (n == "logits") return set(e->logits, e->H, e->W, 1);
  if (n == "dlogits") return set(e->dlogits, e->H, e->W, 1);
  if (n.rfind("blk", 0) == 0) {
    const size_t dot = n.find('.');
    if (dot == std::string::npos) return fail("bad block tensor name");
    const int i = atoi(n.substr(3, dot - 3).c_str());
    if (i < 0 || i >= (int)e->bb.size()) return fail("block index out of range");
    const auto& f = e->bb[i];
    const std::string k = n.substr(dot + 1);
    const std::pair<const char*, Tensor*> named[] = {{"t1", f.t1}, {"t2", f.t2}, {"out", f.out}, {"g_t1", f.g_t1}, {"g_t2", f.g_t2},
                                                     {"g_out", f.g_out}, {"dsb", f.dsb}};
    for (const auto& kv : named)
      if (k == kv.first && kv.second) return tensor(kv.second);
  }
  // GroupNorm mode, "z<ci>": the raw output of normalised conv ci after a forward, its gradient after a backward
  if (n.size() > 1 && n.size() <= 5 && n[0] == 'z' && n.find_first_not_of("0123456789", 1) == std::string::npos) {
    const int ci = atoi(n.c_str() + 1);
    if (ci < (int)e->zbuf.size() && e->zbuf[ci]) return tensor(e->zbuf[ci]);
  }
  return fail("unknown debug tensor " + n);
}

// ---- low-level op entry points for the kernel parity tests -----------------------------------------
// One convolution through the PRODUCTION paths (conv_fwd / conv_dgrad / conv_wgrad incl. tap tables, tail
// launches, the coarse-grid stride-2 gradient and -- forced by `algo` -- the Winograd F(2x2,3x3) / F(4x4,3x3)
// transforms and batched GEMMs): a scratch engine whose topology is that single conv borrows the caller's stream.
namespace {
struct ScratchEngine {
  eosvos_engine t;
  bool ok = false;
  ScratchEngine(eosvos_engine* e, int algo, int B, int H, int W, int Cin, int Cout, int k, int stride, int dil, int pad,
                bool norm) {
    ConvL c{Cin, Cout, k, stride, dil, pad, norm, false, 0, 0, 0};
    t.t.convs.push_back(c);
    t.t.dec_a = t.t.dec_b = -1;
    t.t.nparam = c.wsize(); t.t.nlr = Cout; t.t.nnorm = Cout;
    t.arch = e->arch; t.H = H; t.W = W; t.maxB = B; t.dev = e->dev; t.s = e->s; t.s2 = nullptr;
    t.norm_mode = EOSVOS_NORM_BN_FROZEN;
    t.force_algo = algo;
    t.wg_budget = e->wg_budget;          // the launches plan under the caller's eosvos_set_wg_budget
    t.zbuf.assign(1, nullptr); t.gn_stats.assign(1, nullptr);
    t.ws_off.assign(1, 0); t.upd_splits.assign(1, 1);
    t.wino.assign(1, eosvos_engine::WinoRec());
    const int Ho = conv_out(H, k, stride, dil, pad), Wo = conv_out(W, k, stride, dil, pad);
    t.Wp = t.falloc(c.wsize()); t.na = t.falloc(Cout); t.nb = t.falloc(Cout);
    t.ws_conv = t.falloc(conv_ws_floats());
    // slabs for every budget eosvos_set_wg_budget accepts, as eosvos_create sizes them: the split count is not monotone in the
    // budget (the Winograd-domain gradient plans for half of it, which rounds up to another accepted budget)
    int64_t slab = 0;
    for (int b = 1; b <= B; ++b)
      for (int wb = 0; wb <= 512; wb += 64)
        slab = max64(slab, (int64_t)wgrad_max_splits(b * Ho * Wo, Cout, Cin, k * k, wb) * c.wsize());
    const bool wino = algo == EOSVOS_ALGO_WINO_F2 || algo == EOSVOS_ALGO_WINO_F4;
    if (wino) {
      if (!wino_shape(c)) return;
      const WinoGeom g = wino_geom(&t, c, B, Ho, Wo);
      for (int wb = 0; wb <= 512; wb += 64)
        slab = max64(slab, c.wsize() + (int64_t)wgrad_max_splits((int)g.ntile, Cout, Cin, g.np, wb) * Cout * g.np * Cin);
      auto& w = t.wino[0];
      w.V = t.falloc(g.np * g.prow * Cin);
      w.U = t.falloc((int64_t)g.np * Cout * Cin);
      w.Us = t.falloc((int64_t)g.np * Cout * Cin);
      w.dM = t.falloc(g.np * g.prow * Cout);
      t.wino_m_n = g.np * g.prow * max64(Cout, Cin);
      t.wino_m = t.falloc(t.wino_m_n); t.wino_dv = t.falloc(t.wino_m_n);
      if (!w.V || !w.U || !w.Us || !w.dM || !t.wino_m || !t.wino_dv) return;
    }
    t.ws_wg = t.falloc(slab);
    ok = t.Wp && t.na && t.nb && t.ws_conv && t.ws_wg;
  }
  // the caller's buffer at `key` as a tensor of this engine
  Tensor* tensor(const float* key, int H, int W, int C, int phase) { return t.ts.add(const_cast<float*>(key), H, W, C, phase); }
  // an eosvos_view of C channels: the slice [p - key, p - key + C) of the tensor at its key, or the tensor at p itself
  View view(const eosvos_view& v, int H, int W, int C, int phase) {
    if (!v.p) return View();
    return View(tensor(v.key ? v.key : v.p, H, W, v.ld, phase), v.key ? (int)(v.p - v.key) : 0, C);
  }
  ~ScratchEngine() {
    (void)hipStreamSynchronize(t.s);
    for (void* q : t.allocs) (void)hipFree(q);
  }
};
}  // namespace

int eosvos_test_conv_algo(eosvos_engine* e, int algo, const float* x, const float* w_oihw, const float* scale,
                          const float* bias, const float* res, int relu, int B, int H, int W, int Cin, int Cout, int k,
                          int stride, int dil, int pad, float* y) {
  ModeScope mode_scope(e);
  if (!e || !x || !w_oihw || !y) return fail("null argument");
  if (Cin % 4 || Cout % 4) return fail("channels must be multiples of 4");
  if (algo < EOSVOS_ALGO_AUTO || algo > EOSVOS_ALGO_WINO_F4) return fail("unknown conv algorithm");
  if ((scale == nullptr) != (bias == nullptr)) return fail("scale and bias go together (folded norm)");
  ScratchEngine se(e, algo, B, H, W, Cin, Cout, k, stride, dil, pad, scale != nullptr);
  if (!se.ok) return fail("scratch engine: shape not eligible for the requested algorithm, or out of memory");
  eosvos_engine* t = &se.t;
  amax_new_phase(t, 0);
  launch_oihw_to_ohwi(w_oihw, t->Wp, Cout, Cin, k * k, t->s);
  if (scale) {
    HIPOK(hipMemcpyAsync(t->na, scale, (size_t)Cout * 4, hipMemcpyDeviceToDevice, t->s));
    HIPOK(hipMemcpyAsync(t->nb, bias, (size_t)Cout * 4, hipMemcpyDeviceToDevice, t->s));
  }
  const int Ho = conv_out(H, k, stride, dil, pad), Wo = conv_out(W, k, stride, dil, pad);
  if (res && wino_on(t, 0, B, Ho, Wo)) return fail("the Winograd output transform has no residual input (the network never needs one)");
  conv_fwd(t, 0, se.tensor(x, H, W, Cin, 0), se.tensor(y, Ho, Wo, Cout, 0), B,
           Opt().relu(relu != 0).add(res ? View(se.tensor(res, Ho, Wo, Cout, 0)) : View()));
  HIPOK(hipStreamSynchronize(t->s));
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_test_conv_bwd_algo(eosvos_engine* e, int algo, const float* x, const float* w_oihw, const float* g,
                              const float* scale, const uint8_t* m8, int B, int H, int W, int Cin, int Cout, int k, int stride,
                              int dil, int pad, float* dx, float* dw_oihw) {
  ModeScope mode_scope(e);
  if (!e || !x || !w_oihw || !g || !dx || !dw_oihw) return fail("null argument");
  if (Cin % 4 || Cout % 4) return fail("channels must be multiples of 4");
  if (algo < EOSVOS_ALGO_AUTO || algo > EOSVOS_ALGO_WINO_F4) return fail("unknown conv algorithm");
  ScratchEngine se(e, algo, B, H, W, Cin, Cout, k, stride, dil, pad, scale != nullptr);
  if (!se.ok) return fail("scratch engine: shape not eligible for the requested algorithm, or out of memory");
  eosvos_engine* t = &se.t;
  const int T = k * k;
  amax_new_phase(t, 0);
  amax_new_phase(t, 1);
  launch_oihw_to_ohwi(w_oihw, t->Wp, Cout, Cin, T, t->s);
  if (scale) HIPOK(hipMemcpyAsync(t->na, scale, (size_t)Cout * 4, hipMemcpyDeviceToDevice, t->s));
  // the order of the backward pass: weight gradient first (it makes the shared Winograd-domain dM), then data gradient
  Tensor* const xt = se.tensor(x, H, W, Cin, 0);
  Tensor* const gt = se.tensor(g, conv_out(H, k, stride, dil, pad), conv_out(W, k, stride, dil, pad), Cout, 1);
  conv_wgrad(t, 0, gt, xt, B);
  xt->mask = const_cast<uint8_t*>(m8);        // the mask bytes of x, as the forward pass would have left them
  if (conv_dgrad(t, 0, gt, se.tensor(dx, H, W, Cin, 1), B, Opt().mask(m8 ? xt : nullptr))) return 1;
  float* dw = t->falloc((int64_t)Cout * Cin * T);
  if (!dw) return fail("hipMalloc dw");
  const int64_t n = (int64_t)Cout * Cin * T;
  launch_sgd_update(dw, t->ws_wg, t->upd_splits[0], n, scale ? t->na : nullptr, nullptr, nullptr, dw, (int64_t)T * Cin, n, t->s);
  launch_ohwi_to_oihw(dw, dw_oihw, Cout, Cin, T, 1.f, 0, t->s);
  HIPOK(hipStreamSynchronize(t->s));
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_test_conv(eosvos_engine* e, const float* x, const float* w_oihw, const float* scale, const float* bias,
                     const float* res, int relu, int B, int H, int W, int Cin, int Cout, int k, int stride, int dil,
                     int pad, float* y) {
  ModeScope mode_scope(e);
  return eosvos_test_conv_algo(e, EOSVOS_ALGO_DIRECT, x, w_oihw, scale, bias, res, relu, B, H, W, Cin, Cout, k, stride, dil, pad, y);
}
int eosvos_test_conv_bwd(eosvos_engine* e, const float* x, const float* w_oihw, const float* g, int B, int H, int W,
                         int Cin, int Cout, int k, int stride, int dil, int pad, float* dx, float* dw_oihw) {
  ModeScope mode_scope(e);
  return eosvos_test_conv_bwd_algo(e, EOSVOS_ALGO_DIRECT, x, w_oihw, g, nullptr, nullptr, B, H, W, Cin, Cout, k, stride, dil, pad, dx,
                                   dw_oihw);
}

// ---- the same convolution in the forms the network's passes use: channel slices of wider tensors (absmax slot, mask bytes
// and pitch of the TENSOR), accumulating / adding / partially masked data gradients ------------------------------------
namespace {
// the tensor's absmax slot as a consumer would read it: maximum of its words; valid = tlookup would return it
int read_tslot(eosvos_engine* t, const Tensor& x, unsigned* bits, int* valid) {
  *bits = 0; *valid = 0;
  if (!h3_mode() || !t->amax || x.slot < 0) return 0;
  unsigned w[AMAX_SUB];
  HIPOK(hipMemcpy2D(w, sizeof(unsigned), t->amax + amax_tcol(t, x.phase, x.slot), (size_t)AMAX_ROW * sizeof(unsigned),
                    sizeof(unsigned), AMAX_SUB, hipMemcpyDeviceToHost));
  for (int i = 0; i < AMAX_SUB; ++i) *bits = w[i] > *bits ? w[i] : *bits;
  *valid = x.valid ? 1 : 0;
  return 0;
}
// a producer's part for a source tensor that the caller filled: max|tensor| over ALL its channels into its slot, trusted
int seed_tslot(eosvos_engine* t, Tensor& x, long rows) {
  if (!h3_mode()) return 0;
  if (amax_init(t)) return fail("absmax arena");
  unsigned* sl = tslot(t, x);
  if (!sl) return fail("no absmax slot left for the source tensor");
  launch_absmax(x.p, rows, x.C, x.C, sl, t->s);
  tmark_valid(x);
  return 0;
}
bool view_ok(const eosvos_view& v, int C) {
  if (!v.p || v.ld < C || (v.ld & 3)) return false;
  if (!v.key) return true;
  const long off = v.p - v.key;
  return v.ldkey == v.ld && off >= 0 && !(off & 3) && off + C <= v.ldkey;
}
}  // namespace

int eosvos_test_conv_views(eosvos_engine* e, eosvos_conv_views* v) {
  ModeScope mode_scope(e);
  if (!e || !v || !v->w_oihw) return fail("null argument");
  const int B = v->B, H = v->H, W = v->W, Cin = v->Cin, Cout = v->Cout, k = v->k;
  if (B < 1 || H < 1 || W < 1 || Cin < 4 || Cout < 4 || (Cin % 4) || (Cout % 4)) return fail("bad geometry (channels must be multiples of 4)");
  if (v->algo < EOSVOS_ALGO_AUTO || v->algo > EOSVOS_ALGO_WINO_F4) return fail("unknown conv algorithm");
  const bool fwd = v->passes & EOSVOS_VIEWS_FWD, dg = v->passes & EOSVOS_VIEWS_DGRAD, wg = v->passes & EOSVOS_VIEWS_WGRAD;
  if (!fwd && !dg && !wg) return fail("no pass selected");
  if (fwd && (v->scale == nullptr) != (v->bias == nullptr)) return fail("scale and bias go together (folded norm)");
  if (fwd && (!view_ok(v->x, Cin) || !view_ok(v->y, Cout) || (v->res.p && !view_ok(v->res, Cout)))) return fail("bad forward view");
  const int nsl = v->fwd_slices > 1 ? v->fwd_slices : 1;
  if (nsl > 1) {      // slice i reads x.p + i * Cin and writes y.p + i * Cout: both must be slices of keyed tensors wide enough for all
    if (!fwd || dg || wg || v->res.p || !v->x.key || !v->y.key) return fail("fwd_slices: forward only, keyed x and y, no residual");
    if ((v->x.p - v->x.key) + (long)nsl * Cin > v->x.ldkey || (v->y.p - v->y.key) + (long)nsl * Cout > v->y.ldkey) return fail("fwd_slices: past the tensor");
  }
  if ((dg || wg) && !view_ok(v->g, Cout)) return fail("bad gradient view");
  if (dg && (!view_ok(v->gx, Cin) || (v->add.p && !view_ok(v->add, Cin)) || v->mask_c0 < 0 || (v->mask_c0 & 3))) return fail("bad data-gradient view");
  if (wg && (!view_ok(v->x, Cin) || !v->dw_oihw)) return fail("bad weight-gradient view");
  ScratchEngine se(e, v->algo, B, H, W, Cin, Cout, k, v->stride, v->dil, v->pad, v->scale != nullptr);
  if (!se.ok) return fail("scratch engine: shape not eligible for the requested algorithm, or out of memory");
  eosvos_engine* t = &se.t;
  const int T = k * k;
  const int Ho = conv_out(H, k, v->stride, v->dil, v->pad), Wo = conv_out(W, k, v->stride, v->dil, v->pad);
  const long Pin = (long)B * H * W, Pout = (long)B * Ho * Wo;
  launch_oihw_to_ohwi(v->w_oihw, t->Wp, Cout, Cin, T, t->s);
  if (v->scale) HIPOK(hipMemcpyAsync(t->na, v->scale, (size_t)Cout * 4, hipMemcpyDeviceToDevice, t->s));
  if (v->bias) HIPOK(hipMemcpyAsync(t->nb, v->bias, (size_t)Cout * 4, hipMemcpyDeviceToDevice, t->s));
  const View x = se.view(v->x, H, W, Cin, 0);
  v->slot_bits[0] = v->slot_bits[1] = v->src_slot_bits[0] = v->src_slot_bits[1] = 0;
  v->slot_valid[0] = v->slot_valid[1] = v->src_slot_valid[0] = v->src_slot_valid[1] = 0;
  amax_new_phase(t, 0);
  if ((fwd || wg) && v->x.key && seed_tslot(t, *x.t, Pin)) return 1;
  if (fwd) {
    if (v->res.p && wino_on(t, 0, B, Ho, Wo)) return fail("the Winograd output transform has no residual input (the network never needs one)");
    const View y = se.view(v->y, Ho, Wo, Cout, 0);
    y.t->mask = v->y_m8;
    for (int i = 0; i < nsl; ++i)
      conv_fwd(t, 0, View(x.t, x.c0 + i * Cin, Cin), View(y.t, y.c0 + i * Cout, Cout), B,
               Opt().relu(v->relu != 0).add(se.view(v->res, Ho, Wo, Cout, 0)));
    HIPOK(hipStreamSynchronize(t->s));
    HIPOK(hipGetLastError());
    if (read_tslot(t, *y.t, &v->slot_bits[0], &v->slot_valid[0])) return 1;
  }
  if ((fwd || wg) && v->x.key && read_tslot(t, *x.t, &v->src_slot_bits[0], &v->src_slot_valid[0])) return 1;
  const View g = se.view(v->g, Ho, Wo, Cout, 1);
  if (dg || wg) {
    amax_new_phase(t, 1);
    if (v->g.key && seed_tslot(t, *g.t, Pout)) return 1;
    // the order of the backward pass: weight gradient first (it makes the shared Winograd-domain dM), then data gradient
    if (wg) conv_wgrad(t, 0, g, x, B);
    if (dg) {
      const View gx = se.view(v->gx, H, W, Cin, 1);
      // the mask bytes of the activation gx is the gradient of: a tensor laid out like the view gx
      Tensor* const relu_x = v->gx_m8 ? se.tensor(v->gx.p, H, W, v->gx.ld, 0) : nullptr;
      if (relu_x) relu_x->mask = const_cast<uint8_t*>(v->gx_m8);
      if (conv_dgrad(t, 0, g, gx, B, Opt().accum(v->accum != 0).mask(relu_x, v->mask_c0).add(se.view(v->add, H, W, Cin, 1)))) return 1;
      HIPOK(hipStreamSynchronize(t->s));
      HIPOK(hipGetLastError());
      if (read_tslot(t, *gx.t, &v->slot_bits[1], &v->slot_valid[1])) return 1;
    }
    if (wg) {
      const int64_t n = (int64_t)Cout * Cin * T;
      float* dw = t->falloc(n);
      if (!dw) return fail("hipMalloc dw");
      launch_sgd_update(dw, t->ws_wg, t->upd_splits[0], n, v->scale ? t->na : nullptr, nullptr, nullptr, dw, (int64_t)T * Cin, n, t->s);
      launch_ohwi_to_oihw(dw, v->dw_oihw, Cout, Cin, T, 1.f, 0, t->s);
    }
  }
  HIPOK(hipStreamSynchronize(t->s));
  HIPOK(hipGetLastError());
  if ((dg || wg) && v->g.key && read_tslot(t, *g.t, &v->src_slot_bits[1], &v->src_slot_valid[1])) return 1;
  return 0;
}

int eosvos_test_aspp_dgrad(eosvos_engine* e, int batch, const float* g_cat, const uint8_t* l4_m8, float* g_l4_inout,
                           int force_fallback, int* merged_ran, unsigned* slot_bits, int* slot_valid) {
  ModeScope mode_scope(e);
  if (!e || !g_cat || !l4_m8 || !g_l4_inout || !merged_ran || !slot_bits || !slot_valid) return fail("null argument");
  if (batch < 1 || batch > e->maxB) return fail("batch out of range");
  const Topo& t = e->t;
  Tensor* const g_l4 = e->bb.back().g_out;
  Tensor* const l4 = e->bb.back().out;
  const int cin = t.convs[t.aspp[0]].cin;
  uint8_t* m8 = l4->mask;
  if (cin != 2048 || e->gn() || !m8) return fail("eosvos_test_aspp_dgrad needs the frozen-norm ResNet-50/101 ASPP with mask bytes");
  const size_t P = (size_t)batch * e->h16 * e->w16;
  plans_match_mode(e);
  e->masks_valid = false;                         // the mask bytes of l4 and the gradient buffers no longer belong to a forward
  e->have_loss_grad = false;
  HIPOK(hipMemcpyAsync(e->g_cat->p, g_cat, P * e->g_cat->C * sizeof(float), hipMemcpyDeviceToDevice, e->s));
  HIPOK(hipMemcpyAsync(m8, l4_m8, P * (cin / 4), hipMemcpyDeviceToDevice, e->s));
  HIPOK(hipMemcpyAsync(g_l4->p, g_l4_inout, P * cin * sizeof(float), hipMemcpyDeviceToDevice, e->s));
  amax_new_phase(e, 1);
  if (seed_tslot(e, *e->g_cat, (long)P)) return 1;      // as the projection's data gradient, the writer of g_cat, leaves it
  twrite_plain(*g_l4);                       // the pooling branch's broadcast has no fused absmax
  bool merged = false;
  if (aspp_dgrad(e, batch, g_l4, l4, force_fallback != 0, &merged)) return 1;
  *merged_ran = merged ? 1 : 0;
  HIPOK(hipMemcpyAsync(g_l4_inout, g_l4->p, P * cin * sizeof(float), hipMemcpyDeviceToDevice, e->s));
  HIPOK(hipStreamSynchronize(e->s));
  HIPOK(hipGetLastError());
  return read_tslot(e, *g_l4, slot_bits, slot_valid);
}

// ---- op-level entry points of the other kernels (misc_kernels.hip) --------------------------------------------------
// Each runs the production launcher with the engine's own geometry helpers (gn_geom inside launch_gn_*, make_resize +
// upload_resize, COLSUM_CHUNKS, last_bwd_chunks) on caller DEVICE tensors, on the engine's stream; scratch lives for one call.
namespace {
struct OpScratch {
  eosvos_engine t;                 // only its allocator and stream (upload_resize allocates through an engine)
  explicit OpScratch(eosvos_engine* e) { t.s = e->s; t.s2 = nullptr; t.dev = e->dev; }
  ~OpScratch() {
    (void)hipStreamSynchronize(t.s);
    for (void* q : t.allocs) (void)hipFree(q);
  }
};
}  // namespace

int eosvos_test_groupnorm(eosvos_engine* e, int bwd, float* z, int ldz, const float* g, int ldg, const float* gamma,
                          const float* beta, const float* res, int ldres, int relu, int B, int P, int C, float eps, float* y,
                          int ldy, float* stats, uint8_t* m8, int ldm8) {
  ModeScope mode_scope(e);
  if (!e || !z || !gamma || !stats) return fail("null argument");
  if (B < 1 || P < 1 || C < 16 || C % 16 || ldz < C || ldz % 4) return fail("bad GroupNorm geometry");
  const int C4 = C / 4, colblocks = (C4 + 255) / 256, ncol = C4 / colblocks;
  if (ncol * colblocks != C4 || (ncol * 4) % (C / 16)) return fail("channel count not supported by the GroupNorm kernels");
  OpScratch sc(e);
  float* partial = sc.t.falloc(gn_partial_floats(B));
  if (!partial) return fail("hipMalloc GroupNorm partials");
  if (bwd) {
    if (!g || ldg < C || ldg % 4) return fail("bad gradient argument");
    launch_gn_backward(z, ldz, g, ldg, gamma, stats, partial, B, P, C, e->s);
  } else {
    if (!beta || !y || ldy < C || ldy % 4 || (res && (ldres < C || ldres % 4))) return fail("bad forward argument");
    if (m8 && (!relu || ldm8 < C4)) return fail("the ReLU mask needs relu and ldm8 >= C / 4");
    launch_gn_forward(z, ldz, gamma, beta, res, ldres, y, ldy, stats, partial, B, P, C, eps, relu, e->s, nullptr, m8, ldm8);
  }
  HIPOK(hipStreamSynchronize(e->s));
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_test_maxpool(eosvos_engine* e, const float* x, int B, int H, int W, int C, float* y, uint8_t* idx, const float* gy,
                        float* gx) {
  ModeScope mode_scope(e);
  if (!e || !x || !y || !idx) return fail("null argument");
  if (B < 1 || H < 1 || W < 1 || C < 4 || C % 4) return fail("bad max-pool geometry");
  if ((gy == nullptr) != (gx == nullptr)) return fail("gy and gx go together");
  const int Ho = conv_out(H, 3, 2, 1, 1), Wo = conv_out(W, 3, 2, 1, 1);
  launch_maxpool_fwd(x, y, idx, B, H, W, C, Ho, Wo, e->s);
  if (gy) launch_maxpool_bwd(gy, idx, gx, B, H, W, C, Ho, Wo, e->s);
  HIPOK(hipStreamSynchronize(e->s));
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_test_resize(eosvos_engine* e, int align_corners, int hin, int win, int hout, int wout, int B, int C, const float* x,
                       int ldx, float* y, int ldy, const float* gy, int ldgy, float* gx, int ldgx, const uint8_t* m8, int ldm8) {
  ModeScope mode_scope(e);
  if (!e) return fail("null engine");
  if (hin < 1 || win < 1 || hout < 1 || wout < 1 || B < 1 || C < 1) return fail("bad resize geometry");
  if ((x == nullptr) != (y == nullptr) || (gy == nullptr) != (gx == nullptr)) return fail("x / y and gy / gx go together");
  if ((x && (ldx < C || ldy < C)) || (gy && (ldgy < C || ldgx < C)) || (m8 && ldm8 < C / 4)) return fail("bad leading dimension");
  if (m8 && C % 4) return fail("a masked resize backward needs C % 4 == 0 (one mask byte per 4 channels)");
  OpScratch sc(e);
  ResizeTab th, tw;
  if (upload_resize(&sc.t, make_resize(hin, hout, align_corners != 0), hin, hout, th)) return 1;
  if (upload_resize(&sc.t, make_resize(win, wout, align_corners != 0), win, wout, tw)) return 1;
  if (x) launch_resize_fwd(x, ldx, y, ldy, B, C, th, tw, e->s);
  if (gy) launch_resize_bwd(gy, ldgy, gx, ldgx, m8, ldm8, B, C, th, tw, e->s);
  HIPOK(hipStreamSynchronize(e->s));
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_test_aspp_pool(eosvos_engine* e, int B, int P, int K, int N, const float* w, const float* a, const float* bias,
                          const float* x, int ldx, float* v, float* pool, float* y, int ldy, uint8_t* m8, int ldm8,
                          const float* gy, int ldgy, float* gpool, float* gv, float* dw, float* gx, int ldgx) {
  ModeScope mode_scope(e);
  if (!e || !w || !x || !v || !pool || !y) return fail("null argument");
  if (B < 1 || P < 1 || K < 4 || K % 4 || N < 4 || N % 4 || ldx < K || ldx % 4 || ldy < N || ldy % 4) return fail("bad pooling geometry");
  if ((a == nullptr) != (bias == nullptr)) return fail("a and bias go together (folded norm)");
  if (m8 && ldm8 < N / 4) return fail("ldm8 < N / 4");
  if (gy && (!gpool || !gv || !dw || !gx || ldgy < N || ldgy % 4 || ldgx < K || ldgx % 4)) return fail("bad backward argument");
  OpScratch sc(e);
  float* colscratch = sc.t.falloc((int64_t)B * 64 * (K > N ? K : N));      // COLSUM_CHUNKS partial sums, as the engine sizes it
  float* slab = gy ? sc.t.falloc((int64_t)N * K) : nullptr;
  if (!colscratch || (gy && !slab)) return fail("hipMalloc pooling scratch");
  // forward (engine.cpp forward_impl, pool_branch): mean over pixels -> relu?(a * W v + b) -> every pixel of the channel slice
  launch_colsum(x, ldx, v, B, P, K, 1.0f / (float)P, colscratch, e->s);
  launch_gemv_fwd(w, v, a, bias, pool, B, N, K, e->s);
  launch_bcast_pixels(pool, y, ldy, B, P, N, 1.f, e->s, m8, ldm8);
  if (gy) {
    // backward (backward_impl): the slice's gradient summed over pixels (the ReLU mask is the consumer's: its data gradient
    // applies it) -> gv = a W^T gp, dW = gp v^T -> gv / P to every pixel
    launch_colsum(gy, ldgy, gpool, B, P, N, 1.f, colscratch, e->s);
    launch_gemv_bwd(w, v, gpool, a, gv, slab, B, N, K, e->s);
    launch_bcast_pixels(gv, gx, ldgx, B, P, K, 1.0f / (float)P, e->s);
    // the weight update's reduction (flush_updates): the slab times the folded-norm scale of each output channel
    launch_sgd_update(dw, slab, 1, (int64_t)N * K, a, nullptr, nullptr, dw, K, (int64_t)N * K, e->s);
  }
  HIPOK(hipStreamSynchronize(e->s));
  HIPOK(hipGetLastError());
  return 0;
}
int eosvos_test_head(eosvos_engine* e, const float* x, const float* w, const float* bias, int64_t P, int C, float* y,
                     const float* g, float* gx, float* dw) {
  ModeScope mode_scope(e);
  if (!e || !x || !w || !bias || !y) return fail("null argument");
  if (P < 1 || C < 4 || C % 4) return fail("bad head geometry");
  if (g && (!gx || !dw)) return fail("the backward needs gx and dw");
  OpScratch sc(e);
  launch_last_fwd(x, w, bias, y, P, C, e->s);
  if (g) {
    const int chunks = last_bwd_chunks(P);
    float* ws = sc.t.falloc((int64_t)chunks * (C + 1));
    if (!ws) return fail("hipMalloc head weight-gradient slabs");
    launch_last_bwd(x, w, g, gx, ws, P, C, chunks, e->s);
    launch_sgd_update(dw, ws, chunks, C + 1, nullptr, nullptr, nullptr, dw, C + 1, C + 1, e->s);      // slab sum, as flush_updates
  }
  HIPOK(hipStreamSynchronize(e->s));
  HIPOK(hipGetLastError());
  return 0;
}

// Weight gradient on pre-split operands (presplit_kernels.hip), stand-alone: no engine.  Device pointers; g / x NHWC fp32,
// ws [splits][Cout][k*k][Cin], g2 / x2 scratch of the operands' size, amax = AMAX_SUB * AMAX_ROW zeroed words, sc = 2 floats,
// zero = 2 KB of zeros.  which: 0 = absmax -> scale (with `margin` spare bits) -> split passes -> wgrad_p; 1 = wgrad_p only (siblings
// of an earlier call); 2 = the register-staged f16x3 kernel (wgrad_h3_kernel) on the fp32 operands; 3 = the two split passes only.
int eosvos_test_wgrad_presplit(const float* g, const float* x, float* ws, void* g2, void* x2, unsigned* amax, float* sc,
                               const void* zero, int B, int Ho, int Wo, int Cout, int Hi, int Wi, int Cin, int k, int stride,
                               int pad, int dil, int splits, int groups, int margin, int which, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!g || !x || !ws || !g2 || !x2 || !amax || !sc || !zero) return fail("null argument");
  if (groups < 0 || groups > splits) return fail("groups: 0 (one workgroup per chunk) ... splits");
  if (which == 0 || which == 2 || which == 4) {
    launch_absmax(g, (long)B * Ho * Wo, Cout, Cout, amax + 0, s);
    launch_absmax(x, (long)B * Hi * Wi, Cin, Cin, amax + 1, s);
  }
  if (which == 0 || which == 3) {
    launch_pair_split(g, g2, (long)B * Ho * Wo, Cout, Cout, amax + 0, margin, sc + 0, s);
    launch_pair_split(x, x2, (long)B * Hi * Wi, Cin, Cin, amax + 1, margin, sc + 1, s);
  }
  if (which == 0 || which == 1 || which == 4) {
    WgradPArgs a{};
    a.g2 = (const unsigned char*)g2; a.x2 = (const unsigned char*)x2; a.ws = ws;
    a.B = B; a.Ho = Ho; a.Wo = Wo; a.ldg = Cout; a.Cout = Cout; a.Hi = Hi; a.Wi = Wi; a.ldx = Cin; a.Cin = Cin;
    a.KH = a.KW = k; a.stride = stride; a.pad = pad; a.dil = dil; a.splits = splits; a.groups = groups;
    a.zero = (const unsigned char*)zero;
    a.scp_g = sc; a.scp_x = sc + 1; a.slot_g = amax; a.slot_x = amax + 1; a.scn_g = sc + 2; a.scn_x = sc + 3;
    a.margin_g = a.margin_x = margin; a.g = g; a.x = x;
    if (!wgrad_p_supported(a)) return fail("wgrad_p: channels must be multiples of 256");
    if (which == 4) HIPOK(hipMemsetAsync(sc, 0, 16, s));     // no producer scale: both operands staged from the fp32 tensors
    launch_wgrad_p(a, s);
  }
  if (which == 2) {
    WgradArgs a{};
    a.g = g; a.x = x; a.ws = ws; a.B = B; a.Ho = Ho; a.Wo = Wo; a.ldg = Cout; a.Cout = Cout; a.Hi = Hi; a.Wi = Wi; a.ldx = Cin;
    a.Cin = Cin; a.KH = a.KW = k; a.stride = stride; a.pad = pad; a.dil = dil; a.splits = splits; a.amax_g = amax; a.amax_x = amax + 1;
    const int keep = conv_thread_mfma_mode();
    conv_set_thread_mfma_mode(2);
    launch_wgrad(a, s);
    conv_set_thread_mfma_mode(keep);
  }
  HIPOK(hipGetLastError());
  return 0;
}

}  // extern "C"
