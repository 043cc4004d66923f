// Launcher declarations of the gfx950 kernels (conv_kernels.hip, misc_kernels.hip, crf_kernels.hip, ccl_kernels.hip, ...).
// Host code (engine.cpp) only sees these plain-C++ functions; every launcher enqueues on
// the given stream and never synchronises or allocates.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace eosvos {
#define AMAX_SUB 32        // words per absmax slot
#define AMAX_ROW 2048      // distance (in words) between the words of a slot = slots per arena
#if defined(__HIPCC__)
// absmax bookkeeping of the f16x3 matrix mode: |x| bit patterns compare like unsigned integers
// Only finite values count: a NaN / inf element must not set the scale of the whole tensor (it still propagates as NaN
// through the split of its own products).
__device__ __forceinline__ unsigned amax_f1(float x) {
  const unsigned a = __float_as_uint(x) & 0x7fffffffu;
  return a < 0x7f800000u ? a : 0u;
}
__device__ __forceinline__ unsigned amax_f4(unsigned m, const float4& v) {
  const unsigned a = amax_f1(v.x), b = amax_f1(v.y), c = amax_f1(v.z), d = amax_f1(v.w);
  const unsigned ab = a > b ? a : b, cd = c > d ? c : d;
  const unsigned q = ab > cd ? ab : cd;
  return m > q ? m : q;
}
// ReLU mask bytes (ConvArgs::mask8): bit j of a byte = (channel 4q + j > 0)
__device__ __forceinline__ uint8_t relu_bits(const float4& v) {
  return (uint8_t)((v.x > 0.f ? 1 : 0) | (v.y > 0.f ? 2 : 0) | (v.z > 0.f ? 4 : 0) | (v.w > 0.f ? 8 : 0));
}
__device__ __forceinline__ void relu_mask8(float4& v, unsigned bits) {
  v.x = (bits & 1u) ? v.x : 0.f; v.y = (bits & 2u) ? v.y : 0.f; v.z = (bits & 4u) ? v.z : 0.f; v.w = (bits & 8u) ? v.w : 0.f;
}
// An absmax slot is AMAX_SUB words, AMAX_ROW words apart (word j of slot s = base[j * AMAX_ROW + s]): a workgroup
// raises word (its index % AMAX_SUB) with one fire-and-forget atomic, the consumer takes the maximum of the AMAX_SUB
// words.  Measured (tools/probes/atomic_probe.cpp, 2048 workgroups): all on ONE word 25 us (11 ns per atomic, they
// serialise in L2), on 32 words of one 128-byte line 13 us, on 32 words >= 256 bytes apart 0 us over the kernel
// without atomics; reading the word first and skipping the atomic unless it raises it costs nothing there either, but a
// fix-up workgroup that lives 5 us paid 2.5-9 us per launch for that dependent load.
template <int WAVES = 4>          // waves of the workgroup
__device__ __forceinline__ void amax_block_commit(unsigned m, unsigned* slot) {
  __shared__ unsigned wmax[WAVES];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = (unsigned)__shfl_xor((int)m, o);
    m = m > t ? m : t;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned q = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) q = q > wmax[i] ? q : wmax[i];
    if (q) atomicMax(slot + (size_t)((blockIdx.x + blockIdx.y) & (AMAX_SUB - 1)) * AMAX_ROW, q);
  }
}
// the value of a slot: every lane returns the maximum of its AMAX_SUB words (call with the whole wave active)
__device__ __forceinline__ unsigned amax_read(const unsigned* slot) {
  const int lane = threadIdx.x & 63;
  unsigned m = lane < AMAX_SUB ? slot[(size_t)lane * AMAX_ROW] : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = (unsigned)__shfl_xor((int)m, o);
    m = m > t ? m : t;
  }
  return m;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// integer sum over a 256-thread block, valid in every thread
__device__ __forceinline__ int block_sum_i(int v, int* sh /*4*/) {
  v = wave_sum_i(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
// Source of output index o under torch's bilinear align_corners=False rule, scale = (float)in / (float)out: the coordinate
// max(0, scale * (o + 0.5) - 0.5) in fp32, its lower neighbour i0, the upper one i1 clamped at the edge, and the weight of i1
// (the arithmetic of resize_fwd_kernel's tables; tta_accumulate_kernel and the zoom kernels compute it in place).
__device__ __forceinline__ void tta_src(int o, float scale, int in, int& i0, int& i1, float& lam) {
  float src = scale * ((float)o + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  lam = src - (float)i0;
}
// An entry of cv::warpAffine's fixed-point tables (10 fractional bits), computed where it is used: (a * i) * 1024 per column
// and (a * i + b) * 1024 + round_delta per row, in double with each operation rounded on its own (no fused multiply-add),
// then round-half-even to int like lrint (warp_affine_kernel, lucid_compose_kernel).
__device__ __forceinline__ int warp_fix(double a, int i) { return __double2int_rn(__dmul_rn(__dmul_rn(a, (double)i), 1024.0)); }
__device__ __forceinline__ int warp_fix(double a, int i, double b, int rd) {
  return __double2int_rn(__dmul_rn(__dadd_rn(__dmul_rn(a, (double)i), b), 1024.0)) + rd;
}
#endif

// ---------------------------------------------------------------------------------
// Implicit-GEMM convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32).
//   out[m][n] = epilogue( sum_{tap,k} A[m][(tap,k)] * Wt[(tap,k)][n] )
// m runs over destination pixels (B*Ho*Wo, NHWC), A is gathered from the NHWC source at
//   sy = oy*mul + off0 + ky*kstep   (valid iff sy % up == 0, 0 <= sy/up < Hi; same in x)
// which expresses both the forward conv (mul=stride, off0=-pad, kstep=dil, up=1) and its
// data gradient (mul=1, off0=pad, kstep=-dil, up=stride).
// Weights are always the engine layout W[cout][tap][cin]:
//   forward : n = cout (rows of W, "n-major" B operand), k = cin
//   dgrad   : n = cin, k = cout ("k-major" B operand read straight from W; the frozen-norm
//             scale a[cout] is applied to A's k index while staging)
// ---------------------------------------------------------------------------------
struct ConvArgs {
  const float* x;       // gather source, NHWC, channel offset already applied
  const float* w;       // W[cout][T][cin]
  float* y;             // destination, NHWC, channel offset already applied
  float* ws;            // partial-tile slabs, conv_ws_floats() floats
  int B, Hi, Wi, ldx;   // source geometry, floats per source pixel
  int Kc;               // reduction channels per tap
  int Ho, Wo, N, ldy;   // destination geometry
  int KH, KW;
  int mul, off0, kstep, upshift;  // up = 1 << upshift
  int M;                // B*Ho*Wo
  int wN, wK;           // dims of W as stored: W[wN][T][wK]  (fwd: N,Kc ; dgrad: Kc,N)
  int kmajor;           // 0 forward, 1 dgrad
  const float* scale;   // per-n multiply (fwd norm a), may be null
  const float* bias;    // per-n add (fwd norm b / conv bias), may be null
  const float* kscale;  // per-k multiply on A (dgrad: norm a of the conv), may be null
  const float* res;     // fwd: residual added before ReLU; NHWC with ldres
  int ldres;
  // ReLU masks as bytes: one byte per 4 consecutive channels of a pixel, bit j = (channel 4q + j of the forward activation
  // > 0), ldm8 bytes per pixel (= the tensor's floats per pixel / 4).  The forward epilogue that applies the ReLU writes
  // them (mask8_out), the data gradient reads them (mask8: out = 0 where the bit is clear, for n >= mask_c0): 1/16 of the
  // fp32 activation.  Pointers carry the same channel offset (/ 4) as the views they describe.
  const uint8_t* mask8;
  int ldm8, mask_c0;
  uint8_t* mask8_out;
  int ldm8_out;
  int relu;
  int accum;            // dgrad: add the existing contents of y
  int plane_rows;       // != 0: batched GEMM -- rows [k*plane_rows, (k+1)*plane_rows) use the weights w + k*w_plane
  long w_plane;
  int nplanes;          // planes of a batched GEMM (16: Winograd F(2,3); 36: F(4,3))
  int row_chunks;       // streaming kernel, batched GEMM: workgroups (row chunks) per plane and column range (set by the launcher)
  int par;              // 1: GEMM rows enumerate the Ho x Wo grid parity class by parity class (stride-2 3x3 dgrad)
  int dst_up, Hf, Wf;   // dst_up=1: GEMM row (b,oy,ox) is written to pixel (b,2oy,2ox) of an Hf x Wf grid
  const int* tprefix;   // optional (device): compacted K-step prefix per tile (tiles+1), see conv_build_tap_table
  const int* tmask;     // optional (device): valid-tap bit mask per tile
  const int* torder;    // optional (device): the tiles sorted by descending K steps (whole-tile plan of a tap-table launch)
  long total_units;     // sum of valid K steps when tprefix is set, else 0
  int deep;             // set by conv_plan: 1 / 2 = the 3-workgroups-per-CU kernel variants (K step 32 single stage / 16)
  int dp_q, per, nwg;   // set by conv_plan: whole tiles per workgroup, streamed units per workgroup, workgroups
  int splitk;           // set by conv_plan: > 0 = uniform split-K, workgroup b takes K chunk b / tiles of tile b % tiles
  int wg_budget;        // workgroups the launch may plan for (0: two per CU); engines that run beside others split less
  // K-concatenated launch (nseg > 0; data gradients only): the reduction runs over `nseg` convolutions that ADD into the same
  // output -- the four ASPP branches' data gradients into d(layer4 output) as one launch: no accumulate read-modify-write
  // between them, one fix-up pass instead of one each.  The convs share the gather source tensor (x, ldx; segment s reads
  // channels [xoff_s, xoff_s + Kc)) and the destination; each has its own filter (taps / dilation / padding), weights
  // (offset from w), norm scale (offset from kscale) and -- f16x3 -- its own operand scales (the accumulators are rescaled by
  // an exact power of two where the K loop crosses into the next segment).  `taps` (device) describes every (segment, ky, kx)
  // as a global tap id, `taplist` (device, 32 bytes per tile) lists the ids a tile keeps, tprefix counts its K steps.
  int nseg;
  const struct ConvTap* taps;
  const unsigned char* taplist;
  long w_floats;                // extent of the weights of all segments from `w`
  const unsigned* seg_amax_w[4];
  const unsigned* seg_amax_ks[4];
  // f16x3 mode: device words holding the bit pattern of max|x| over the gather source, over the weights as passed in `w`
  // (all planes of a batched GEMM) and -- data gradient -- over `kscale`; see launch_absmax
  const unsigned* amax_x;
  const unsigned* amax_w;
  const unsigned* amax_ks;
  unsigned* amax_y;     // optional: atomicMax of the bit patterns of |y| as written (the absmax slot of the destination tensor)
  // pre-split operand path: the epilogue also writes the destination's "pair8" sibling (presplit_kernels.hip) -- every float4 it
  // stores as 4 fp16 hi + 4 fp16 lo under the scale *y2_sc (chosen from the PREVIOUS iteration's absmax; the consumer side
  // validates it against this iteration's and re-splits if it does not fit).  y2 has y's addressing (ldy, same channel offset).
  unsigned char* y2;
  const float* y2_sc;
  int y2_done;          // set by launch_conv: the kernel it chose writes the sibling (the tiled f16x3 kernels and their fix-up pass)
};
struct ConvTap {
  int dy, dx;      // source pixel = destination pixel + (dy, dx)   (data gradient: pad - k * dilation)
  int xoff;        // channel offset of the segment's slice in the gather source
  int wbase;       // offset (floats, from ConvArgs::w) of W_seg[k = 0][this tap][n = 0]
  int wrow;        // floats between consecutive k rows of W_seg (= taps of the segment x wK)
  int ksoff;       // offset of the segment's norm scale from ConvArgs::kscale
  int seg, pad_;
};
// Parity-major row order of a stride-2 data gradient: rows [0, M) walk the (even,even) output pixels of all
// images, then (even,odd), (odd,even), (odd,odd).  A pixel of parity (py,px) only receives the filter taps with
// ky = (py+pad) mod 2, kx likewise: 1, 2, 2 or 4 of the 9 taps of a 3x3 kernel, so tiles that are pure in parity
// skip the other taps through the per-tile tap table.  Returns the ordinary index (b*Ho + oy)*Wo + ox.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int conv_par_pixel(int B, int Ho, int Wo, int m) {
  const int He = (Ho + 1) >> 1, Hod = Ho >> 1, We = (Wo + 1) >> 1, Wod = Wo >> 1;
  const int n00 = B * He * We, n01 = B * He * Wod, n10 = B * Hod * We;
  int py, px, r = m;
  if (r < n00) { py = 0; px = 0; }
  else if ((r -= n00) < n01) { py = 0; px = 1; }
  else if ((r -= n01) < n10) { py = 1; px = 0; }
  else { r -= n10; py = 1; px = 1; }
  const int Hc = py ? Hod : He, Wc = px ? Wod : We;
  const int nc = Hc * Wc;
  const int b = r / nc, rr = r - b * nc;
  const int cy = rr / Wc, cx = rr - cy * Wc;
  return (b * Ho + 2 * cy + py) * Wo + 2 * cx + px;
}
// plans the launch (conv_plan, unless a streaming kernel takes it), launches the kernel (+ the fix-up kernel when tiles are
// shared); sets a.y2_done
void launch_conv(ConvArgs& a, hipStream_t s);
int conv_bn(const ConvArgs& a);      // tile width in N (64 or 128)
int conv_plan(ConvArgs& a);          // number of workgroups; sets a.deep, a.dp_q, a.per, a.nwg, a.splitk
void conv_set_mfma_mode(int mode);
void conv_set_thread_mfma_mode(int mode);   // >= 0: overrides the process-wide mode on this host thread (an engine's own mode, per call); -1: none
int conv_thread_mfma_mode();
// per-launch HIP-event timing of the MFMA kernels (conv_kernels.hip)
void conv_prof_enable(int on);
int conv_prof_read(int max, const char** names, long* counts, double* ms, double* flops);
void conv_prof_mark_begin(int kernel, double flops, hipStream_t s);   // launchers outside conv_kernels.hip; kernel = a ProfKernel id
void conv_prof_mark_end(hipStream_t s);
// Plan log for the tests (host bookkeeping only, off by default): one record per launch_conv call since conv_plan_log_enable(1),
// the first kConvPlanLogCap of them.  A launch a streaming kernel took has its kernel id and zeros in the plan fields.
struct ConvPlanRec {
  int kernel;                       // ProfKernel id of the main kernel
  int kmajor, bn;                   // gather side, column-tile width
  int tiles, ksteps;                // output tiles, nominal K steps of one tile (of 16 channels for deep == 2)
  int deep, dp_q, per, nwg, splitk; // what conv_plan set
  int tprefix, torder;              // 1: the launch had a tap table / its longest-first tile order
  int fixup;                        // 1: the fix-up pass was launched
  int budget;                       // conv_wg_budget_of(a.wg_budget): the workgroups the launch planned for
};
constexpr int kConvPlanLogCap = 16;
constexpr int kConvPlanLogFields = sizeof(ConvPlanRec) / sizeof(int);
void conv_plan_log_enable(int on);  // 1: clear and record; 0: stop (the records stay readable)
// copies min(launches, max, kConvPlanLogCap) records and their kernel names; returns the launches seen since the enable
int conv_plan_log_read(ConvPlanRec* out, const char** names, int max);
// The profiled kernels: id and reported name of every record, in the order conv_prof_read reports them.  Families of four
// are <128, false>, <128, true>, <64, false>, <64, true> (convs: tile width, K-major) or <128, 128>, <128, 64>, <64, 128>,
// <64, 64> (weight gradients); a launcher adds the member's offset to the family's first id.
#define EOSVOS_PROF_KERNELS(X) \
  X(kProfConvX6, "conv_x6_kernel<128, false>") X(kProfConvX6_1, "conv_x6_kernel<128, true>") \
  X(kProfConvX6_2, "conv_x6_kernel<64, false>") X(kProfConvX6_3, "conv_x6_kernel<64, true>") \
  X(kProfWgradX6, "wgrad_x6_kernel<128, 128>") X(kProfWgradX6_1, "wgrad_x6_kernel<128, 64>") \
  X(kProfWgradX6_2, "wgrad_x6_kernel<64, 128>") X(kProfWgradX6_3, "wgrad_x6_kernel<64, 64>") \
  X(kProfConvIgemm, "conv_igemm_kernel<128, false, *>") X(kProfConvIgemm_1, "conv_igemm_kernel<128, true, *>") \
  X(kProfConvIgemm_2, "conv_igemm_kernel<64, false, 0>") X(kProfConvIgemm_3, "conv_igemm_kernel<64, true, 0>") \
  X(kProfWgrad, "wgrad_kernel<128, 128>") X(kProfWgrad_1, "wgrad_kernel<128, 64>") \
  X(kProfWgrad_2, "wgrad_kernel<64, 128>") X(kProfWgrad_3, "wgrad_kernel<64, 64>") \
  X(kProfFixup, "conv_fixup_kernel") \
  X(kProfWgradX6Group, "wgrad_x6_group_kernel<128, 128>") X(kProfWgradX6Group_1, "wgrad_x6_group_kernel<128, 64>") \
  X(kProfWgradX6Group_2, "wgrad_x6_group_kernel<64, 128>") X(kProfWgradX6Group_3, "wgrad_x6_group_kernel<64, 64>") \
  X(kProfConvH3, "conv_h3_kernel<128, false>") X(kProfConvH3_1, "conv_h3_kernel<128, true>") \
  X(kProfConvH3_2, "conv_h3_kernel<64, false>") X(kProfConvH3_3, "conv_h3_kernel<64, true>") \
  X(kProfWgradH3, "wgrad_h3_kernel<128, 128>") X(kProfWgradH3_1, "wgrad_h3_kernel<128, 64>") \
  X(kProfWgradH3_2, "wgrad_h3_kernel<64, 128>") X(kProfWgradH3_3, "wgrad_h3_kernel<64, 64>") \
  X(kProfWgradH3Group, "wgrad_h3_group_kernel<128, 128>") X(kProfWgradH3Group_1, "wgrad_h3_group_kernel<128, 64>") \
  X(kProfWgradH3Group_2, "wgrad_h3_group_kernel<64, 128>") X(kProfWgradH3Group_3, "wgrad_h3_group_kernel<64, 64>") \
  X(kProfConvH3Multi, "conv_h3_multi_kernel") X(kProfConvX6Multi, "conv_x6_multi_kernel") \
  X(kProfStream1x1_128, "conv1x1_stream_kernel<*, 128>") X(kProfStream1x1_64, "conv1x1_stream_kernel<*, 64>") \
  X(kProfStream3x3, "conv3x3_stream_kernel") \
  X(kProfWgradP, "wgrad_p_kernel<256, 256>") X(kProfWgradPGroup, "wgrad_p_group_kernel<256, 256>")      /* presplit_kernels.hip */
enum ProfKernel {
#define EOSVOS_PROF_ID(id, name) id,
  EOSVOS_PROF_KERNELS(EOSVOS_PROF_ID)
#undef EOSVOS_PROF_ID
  kProfKernels
};
double conv_exec_frac(const struct ConvArgs& a);
double wgrad_exec_frac(const struct WgradArgs& a);
int conv_mfma_mode();                // 2: f16x3 split kernels (default), 1: bf16x6 (EOSVOS_MFMA=bf16x6), 0: fp32 MFMA kernels (EOSVOS_MFMA=f32)
// max|x| over rows x C floats (row pitch ld): atomicMax of the bit patterns into *slot (the caller zeroes the slot first)
void launch_absmax(const float* x, long rows, int C, int ld, unsigned* slot, hipStream_t s);
// zero `count` consecutive absmax slots (every word of each)
void launch_amax_zero(unsigned* first, int count, hipStream_t s);
// many dense tensors in one launch: segment y = floats [dev_off[y], dev_off[y] + dev_n[y]) of base (dev_n % 4 == 0) -> slots[y]
void launch_absmax_segments(const float* base, const long* dev_off, const int* dev_n, int nseg, unsigned* slots, hipStream_t s);
// calibration: back-to-back fp32 MFMAs, returns the FLOPs the launch performs
double launch_mfma_probe(float* scratch, int iters, hipStream_t s);
int64_t conv_ws_floats();
}  // namespace eosvos
#include <vector>
namespace eosvos {
// per-tile compacted K-step prefix (tiles + 1 entries) and valid-tap masks; returns the total number of valid K steps
long conv_build_tap_table(const ConvArgs& a, std::vector<int>& prefix, std::vector<int>& mask);
// K-concatenated data gradient: per segment (kernel size k, dilation, padding, channel offset, weight offset, norm-scale
// offset); fills the global tap descriptors, the per-tile tap lists (32 bytes per tile) and the K-step prefix; returns the
// total number of K steps
struct ConvSegHost { int k, dil, pad, xoff; long woff; int ksoff; };
long conv_build_multi_table(const ConvArgs& a, const ConvSegHost* segs, int nseg, std::vector<int>& prefix,
                            std::vector<unsigned char>& taplist, std::vector<ConvTap>& taps);
bool conv_multi_supported();     // the current matrix mode has the K-concatenated kernel (the split modes)

// Weight gradient: ws[z][cout][tap][cin] = sum over the z-th pixel chunk of
//   G[p][cout] * X[src(p,tap)][cin]
struct WgradArgs {
  const float* g;       // NHWC gradient w.r.t. the (pre-ReLU, post-norm) conv output
  const float* x;       // NHWC conv input
  float* ws;            // [splits][Cout][T][Cin]
  int B, Ho, Wo, ldg, Cout;
  int Hi, Wi, ldx, Cin;
  int KH, KW, stride, pad, dil;
  int splits;
  long g_tap_stride, x_tap_stride;   // != 0: tap t reads plane g + t*stride / x + t*stride (batched GEMMs, Winograd)
  const unsigned* amax_g;            // f16x3 mode: bit pattern of max|g| / max|x| over the tensors (all planes), device words
  const unsigned* amax_x;
  // pre-split operand path: this launch stands in for the pre-split kernel (siblings not written this iteration); workgroup 0
  // leaves the scales for the next iteration's producers (absmax + margin spare bits), nullptr: none
  float* scn_g; float* scn_x;
  int margin_g, margin_x;
};
void launch_wgrad(const WgradArgs& a, hipStream_t s);
int wgrad_pick_splits(int P, int Cout, int Cin, int T, int wg_budget = 0, int mode = -1);   // mode -1: the current matrix mode
// grouped launch (bf16x6 mode): entries of one tile shape bm x bn = wgrad_group_tile(Cout) x wgrad_group_tile(Cin);
// dev_map holds (entry, workgroup-of-entry) pairs, workgroup-of-entry = split * tiles + tile as in launch_wgrad
int wgrad_group_tile(int channels);
void launch_wgrad_group(const WgradArgs* dev_tab, const int* dev_map, int nwg, int bm, int bn, double flops, hipStream_t s);
// ---- pre-split operand path (presplit_kernels.hip) ----
// "pair8" sibling of an fp32 NHWC tensor: same addressing (4 bytes per element), every 8 consecutive channels of a pixel stored as
// [8 x fp16 hi | 8 x fp16 lo] under one power-of-two scale per tensor (the two pieces of the f16x3 product).
struct WgradPArgs {
  const unsigned char* g2;   // pair8 sibling of the gradient w.r.t. the conv output (WgradArgs::g)
  const unsigned char* x2;   // pair8 sibling of the conv input (WgradArgs::x)
  float* ws;                 // [splits][Cout][T][Cin]
  int B, Ho, Wo, ldg, Cout;
  int Hi, Wi, ldx, Cin;
  int KH, KW, stride, pad, dil;
  int splits;                // K chunks = slabs: the K partition (and with it the order of every fp32 sum) of WgradArgs::splits
  int groups;                // workgroups per tile that share the chunks (0: one per chunk); 1 <= groups <= splits
  long g_tap_stride, x_tap_stride;   // floats, as WgradArgs
  const unsigned char* zero; // >= 2 KB of zero bytes (rows past the last contributing pixel)
  // Scales.  scp_*: the scale the sibling's producer used (chosen from the previous iteration's absmax); slot_*: the tensor's
  // COMPLETE absmax slot of this iteration.  The kernel checks that the producer's scale fits (no overflow: max * scale < 2^15,
  // at most PAIR_HEADROOM spare bits); an operand whose scale does not fit is staged from the fp32 tensor (g / x) with the
  // split done on the fly under the fresh scale -- slower, never wrong.  Workgroup 0 leaves the scales for the NEXT iteration's
  // producers in *scn_* (fresh absmax + margin_* spare bits; scp and scn are different words: iteration parity).
  const float* scp_g; const float* scp_x;
  const unsigned* slot_g; const unsigned* slot_x;
  float* scn_g; float* scn_x;
  int margin_g, margin_x;
  const float* g; const float* x;
};
#define PAIR_HEADROOM 10      // spare bits a producer's scale may have over the tensor's absmax before the operand is re-split
bool wgrad_p_supported(const WgradPArgs& a);
int wgrad_p_tiles(const WgradPArgs& a);
void launch_wgrad_p(const WgradPArgs& a, hipStream_t s);
int wgrad_p_pick_splits(int P, int Cout, int Cin, int T, int wg_budget);
int wgrad_p_resident(int wg_budget);
void launch_wgrad_p_group(const WgradPArgs* dev_tab, const int* dev_map, int nwg, double flops, hipStream_t s);
// fp32 view [rows][C] (row pitch ld) -> pair8 sibling `out` (same addressing) under the scale of the view's complete absmax slot
// (+ `margin` spare bits); the scale is left in *sc
void launch_pair_split(const float* x, void* out, long rows, int C, int ld, const unsigned* slot, int margin, float* sc, hipStream_t s);
int conv_wg_budget_of(int requested);   // workgroups a launch plans for under eosvos_set_wg_budget(requested)
int conv_clamp_wg_budget(int n);     // the budgets the slab arenas are sized for: 0 (default) or a multiple of 64 in [64, 512]
// Winograd F(tm x tm, 3x3) transform passes (misc_kernels.hip), tm = 2 or 4: V = B^T d B, dM = A dY A^T, U = G w G^T,
// y = epilogue(A^T M A), dX = mask8?(B dV B^T, overlapped), dW = G^T sum_z dU_z G
// planes are [(tm+2)^2][prow][C] with prow >= B*dil*dil*th*tw rows (padded to the GEMM tile so that a row tile never straddles planes)
// dil: dilation of the 3x3 conv = dil*dil interleaved sub-grids; tiles are (image, sy, sx, ty, tx), th x tw tiles of tm x tm outputs per sub-grid
void launch_wino_input(int tm, const float* x, int ldx, int C, int B, int H, int W, int th, int tw, int dil, long prow, float* V,
                       hipStream_t s, unsigned* amax = nullptr);
void launch_wino_grad(int tm, const float* g, int ldg, int C, int B, int H, int W, int th, int tw, int dil, long prow, float* M,
                      hipStream_t s, unsigned* amax = nullptr);
void launch_wino_weight(int tm, const float* w, int Cout, int Cin, const float* rowscale, float* U, float* Us, hipStream_t s,
                        unsigned* amax_u = nullptr, unsigned* amax_us = nullptr);   // Us = rowscale * U
void launch_wino_output(int tm, const float* M, long prow, int C, int B, int H, int W, int th, int tw, int dil, const float* scale,
                        const float* bias, int relu, float* y, int ldy, hipStream_t s, unsigned* amax = nullptr,
                        uint8_t* mask8_out = nullptr, int ldm8 = 0);
void launch_wino_wgrad_finish(int tm, const float* ws, int splits, int Cout, int Cin, float* dst, hipStream_t s);
void launch_wino_dgrad_output(int tm, const float* dV, long prow, int C, int B, int H, int W, int th, int tw, int dil,
                              const uint8_t* mask8, int ldm8, int mask_c0, int accum, float* gx, int ldgx, hipStream_t s,
                              unsigned* amax = nullptr);

// ---------------------------------------------------------------------------------
// misc_kernels.hip
// ---------------------------------------------------------------------------------
void launch_nchw_to_nhwc_pad(const float* src, float* dst, int B, int C, int H, int W, int pad,
                             hipStream_t s, unsigned* amax = nullptr, int mirror = 0);      // amax: absmax slot of the frame (f16x3 mode)
                                                                                               // mirror: source column x -> padded column W-1-x
void launch_fill(float* p, int64_t n, float v, hipStream_t s);
// OIHW <-> engine layout O,(kh,kw),I for one tensor
void launch_oihw_to_ohwi(const float* src, float* dst, int O, int I, int T, hipStream_t s);
void launch_ohwi_to_oihw(const float* src, float* dst, int O, int I, int T, float alpha, int add,
                         hipStream_t s);
void launch_fold_norm(const float* gamma, const float* beta, const float* mean, const float* var,
                      float eps, float* a, float* b, int64_t n, hipStream_t s);

// stem: 7x7 s2 conv on the zero-padded (3 px) NHWC3 frame + affine + ReLU; and its wgrad
void launch_stem_fwd(const float* xpad, const float* w /*[64][49][3]*/, const float* a,
                     const float* b, float* y, int B, int H, int W, int Ho, int Wo, hipStream_t s);
void launch_stem_wgrad(const float* xpad, const float* g, float* ws /*[chunks][64*147]*/, int B,
                       int H, int W, int Ho, int Wo, int chunks, hipStream_t s);
int stem_wgrad_chunks(int B, int Ho, int Wo);
// f16x3 mode: the stem on the fp16 matrix cores (conv_kernels.hip); amax_x = absmax slot of the padded frame
void launch_stem_fwd_h3(const float* xpad, const float* w /*[64][49][3]*/, const float* a, const float* b, float* y, int B,
                        int H, int W, int Ho, int Wo, const unsigned* amax_x, hipStream_t s);
void launch_stem_wgrad_h3(const float* xpad, const float* g, float* ws /*[chunks][64*147]*/, int B, int H, int W, int Ho,
                          int Wo, int chunks, const unsigned* amax_g, const unsigned* amax_x, hipStream_t s);

void launch_maxpool_fwd(const float* x, float* y, uint8_t* idx, int B, int H, int W, int C, int Ho,
                        int Wo, hipStream_t s, unsigned* amax = nullptr);      // amax: absmax slot of y (f16x3 mode)
// g_x = relu_mask(x) * scatter(g_y)   (x = the ReLU output that was pooled: bit 7 of idx = "the window's maximum is > 0",
// i.e. the ReLU mask of the one input pixel the gradient goes to -- the backward pass does not read x)
void launch_maxpool_bwd(const float* gy, const uint8_t* idx, float* gx, int B, int H,
                        int W, int C, int Ho, int Wo, hipStream_t s, unsigned* amax = nullptr);      // amax: absmax slot of gx

// Bilinear resize tables (host-built, PyTorch's index/weight rule) live in device memory:
struct ResizeTab {
  int in, out;
  const int* i0;      // [out]
  const int* i1;      // [out]
  const float* lam;   // [out] weight of i1
  const int* lo;      // [in]  first output index touching input i
  const int* hi;      // [in]  last  output index touching input i (inclusive)
};
void launch_resize_fwd(const float* x, int ldx, float* y, int ldy, int B, int C, ResizeTab th,
                       ResizeTab tw, hipStream_t s);
// gx = resize_backward(gy), zero where the ReLU mask byte's bit is clear (m8 / ldm8 as ConvArgs::mask8; C % 4 == 0 only --
// the 1-channel form takes no mask)
void launch_resize_bwd(const float* gy, int ldgy, float* gx, int ldgx, const uint8_t* m8, int ldm8,
                       int B, int C, ResizeTab th, ResizeTab tw, hipStream_t s, unsigned* amax = nullptr);   // amax: absmax slot of gx

// ASPP image-pooling branch
void launch_colsum(const float* x, int ldx, float* out /*[B][C]*/, int B, int P, int C, float alpha,
                   float* scratch, hipStream_t s);
// y[b][n] = relu(a[n]*sum_k W[n][k]*v[b][k] + b[n])
void launch_gemv_fwd(const float* W, const float* v, const float* a, const float* b, float* y, int B,
                     int N, int K, hipStream_t s);
// gv[b][k] = sum_n gp[b][n]*a[n]*W[n][k] ;  dW[n][k] = sum_b gp[b][n]*v[b][k]  (gv may be nullptr: dW only)
void launch_gemv_bwd(const float* W, const float* v, const float* gp, const float* a, float* gv,
                     float* dW, int B, int N, int K, hipStream_t s);
void launch_bcast_pixels(const float* v /*[B][C]*/, float* y, int ldy, int B, int P, int C, float alpha,
                         hipStream_t s, uint8_t* mask8_out = nullptr, int ldm8 = 0);   // mask8_out: (value > 0) bytes, see ConvArgs

// classifier 1x1 conv with Cout = 1 (+bias) and its backward
void launch_last_fwd(const float* x, const float* w, const float* bias, float* y, int64_t P, int C,
                     hipStream_t s);
void launch_last_bwd(const float* x, const float* w, const float* g, float* gx, float* ws_dw,
                     int64_t P, int C, int chunks, hipStream_t s);
int last_bwd_chunks(int64_t P);

// The device losses.  `ignore`: null, or a host pointer to the void label (finite, outside [0, 1]): a pixel with gt == *ignore is in no
// sum, count or sort and its gradient is +0; an empty valid set gives loss 0; without a void pixel the result has the bits of
// the launch without a label (each kernel is one `template <bool VOID>` source, the label compiled out of the plain instance).
// launch_loss, the whole batch flattened, sums in a fixed order through `partial` (LOSS_PARTIAL_FLOATS floats): kind 0 BCE-with-
// logits mean (gradient fused into the loss pass; with a label a third launch, 1 / |V| being known only after the count),
// 1 dice, 2 BCE - log(1 - dice), 3 class-balanced BCE (sums and counts over the valid pixels, the trailing divisions by n).
constexpr int LOSS_BLOCKS = 1024;                 // cap of the partial grids
// partial: [0, LOSS_SCAL) per-block sums (up to a float4 each), 16 scalars of the final kernel, per-block valid counts
constexpr int LOSS_SCAL = 4 * LOSS_BLOCKS, LOSS_CNT = LOSS_SCAL + 16, LOSS_PARTIAL_FLOATS = LOSS_CNT + LOSS_BLOCKS;
void launch_loss(int kind, const float* logits, const float* gt, float* dlogits, float* loss, float* partial, int64_t n,
                 const float* ignore, hipStream_t s);
// Lovasz hinge (lovasz_kernels.hip; loss_lovasz.py:78-111): `images` sets of n_per_image pixels, the loss their mean and each
// gradient scaled by 1 / images -- or, with `flat`, the whole batch as one set.  A per-image stable radix sort of the
// positive errors, a scan of the label bits and a scatter of the gradient; bit-reproducible.  The void pixels are dropped
// before the ranking (flatten_binary_scores, loss_lovasz.py:114-126).  scratch: lovasz_scratch_floats
// (n_per_image * images, images) floats; n_per_image * images < 2^31.
int64_t lovasz_scratch_floats(int64_t n_total, int max_images);
void launch_lovasz(const float* logits, const float* gt, float* dlogits, float* loss, float* scratch, int64_t n_per_image,
                   int images, int flat, const float* ignore, hipStream_t s);
// Bootstrapped BCE (bootstrap_kernels.hip): `sets` sets of n_per_set pixels; per set the k = max(1, (|V| * q + 32768) >> 16)
// valid pixels with the largest keys -x * (2 * (t >= .5) - 1) are kept (ties at the threshold share the remaining slots
// with weight r / T), their BCE terms summed and divided by k; the loss is the mean over the sets, each gradient scaled by
// 1 / (k * sets) and exactly +0 at a dropped or void pixel.  An exact three-pass radix select (11 + 11 + 10 bits) on integer
// histograms, fixed-order float sums: bit-reproducible.  q in [1, 65536]; n_per_set < 2^31; scratch:
// bootstrap_scratch_floats(sets) floats, zeroed by the call itself.
constexpr int BOOTSTRAP_BLOCKS = 256;             // cap of the grid per set (256 threads each)
int64_t bootstrap_scratch_floats(int max_sets);
void launch_bootstrap_bce(const float* logits, const float* gt, float* dlogits, float* loss, float* scratch, int64_t n_per_set,
                          int sets, int q, const float* ignore, hipStream_t s);
// Soft boundary-F loss (boundary_kernels.hip; the definition: include/eosvos.h at EOSVOS_LOSS_BOUNDARY_F): `images` maps of
// H x W pixels, radius in [1, 16]; the loss is the mean over the images of 1 - BF, the gradient goes to dlogits.  `add`: loss and
// dlogits already hold the cross-entropy term of the combined kind and are added to.  No atomics, fixed-order sums: bit-
// reproducible.  scratch: boundary_scratch_floats(images * H * W, images) floats, every word written before it is read.
constexpr int BOUNDARY_BLOCKS = 1024;            // cap of the grid per image (256 threads each)
int64_t boundary_scratch_floats(int64_t n_total, int max_images);
void launch_boundary_f(const float* logits, const float* gt, float* dlogits, float* loss, float* scratch, int H, int W, int images,
                       int radius, int add, const float* ignore, hipStream_t s);
// Distance-weighted surface loss (surface_kernels.hip; the definition: include/eosvos.h at EOSVOS_LOSS_SURFACE): `images` maps
// of H x W pixels (H, W <= 4096, images <= 65535), cap in [1, 4095].  No atomics, fixed-order sums: bit-reproducible.  Every
// word of g, c and the partials that a launch reads is written by a launch before it.
//   launch_surface_distance  2 launches: c [image][H][W] int32 = min(D^2 to the other class, cap^2 + 1), 0 at void pixels;
//                            g: [image][H][W] 32-bit scratch, which c may alias
//   launch_surface_weights   1 launch: w = (c > cap^2 ? cap : sqrt(c)) / cap over n elements
//   launch_surface_loss      2 launches, 3 with dlogits: the mean over the images of sum_V w e / |V|, and its gradient;
//                            partial: images * (2 * SURFACE_BLOCKS + 1) words
//   launch_surface           all of it on one scratch of surface_scratch_floats(images * H * W, images) words: c over g, then
//                            the partials
constexpr int SURFACE_BLOCKS = 256;              // cap of the partial grid per image (256 threads each)
int64_t surface_scratch_floats(int64_t n_total, int max_images);
void launch_surface_distance(const float* gt, int images, int H, int W, int cap, const float* ignore, uint32_t* g, int32_t* c,
                             hipStream_t s);
void launch_surface_weights(const int32_t* c, float* w, int64_t n, int cap, hipStream_t s);
void launch_surface_loss(const float* logits, const float* gt, const int32_t* c, float* dlogits, float* loss, float* partial, int H,
                         int W, int images, int cap, const float* ignore, hipStream_t s);
void launch_surface(const float* logits, const float* gt, float* dlogits, float* loss, float* scratch, int H, int W, int images,
                    int cap, const float* ignore, hipStream_t s);
// Topology-aware centreline loss (cldice_kernels.hip; the definition: include/eosvos.h at EOSVOS_LOSS_CLDICE): `images` maps of
// H x W pixels (H, W <= 4096, images <= 65535), depth in [1, CLDICE_MAX_DEPTH].  No atomics, fixed-order sums, exact selections:
// bit-reproducible.  Every word of the scratch that a launch reads is written by a launch of the same call before it.
//   launch_cldice            3 depth + 8 launches (2 depth + 5 without dlogits, which may be null): the mean over the images of
//                            1 - 2 Tp Ts / (Tp + Ts), and its gradient; scratch: cldice_scratch_floats(images * H * W, images,
//                            depth) words, 6 (depth + 1) + 24 bytes per pixel and the partials, 8-byte aligned
//   launch_cldice_skeleton   2 depth + 3 launches: out [image][H][W] = the soft skeleton S of maps in [0, 1], 0 where `masks`
//                            (null: the maps themselves) hold the void label; scratch: two planes
constexpr int CLDICE_MAX_DEPTH = 16;
constexpr int CLDICE_BLOCKS = 1024;              // cap of the grid per image (256 threads each; more pixels: grid-stride)
int64_t cldice_scratch_floats(int64_t n_total, int max_images, int depth);
int64_t cldice_skeleton_scratch_floats(int64_t n_total);
void launch_cldice(const float* logits, const float* gt, float* dlogits, float* loss, float* scratch, int H, int W, int images,
                   int depth, const float* ignore, hipStream_t s);
void launch_cldice_skeleton(const float* maps, const float* masks, float* out, float* scratch, int H, int W, int images, int depth,
                            const float* ignore, hipStream_t s);
// Weighted sum of n_terms (1 .. EOSVOS_LOSS_MAX_TERMS) evaluated losses (misc_kernels.hip; the rule: include/eosvos.h at
// eosvos_set_loss_sum): out[i] = w0 * g0[i] (+ w1 * g1[i] ...) over n elements, *loss the same expression of vals[0 .. n_terms),
// which are copied unweighted to terms[0 .. n_terms).  grads / weights: host arrays; vals, out, loss, terms: device.  Every
// product and sum is rounded on its own (no fused multiply-add); one launch, no atomics; `out` may be unaligned.
void launch_loss_sum(int n_terms, const float* const* grads, const float* weights, const float* vals, float* out, float* loss,
                     float* terms, int64_t n, hipStream_t s);
// targets = 1 where probs >= hi, 0 where probs < lo, `ignore` between, for n_frames maps of n_pix; n_pos[frame] (zeroed by the
// caller) += the frame's number of 1s
void launch_propagation_targets(const float* probs, float* targets, int* n_pos, int n_frames, int64_t n_pix, float lo, float hi,
                                float ignore, hipStream_t s);
void launch_sigmoid(const float* x, float* y, int64_t n, hipStream_t s);
// test-time augmentation: acc (B, H, W) = (first ? 0 : acc) + weight * sigmoid(bilinear_{align_corners=False}(unmirror(logits (B, h, w))))
void launch_tta_accumulate(const float* logits, float* acc, int B, int h, int w, int H, int W, int mirror, float weight,
                           int first, hipStream_t s);
void launch_merge_labels(const float* probs, int n_obj, int64_t n_pix, uint8_t* labels, hipStream_t s);
// cv2.warpAffine (+ optional horizontal flip of the source) of C planes; tables = adelta[W] bdelta[W] X0[H] Y0[H]
void launch_warp_affine(const float* src, float* dst, int C, int H, int W, const double* inv_matrix, int round_delta,
                        const float* ctab, int cubic, int flip, int* nonzero, hipStream_t s);
// DAVIS counts (metrics_kernels.hip) of `frames` uint8 label-map pairs: counts [frames][n_obj][6] int64, zeroed by the caller,
// receive atomic sums; bmp / bmg: frames * n_obj * H * ceil(W/64) words each.  W <= 4096, r <= 63, 1 <= n_obj <= 255
void launch_davis_counts(const uint8_t* pred, const uint8_t* gt, int frames, int H, int W, int n_obj, int r,
                         unsigned long long* bmp, unsigned long long* bmg, int64_t* counts, hipStream_t s);
// Locally connected dense CRF over the merged probabilities (crf_kernels.hip; the model: include/eosvos.h, eosvos_crf_labels).
// Planes are [frame][label][H][W] fp32 with n_lab = n_obj + 1 labels, label maps [frame][H][W].
// launch_crf_prepare: probs [frame][n_obj][n_pix] -> q0 = Q^0 and u = -log Q^0 (both may be null: nothing of the model is
// computed), labels (may be null) = merge_labels_kernel's decision on probs.
// launch_crf_iteration: one mean-field update q_out = softmax(-unary + messages(q_in)), q_in != q_out; labels (may be null)
// receives the decision on q_out.  1 <= r <= 7, 1 <= d <= 4, r * d <= 16, n_frames <= 65535; `tab` from crf_fill_tables.
#define CRF_MAX_SIDE 15      // 2 * 7 + 1 offsets per axis
struct CrfTables { float wa[CRF_MAX_SIDE * CRF_MAX_SIDE], ws[CRF_MAX_SIDE * CRF_MAX_SIDE]; };   // exp(-|delta|^2 / (2 theta^2)), [(dy + r) * (2r + 1) + dx + r]
void crf_fill_tables(CrfTables& tab, int r, int d, float theta_alpha, float theta_gamma);
void launch_crf_prepare(const float* probs, int n_frames, int n_obj, int64_t n_pix, float* q0, float* u, uint8_t* labels,
                        hipStream_t s);
void launch_crf_iteration(const float* images, const float* unary, const float* q_in, float* q_out, uint8_t* labels,
                          int n_frames, int n_lab, int H, int W, int r, int d, float w_a, float w_s, float theta_beta,
                          const CrfTables& tab, hipStream_t s);
// Image-aware pairwise (Potts) loss (potts_kernels.hip; the rule: include/eosvos.h at EOSVOS_LOSS_POTTS): `images` maps of
// H x W logits (H, W <= 4096, images <= 65535) against their frames, the CRF's window limits (1 <= r <= 7, 1 <= d <= 4,
// r * d <= 16), sigma_xy, sigma_rgb finite and > 0.  `frames`: with pad > 0 fp32 [image][H + 2 pad][W + 2 pad][3] (the
// engine's copy of the last forward's frames), with pad 0 fp32 [image][3][H][W]; both give the same bits.  Three launches
// (two without dlogits, which may be null), no atomics, fixed-order sums: bit-reproducible.  scratch: potts_scratch_floats
// words (two partials per 32 x 8 tile and one scale per image), all written before they are read.
struct PottsTable { float w[CRF_MAX_SIDE * CRF_MAX_SIDE]; };    // exp(-d^2 (dy^2 + dx^2) / (2 sigma_xy^2)), [(dy + r) * (2r + 1) + dx + r]
void potts_fill_table(PottsTable& tab, int r, int d, float sigma_xy);
int64_t potts_scratch_floats(int H, int W, int images);
void launch_potts(const float* logits, const float* frames, int pad, float* dlogits, float* loss, float* scratch, int H, int W,
                  int images, int r, int d, float sigma_xy, float sigma_rgb, hipStream_t s);

// Connected components of uint8 label maps and the component filter (ccl_kernels.hip; the rules: include/eosvos.h,
// eosvos_label_components / eosvos_filter_components).  Maps are [frame][H][W]; H, W <= 4096, H * W < 2^24, frames <= 65535.
// launch_ccl_label: ids [frame][H * W] = 1 + the smallest frame-local pixel index of the pixel's component (0: background);
// parent / tarea: scratch of the same size; area (may be null; zeroed by the caller) receives at [root] the pixel count.
// launch_ccl_presence: pres[256] (zeroed by the caller) = 1 for every non-zero value of `map`.
// launch_ccl_gate (one frame): cand [H * W] (zeroed by the caller) = 1 at the root of every component with a pixel within
// Chebyshev distance gate <= 63 of a pixel of R with its label, for the labels R contains (pres).
// launch_ccl_filter: the area rules over the candidates (pres null: every component is one; pres is per launch, so with pres
// the launch takes one frame) -> out, pres_out [frame][256] and removed [frame] (both zeroed by the caller); best
// [frame][256] is zeroed scratch.  keep_all: the frames are copied unchanged (pres_out is still written).
void launch_ccl_label(const uint8_t* labels, int n_frames, int H, int W, int connectivity, int* parent, int* tarea, int* ids,
                      int* area, hipStream_t s);
void launch_ccl_presence(const uint8_t* map, int n_pix, uint8_t* pres, hipStream_t s);
void launch_ccl_gate(const uint8_t* labels, const uint8_t* R, const uint8_t* pres, const int* ids, int H, int W, int gate,
                     uint8_t* cand, hipStream_t s);
void launch_ccl_filter(const uint8_t* labels, const int* ids, const int* area, const uint8_t* pres, const uint8_t* cand,
                       int keep_all, int n_frames, int n_pix, int min_area, unsigned rel_q16, int largest_only,
                       unsigned long long* best, uint8_t* out, uint8_t* pres_out, unsigned long long* removed, hipStream_t s);

// Hole filling of uint8 label maps (ccl_kernels.hip; the rules: include/eosvos.h, eosvos_fill_holes).
// launch_ccl_label_zero: launch_ccl_label over the pixels that hold 0 (one label; object pixels are its background): ids =
// 1 + root of a zero pixel's background component, area[root] = its pixel count.  Pass the BACKGROUND's connectivity.
// launch_hole_scan: rec [frame][H * W] (per root: border bit, smallest and largest non-zero neighbour label) and hist
// [frame][256] (pixels per label), both zeroed by the caller; `connectivity` is the OBJECTS' (4: corner neighbours count).
// launch_hole_overlap (one frame): cnt [H * W] (zeroed by the caller) at [root] = pixels of the hole that hold its label in R,
// for holes that are candidates of a label R contains (pres) and pass the size rule.
// launch_hole_apply: the size rule and, with pres (per launch, so one frame), the overlap rule -> out, pres_out [frame][256]
// and filled [frame] (both zeroed by the caller).  keep_all: the frames are copied unchanged (pres_out is still written).
void launch_ccl_label_zero(const uint8_t* labels, int n_frames, int H, int W, int connectivity, int* parent, int* tarea, int* ids,
                           int* area, hipStream_t s);
void launch_hole_scan(const uint8_t* labels, const int* ids, int n_frames, int H, int W, int connectivity, unsigned* rec,
                      unsigned* hist, hipStream_t s);
void launch_hole_overlap(const uint8_t* labels, const uint8_t* R, const uint8_t* pres, const int* ids, const int* area,
                         const unsigned* rec, const unsigned* hist, int n_pix, int max_area, unsigned rel_q16, unsigned* cnt,
                         hipStream_t s);
void launch_hole_apply(const uint8_t* labels, const int* ids, const int* area, const unsigned* rec, const unsigned* hist,
                       const unsigned* cnt, const uint8_t* pres, int keep_all, int n_frames, int n_pix, int max_area,
                       unsigned rel_q16, unsigned overlap_q16, uint8_t* out, uint8_t* pres_out, unsigned long long* filled,
                       hipStream_t s);

// SLIC superpixels of uint8 frames and the superpixel vote on uint8 label maps (slic_kernels.hip; the rules: include/eosvos.h,
// eosvos_superpixels / eosvos_snap_labels).  rgb [frame][3][H][W]; K = ceil(H / S) * ceil(W / S) clusters per frame; centres
// [frame][K][5] (y, x, R, G, B), sums [frame][K][6] (n and the sums of y, x, R, G, B; zeroed by the caller once, kept zero by
// launch_slic_iterate), ids [frame][H * W], votes [frame][K][n_obj + 1] and changed [frame] (both zeroed by the caller).
// launch_slic_init: the centres of rule 1.  launch_slic_iterate: one assign + update (two launches).  launch_slic_last: the
// last assign -> ids; with labels (not null) also the votes.  launch_slic_apply: winner and share rule per cluster -> out and
// the pixels changed per frame; keep_all: the frames are copied unchanged.
void launch_slic_init(const uint8_t* rgb, int n_frames, int H, int W, int S, int* centres, hipStream_t s);
void launch_slic_iterate(const uint8_t* rgb, int n_frames, int H, int W, int S, int m, int* centres, unsigned* sums, hipStream_t s);
void launch_slic_last(const uint8_t* rgb, const uint8_t* labels, int n_frames, int H, int W, int S, int m, int n_obj,
                      const int* centres, int* ids, unsigned* votes, hipStream_t s);
void launch_slic_apply(const uint8_t* labels, const int* ids, const unsigned* votes, int keep_all, int n_frames, int H, int W,
                       int S, int n_obj, unsigned q16, uint8_t* out, unsigned long long* changed, hipStream_t s);

// Block motion on 8-bit luma and the warp of label maps by it (motion_kernels.hip; the rules: include/eosvos.h,
// eosvos_block_motion / eosvos_warp_labels).  rgb [frame][3][H][W], prev_rgb [3][H][W] or null; luma: n_frames + 1 planes of
// H * LW words, LW = ceil(W / 4) (plane 0: prev_rgb, plane 1 + f: frame f; padding bytes 0); mv [frame][by][bx][2] (dy, dx).
// launch_motion_luma: the planes (plane 0 only with prev_rgb).  launch_motion_search: the vectors of frames first .. n_frames - 1
// (first = 1 without prev_rgb: frame 0 is the caller's to zero).  launch_motion_warp: out(y, x) = labels(y + dy, x + dx),
// clamped to the frame.
void launch_motion_luma(const uint8_t* rgb, const uint8_t* prev_rgb, int n_frames, int H, int W, unsigned* luma, hipStream_t s);
void launch_motion_search(const unsigned* luma, int first, int n_frames, int H, int W, int block, int radius, int bias, int8_t* mv,
                          hipStream_t s);
void launch_motion_warp(const uint8_t* labels, const int8_t* mv, int n_frames, int H, int W, int block, uint8_t* out, hipStream_t s);

// Object-centred zoom pass of the inference path (zoom_kernels.hip; the rules: include/eosvos.h, eosvos_zoom_boxes ..
// eosvos_zoom_blend).  probs / pz [frame][H][W] fp32, boxes [frame][5] int32 (valid, y0, x0, bh, bw), read from device memory
// and clamped into the frame by every consumer.  launch_zoom_boxes: two launches; rec [frame][8] int32 scratch, ZEROED BY THE
// CALLER on the same stream (the bounds are kept as maxima of H - 1 - y, y, W - 1 - x, x, and the count).  H, W <= 4096,
// frames <= 65535.  launch_zoom_crop: out = the frames cut to their boxes at H x W (invalid: copied).  launch_zoom_accumulate:
// pz inside valid boxes (+)= weight * sigmoid(bilinear(unmirror(logits)) -> bh x bw).  launch_zoom_blend: probs = probs +
// (weight * ramp) * (pz - probs) inside valid boxes, in place.
void launch_zoom_boxes(const float* probs, int n_frames, int H, int W, float threshold, int min_pixels, int margin_q16, int margin_px,
                       int min_zoom_q16, int max_zoom_q16, int* rec, int* boxes, hipStream_t s);
void launch_zoom_crop(const float* frames, const int* boxes, int B, int C, int H, int W, float* out, hipStream_t s);
void launch_zoom_accumulate(const float* logits, const int* boxes, int B, int H, int W, int mirror, float weight, int first, float* pz,
                            hipStream_t s);
void launch_zoom_blend(const int* boxes, int B, int H, int W, float weight, int feather, const float* pz, float* probs, hipStream_t s);

// Lucid first-frame synthesis (lucid_kernels.hip; the rules: include/eosvos.h, eosvos_lucid_plate / eosvos_lucid_compose).
// frame / plate [C][H][W] fp32, mask [H][W] fp32 (object = != 0), H, W <= 4096.  launch_lucid_plate: 2 + 2 (levels - 1) small
// launches; vbuf / kbuf hold `floats` floats and `bytes` bytes of lucid_scratch, every element a call reads is written by it
// first.  launch_lucid_compose: ONE launch for n_samples <= LUCID_MAX_SAMPLES; flips [n] and matrices [n][12] (the inverse
// background matrix, then the inverse object matrix) are HOST arrays copied into the launch's arguments; images
// [n][C][H][W], labels [n][H][W]; counts [n] int32 on the device, ZEROED BY THE CALLER on the same stream.
#define LUCID_MAX_SAMPLES 16
void lucid_scratch(int C, int H, int W, size_t* floats, size_t* bytes);
void launch_lucid_plate(const float* frame, const float* mask, int C, int H, int W, int dilate, float* plate, float* vbuf,
                        uint8_t* kbuf, hipStream_t s);
void launch_lucid_compose(const float* frame, const float* mask, const float* plate, int C, int H, int W, int n_samples,
                          const int* flips, const double* matrices, const float* ctab, float* images, float* labels, int* counts,
                          hipStream_t s);
// launch_lucid_layers (rules L2-L5 of eosvos_lucid_compose_layers): ONE launch for n_samples <= LUCID_LAYERS_MAX_SAMPLES, each
// with n_layers[i] in [1, LUCID_MAX_LAYERS] layers, back to front.  ids [H][W] uint8 (0 = background); flips [n], n_layers [n],
// layer_ids [n][8] and matrices [n][9][6] (Bi, then Oi_0 .. Oi_7) are HOST arrays copied into the launch's arguments (8 samples
// of 9 matrices are 3.5 KB of HIP's 4 KB); labels = 1.f where the visible layer carries target_id; ids_out [n][H][W] may be
// null; counts [n][8] int32 on the device, ZEROED BY THE CALLER on the same stream.
#define LUCID_MAX_LAYERS 8
#define LUCID_LAYERS_MAX_SAMPLES 8
void launch_lucid_layers(const float* frame, const uint8_t* ids, const float* plate, int C, int H, int W, int n_samples,
                         const int* flips, const int* n_layers, const uint8_t* layer_ids, const double* matrices, int target_id,
                         const float* ctab, float* images, float* labels, uint8_t* ids_out, int* counts, hipStream_t s);

// Capped squared distance transform and the distance-gated targets of online adaptation (edt_kernels.hip; the rules:
// include/eosvos.h, eosvos_distance_sq / eosvos_adapt_targets).  probs / anchors / targets [frame][H][W] fp32, H, W <= 4096,
// frames <= 65535, limits in [1, 4095].  g: [frame][H][W] 16-bit scratch, eroded: [frame][H][W] byte scratch (erode > 0 only);
// every word of both that a launch reads is written by the launch before it.  launch_edt_distance: 2 launches, out [frame][H][W]
// int32 = min(D^2, limit^2 + 1).  launch_edt_targets: 2 launches (4 with erode > 0); count_e / n_pos [frame] int32 on the
// device, ZEROED BY THE CALLER on the same stream.
void launch_edt_distance(const float* probs, int n_frames, int H, int W, float threshold, int invert, int limit, uint16_t* g,
                         int32_t* out, hipStream_t s);
void launch_edt_targets(const float* probs, const float* anchors, int n_frames, int H, int W, float lo, float hi, float anchor_thr,
                        int erode, int neg_dist, float ignore, uint16_t* g, uint8_t* eroded, int* count_e, int* n_pos, float* targets,
                        hipStream_t s);

// theta' = theta - lr[cout]*g, g = rowscale[cout] * sum_z ws[z][...]; optional gsum += g; g_out = g
void launch_sgd_update(float* w, const float* ws, int splits, int64_t slab, const float* rowscale,
                       const float* lr, float* gsum, float* gout, int64_t rowlen, int64_t n,
                       hipStream_t s);
// GroupNorm(16, C), frozen affine.  forward: stats + y = relu?(gn(z) (+res)); backward: z <- dL/dz.
// `amax_y` / `amax_dz`: absmax slot of the tensor the pass writes (f16x3 mode), or null.  `partial`: gn_partial_floats(B) floats.
// `m8`: ReLU mask bytes of y (one per 4 channels, row pitch ldm8 bytes), written when `relu`.
void launch_gn_forward(const float* z, int ldz, const float* gamma, const float* beta, const float* res, int ldres,
                       float* y, int ldy, float* stats, float* partial, int B, int P, int C, float eps, int relu,
                       hipStream_t s, unsigned* amax_y = nullptr, uint8_t* m8 = nullptr, int ldm8 = 0);
void launch_gn_backward(float* z, int ldz, const float* g, int ldg, const float* gamma, const float* stats,
                        float* partial, int B, int P, int C, hipStream_t s, unsigned* amax_dz = nullptr);
int gn_partial_floats(int B);
// Whole-network update in one launch: per-layer table over one slab arena.
struct UpdEntry {
  long w_off;      // offset of the tensor (weight [+ bias]) in the parameter / gsum / gout arenas
  long ws_off;     // offset of its first slab in the slab arena (multiple of 4 floats)
  long slab;       // floats per slab
  int splits;      // number of slabs to sum
  int rowlen;      // elements per output channel (per-neuron lr / norm-scale granularity)
  int n;           // elements
  int lr_off;      // offset of its per-neuron learning rates
  int norm_off;    // offset of its frozen-norm scale, -1 if none
  int blk0;        // first workgroup of this entry (UPD_CHUNKS x 1024 elements per workgroup)
  int amax_idx;    // f16x3 mode: index of the tensor's absmax word in `amax_w` (the conv index), -1: none
};
#define UPD_CHUNKS 1      // 1024-element chunks per workgroup of the update kernel (UpdEntry::blk0 counts those)
void launch_sgd_update_all(const UpdEntry* tab, int nent, int nblocks, float* W, const float* ws, const float* na,
                           const float* lr, const float* lr_elem, float* gsum, float* gout, hipStream_t s,
                           unsigned* amax_w = nullptr);   // amax_w: max|w| of the updated weights, per UpdEntry::amax_idx
// learning-rate hierarchy (meta_optim.py:27-67): stored lr state -> effective per-neuron lr, and back
void launch_lr_expand(const float* store, const int* row_tensor, float* lr, int nlr, int level, int use_log,
                      hipStream_t s);
void launch_exp_inplace(float* p, int64_t n, hipStream_t s);
void launch_lr_grad_reduce(const float* g, const float* lr, const int* row0, float* out, int ngroups, int use_log,
                           hipStream_t s);
void launch_lr_grad_neuron(const float* g, const float* lr, float* out, int n, int use_log, hipStream_t s);
void launch_meta_lr_grad_elem(const float* gsum, const float* G, const float* lr_elem, float* out, int64_t n,
                              hipStream_t s);
// g_lr[c] += -sum_row(gsum*G) ;  (G itself is exported by launch_ohwi_to_oihw with add=1)
void launch_meta_lr_grad_all(const float* gsum, const float* G, float* glr, const long* rbase, const int* rlen, int rows,
                             float weight, hipStream_t s);      // every tensor's rows in one launch
void launch_ohwi_to_oihw_all(const float* src, float* dst, const long* toff, const int2* tit, int nent, int64_t n, float alpha,
                             int add, hipStream_t s);           // the whole arena in one launch
void launch_meta_lr_grad(const float* gsum, const float* G, float* glr, int rows, int64_t rowlen, float weight,
                         hipStream_t s);
void launch_radam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float wd,
                  float beta1, float beta2, float eps, float step_size, int use_denom,
                  float grad_scale, float grad_clip, hipStream_t s);
void launch_clamp(float* p, int64_t n, float lo, float hi, hipStream_t s);
// Whole outer step of meta-training in ONE launch over the flat learned state [lr state | model_init (OIHW)]
// (train_meta.py:361-373, radam.py:28-94, meta_optim.py:116-133): g = clip(grad * scale); RAdam with the per-group lr /
// weight decay; lr-state clamp; grad <- 0; and the engine's copies written on the way out -- the effective per-neuron lr
// and the init / current weights in the engine layout O,(kh,kw),I.  Tensor entries of the init part:
struct OuterEnt {
  long off;        // flat offset of the tensor (weight [+ bias]) = its offset in the engine arena
  int O, I, T;     // OIHW dims (T = kh * kw)
  int n;           // elements incl. the bias that follows the weight
  int blk0;        // first workgroup of this entry (1024 elements per workgroup), counted after the lr-state workgroups
};
struct OuterHyper {
  long n_lr, frozen_lr, frozen_param;     // lr-state elements; leading elements of each part whose group lr is 0 (freeze_encoder)
  float lr_lr, init_lr, wd, beta1, beta2, eps, step_size, grad_scale, grad_clip, lr_lo, lr_hi;
  int use_denom, use_log;
};
void launch_outer_step(const OuterEnt* tab, int nent, int lr_blocks, int nblocks, float* state, float* grad, float* m, float* v,
                       float* Winit, float* Wp, float* lr_eff, const OuterHyper& h, hipStream_t s);

}  // namespace eosvos
