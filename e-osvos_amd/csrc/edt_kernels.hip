// Capped squared Euclidean distance transform and the distance-gated pseudo-labels of online adaptation, for gfx950.  The rules
// are stated in include/eosvos.h (eosvos_distance_sq, eosvos_adapt_targets) and restated in numpy by eosvos_amd/adapt.py
// (distance_sq_host, targets_host).  Integer arithmetic only; the two passes of the separable transform:
//
//   edt_column_kernel   one thread per column (coalesced across x), the frame in grid.y.  A down sweep and an up sweep leave
//                       g(y, x) = the vertical distance to the nearest seed of the column, capped at L + 1 <= 4096, as 16-bit
//                       words.  Each sweep loads 16 rows at a time before it walks through them: the running distance is the
//                       only dependence, the memory latency is paid once per 16 rows.  The seed predicate is a template
//                       parameter: p >= t, !(p >= t) (a NaN is never a seed of the first and always one of the second), or a
//                       byte != 0.  With COUNT the frame's seeds are counted: a wave reduction, then one integer atomic per
//                       wave.
//   edt_row_kernel      one workgroup per row, the frame in grid.y.  The row's min(g^2, L^2 + 1) is staged in LDS (W words);
//                       pixel x takes best = g2[x], then for k = 1, 2, .. while k <= L and k^2 < best:
//                       best = min(best, k^2 + g2[x - k], k^2 + g2[x + k]), taps outside the row skipped.  k^2 + g2 >= k^2, so
//                       nothing beyond the exit can lower best: the result is min(D^2, L^2 + 1) exactly, and a pixel near a seed
//                       stops early.  The epilogue is a template parameter: the int32 distances; the eroded mask bytes
//                       (best > L^2) and their count; or the targets and the count of 1s straight from the frame's
//                       probabilities, so the distances of the adaptation path never reach memory.
//
// Every word of g and of the mask a launch reads was written by the launch before it on the same stream; the count words are
// zeroed by the caller's memset on that stream.  Integer atomics for the two counts only (integer adds commute).  No launch is
// cooperative, no workgroup waits for another, one writer per element.  Vector stores only.
#include "kernels.h"

namespace eosvos {
namespace {
enum { EDT_SEED_GE = 0, EDT_SEED_NOT_GE = 1, EDT_SEED_BYTE = 2 };
enum { EDT_OUT_DIST = 0, EDT_OUT_ERODE = 1, EDT_OUT_TARGETS = 2 };
constexpr int EDT_ROWS = 16;                         // rows of a column in flight per thread

template <int SEED>
__device__ __forceinline__ bool edt_seed(const void* __restrict__ src, size_t i, float thr) {
  if (SEED == EDT_SEED_BYTE) return ((const uint8_t*)src)[i] != 0;
  const bool ge = ((const float*)src)[i] >= thr;
  return SEED == EDT_SEED_GE ? ge : !ge;
}

__device__ __forceinline__ int edt_wave_sum(int c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}

// grid (ceil(W / 256), frames), block 256.  cap = L + 1.  No thread leaves before the wave reduction.
template <int SEED, bool COUNT>
__global__ __launch_bounds__(256) void edt_column_kernel(const void* __restrict__ src, float thr, int H, int W, int cap,
                                                          uint16_t* __restrict__ g, int* __restrict__ count) {
  const int x = (int)blockIdx.x * 256 + (int)threadIdx.x;
  const size_t base = (size_t)blockIdx.y * H * W;
  int seeds = 0;
  if (x < W) {
    // EDT_ROWS rows at a time, their loads issued together before the running distance walks through them; the rows that do
    // not fill a batch go one by one
    int d = cap, y = 0;
    auto down_step = [&](size_t i, bool s) {
      d = s ? 0 : min(d + 1, cap);
      g[i] = (uint16_t)d;
      seeds += s ? 1 : 0;
    };
    for (; y + EDT_ROWS <= H; y += EDT_ROWS) {
      const size_t i0 = base + (size_t)y * W + x;
      bool s[EDT_ROWS];
#pragma unroll
      for (int r = 0; r < EDT_ROWS; ++r) s[r] = edt_seed<SEED>(src, i0 + (size_t)r * W, thr);
#pragma unroll
      for (int r = 0; r < EDT_ROWS; ++r) down_step(i0 + (size_t)r * W, s[r]);
    }
    for (; y < H; ++y) down_step(base + (size_t)y * W + x, edt_seed<SEED>(src, base + (size_t)y * W + x, thr));
    d = cap;
    y = H - 1;
    auto up_step = [&](size_t i, int down) {         // down: this thread's own store of the sweep above
      d = down == 0 ? 0 : min(d + 1, cap);
      if (d < down) g[i] = (uint16_t)d;
    };
    for (; y - EDT_ROWS + 1 >= 0; y -= EDT_ROWS) {
      const size_t i0 = base + (size_t)y * W + x;
      int down[EDT_ROWS];
#pragma unroll
      for (int r = 0; r < EDT_ROWS; ++r) down[r] = g[i0 - (size_t)r * W];
#pragma unroll
      for (int r = 0; r < EDT_ROWS; ++r) up_step(i0 - (size_t)r * W, down[r]);
    }
    for (; y >= 0; --y) up_step(base + (size_t)y * W + x, g[base + (size_t)y * W + x]);
  }
  if (COUNT) {
    seeds = edt_wave_sum(seeds);
    if ((threadIdx.x & 63) == 0 && seeds) atomicAdd(count + blockIdx.y, seeds);
  }
}

// grid (H, frames), block 256, W * 4 bytes of dynamic LDS.  The x loop has the same trip count for every thread of the
// workgroup: no thread leaves before the wave reduction.
//   EDT_OUT_DIST     dist = min(D^2, L^2 + 1)
//   EDT_OUT_ERODE    mask = (best > L^2), count[frame] += the row's mask pixels
//   EDT_OUT_TARGETS  count[frame] is READ (the seeds of this transform: 0 = no anchor): the band's target of p, overridden by 0
//                    where best > L^2 if the frame has an anchor; n_pos[frame] += the row's 1s if it has one
template <int OUT>
__global__ __launch_bounds__(256) void edt_row_kernel(const uint16_t* __restrict__ g, int H, int W, int L, int32_t* __restrict__ dist,
                                                       uint8_t* __restrict__ mask, int* __restrict__ count,
                                                       const float* __restrict__ probs, float lo, float hi, float ign,
                                                       float* __restrict__ targets, int* __restrict__ n_pos) {
  extern __shared__ int edt_g2[];
  const int f = blockIdx.y;
  const size_t base = ((size_t)f * H + blockIdx.x) * W;
  const int l2 = L * L, cap2 = l2 + 1;
  for (int x = threadIdx.x; x < W; x += 256) {
    const int v = g[base + x];                       // <= 4096: v * v <= 2^24
    edt_g2[x] = min(v * v, cap2);
  }
  __syncthreads();
  const bool anchored = OUT == EDT_OUT_TARGETS ? count[f] != 0 : true;
  int c = 0;
  for (int x0 = 0; x0 < W; x0 += 256) {
    const int x = x0 + (int)threadIdx.x;
    if (x < W) {
      int best = edt_g2[x];
      const int kmax = min(L, max(x, W - 1 - x));    // beyond it both taps are outside the row
      for (int k = 1; k <= kmax && k * k < best; ++k) {
        const int kk = k * k;                        // kk + g2 <= 4095^2 + 4095^2 + 1 < 2^31
        if (x - k >= 0) best = min(best, kk + edt_g2[x - k]);
        if (x + k < W) best = min(best, kk + edt_g2[x + k]);
      }
      if (OUT == EDT_OUT_DIST) {
        dist[base + x] = best;
      } else if (OUT == EDT_OUT_ERODE) {
        const bool in = best > l2;
        mask[base + x] = in ? 1 : 0;
        c += in ? 1 : 0;
      } else {
        const float p = probs[base + x];
        const bool far = anchored && best > l2;
        const bool pos = p >= hi;
        targets[base + x] = far ? 0.f : (pos ? 1.f : (p < lo ? 0.f : ign));
        c += anchored && pos && !far ? 1 : 0;
      }
    }
  }
  if (OUT != EDT_OUT_DIST) {
    c = edt_wave_sum(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd((OUT == EDT_OUT_ERODE ? count : n_pos) + f, c);
  }
}

template <int SEED, bool COUNT>
void edt_columns(const void* src, float thr, int n_frames, int H, int W, int L, uint16_t* g, int* count, hipStream_t s) {
  hipLaunchKernelGGL((edt_column_kernel<SEED, COUNT>), dim3((W + 255) / 256, n_frames), dim3(256), 0, s, src, thr, H, W, L + 1, g,
                     count);
}
}  // namespace

void launch_edt_distance(const float* probs, int n_frames, int H, int W, float threshold, int invert, int limit, uint16_t* g,
                         int32_t* out, hipStream_t s) {
  if (invert) edt_columns<EDT_SEED_NOT_GE, false>(probs, threshold, n_frames, H, W, limit, g, nullptr, s);
  else edt_columns<EDT_SEED_GE, false>(probs, threshold, n_frames, H, W, limit, g, nullptr, s);
  hipLaunchKernelGGL((edt_row_kernel<EDT_OUT_DIST>), dim3(H, n_frames), dim3(256), (size_t)W * sizeof(int), s, g, H, W, limit, out,
                     (uint8_t*)nullptr, (int*)nullptr, (const float*)nullptr, 0.f, 0.f, 0.f, (float*)nullptr, (int*)nullptr);
}

void launch_edt_targets(const float* probs, const float* anchors, int n_frames, int H, int W, float lo, float hi, float anchor_thr,
                        int erode, int neg_dist, float ignore, uint16_t* g, uint8_t* eroded, int* count_e, int* n_pos, float* targets,
                        hipStream_t s) {
  const size_t lds = (size_t)W * sizeof(int);
  if (erode > 0) {
    // rule 3: seeds = the frame's pixels outside the anchor, L = erode; E = the pixels farther than erode from all of them
    edt_columns<EDT_SEED_NOT_GE, false>(anchors, anchor_thr, n_frames, H, W, erode, g, nullptr, s);
    hipLaunchKernelGGL((edt_row_kernel<EDT_OUT_ERODE>), dim3(H, n_frames), dim3(256), lds, s, g, H, W, erode, (int32_t*)nullptr,
                       eroded, count_e, (const float*)nullptr, 0.f, 0.f, 0.f, (float*)nullptr, (int*)nullptr);
    edt_columns<EDT_SEED_BYTE, false>(eroded, 0.f, n_frames, H, W, neg_dist, g, nullptr, s);
  } else {
    edt_columns<EDT_SEED_GE, true>(anchors, anchor_thr, n_frames, H, W, neg_dist, g, count_e, s);
  }
  hipLaunchKernelGGL((edt_row_kernel<EDT_OUT_TARGETS>), dim3(H, n_frames), dim3(256), lds, s, g, H, W, neg_dist, (int32_t*)nullptr,
                     (uint8_t*)nullptr, count_e, probs, lo, hi, ignore, targets, n_pos);
}
}  // namespace eosvos
