// Distance-weighted surface loss (`surface`; the rules: include/eosvos.h at EOSVOS_LOSS_SURFACE, restated in numpy by
// eosvos_amd/surface.py), for gfx950.  The transform is the capped squared Euclidean one of edt_kernels.hip with two seed sets
// at once: ONE column pass and ONE row pass give every valid pixel its distance to the nearest valid pixel of the OTHER class.
//
//   surface_column_kernel   one thread per column (coalesced across x), the image in grid.y.  A down sweep and an up sweep
//                           carry two running distances, to the nearest foreground and to the nearest background pixel of
//                           the column, each capped at L + 1 <= 4096, and leave them as the two 16-bit halves of one 32-bit
//                           word per pixel (low: foreground, high: background).  16 rows are loaded before the running
//                           distances walk through them, as in edt_column_kernel.  A void pixel seeds neither half.
//   surface_row_kernel      one workgroup per row, the image in grid.y.  Both planes of the row are staged in LDS as
//                           min(g^2, L^2 + 1) (2 W words).  The pixel's own class is read off its word (foreground: low half
//                           0, background: high half 0, void: neither); it searches the OTHER class's plane with the early
//                           exit of edt_row_kernel and stores c = min(D^2, L^2 + 1), 0 at a void pixel.  The row is in LDS
//                           before the first store, so c may overwrite the words of g in place.
//   surface_partial_kernel  streaming: w from c (sqrtf and the division are the correctly rounded ones: the build has no
//                           fast-math flag, and hipcc's default keeps fp32 sqrt and divide correctly rounded), the error
//                           term from the logit, per workgroup the sum of w * e and the number of valid pixels.
//   surface_final_kernel    one workgroup: per image the partials in index order, |V|, the image's loss; the mean over the
//                           images; scale[image] = |V| * images for the gradient.
//   surface_grad_kernel     streaming: s * w * p (1 - p) / scale[image], +0 at a void pixel.
//   surface_weight_kernel   streaming: w from c (eosvos_surface_weights).
//
// The streaming launches move 16 bytes per lane and array when an image is a whole number of float4 and every pointer is
// 16-byte aligned, single words otherwise (a template parameter).  No atomics; every sum has a fixed order, so the result is
// bit-identical from run to run; every word a launch reads was written by a launch before it on the same stream.  No launch is
// cooperative, no workgroup waits for another, one writer per element.  Vector stores only.
#include "kernels.h"

namespace eosvos {
namespace {
constexpr int SURFACE_ROWS = 16;                     // rows of a column in flight per thread
enum { SURFACE_VOID = 0, SURFACE_FG = 1, SURFACE_BG = 2 };

template <bool VOID>
__device__ __forceinline__ int surface_class(float y, float v) {
  if (VOID && y == v) return SURFACE_VOID;
  return y >= 0.5f ? SURFACE_FG : SURFACE_BG;        // (a NaN target is background, as in the twin)
}

// grid (ceil(W / 256), images), block 256.  cap = L + 1.
template <bool VOID>
__global__ __launch_bounds__(256) void surface_column_kernel(const float* __restrict__ gt, float v, int H, int W, int cap,
                                                              uint32_t* __restrict__ g) {
  const int x = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (x >= W) return;
  const size_t base = (size_t)blockIdx.y * H * W;
  int df = cap, db = cap, y = 0;
  auto down_step = [&](size_t i, int cls) {
    df = cls == SURFACE_FG ? 0 : min(df + 1, cap);
    db = cls == SURFACE_BG ? 0 : min(db + 1, cap);
    g[i] = (uint32_t)df | ((uint32_t)db << 16);
  };
  for (; y + SURFACE_ROWS <= H; y += SURFACE_ROWS) {
    const size_t i0 = base + (size_t)y * W + x;
    int cls[SURFACE_ROWS];
#pragma unroll
    for (int r = 0; r < SURFACE_ROWS; ++r) cls[r] = surface_class<VOID>(gt[i0 + (size_t)r * W], v);
#pragma unroll
    for (int r = 0; r < SURFACE_ROWS; ++r) down_step(i0 + (size_t)r * W, cls[r]);
  }
  for (; y < H; ++y) down_step(base + (size_t)y * W + x, surface_class<VOID>(gt[base + (size_t)y * W + x], v));
  df = db = cap;
  y = H - 1;
  auto up_step = [&](size_t i, uint32_t down) {      // down: this thread's own store of the sweep above
    const int f0 = (int)(down & 0xffffu), b0 = (int)(down >> 16);
    df = f0 == 0 ? 0 : min(df + 1, cap);
    db = b0 == 0 ? 0 : min(db + 1, cap);
    const uint32_t both = (uint32_t)min(df, f0) | ((uint32_t)min(db, b0) << 16);
    if (both != down) g[i] = both;
  };
  for (; y - SURFACE_ROWS + 1 >= 0; y -= SURFACE_ROWS) {
    const size_t i0 = base + (size_t)y * W + x;
    uint32_t down[SURFACE_ROWS];
#pragma unroll
    for (int r = 0; r < SURFACE_ROWS; ++r) down[r] = g[i0 - (size_t)r * W];
#pragma unroll
    for (int r = 0; r < SURFACE_ROWS; ++r) up_step(i0 - (size_t)r * W, down[r]);
  }
  for (; y >= 0; --y) up_step(base + (size_t)y * W + x, g[base + (size_t)y * W + x]);
}

// grid (H, images), block 256, 2 * W * 4 bytes of dynamic LDS (the only LDS of the kernel).  c may be g.
__global__ __launch_bounds__(256) void surface_row_kernel(const uint32_t* g, int H, int W, int L, int32_t* c) {
  extern __shared__ __attribute__((aligned(16))) int surface_g2[];     // [2][W]: the foreground plane, the background plane
  const size_t base = ((size_t)blockIdx.y * H + blockIdx.x) * W;
  const int cap2 = L * L + 1;
  for (int x = threadIdx.x; x < W; x += 256) {
    const uint32_t both = g[base + x];
    const int f = (int)(both & 0xffffu), b = (int)(both >> 16);          // <= 4096: the squares are <= 2^24
    surface_g2[x] = min(f * f, cap2);
    surface_g2[W + x] = min(b * b, cap2);
  }
  __syncthreads();
  for (int x = threadIdx.x; x < W; x += 256) {
    const int f2 = surface_g2[x], b2 = surface_g2[W + x];
    int best = 0;
    if (f2 == 0 || b2 == 0) {                        // a valid pixel: it searches the plane of the other class
      const int* g2 = surface_g2 + (f2 == 0 ? W : 0);
      best = g2[x];
      const int kmax = min(L, max(x, W - 1 - x));    // beyond it both taps are outside the row
      for (int k = 1; k <= kmax && k * k < best; ++k) {
        const int kk = k * k;                        // kk + g2 <= 4095^2 + 4095^2 + 1 < 2^31
        if (x - k >= 0) best = min(best, kk + g2[x - k]);
        if (x + k < W) best = min(best, kk + g2[x + k]);
      }
    }
    c[base + x] = best;
  }
}

// rule 2: d = L where c > L^2, else sqrt(float(c)) (c <= 4095^2 < 2^24 is exact as fp32); w = d / float(L)
__device__ __forceinline__ float surface_weight(int c, int l2, float lf) {
  const float d = c > l2 ? lf : sqrtf((float)c);
  return d / lf;
}

template <class T, int V> struct SurfaceVec { T a[V]; };
template <class T, int V>
__device__ __forceinline__ SurfaceVec<T, V> surface_load(const T* p, size_t i) {
  SurfaceVec<T, V> r;
  if constexpr (V == 4) {
    const uint4 q = ((const uint4*)p)[i];            // 16 bytes (the caller checked the alignment)
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < V; ++j) r.a[j] = __builtin_bit_cast(T, w[j]);
  } else {
    r.a[0] = p[i];
  }
  return r;
}
template <int V>
__device__ __forceinline__ void surface_store(float* p, size_t i, const SurfaceVec<float, V>& r) {
  if constexpr (V == 4) ((float4*)p)[i] = make_float4(r.a[0], r.a[1], r.a[2], r.a[3]);
  else p[i] = r.a[0];
}

// the fixed-order sum of a 256-thread workgroup's values: the xor butterfly inside each wave, then the four waves in order;
// the result in thread 0
template <class T>
__device__ __forceinline__ T surface_block_sum(T x, T* lds /*[4]*/) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

// grid (blocks <= SURFACE_BLOCKS, images), block 256.  nv = the image's pixels / V.  psum / pcnt: [image][gridDim.x].
template <bool VOID, int V>
__global__ __launch_bounds__(256) void surface_partial_kernel(const float* __restrict__ logits, const float* __restrict__ gt,
                                                               const int32_t* __restrict__ c, float v, int nv, int L,
                                                               float* __restrict__ psum, int* __restrict__ pcnt) {
  __shared__ float lds_s[4];
  __shared__ int lds_n[4];
  const size_t base = (size_t)blockIdx.y * nv;
  const int l2 = L * L;
  const float lf = (float)L;
  float s = 0.f;
  int n = 0;
  for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < nv; i += (int)gridDim.x * 256) {
    const auto y = surface_load<float, V>(gt, base + i);
    const auto z = surface_load<float, V>(logits, base + i);
    const auto d = surface_load<int32_t, V>(c, base + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int cls = surface_class<VOID>(y.a[j], v);
      if (cls == SURFACE_VOID) continue;             // its logit never reaches the result
      const float e = expf(-fabsf(z.a[j])), hi = 1.f / (1.f + e), lo = e / (1.f + e);   // sigmoid(|z|), sigmoid(-|z|)
      const float err = ((z.a[j] >= 0.f) == (cls == SURFACE_FG)) ? lo : hi;             // 1 - p on F, p on B
      s += surface_weight(d.a[j], l2, lf) * err;
      ++n;
    }
  }
  s = surface_block_sum(s, lds_s);
  n = surface_block_sum(n, lds_n);
  if (threadIdx.x == 0) {
    psum[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    pcnt[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = n;
  }
}

// grid 1, block 256.  Thread t takes the images t, t + 256, ..: the image's partials in index order, then the images' losses
// in the workgroup's fixed order.
__global__ __launch_bounds__(256) void surface_final_kernel(const float* __restrict__ psum, const int* __restrict__ pcnt, int blocks,
                                                             int images, float* __restrict__ loss, float* __restrict__ scale) {
  __shared__ float lds_s[4];
  float acc = 0.f;
  for (int m = threadIdx.x; m < images; m += 256) {
    float s = 0.f;
    int n = 0;
    for (int b = 0; b < blocks; ++b) {
      s += psum[(size_t)m * blocks + b];
      n += pcnt[(size_t)m * blocks + b];
    }
    scale[m] = (float)n * (float)images;
    acc += n ? s / (float)n : 0.f;
  }
  acc = surface_block_sum(acc, lds_s);
  if (threadIdx.x == 0) *loss = acc / (float)images;
}

// grid (ceil(nv / 256), images), block 256
template <bool VOID, int V>
__global__ __launch_bounds__(256) void surface_grad_kernel(const float* __restrict__ logits, const float* __restrict__ gt,
                                                            const int32_t* __restrict__ c, float v, int nv, int L,
                                                            const float* __restrict__ scale, float* __restrict__ dlogits) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= nv) return;
  const size_t at = (size_t)blockIdx.y * nv + i;
  const int l2 = L * L;
  const float lf = (float)L, sc = scale[blockIdx.y];
  const auto y = surface_load<float, V>(gt, at);
  const auto z = surface_load<float, V>(logits, at);
  const auto d = surface_load<int32_t, V>(c, at);
  SurfaceVec<float, V> out;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int cls = surface_class<VOID>(y.a[j], v);
    const float e = expf(-fabsf(z.a[j])), hi = 1.f / (1.f + e), lo = e / (1.f + e);
    const float grad = surface_weight(d.a[j], l2, lf) * (hi * lo) / sc;                  // p (1 - p) = hi * lo
    out.a[j] = cls == SURFACE_VOID ? 0.f : cls == SURFACE_FG ? -grad : grad;
  }
  surface_store<V>(dlogits, at, out);
}

// grid ceil(nv / 256), block 256: w of n = nv * V elements
template <int V>
__global__ __launch_bounds__(256) void surface_weight_kernel(const int32_t* __restrict__ c, int64_t nv, int L, float* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  const int l2 = L * L;
  const float lf = (float)L;
  const auto d = surface_load<int32_t, V>(c, (size_t)i);
  SurfaceVec<float, V> out;
#pragma unroll
  for (int j = 0; j < V; ++j) out.a[j] = surface_weight(d.a[j], l2, lf);
  surface_store<V>(w, (size_t)i, out);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool VOID, int V>
void surface_loss_launches(const float* logits, const float* gt, const int32_t* c, float* dlogits, float* loss, float* psum, int* pcnt,
                           float* scale, int64_t n_per_image, int images, int cap, float v, hipStream_t s) {
  const int nv = (int)(n_per_image / V);
  const int blocks = (int)std::min<int64_t>(SURFACE_BLOCKS, ((int64_t)nv + 255) / 256);
  hipLaunchKernelGGL((surface_partial_kernel<VOID, V>), dim3(blocks, images), dim3(256), 0, s, logits, gt, c, v, nv, cap, psum, pcnt);
  hipLaunchKernelGGL(surface_final_kernel, dim3(1), dim3(256), 0, s, psum, pcnt, blocks, images, loss, scale);
  if (dlogits)
    hipLaunchKernelGGL((surface_grad_kernel<VOID, V>), dim3((nv + 255) / 256, images), dim3(256), 0, s, logits, gt, c, v, nv, cap, scale,
                       dlogits);
}
}  // namespace

int64_t surface_scratch_floats(int64_t n_total, int max_images) {
  return n_total + (int64_t)max_images * (2 * SURFACE_BLOCKS + 1);
}

void launch_surface_distance(const float* gt, int images, int H, int W, int cap, const float* ignore, uint32_t* g, int32_t* c,
                             hipStream_t s) {
  const dim3 grid((W + 255) / 256, images);
  if (ignore) hipLaunchKernelGGL(surface_column_kernel<true>, grid, dim3(256), 0, s, gt, *ignore, H, W, cap + 1, g);
  else hipLaunchKernelGGL(surface_column_kernel<false>, grid, dim3(256), 0, s, gt, 0.f, H, W, cap + 1, g);
  hipLaunchKernelGGL(surface_row_kernel, dim3(H, images), dim3(256), 2 * (size_t)W * sizeof(int), s, g, H, W, cap, c);
}

void launch_surface_weights(const int32_t* c, float* w, int64_t n, int cap, hipStream_t s) {
  if (n % 4 == 0 && aligned16(c) && aligned16(w))
    hipLaunchKernelGGL(surface_weight_kernel<4>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, c, n / 4, cap, w);
  else
    hipLaunchKernelGGL(surface_weight_kernel<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c, n, cap, w);
}

void launch_surface_loss(const float* logits, const float* gt, const int32_t* c, float* dlogits, float* loss, float* partial, int H,
                         int W, int images, int cap, const float* ignore, hipStream_t s) {
  const int64_t n = (int64_t)H * W;
  float* psum = partial;
  int* pcnt = (int*)(partial + (size_t)images * SURFACE_BLOCKS);
  float* scale = partial + 2 * (size_t)images * SURFACE_BLOCKS;
  const bool vec = n % 4 == 0 && aligned16(logits) && aligned16(gt) && aligned16(c) && (!dlogits || aligned16(dlogits));
  const float v = ignore ? *ignore : 0.f;
  auto go = ignore ? (vec ? surface_loss_launches<true, 4> : surface_loss_launches<true, 1>)
                   : (vec ? surface_loss_launches<false, 4> : surface_loss_launches<false, 1>);
  go(logits, gt, c, dlogits, loss, psum, pcnt, scale, n, images, cap, v, s);
}

void launch_surface(const float* logits, const float* gt, float* dlogits, float* loss, float* scratch, int H, int W, int images,
                    int cap, const float* ignore, hipStream_t s) {
  const int64_t n_total = (int64_t)images * H * W;
  launch_surface_distance(gt, images, H, W, cap, ignore, (uint32_t*)scratch, (int32_t*)scratch, s);
  launch_surface_loss(logits, gt, (const int32_t*)scratch, dlogits, loss, scratch + n_total, H, W, images, cap, ignore, s);
}
}  // namespace eosvos
