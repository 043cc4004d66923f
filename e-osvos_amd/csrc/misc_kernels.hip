// HBM-bound and small kernels of the e-OSVOS inner loop for gfx950: layout changes, the
// 7x7 stem, max-pool, bilinear resize (+ gather-form backward), the ASPP image-pooling
// branch, the 1-channel classifier conv, the losses and their gradients (one templated kernel family each, with or without a
// void label), the fused
// per-neuron-lr SGD update (split-K slab reduction included), meta-gradient reduction,
// RAdam, the Winograd transform passes (one templated family, at the end of the file).
// 64-lane waves, 16-byte accesses where the layout allows, deterministic (atomic-free)
// reductions everywhere so fine-tuning trajectories are reproducible.
#include <cassert>

#include "kernels.h"
#include "loss_expr.h"

namespace eosvos {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over a 256-thread block; result valid in every thread
__device__ __forceinline__ float block_sum_256(float v, float* sh /*>=4 floats*/) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
static inline int grid_for(long n, int per_block, int cap = 4096) {
  long b = (n + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}
#define GRID_STRIDE(i, n) \
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

// ---- layout ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nchw_to_nhwc_pad_kernel(const float* __restrict__ src, float* __restrict__ dst, int B,
                                                               int C, int H, int W, int pad, unsigned* __restrict__ amax,
                                                               int mirror) {
  const long n = (long)B * H * W;
  const int Wp = W + 2 * pad, Hp = H + 2 * pad;
  unsigned am = 0;
  GRID_STRIDE(i, n) {
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    const int b = (int)(i / ((long)W * H));
    const int xd = mirror ? W - 1 - x : x;            // mirrored view (test-time augmentation): the frame is flipped on its way in
    float* d = dst + (((long)b * Hp + y + pad) * Wp + xd + pad) * C;
    for (int c = 0; c < C; ++c) {
      const float v = src[(((long)b * C + c) * H + y) * W + x];
      d[c] = v;
      const unsigned ab = amax_f1(v);
      am = am > ab ? am : ab;
    }
  }
  if (amax) amax_block_commit(am, amax);            // f16x3 mode: absmax of the frame for the stem on the matrix cores
}
void launch_nchw_to_nhwc_pad(const float* src, float* dst, int B, int C, int H, int W, int pad,
                             hipStream_t s, unsigned* amax, int mirror) {
  const long n = (long)B * H * W;
  hipLaunchKernelGGL(nchw_to_nhwc_pad_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, src, dst, B, C, H,
                     W, pad, amax, mirror);
}

__global__ void fill_kernel(float* p, long n, float v) { GRID_STRIDE(i, n) p[i] = v; }
void launch_fill(float* p, int64_t n, float v, hipStream_t s) {
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, p, (long)n, v);
}

__global__ void oihw_to_ohwi_kernel(const float* __restrict__ src, float* __restrict__ dst, int O, int I,
                                    int T) {
  const long n = (long)O * I * T;
  GRID_STRIDE(e, n) {   // e indexes dst [o][t][i]
    const int i = (int)(e % I);
    const int t = (int)((e / I) % T);
    const long o = e / ((long)I * T);
    dst[e] = src[(o * I + i) * T + t];
  }
}
void launch_oihw_to_ohwi(const float* src, float* dst, int O, int I, int T, hipStream_t s) {
  const long n = (long)O * I * T;
  hipLaunchKernelGGL(oihw_to_ohwi_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, src, dst, O, I, T);
}
__global__ void ohwi_to_oihw_kernel(const float* __restrict__ src, float* __restrict__ dst, int O, int I,
                                    int T, float alpha, int add) {
  const long n = (long)O * I * T;
  GRID_STRIDE(e, n) {   // e indexes dst [o][i][t]
    const int t = (int)(e % T);
    const int i = (int)((e / T) % I);
    const long o = e / ((long)I * T);
    const float v = alpha * src[(o * T + t) * I + i];
    dst[e] = add ? dst[e] + v : v;
  }
}
void launch_ohwi_to_oihw(const float* src, float* dst, int O, int I, int T, float alpha, int add,
                         hipStream_t s) {
  const long n = (long)O * I * T;
  hipLaunchKernelGGL(ohwi_to_oihw_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, src, dst, O, I, T, alpha,
                     add);
}
// every tensor of the arena in one launch: ent[k] = {offset, I, T, 0} of tensor k (biases: I = T = 1), sorted by offset;
// an element finds its tensor by binary search in LDS
__global__ __launch_bounds__(256) void ohwi_to_oihw_all_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                const long* __restrict__ toff, const int2* __restrict__ tit,
                                                                int nent, long n, float alpha, int add) {
  __shared__ long s_off[160];
  __shared__ int2 s_it[160];
  for (int i = threadIdx.x; i < nent; i += 256) { s_off[i] = toff[i]; s_it[i] = tit[i]; }
  __syncthreads();
  GRID_STRIDE(e, n) {   // e indexes dst (flat OIHW order of every tensor)
    int lo = 0, hi = nent - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (e >= s_off[mid]) lo = mid; else hi = mid - 1;
    }
    const long r = e - s_off[lo];
    const int I = s_it[lo].x, T = s_it[lo].y;
    const int t = (int)(r % T);
    const int i = (int)((r / T) % I);
    const long o = r / ((long)I * T);
    const float v = alpha * src[s_off[lo] + (o * T + t) * I + i];
    dst[e] = add ? dst[e] + v : v;
  }
}
void launch_ohwi_to_oihw_all(const float* src, float* dst, const long* toff, const int2* tit, int nent, int64_t n, float alpha,
                             int add, hipStream_t s) {
  hipLaunchKernelGGL(ohwi_to_oihw_all_kernel, dim3(grid_for((long)n, 256)), dim3(256), 0, s, src, dst, toff, tit, nent, (long)n,
                     alpha, add);
}

__global__ void fold_norm_kernel(const float* g, const float* be, const float* mu, const float* var,
                                 float eps, float* a, float* b, long n) {
  GRID_STRIDE(i, n) {
    // torch's eval-mode batch norm (ATen batch_norm_cpu_collect_linear_and_constant_terms, what the reference's
    // `/root/reference/src/networks/deeplabv3plus.py:259-280` BN layers run): inv_std = 1 / sqrt(var + eps), alpha = inv_std *
    // weight, beta = bias - mean * alpha -- the SAME roundings, not the one-rounding g / sqrt(...): a 1-ulp difference of a
    // channel's scale is coherent over every pixel and every iteration (fixture g19t50: 9.6e-4 -> see DESIGN 5d)
    const float inv = 1.0f / sqrtf(var[i] + eps);
    const float s = inv * g[i];
    a[i] = s;
    b[i] = be[i] - mu[i] * s;
  }
}
void launch_fold_norm(const float* gamma, const float* beta, const float* mean, const float* var,
                      float eps, float* a, float* b, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(fold_norm_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, gamma, beta, mean, var, eps,
                     a, b, (long)n);
}

// ---- stem: 7x7 stride-2 conv, 3 -> 64, on the 3-pixel zero-padded NHWC3 frame ------------
// One thread per output pixel, 64 accumulators; the 147x64 weight panel sits in LDS as
// [k][cout] and is read with broadcast ds_read_b128 (every lane the same address).
// One thread = 4 consecutive output pixels of a row x 16 output channels (64 accumulators): a weight float4 read from LDS
// feeds 16 FMAs (the one-pixel-per-thread form read one per 4 FMAs and was LDS-bound: 125 us at batch 3), and the 39
// contiguous input floats the 4 pixels share per filter row come in as 20 float2 loads instead of 84 scalar ones.  Same (ky, kx, c) order per output as before:
// bit-identical results.
__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* __restrict__ xpad,
                                                        const float* __restrict__ w,
                                                        const float* __restrict__ a,
                                                        const float* __restrict__ bb, float* __restrict__ y,
                                                        int B, int H, int W, int Ho, int Wo) {
  __shared__ __attribute__((aligned(16))) float wl[147 * 64];
  for (int i = threadIdx.x; i < 147 * 64; i += 256) {
    const int k = i >> 6, co = i & 63;
    wl[i] = w[co * 147 + k];
  }
  __syncthreads();
  const int cg = threadIdx.x & 3;                               // channels [16 cg, 16 cg + 16)
  const int qrow = (Wo + 3) >> 2;                               // pixel quads per output row (the last may be partial)
  const long quad = (long)blockIdx.x * 64 + (threadIdx.x >> 2);
  if (quad >= (long)B * Ho * qrow) return;
  const int qx = (int)(quad % qrow), oy = (int)((quad / qrow) % Ho), b = (int)(quad / ((long)qrow * Ho));
  const int ox0 = qx * 4;
  const int Wp = W + 6, Hp = H + 6;
  const long p0 = ((long)b * Ho + oy) * Wo + ox0;
  bool ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) ok[i] = ox0 + i < Wo;
  // the 4 pixels read floats [6 i, 6 i + 21) of each of their 7 input rows: 39 contiguous floats, 8-byte aligned
  const float* xrow = xpad + (((long)b * Hp + oy * 2) * Wp + ox0 * 2) * 3;
  const int avail = (Wp - ox0 * 2) * 3;                         // floats left in the padded row (>= 21)
  float acc[4][16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[i][c] = 0.f;
  for (int ky = 0; ky < 7; ++ky) {
    const float* xr = xrow + (long)ky * Wp * 3;
    float xin[40];
#pragma unroll
    for (int t = 0; t < 20; ++t) {
      float2 v = make_float2(0.f, 0.f);
      if (2 * t + 1 < avail) v = *reinterpret_cast<const float2*>(xr + 2 * t);
      else if (2 * t < avail) v.x = xr[2 * t];
      xin[2 * t] = v.x; xin[2 * t + 1] = v.y;
    }
#pragma unroll
    for (int j = 0; j < 21; ++j) {
      const float4* wr = reinterpret_cast<const float4*>(wl + (ky * 21 + j) * 64 + cg * 16);
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        const float4 wv = wr[c4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float xv = xin[6 * i + j];
          acc[i][c4 * 4 + 0] = fmaf(xv, wv.x, acc[i][c4 * 4 + 0]);
          acc[i][c4 * 4 + 1] = fmaf(xv, wv.y, acc[i][c4 * 4 + 1]);
          acc[i][c4 * 4 + 2] = fmaf(xv, wv.z, acc[i][c4 * 4 + 2]);
          acc[i][c4 * 4 + 3] = fmaf(xv, wv.w, acc[i][c4 * 4 + 3]);
        }
      }
    }
  }
  float4 av[4], bv[4];
  if (a) {
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
      av[c4] = *reinterpret_cast<const float4*>(a + cg * 16 + c4 * 4);
      bv[c4] = *reinterpret_cast<const float4*>(bb + cg * 16 + c4 * 4);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!ok[i]) continue;
    float4* out = reinterpret_cast<float4*>(y + (p0 + i) * 64 + cg * 16);
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
      float4 v;
      if (a) {
        v.x = fmaxf(acc[i][c4 * 4 + 0] * av[c4].x + bv[c4].x, 0.f);
        v.y = fmaxf(acc[i][c4 * 4 + 1] * av[c4].y + bv[c4].y, 0.f);
        v.z = fmaxf(acc[i][c4 * 4 + 2] * av[c4].z + bv[c4].z, 0.f);
        v.w = fmaxf(acc[i][c4 * 4 + 3] * av[c4].w + bv[c4].w, 0.f);
      } else {        // raw conv output (GroupNorm mode)
        v.x = acc[i][c4 * 4 + 0]; v.y = acc[i][c4 * 4 + 1]; v.z = acc[i][c4 * 4 + 2]; v.w = acc[i][c4 * 4 + 3];
      }
      out[c4] = v;
    }
  }
}
void launch_stem_fwd(const float* xpad, const float* w, const float* a, const float* b, float* y, int B,
                     int H, int W, int Ho, int Wo, hipStream_t s) {
  const long Q = (long)B * Ho * ((Wo + 3) / 4);        // pixel quads; 64 per workgroup
  hipLaunchKernelGGL(stem_fwd_kernel, dim3((unsigned)((Q + 63) / 64)), dim3(256), 0, s, xpad, w, a, b, y,
                     B, H, W, Ho, Wo);
}

// Stem weight gradient on the matrix cores: dW[64][147] = sum_p G[p][64]^T * patch[p][147].
// Each workgroup reduces one chunk of output pixels into a [64][147] slab.  Per 32-pixel K step
// the G rows are staged with float4 loads and the 7x21 input patch of every pixel with scalar
// loads (the 84-byte patch rows of the NHWC3 frame are only 4-byte aligned) by one thread per k,
// which walks the pixels with carries; 2 x 5 accumulators of 32x32 cover 64 x 160 (147 padded).
typedef float stem_f32x16 __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ xpad,
                                                          const float* __restrict__ g, float* __restrict__ ws,
                                                          int B, int H, int W, int Ho, int Wo, int chunks) {
  constexpr int LDA = 68, LDB = 164;
  __shared__ __attribute__((aligned(16))) float As[2][32 * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[2][32 * LDB];
  const long P = (long)B * Ho * Wo;
  const long per = ((P + chunks - 1) / chunks + 31) / 32 * 32;
  const long p0 = (long)blockIdx.x * per;
  long p1 = p0 + per;
  if (p1 > P) p1 = P;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int Wp = W + 6, Hp = H + 6;
  const int k = tid;                                  // B staging: one thread per patch element k
  const int koff = k < 147 ? (k / 21) * Wp * 3 + (k % 21) : 0;
  const int a_row = tid >> 4, a_c4 = tid & 15;        // A staging: rows a_row, a_row+16
  const int mt = wave & 1, nt0 = wave >> 1;           // accumulator tiles: (mt, nt0 + 2j), j = 0..2
  stem_f32x16 acc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  // zero the padded columns 147..163 of both B buffers once (they feed the unused part of tile 4)
  for (int i = tid; i < 2 * 32 * (LDB - 147); i += 256) {
    const int bb = i / (32 * (LDB - 147)), rem = i % (32 * (LDB - 147));
    Bs[bb][(rem / (LDB - 147)) * LDB + 147 + rem % (LDB - 147)] = 0.f;
  }
  const int nsteps = p1 > p0 ? (int)((p1 - p0 + 31) / 32) : 0;
  float4 ra[2];
  float rb[32];
  auto load_step = [&](int st) {
    const long ps = p0 + (long)st * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long px = ps + a_row + i * 16;
      ra[i] = px < p1 ? *reinterpret_cast<const float4*>(g + px * 64 + a_c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (k < 147) {
      int ox = (int)(ps % Wo), oy = (int)((ps / Wo) % Ho), b = (int)(ps / ((long)Wo * Ho));
      long base = (((long)b * Hp + oy * 2) * Wp + ox * 2) * 3 + koff;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        rb[i] = (ps + i) < p1 ? xpad[base] : 0.f;
        base += 6;
        if (++ox == Wo) {
          ox = 0;
          base += (long)(2 * Wp - 2 * Wo) * 3;
          if (++oy == Ho) { oy = 0; base += (long)(Hp - 2 * Ho) * Wp * 3; }
        }
      }
    }
  };
  auto store_step = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(&As[buf][(a_row + i * 16) * LDA + a_c4 * 4]) = ra[i];
    if (k < 147) {
#pragma unroll
      for (int i = 0; i < 32; ++i) Bs[buf][i * LDB + k] = rb[i];
    }
  };
  if (nsteps > 0) { load_step(0); }
  __syncthreads();
  if (nsteps > 0) store_step(0);
  __syncthreads();
  for (int st = 0; st < nsteps; ++st) {
    const int buf = st & 1;
    const bool more = st + 1 < nsteps;
    if (more) load_step(st + 1);
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) {
      const float av = As[buf][(s2 * 2 + h) * LDA + mt * 32 + r];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int nt = nt0 + 2 * j;
        if (nt < 5) {
          const float bv = Bs[buf][(s2 * 2 + h) * LDB + nt * 32 + r];
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[j], 0, 0, 0);
        }
      }
    }
    if (more) store_step(buf ^ 1);
    __syncthreads();
  }
  float* out = ws + (long)blockIdx.x * (64 * 147);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int nt = nt0 + 2 * j;
    const int kk = nt * 32 + r;
    if (nt < 5 && kk < 147) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = mt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        out[co * 147 + kk] = acc[j][e];
      }
    }
  }
}
int stem_wgrad_chunks(int B, int Ho, int Wo) {
  const long P = (long)B * Ho * Wo;
  long c = P / 128;
  if (c < 1) c = 1;
  if (c > 512) c = 512;
  return (int)c;
}
void launch_stem_wgrad(const float* xpad, const float* g, float* ws, int B, int H, int W, int Ho, int Wo,
                       int chunks, hipStream_t s) {
  hipLaunchKernelGGL(stem_wgrad_kernel, dim3(chunks), dim3(256), 0, s, xpad, g, ws, B, H, W, Ho, Wo, chunks);
}

// ---- max-pool 3x3 s2 p1 ------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                   uint8_t* __restrict__ idx, int B, int H, int W, int C, int Ho, int Wo, unsigned* __restrict__ amax) {
  const int C4 = C >> 2;
  const long n = (long)B * Ho * Wo * C4;
  unsigned am = 0;
  GRID_STRIDE(e, n) {
    const int c4 = (int)(e % C4);
    const long pix = e / C4;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((long)Wo * Ho));
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    unsigned char mi[4] = {0, 0, 0, 0};
    bool first = true;
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * 2 - 1 + ky;
      if (iy < 0 || iy >= H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * 2 - 1 + kx;
        if (ix < 0 || ix >= W) continue;
        const float4 v = *reinterpret_cast<const float4*>(x + (((long)b * H + iy) * W + ix) * C + c4 * 4);
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (first || vv[j] > m[j] || isnan(vv[j])) { m[j] = vv[j]; mi[j] = (unsigned char)(ky * 3 + kx); }   // NaN wins, as in torch
        first = false;
      }
    }
    const float4 out = make_float4(m[0], m[1], m[2], m[3]);
    *reinterpret_cast<float4*>(y + pix * C + c4 * 4) = out;
    am = amax_f4(am, out);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (m[j] > 0.f) mi[j] |= 0x80;            // the ReLU mask of the pixel the gradient will go to
    *reinterpret_cast<uchar4*>(idx + pix * C + c4 * 4) = make_uchar4(mi[0], mi[1], mi[2], mi[3]);
  }
  if (amax) amax_block_commit(am, amax);
}
void launch_maxpool_fwd(const float* x, float* y, uint8_t* idx, int B, int H, int W, int C, int Ho, int Wo,
                        hipStream_t s, unsigned* amax) {
  const long n = (long)B * Ho * Wo * (C >> 2);
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, x, y, idx, B, H, W, C, Ho,
                     Wo, amax);
}
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ gy, const uint8_t* __restrict__ idx,
                                   float* __restrict__ gx, int B, int H, int W,
                                   int C, int Ho, int Wo, unsigned* __restrict__ amax) {
  const int C4 = C >> 2;
  const long n = (long)B * H * W * C4;
  unsigned am = 0;
  GRID_STRIDE(e, n) {
    const int c4 = (int)(e % C4);
    const long pix = e / C4;
    const int ix = (int)(pix % W), iy = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    const int oy_lo = iy >> 1, oy_hi = (iy + 1) >> 1;      // ceil((iy-1)/2) .. floor((iy+1)/2)
    const int ox_lo = ix >> 1, ox_hi = (ix + 1) >> 1;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      if (oy >= Ho) continue;
      const int ky = iy + 1 - 2 * oy;
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        if (ox >= Wo) continue;
        const int kx = ix + 1 - 2 * ox;
        const unsigned char k = (unsigned char)((ky * 3 + kx) | 0x80);      // argmax here AND its value > 0
        const long o = (((long)b * Ho + oy) * Wo + ox) * C + c4 * 4;
        const uchar4 id = *reinterpret_cast<const uchar4*>(idx + o);
        const float4 g = *reinterpret_cast<const float4*>(gy + o);
        if (id.x == k) s[0] += g.x;
        if (id.y == k) s[1] += g.y;
        if (id.z == k) s[2] += g.z;
        if (id.w == k) s[3] += g.w;
      }
    }
    const float4 o = make_float4(s[0], s[1], s[2], s[3]);
    *reinterpret_cast<float4*>(gx + pix * C + c4 * 4) = o;
    am = amax_f4(am, o);
  }
  if (amax) amax_block_commit(am, amax);            // f16x3 mode: the stem's weight gradient runs on the matrix cores
}
void launch_maxpool_bwd(const float* gy, const uint8_t* idx, float* gx, int B, int H, int W,
                        int C, int Ho, int Wo, hipStream_t s, unsigned* amax) {
  const long n = (long)B * H * W * (C >> 2);
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, gy, idx, gx, B, H, W, C,
                     Ho, Wo, amax);
}

// ---- bilinear resize ----------------------------------------------------------------------
template <int V>
__global__ void resize_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, int B,
                                  int C, ResizeTab th, ResizeTab tw) {
  const int CV = C / V;
  const long n = (long)B * th.out * tw.out * CV;
  GRID_STRIDE(e, n) {
    const int cv = (int)(e % CV);
    const long pix = e / CV;
    const int ox = (int)(pix % tw.out), oy = (int)((pix / tw.out) % th.out);
    const int b = (int)(pix / ((long)tw.out * th.out));
    const int y0 = th.i0[oy], y1 = th.i1[oy], x0 = tw.i0[ox], x1 = tw.i1[ox];
    const float ly = th.lam[oy], lx = tw.lam[ox];
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float* base = x + (long)b * th.in * tw.in * ldx + cv * V;
    float o[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float v00 = base[((long)y0 * tw.in + x0) * ldx + j], v01 = base[((long)y0 * tw.in + x1) * ldx + j];
      const float v10 = base[((long)y1 * tw.in + x0) * ldx + j], v11 = base[((long)y1 * tw.in + x1) * ldx + j];
      o[j] = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
    }
    float* d = y + pix * ldy + cv * V;
#pragma unroll
    for (int j = 0; j < V; ++j) d[j] = o[j];
  }
}
void launch_resize_fwd(const float* x, int ldx, float* y, int ldy, int B, int C, ResizeTab th, ResizeTab tw,
                       hipStream_t s) {
  if ((C & 3) == 0) {
    const long n = (long)B * th.out * tw.out * (C / 4);
    hipLaunchKernelGGL((resize_fwd_kernel<4>), dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, x, ldx, y, ldy,
                       B, C, th, tw);
  } else {
    const long n = (long)B * th.out * tw.out * C;
    hipLaunchKernelGGL((resize_fwd_kernel<1>), dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, x, ldx, y, ldy,
                       B, C, th, tw);
  }
}
template <int V>
__global__ __launch_bounds__(256) void resize_bwd_kernel(const float* __restrict__ gy, int ldgy, float* __restrict__ gx, int ldgx,
                                  const uint8_t* __restrict__ m8, int ldm8, int B, int C, ResizeTab th,
                                  ResizeTab tw, unsigned* __restrict__ amax) {
  const int CV = C / V;
  const long n = (long)B * th.in * tw.in * CV;
  unsigned am = 0;
  GRID_STRIDE(e, n) {
    const int cv = (int)(e % CV);
    const long pix = e / CV;
    const int ix = (int)(pix % tw.in), iy = (int)((pix / tw.in) % th.in);
    const int b = (int)(pix / ((long)tw.in * th.in));
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    const float* gb = gy + (long)b * th.out * tw.out * ldgy + cv * V;
    // the column weights of this pixel once, not once per source row (three dependent table loads per element otherwise:
    // the 1-channel logits gradient took 35 us for 5 MB); same products, same order of accumulation
    constexpr int MAXW = 12;
    const int dx0 = tw.lo[ix], dx1 = tw.hi[ix];
    float wxs[MAXW];
    const bool pre = V == 1 && dx1 - dx0 < MAXW;          // (the 4-channel form gains nothing: 47 -> 49 us)
    if (pre) {
#pragma unroll
      for (int t = 0; t < MAXW; ++t) {
        const int dx = dx0 + t;
        if (dx <= dx1) {
          const float lx = tw.lam[dx];
          wxs[t] = (tw.i0[dx] == ix ? 1.f - lx : 0.f) + (tw.i1[dx] == ix ? lx : 0.f);
        } else {
          wxs[t] = 0.f;
        }
      }
    }
    for (int dy = th.lo[iy]; dy <= th.hi[iy]; ++dy) {
      const float ly = th.lam[dy];
      const float wy = (th.i0[dy] == iy ? 1.f - ly : 0.f) + (th.i1[dy] == iy ? ly : 0.f);
      if (pre) {
#pragma unroll
        for (int t = 0; t < MAXW; ++t) {
          const int dx = dx0 + t;
          if (dx <= dx1) {
            const float wgt = wy * wxs[t];
            const float* gp = gb + ((long)dy * tw.out + dx) * ldgy;
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = fmaf(wgt, gp[j], acc[j]);
          }
        }
      } else {
        for (int dx = dx0; dx <= dx1; ++dx) {
          const float lx = tw.lam[dx];
          const float wx = (tw.i0[dx] == ix ? 1.f - lx : 0.f) + (tw.i1[dx] == ix ? lx : 0.f);
          const float wgt = wy * wx;
          const float* gp = gb + ((long)dy * tw.out + dx) * ldgy;
#pragma unroll
          for (int j = 0; j < V; ++j) acc[j] = fmaf(wgt, gp[j], acc[j]);
        }
      }
    }
    float* d = gx + pix * ldgx + cv * V;
    if (V == 4 && m8) {
      // ReLU mask byte of channels cv * 4 .. + 3, addressed through their float offset (= pix * ldm8 + cv): this form
      // shares the channel offset the gradient's own address holds (one VGPR fewer than indexing by cv)
      const unsigned bits = m8[(pix * 4 * ldm8 + cv * V) >> 2];
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = (bits & (1u << j)) ? acc[j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) { d[j] = acc[j]; const unsigned q = amax_f1(acc[j]); am = am > q ? am : q; }
  }
  if (amax) amax_block_commit(am, amax);
}
void launch_resize_bwd(const float* gy, int ldgy, float* gx, int ldgx, const uint8_t* m8, int ldm8, int B,
                       int C, ResizeTab th, ResizeTab tw, hipStream_t s, unsigned* amax) {
  if ((C & 3) == 0) {
    const long n = (long)B * th.in * tw.in * (C / 4);
    hipLaunchKernelGGL((resize_bwd_kernel<4>), dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, gy, ldgy, gx,
                       ldgx, m8, ldm8, B, C, th, tw, amax);
  } else {
    const long n = (long)B * th.in * tw.in * C;
    hipLaunchKernelGGL((resize_bwd_kernel<1>), dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, gy, ldgy, gx,
                       ldgx, nullptr, 0, B, C, th, tw, amax);
  }
}

// ---- ASPP image pooling branch ---------------------------------------------------------------
// scratch[b][chunk][c] = sum over the chunk's pixels ; out[b][c] = alpha * sum over chunks
#define COLSUM_CHUNKS 64
// C % 4 == 0; a thread owns float4 channel groups and walks its chunk's pixels with 8 loads in flight
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ x, int ldx,
                                                              float* __restrict__ scratch, int P, int C) {
  const int b = blockIdx.y, ch = blockIdx.x;
  const int per = (P + COLSUM_CHUNKS - 1) / COLSUM_CHUNKS;
  const int p0 = ch * per;
  int p1 = p0 + per;
  if (p1 > P) p1 = P;
  for (int c = threadIdx.x * 4; c < C; c += 1024) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* xp = x + ((long)b * P) * ldx + c;
    for (int q = p0; q < p1; q += 8) {
      float4 v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        v[i] = (q + i < p1) ? *reinterpret_cast<const float4*>(xp + (long)(q + i) * ldx) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int i = 0; i < 8; ++i) { s.x += v[i].x; s.y += v[i].y; s.z += v[i].z; s.w += v[i].w; }
    }
    *reinterpret_cast<float4*>(scratch + ((long)b * COLSUM_CHUNKS + ch) * C + c) = s;
  }
}
__global__ void colsum_final_kernel(const float* __restrict__ scratch, float* __restrict__ out, int B, int C,
                                    float alpha) {
  const long n = (long)B * C;
  GRID_STRIDE(e, n) {
    const int c = (int)(e % C), b = (int)(e / C);
    float s = 0.f;
#pragma unroll 16
    for (int ch = 0; ch < COLSUM_CHUNKS; ++ch) s += scratch[((long)b * COLSUM_CHUNKS + ch) * C + c];
    out[e] = alpha * s;
  }
}
void launch_colsum(const float* x, int ldx, float* out, int B, int P, int C, float alpha, float* scratch,
                   hipStream_t s) {
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(COLSUM_CHUNKS, B), dim3(256), 0, s, x, ldx, scratch, P, C);
  hipLaunchKernelGGL(colsum_final_kernel, dim3(grid_for((long)B * C, 256)), dim3(256), 0, s, scratch, out, B, C,
                     alpha);
}
// one wave per (b, n)
__global__ __launch_bounds__(256) void gemv_fwd_kernel(const float* __restrict__ W, const float* __restrict__ v,
                                                        const float* __restrict__ a, const float* __restrict__ bb,
                                                        float* __restrict__ y, int B, int N, int K) {
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= B * N) return;
  const int lane = threadIdx.x & 63;
  const int b = wid / N, n = wid - b * N;
  float s = 0.f;
  for (int k = lane * 4; k < K; k += 256) {
    const float4 w4 = *reinterpret_cast<const float4*>(W + (long)n * K + k);
    const float4 v4 = *reinterpret_cast<const float4*>(v + (long)b * K + k);
    s = fmaf(w4.x, v4.x, s); s = fmaf(w4.y, v4.y, s); s = fmaf(w4.z, v4.z, s); s = fmaf(w4.w, v4.w, s);
  }
  s = wave_sum(s);
  if (lane == 0) y[wid] = a ? fmaxf(s * a[n] + bb[n], 0.f) : s;
}
void launch_gemv_fwd(const float* W, const float* v, const float* a, const float* b, float* y, int B, int N,
                     int K, hipStream_t s) {
  hipLaunchKernelGGL(gemv_fwd_kernel, dim3((B * N + 3) / 4), dim3(256), 0, s, W, v, a, b, y, B, N, K);
}
__global__ void gemv_bwd_kernel(const float* __restrict__ W, const float* __restrict__ v,
                                const float* __restrict__ gp, const float* __restrict__ a,
                                float* __restrict__ gv, float* __restrict__ dW, int B, int N, int K) {
  const long nv = gv ? (long)B * K : 0, nw = (long)N * K;      // gv == nullptr: the weight gradient only
  GRID_STRIDE(e, nv + nw) {
    if (e < nv) {
      const int k = (int)(e % K), b = (int)(e / K);
      float s = 0.f;
#pragma unroll 16
      for (int n = 0; n < N; ++n) s = fmaf(gp[b * N + n] * (a ? a[n] : 1.f), W[(long)n * K + k], s);
      gv[e] = s;
    } else {
      const long f = e - nv;
      const int k = (int)(f % K), n = (int)(f / K);
      float s = 0.f;
      for (int b = 0; b < B; ++b) s = fmaf(gp[b * N + n], v[(long)b * K + k], s);
      dW[f] = s;
    }
  }
}
void launch_gemv_bwd(const float* W, const float* v, const float* gp, const float* a, float* gv, float* dW,
                     int B, int N, int K, hipStream_t s) {
  const long n = (gv ? (long)B * K : 0) + (long)N * K;
  hipLaunchKernelGGL(gemv_bwd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, W, v, gp, a, gv, dW, B, N, K);
}
__global__ void bcast_pixels_kernel(const float* __restrict__ v, float* __restrict__ y, int ldy, int B, int P,
                                    int C, float alpha, uint8_t* __restrict__ mask8_out, int ldm8) {
  const int C4 = C >> 2;
  const long n = (long)B * P * C4;
  GRID_STRIDE(e, n) {
    const int c4 = (int)(e % C4);
    const long pix = e / C4;
    const int b = (int)(pix / P);
    float4 t = *reinterpret_cast<const float4*>(v + (long)b * C + c4 * 4);
    t.x *= alpha; t.y *= alpha; t.z *= alpha; t.w *= alpha;
    *reinterpret_cast<float4*>(y + pix * ldy + c4 * 4) = t;
    if (mask8_out) mask8_out[pix * ldm8 + c4] = relu_bits(t);
  }
}
void launch_bcast_pixels(const float* v, float* y, int ldy, int B, int P, int C, float alpha, hipStream_t s, uint8_t* mask8_out, int ldm8) {
  const long n = (long)B * P * (C >> 2);
  hipLaunchKernelGGL(bcast_pixels_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, v, y, ldy, B, P, C, alpha, mask8_out, ldm8);
}

// ---- classifier conv (Cout = 1, bias) ------------------------------------------------------------
__global__ __launch_bounds__(256) void last_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y,
                                                        long P, int C) {
  const int lane = threadIdx.x & 63;
  const long nw = (long)gridDim.x * 4;
  for (long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6); p < P; p += nw) {
    float s = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
      const float4 xv = *reinterpret_cast<const float4*>(x + p * C + c);
      const float4 wv = *reinterpret_cast<const float4*>(w + c);
      s = fmaf(xv.x, wv.x, s); s = fmaf(xv.y, wv.y, s); s = fmaf(xv.z, wv.z, s); s = fmaf(xv.w, wv.w, s);
    }
    s = wave_sum(s);
    if (lane == 0) y[p] = s + bias[0];
  }
}
void launch_last_fwd(const float* x, const float* w, const float* bias, float* y, int64_t P, int C,
                     hipStream_t s) {
  hipLaunchKernelGGL(last_fwd_kernel, dim3(grid_for(P, 4, 4096)), dim3(256), 0, s, x, w, bias, y, (long)P, C);
}
// gx[p][c] = g[p]*w[c]*(x>0);  ws_dw[chunk][c] = sum_p g[p]*x[p][c];  ws_dw[chunk][C] = sum_p g[p]
__global__ __launch_bounds__(256) void last_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ g, float* __restrict__ gx,
                                                        float* __restrict__ ws, long P, int C, int chunks) {
  const long per = (P + chunks - 1) / chunks;
  const long p0 = (long)blockIdx.x * per;
  long p1 = p0 + per;
  if (p1 > P) p1 = P;
  __shared__ float sh[4];
  float gsum = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float wc = w[c];
    float s = 0.f;
    for (long p = p0; p < p1; ++p) {
      const float gv = g[p];
      const float xv = x[p * C + c];
      s = fmaf(gv, xv, s);
      gx[p * C + c] = xv > 0.f ? gv * wc : 0.f;
    }
    ws[(long)blockIdx.x * (C + 1) + c] = s;
  }
  for (long p = p0 + threadIdx.x; p < p1; p += 256) gsum += g[p];
  gsum = block_sum_256(gsum, sh);
  if (threadIdx.x == 0) ws[(long)blockIdx.x * (C + 1) + C] = gsum;
}
int last_bwd_chunks(int64_t P) {
  long c = P / 64;
  if (c < 1) c = 1;
  if (c > 1024) c = 1024;
  return (int)c;
}
void launch_last_bwd(const float* x, const float* w, const float* g, float* gx, float* ws_dw, int64_t P, int C,
                     int chunks, hipStream_t s) {
  hipLaunchKernelGGL(last_bwd_kernel, dim3(chunks), dim3(256), 0, s, x, w, g, gx, ws_dw, (long)P, C, chunks);
}

// ---- sigmoid, test-time augmentation -------------------------------------------------------------------
__global__ void sigmoid_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
  GRID_STRIDE(i, n) {
    const float xv = x[i];
    const float e = expf(-fabsf(xv));
    y[i] = xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
  }
}
void launch_sigmoid(const float* x, float* y, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(sigmoid_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, x, y, (long)n);
}
// Test-time augmentation, one view into the frame's accumulator: acc (B, H, W) (+)= weight * sigmoid(resize(unmirror(logits)))
// with logits (B, h, w).  The resize is torch's bilinear align_corners=False rule (source coordinate
// max(0, (in / out) * (o + 0.5) - 0.5), upper neighbour clamped at the edge; the arithmetic of resize_fwd_kernel) with the
// coordinates computed in place: a view is resampled once, so a table would cost more than it saves.  h == H and w == W
// reads the logit itself.  One thread per output pixel, one writer per pixel: no LDS, no atomics, order-free.  (tta_src: kernels.h,
// shared with zoom_kernels.hip.)
__global__ __launch_bounds__(256) void tta_accumulate_kernel(const float* __restrict__ logits, float* __restrict__ acc, int B,
                                                             int h, int w, int H, int W, float sy, float sx, int mirror,
                                                             float weight, int first) {
  const long n = (long)B * H * W;
  const bool same = h == H && w == W;
  GRID_STRIDE(i, n) {
    const int ox = (int)(i % W), oy = (int)((i / W) % H);
    const float* src = logits + (i / ((long)W * H)) * ((long)h * w);
    float xv;
    if (same) {
      xv = src[(long)oy * w + (mirror ? w - 1 - ox : ox)];
    } else {
      int y0, y1, x0, x1;
      float ly, lx;
      tta_src(oy, sy, h, y0, y1, ly);
      tta_src(ox, sx, w, x0, x1, lx);
      if (mirror) { x0 = w - 1 - x0; x1 = w - 1 - x1; }      // column x of the un-mirrored view is column w - 1 - x of the logits
      const float hy = 1.f - ly, hx = 1.f - lx;
      const float v00 = src[(long)y0 * w + x0], v01 = src[(long)y0 * w + x1];
      const float v10 = src[(long)y1 * w + x0], v11 = src[(long)y1 * w + x1];
      xv = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
    }
    const float e = expf(-fabsf(xv));
    const float p = weight * (xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e));
    acc[i] = first ? p : acc[i] + p;
  }
}
void launch_tta_accumulate(const float* logits, float* acc, int B, int h, int w, int H, int W, int mirror, float weight,
                           int first, hipStream_t s) {
  const long n = (long)B * H * W;
  hipLaunchKernelGGL(tta_accumulate_kernel, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, logits, acc, B, h, w, H, W,
                     (float)h / (float)H, (float)w / (float)W, mirror, weight, first);
}
__global__ void merge_labels_kernel(const float* __restrict__ probs, int n_obj, long n_pix,
                                    uint8_t* __restrict__ labels) {
  GRID_STRIDE(i, n_pix) {
    float best = probs[i];
    int arg = 0;
    for (int o = 1; o < n_obj; ++o) {
      const float v = probs[(long)o * n_pix + i];
      if (v > best) { best = v; arg = o; }
    }
    labels[i] = best < 0.5f ? 0 : (uint8_t)(arg + 1);
  }
}
void launch_merge_labels(const float* probs, int n_obj, int64_t n_pix, uint8_t* labels, hipStream_t s) {
  hipLaunchKernelGGL(merge_labels_kernel, dim3(grid_for(n_pix, 256)), dim3(256), 0, s, probs, n_obj,
                     (long)n_pix, labels);
}

// ---- fused slab reduction + per-neuron-lr SGD ----------------------------------------------------------
__global__ void sgd_update_kernel(float* __restrict__ w, const float* __restrict__ ws, int splits, long slab,
                                  const float* __restrict__ rowscale, const float* __restrict__ lr,
                                  float* __restrict__ gsum, float* __restrict__ gout, long rowlen, long n) {
  GRID_STRIDE(e, n) {
    float g = 0.f;
    for (int z = 0; z < splits; ++z) g += ws[(long)z * slab + e];
    const long row = e / rowlen;
    if (rowscale) g *= rowscale[row];
    if (lr) w[e] = w[e] - lr[row] * g;
    if (gsum) gsum[e] += g;
    if (gout) gout[e] = g;
  }
}
// 16-byte version: rowlen, slab and every base pointer are multiples of 4 floats, n < 2^31
__global__ __launch_bounds__(256) void sgd_update4_kernel(float* __restrict__ w, const float* __restrict__ ws,
                                                           int splits, int slab, const float* __restrict__ rowscale,
                                                           const float* __restrict__ lr, float* __restrict__ gsum,
                                                           float* __restrict__ gout, int rowlen, int n4) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
    const int e = i * 4;
    float4 g = *reinterpret_cast<const float4*>(ws + e);
    for (int z = 1; z < splits; ++z) {
      const float4 t = *reinterpret_cast<const float4*>(ws + (size_t)z * slab + e);
      g.x += t.x; g.y += t.y; g.z += t.z; g.w += t.w;
    }
    const int row = e / rowlen;
    if (rowscale) { const float a = rowscale[row]; g.x *= a; g.y *= a; g.z *= a; g.w *= a; }
    if (lr) {
      const float l = lr[row];
      float4 p = *reinterpret_cast<const float4*>(w + e);
      p.x -= l * g.x; p.y -= l * g.y; p.z -= l * g.z; p.w -= l * g.w;
      *reinterpret_cast<float4*>(w + e) = p;
    }
    if (gsum) {
      float4 q = *reinterpret_cast<const float4*>(gsum + e);
      q.x += g.x; q.y += g.y; q.z += g.z; q.w += g.w;
      *reinterpret_cast<float4*>(gsum + e) = q;
    }
    if (gout) *reinterpret_cast<float4*>(gout + e) = g;
  }
}
void launch_sgd_update(float* w, const float* ws, int splits, int64_t slab, const float* rowscale,
                       const float* lr, float* gsum, float* gout, int64_t rowlen, int64_t n, hipStream_t s) {
  auto al = [](const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; };
  if ((rowlen & 3) == 0 && (slab & 3) == 0 && (n & 3) == 0 && n < (1LL << 31) && al(w) && al(ws) && al(gsum) &&
      al(gout)) {
    hipLaunchKernelGGL(sgd_update4_kernel, dim3(grid_for(n / 4, 256, 2048)), dim3(256), 0, s, w, ws, splits,
                       (int)slab, rowscale, lr, gsum, gout, (int)rowlen, (int)(n / 4));
    return;
  }
  hipLaunchKernelGGL(sgd_update_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, w, ws, splits, (long)slab,
                     rowscale, lr, gsum, gout, (long)rowlen, (long)n);
}
// one block per row: glr[row] += -sum_e gsum[row][e] * G[row][e]
__global__ __launch_bounds__(256) void meta_lr_grad_kernel(const float* __restrict__ gsum,
                                                            const float* __restrict__ G, float* __restrict__ glr,
                                                            long rowlen, float weight) {
  __shared__ float sh[4];
  const long base = (long)blockIdx.x * rowlen;
  float s = 0.f;
  for (long e = threadIdx.x; e < rowlen; e += 256) s = fmaf(gsum[base + e], G[base + e], s);
  s = block_sum_256(s, sh);
  if (threadIdx.x == 0) glr[blockIdx.x] -= weight * s;
}
void launch_meta_lr_grad(const float* gsum, const float* G, float* glr, int rows, int64_t rowlen, float weight,
                         hipStream_t s) {
  hipLaunchKernelGGL(meta_lr_grad_kernel, dim3(rows), dim3(256), 0, s, gsum, G, glr, (long)rowlen, weight);
}
// the same for every trainable tensor in one launch: row r of the per-neuron lr vector covers elements
// [rbase[r], rbase[r] + rlen[r]) of the parameter arena (one launch per tensor before: 64 launches of ~6 us per meta task)
__global__ __launch_bounds__(256) void meta_lr_grad_all_kernel(const float* __restrict__ gsum, const float* __restrict__ G,
                                                                float* __restrict__ glr, const long* __restrict__ rbase,
                                                                const int* __restrict__ rlen, float weight) {
  __shared__ float sh[4];
  const long base = rbase[blockIdx.x];
  const long rowlen = rlen[blockIdx.x];
  float s = 0.f;
  for (long e = threadIdx.x; e < rowlen; e += 256) s = fmaf(gsum[base + e], G[base + e], s);
  s = block_sum_256(s, sh);
  if (threadIdx.x == 0) glr[blockIdx.x] -= weight * s;
}
void launch_meta_lr_grad_all(const float* gsum, const float* G, float* glr, const long* rbase, const int* rlen, int rows,
                             float weight, hipStream_t s) {
  hipLaunchKernelGGL(meta_lr_grad_all_kernel, dim3(rows), dim3(256), 0, s, gsum, G, glr, rbase, rlen, weight);
}

// ---- RAdam (radam.py:28-94) -----------------------------------------------------------------------------
__global__ void radam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, long n, float lr, float wd, float beta1, float beta2,
                             float eps, float step_size, int use_denom, float grad_scale, float grad_clip) {
  GRID_STRIDE(i, n) {
    float gr = g[i] * grad_scale;
    if (grad_clip > 0.f) gr = fminf(fmaxf(gr, -grad_clip), grad_clip);
    float vv, mm, pv = p[i];
    {   // every product rounded on its own, as the separate tensor ops of radam.py:58-59,83-84 round them: only the final
        // multiply-add below may be contracted
#pragma clang fp contract(off)
      vv = v[i] * beta2 + (1.f - beta2) * gr * gr;
      mm = m[i] * beta1 + (1.f - beta1) * gr;
      if (wd != 0.f) pv += (-wd * lr) * pv;
    }
    v[i] = vv;
    m[i] = mm;
    if (use_denom) pv += (-step_size * lr) * (mm / (sqrtf(vv) + eps));
    else pv += (-step_size * lr) * mm;
    p[i] = pv;
  }
}
void launch_radam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float wd, float beta1,
                  float beta2, float eps, float step_size, int use_denom, float grad_scale, float grad_clip,
                  hipStream_t s) {
  hipLaunchKernelGGL(radam_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, p, g, m, v, (long)n, lr, wd, beta1,
                     beta2, eps, step_size, use_denom, grad_scale, grad_clip);
}
// one RAdam element update, the arithmetic (and its order) of radam_kernel above
__device__ __forceinline__ float outer_radam(float pv, float graw, float& mm, float& vv, float lr, float wd, const OuterHyper& h) {
  float gr = graw * h.grad_scale;
  if (h.grad_clip > 0.f) gr = fminf(fmaxf(gr, -h.grad_clip), h.grad_clip);
  {   // (no contraction here either: see radam_kernel)
#pragma clang fp contract(off)
    vv = vv * h.beta2 + (1.f - h.beta2) * gr * gr;
    mm = mm * h.beta1 + (1.f - h.beta1) * gr;
    if (wd != 0.f) pv += (-wd * lr) * pv;
  }
  if (h.use_denom) pv += (-h.step_size * lr) * (mm / (sqrtf(vv) + h.eps));
  else pv += (-h.step_size * lr) * mm;
  return pv;
}
// Workgroups [0, lr_blocks): the lr state (1024 elements each); the rest: the init part, tensor by tensor in OIHW order
// (the 4 state streams are read and written coalesced; the two engine-layout writes are scattered by the O,(kh,kw),I permute
// -- neighbouring threads of a 3x3 conv write kh*kw lines apart, the L2 merges them into full lines).
__global__ __launch_bounds__(256) void outer_step_kernel(const OuterEnt* __restrict__ tab, int nent, int lr_blocks,
                                                          float* __restrict__ state, float* __restrict__ grad, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ Winit, float* __restrict__ Wp,
                                                          float* __restrict__ lr_eff, const OuterHyper h) {
  if ((int)blockIdx.x < lr_blocks) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long i = (long)blockIdx.x * 1024 + j * 256 + threadIdx.x;
      if (i >= h.n_lr) break;
      float mm = m[i], vv = v[i];
      float pv = outer_radam(state[i], grad[i], mm, vv, i < h.frozen_lr ? 0.f : h.lr_lr, 0.f, h);
      pv = fminf(fmaxf(pv, h.lr_lo), h.lr_hi);                 // clamp_init_lr
      m[i] = mm; v[i] = vv; state[i] = pv; grad[i] = 0.f;
      if (lr_eff) lr_eff[i] = h.use_log ? expf(pv) : pv;
    }
    return;
  }
  __shared__ int blk0s[256];
  for (int i = threadIdx.x; i < nent; i += 256) blk0s[i] = tab[i].blk0;
  __syncthreads();
  const int wb = (int)blockIdx.x - lr_blocks;
  int lo = 0, hi = nent - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (wb >= blk0s[mid]) lo = mid; else hi = mid - 1;
  }
  const OuterEnt t = tab[lo];
  const int wsize = t.O * t.I * t.T;
  float* const st = state + h.n_lr;
  float* const gr = grad + h.n_lr;
  float* const mo = m + h.n_lr;
  float* const vo = v + h.n_lr;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = (wb - t.blk0) * 1024 + j * 256 + threadIdx.x;
    if (e >= t.n) break;
    const long f = t.off + e;                                 // flat (OIHW) index = [o][i][t]
    float mm = mo[f], vv = vo[f];
    const float pv = outer_radam(st[f], gr[f], mm, vv, f < h.frozen_param ? 0.f : h.init_lr, h.wd, h);
    mo[f] = mm; vo[f] = vv; st[f] = pv; gr[f] = 0.f;
    long d = f;                                               // engine layout [o][t][i]; the bias keeps its place
    if (e < wsize && t.T > 1) {
      const int tt = e % t.T, io = e / t.T;
      const int ii = io % t.I, oo = io / t.I;
      d = t.off + ((long)oo * t.T + tt) * t.I + ii;
    }
    Winit[d] = pv;
    Wp[d] = pv;
  }
}
void launch_outer_step(const OuterEnt* tab, int nent, int lr_blocks, int nblocks, float* state, float* grad, float* m, float* v,
                       float* Winit, float* Wp, float* lr_eff, const OuterHyper& h, hipStream_t s) {
  hipLaunchKernelGGL(outer_step_kernel, dim3(nblocks), dim3(256), 0, s, tab, nent, lr_blocks, state, grad, m, v, Winit, Wp, lr_eff, h);
}
__global__ void clamp_kernel(float* p, long n, float lo, float hi) {
  GRID_STRIDE(i, n) p[i] = fminf(fmaxf(p[i], lo), hi);
}
void launch_clamp(float* p, int64_t n, float lo, float hi, hipStream_t s) {
  hipLaunchKernelGGL(clamp_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, p, (long)n, lo, hi);
}

// ---- learning-rate hierarchy levels (meta_optim.py:27-67,157-163,180-185) -------------------------
// The update always consumes a per-neuron (or per-element) EFFECTIVE lr; the learned state is stored
// per tensor (TENSOR), once (SINGLE), per neuron or per element, possibly as log(lr).
// level: 0 NEURON, 1 TENSOR, 2 SINGLE
__global__ void lr_expand_kernel(const float* __restrict__ store, const int* __restrict__ row_tensor,
                                 float* __restrict__ lr, int nlr, int level, int use_log) {
  GRID_STRIDE(r, nlr) {
    const float v = store[level == 0 ? r : (level == 1 ? row_tensor[r] : 0)];
    lr[r] = use_log ? expf(v) : v;
  }
}
void launch_lr_expand(const float* store, const int* row_tensor, float* lr, int nlr, int level, int use_log,
                      hipStream_t s) {
  hipLaunchKernelGGL(lr_expand_kernel, dim3(grid_for(nlr, 256)), dim3(256), 0, s, store, row_tensor, lr, nlr, level,
                     use_log);
}
__global__ void exp_inplace_kernel(float* p, long n) {
  GRID_STRIDE(i, n) p[i] = expf(p[i]);
}
void launch_exp_inplace(float* p, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(exp_inplace_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, p, (long)n);
}
// d/d store from the per-neuron d/d lr: chain rule of exp() for log storage, then the sum over the
// neurons that share a stored value (autograd of `repeat` / broadcasting).  One block per stored value
// group: block t reduces rows [row0[t], row0[t+1]).
__global__ __launch_bounds__(256) void lr_grad_reduce_kernel(const float* __restrict__ g, const float* __restrict__ lr,
                                                              const int* __restrict__ row0, float* __restrict__ out,
                                                              int use_log) {
  __shared__ float sh[4];
  const int lo = row0[blockIdx.x], hi = row0[blockIdx.x + 1];
  float s = 0.f;
  for (int r = lo + threadIdx.x; r < hi; r += 256) s += use_log ? g[r] * lr[r] : g[r];
  s = block_sum_256(s, sh);
  if (threadIdx.x == 0) out[blockIdx.x] += s;
}
void launch_lr_grad_reduce(const float* g, const float* lr, const int* row0, float* out, int ngroups, int use_log,
                           hipStream_t s) {
  hipLaunchKernelGGL(lr_grad_reduce_kernel, dim3(ngroups), dim3(256), 0, s, g, lr, row0, out, use_log);
}
__global__ void lr_grad_neuron_kernel(const float* __restrict__ g, const float* __restrict__ lr,
                                      float* __restrict__ out, int n, int use_log) {
  GRID_STRIDE(r, n) out[r] += use_log ? g[r] * lr[r] : g[r];
}
void launch_lr_grad_neuron(const float* g, const float* lr, float* out, int n, int use_log, hipStream_t s) {
  hipLaunchKernelGGL(lr_grad_neuron_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, g, lr, out, n, use_log);
}
// PARAM level: out[e] = -gsum[e] * G[e] (* lr_elem[e] for log storage), engine layout
__global__ void meta_lr_grad_elem_kernel(const float* __restrict__ gsum, const float* __restrict__ G,
                                         const float* __restrict__ lr_elem, float* __restrict__ out, long n) {
  GRID_STRIDE(i, n) {
    float v = -gsum[i] * G[i];
    if (lr_elem) v *= lr_elem[i];
    out[i] = v;
  }
}
void launch_meta_lr_grad_elem(const float* gsum, const float* G, const float* lr_elem, float* out, int64_t n,
                              hipStream_t s) {
  hipLaunchKernelGGL(meta_lr_grad_elem_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, gsum, G, lr_elem, out,
                     (long)n);
}

}  // namespace eosvos

// ---- one launch for the whole network's update ----------------------------------------------------
// All weight-gradient slabs of a backward pass stay parked in one arena; this kernel walks a
// per-layer table and, for every parameter, sums its slabs in order, applies the frozen-norm
// row scale and the per-neuron learning rate (theta <- theta - lr[cout] * g), and optionally
// accumulates / exports g.  One launch instead of 64, every CU busy, weights read+written once.
namespace eosvos {
__global__ __launch_bounds__(256) void sgd_update_all_kernel(const UpdEntry* __restrict__ tab, int nent,
                                                              float* __restrict__ W, const float* __restrict__ ws,
                                                              const float* __restrict__ na, const float* __restrict__ lr,
                                                              const float* __restrict__ lr_elem,
                                                              float* __restrict__ gsum, float* __restrict__ gout,
                                                              unsigned* __restrict__ amax_w) {
  // locate this workgroup's table entry: first-block offsets to LDS, then a binary search
  __shared__ int blk0s[256];
  for (int i = threadIdx.x; i < nent; i += 256) blk0s[i] = tab[i].blk0;
  __syncthreads();
  int lo = 0, hi = nent - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)blockIdx.x >= blk0s[mid]) lo = mid; else hi = mid - 1;
  }
  const UpdEntry t = tab[lo];
  unsigned* const aslot = (amax_w && t.amax_idx >= 0) ? amax_w + t.amax_idx : nullptr;
  unsigned am = 0;
  constexpr int CH = UPD_CHUNKS;        // 1024-element chunks per workgroup, all in flight together
  const int base = ((int)blockIdx.x - t.blk0) * (1024 * CH) + threadIdx.x * 4;
  const size_t zstride = (size_t)t.slab;
  if (((t.slab | t.n) & 3) == 0) {
    // the weights and the first slabs of all chunks are
    // requested before anything is consumed (the large layers have only 4-8 slabs, so a one-chunk loop
    // left the memory pipe nearly empty)
    float4 w4[CH], g4[CH];
    bool ok[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = base + c * 1024;
      ok[c] = e < t.n;
      g4[c] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ok[c]) w4[c] = *reinterpret_cast<const float4*>(W + t.w_off + e);
    }
    // slabs in groups of 8 predicated loads: all of a group are in flight together whatever the trip count
    // (a plain loop's remainder iterations each waited for their own load: 4-8 slabs = 4-8 serial latencies)
    for (int z0 = 0; z0 < t.splits; z0 += 8) {
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        if (!ok[c]) continue;
        const float* sp = ws + t.ws_off + base + c * 1024;
        float4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          v[i] = (z0 + i < t.splits) ? *reinterpret_cast<const float4*>(sp + (size_t)(z0 + i) * zstride)
                                     : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 8; ++i) { g4[c].x += v[i].x; g4[c].y += v[i].y; g4[c].z += v[i].z; g4[c].w += v[i].w; }
      }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (!ok[c]) continue;
      const int e = base + c * 1024;
      const int row = e / t.rowlen;
      float4 g = g4[c];
      const bool one_row = (t.rowlen & 3) == 0;       // else the float4 may straddle output channels (stem: 147)
      int r1 = row, r2 = row, r3 = row;
      if (!one_row) { r1 = (e + 1) / t.rowlen; r2 = (e + 2) / t.rowlen; r3 = (e + 3) / t.rowlen; }
      if (t.norm_off >= 0) {
        const float* a = na + t.norm_off;
        g.x *= a[row]; g.y *= a[r1]; g.z *= a[r2]; g.w *= a[r3];
      }
      if (lr_elem) {                                  // lr_hierarchy_level PARAM
        const float4 l = *reinterpret_cast<const float4*>(lr_elem + t.w_off + e);
        w4[c].x -= l.x * g.x; w4[c].y -= l.y * g.y; w4[c].z -= l.z * g.z; w4[c].w -= l.w * g.w;
        *reinterpret_cast<float4*>(W + t.w_off + e) = w4[c];
      } else if (lr) {
        const float* l = lr + t.lr_off;
        w4[c].x -= l[row] * g.x; w4[c].y -= l[r1] * g.y; w4[c].z -= l[r2] * g.z; w4[c].w -= l[r3] * g.w;
        *reinterpret_cast<float4*>(W + t.w_off + e) = w4[c];
      }
      if (gsum) {
        float4 q = *reinterpret_cast<const float4*>(gsum + t.w_off + e);
        q.x += g.x; q.y += g.y; q.z += g.z; q.w += g.w;
        *reinterpret_cast<float4*>(gsum + t.w_off + e) = q;
      }
      if (gout) *reinterpret_cast<float4*>(gout + t.w_off + e) = g;
      am = amax_f4(am, w4[c]);
    }
    if (aslot) amax_block_commit(am, aslot);
    return;
  }
  // odd-sized tensors (the classifier's 256 weights + bias): element per thread, coalesced, the slab
  // loop unrolled so that 8 loads per element are in flight (these tensors come with ~1000 slabs)
  const int cbase = ((int)blockIdx.x - t.blk0) * (1024 * CH);
  for (int j = 0; j < 4 * CH; ++j) {
    const int e = cbase + j * 256 + threadIdx.x;
    if (e >= t.n) break;
    const float* sp = ws + t.ws_off + e;
    float acc8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int z = 0;
    for (; z + 8 <= t.splits; z += 8) {
#pragma unroll
      for (int i = 0; i < 8; ++i) acc8[i] += sp[(size_t)(z + i) * zstride];
    }
    // sequential order of the additions is kept per lane i; lanes are combined in a fixed order
    for (; z < t.splits; ++z) acc8[z & 7] += sp[(size_t)z * zstride];
    float gv = ((acc8[0] + acc8[1]) + (acc8[2] + acc8[3])) + ((acc8[4] + acc8[5]) + (acc8[6] + acc8[7]));
    const int row = e / t.rowlen;
    if (t.norm_off >= 0) gv *= na[t.norm_off + row];
    float* wp = W + t.w_off + e;
    if (lr_elem) *wp = *wp - lr_elem[t.w_off + e] * gv;
    else if (lr) *wp = *wp - lr[t.lr_off + row] * gv;
    if (gsum) gsum[t.w_off + e] += gv;
    if (gout) gout[t.w_off + e] = gv;
  }
}
void launch_sgd_update_all(const UpdEntry* tab, int nent, int nblocks, float* W, const float* ws, const float* na,
                           const float* lr, const float* lr_elem, float* gsum, float* gout, hipStream_t s, unsigned* amax_w) {
  hipLaunchKernelGGL(sgd_update_all_kernel, dim3(nblocks), dim3(256), 0, s, tab, nent, W, ws, na, lr, lr_elem, gsum,
                     gout, amax_w);
}
}  // namespace eosvos

// ---- GroupNorm(16, C) with frozen affine (deeplabv3plus.py:180-191) ---------------------------------
// NHWC tensors / channel slices (ld = floats per pixel, C % 4 == 0).  Statistics per (image, group) over P pixels x C/16
// channels.  Round 5: every pass moves whole float4 rows (the round-1 kernels read one float per thread and divided a
// 64-bit index per element: 2.5 TB/s): a workgroup owns a run of pixels of ONE image and a block of <= 256 float4 columns,
// a thread keeps its column, so its 4 channels' group constants are computed once; the statistics are reduced per thread ->
// per column -> per group in a fixed order (deterministic), one float2 partial per (image, group, pixel chunk), summed in
// double by one wave per (image, group).  The passes that WRITE a tensor a contraction will read (y = gn(z), dz) also reduce
// its absmax for the f16x3 mode (round 4 ran a standalone pass per consumer: 114 launches per iteration).
namespace eosvos {
#define GN_UNROLL 8
#define GN_MAX_CHUNKS 128      // (16 lanes x 8 loads in flight finish a group in the apply pass's prologue)
struct GnGeom { int ncol, rows, chunks, colblocks, per; };
static inline GnGeom gn_geom(int B, int P, int C) {
  GnGeom g;
  const int C4 = C / 4;
  g.colblocks = (C4 + 255) / 256;
  g.ncol = C4 / g.colblocks;                       // C4 in {12, 16, 32, ..., 256, 512}: divides evenly
  g.rows = 256 / g.ncol;
  // about 4 workgroups per CU over the whole launch, 8 rows (128 bytes per lane) in flight each; >= 8 passes per workgroup
  long want = 1024 / ((long)B * g.colblocks);
  long most = P / (8L * g.rows);
  if (want > most) want = most;
  if (want > GN_MAX_CHUNKS) want = GN_MAX_CHUNKS;
  if (want < 1) want = 1;
  g.chunks = (int)want;
  g.per = (P + g.chunks - 1) / g.chunks;
  return g;
}
// per-thread sums -> partial[(b * 16 + grp) * chunks + chunk]; s1 / s2: this thread's 4 channels
__device__ __forceinline__ void gn_reduce_groups(float (&s1)[4], float (&s2)[4], float* sh /*[8][256]*/, int ncol, int rows, int col0,
                                                 int cg, int b, int chunk, int chunks, float2* __restrict__ partial) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) { sh[j * 256 + tid] = s1[j]; sh[(4 + j) * 256 + tid] = s2[j]; }
  __syncthreads();
  if (tid < ncol) {                                // rows of one column, in row order
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float a = sh[k * 256 + tid];
      for (int r = 1; r < rows; ++r) a += sh[k * 256 + r * ncol + tid];
      sh[k * 256 + tid] = a;
    }
  }
  __syncthreads();
  const int ch0 = col0 * 4, nch = ncol * 4;        // channels [ch0, ch0 + nch) belong to this workgroup
  const int g0 = ch0 / cg, ng = nch / cg;          // whole groups (cg divides nch for every C of the network)
  if (tid < ng) {
    float a = 0.f, q = 0.f;
    for (int c = tid * cg; c < (tid + 1) * cg; ++c) { a += sh[(c & 3) * 256 + (c >> 2)]; q += sh[(4 + (c & 3)) * 256 + (c >> 2)]; }
    partial[((size_t)b * 16 + g0 + tid) * chunks + chunk] = make_float2(a, q);
  }
}
// The forward sums are shifted by a pivot per (image, group), the group's first channel at pixel 0 (gn_pivot): E[d^2] - E[d]^2
// of d = z - pivot loses no precision to a mean far from zero (unshifted fp32 sums of z^2 cancel like (mean / std)^2).
__device__ __forceinline__ float gn_pivot(const float* __restrict__ z, int ldz, int b, int P, int ch, int cg) {
  return z[(size_t)b * P * ldz + (ch / cg) * cg];
}
// forward: (u, v) = (d, d^2), d = z - pivot;  backward: (gamma g, gamma g zhat)
template <bool BWD>
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ z, int ldz, const float* __restrict__ g, int ldg,
                                                        const float* __restrict__ gamma, const float* __restrict__ stats,
                                                        float2* __restrict__ partial, int P, int C, GnGeom gm) {
  __shared__ float sh[8 * 256];
  const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y, col0 = blockIdx.z * gm.ncol;
  const int cg = C >> 4;
  const int col = tid % gm.ncol, row = tid / gm.ncol;
  const bool act = row < gm.rows;
  const int c = (col0 + col) * 4;
  const int p0 = chunk * gm.per;
  int p1 = p0 + gm.per;
  if (p1 > P) p1 = P;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  float ga[4] = {1.f, 1.f, 1.f, 1.f}, mu[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {1.f, 1.f, 1.f, 1.f};
  if (BWD && act) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int bg = b * 16 + (c + j) / cg;
      ga[j] = gamma[c + j]; mu[j] = stats[bg * 2]; rs[j] = stats[bg * 2 + 1];
    }
  } else if (act) {
#pragma unroll
    for (int j = 0; j < 4; ++j) mu[j] = gn_pivot(z, ldz, b, P, c + j, cg);     // forward: mu = the pivot
  }
  if (act) {
    const float* zp = z + (size_t)b * P * ldz + c;
    const float* gp = BWD ? g + (size_t)b * P * ldg + c : nullptr;
    int p = p0 + row;
    for (; p + (GN_UNROLL - 1) * gm.rows < p1; p += GN_UNROLL * gm.rows) {            // GN_UNROLL rows in flight
      float4 zv[GN_UNROLL], gv[GN_UNROLL];
#pragma unroll
      for (int u = 0; u < GN_UNROLL; ++u) {
        zv[u] = *reinterpret_cast<const float4*>(zp + (size_t)(p + u * gm.rows) * ldz);
        if (BWD) gv[u] = *reinterpret_cast<const float4*>(gp + (size_t)(p + u * gm.rows) * ldg);
      }
#pragma unroll
      for (int u = 0; u < GN_UNROLL; ++u) {
        const float zz[4] = {zv[u].x, zv[u].y, zv[u].z, zv[u].w};
        const float gg[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (BWD) { const float t = ga[j] * gg[j]; s1[j] += t; s2[j] += t * ((zz[j] - mu[j]) * rs[j]); }
          else { const float d = zz[j] - mu[j]; s1[j] += d; s2[j] += d * d; }
        }
      }
    }
    for (; p < p1; p += gm.rows) {
      const float4 zv = *reinterpret_cast<const float4*>(zp + (size_t)p * ldz);
      float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (BWD) gv = *reinterpret_cast<const float4*>(gp + (size_t)p * ldg);
      const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
      const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (BWD) { const float t = ga[j] * gg[j]; s1[j] += t; s2[j] += t * ((zz[j] - mu[j]) * rs[j]); }
        else { const float d = zz[j] - mu[j]; s1[j] += d; s2[j] += d * d; }
      }
    }
  }
  gn_reduce_groups(s1, s2, sh, gm.ncol, gm.rows, col0, cg, b, chunk, gm.chunks, partial);
}
// The (image, group) totals of this workgroup's groups from the per-chunk partials, summed in double in a fixed order by 16
// lanes per group (every workgroup of the launch computes the same bits; round 5: this replaces a 5 us launch per pass, 124
// per iteration).  st[g] = {mean, rstd} (forward; also written to `stats_out` by the chunk-0 workgroups: the backward pass
// reads it) or {S1 / n, S2 / n} (backward).  Forward: the partials are shifted by gn_pivot of z.
__device__ __forceinline__ void gn_finish_groups(const float2* __restrict__ partial, int chunks, int b, int g0, int ng, double inv_n,
                                                 float eps, bool bwd, float* __restrict__ stats_out, float (*st)[2],
                                                 const float* __restrict__ z, int ldz, int P, int cg) {
  const int gi = threadIdx.x >> 4, l = threadIdx.x & 15;
  double a = 0.0, q = 0.0;
  if (gi < ng) {
    const float2* pp = partial + ((size_t)b * 16 + g0 + gi) * chunks;
    float2 v[GN_MAX_CHUNKS / 16];
#pragma unroll
    for (int k = 0; k < GN_MAX_CHUNKS / 16; ++k) v[k] = (l + 16 * k) < chunks ? pp[l + 16 * k] : make_float2(0.f, 0.f);      // all in flight
#pragma unroll
    for (int k = 0; k < GN_MAX_CHUNKS / 16; ++k) { a += v[k].x; q += v[k].y; }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); q += __shfl_xor(q, o, 64); }
  if (gi < ng && l == 0) {
    if (bwd) { st[gi][0] = (float)(a * inv_n); st[gi][1] = (float)(q * inv_n); }
    else {
      const double dm = a * inv_n;
      double var = q * inv_n - dm * dm;
      if (var < 0.0) var = 0.0;
      st[gi][0] = (float)((double)gn_pivot(z, ldz, b, P, (g0 + gi) * cg, cg) + dm);
      st[gi][1] = (float)(1.0 / sqrt(var + (double)eps));
      if (stats_out && blockIdx.x == 0) { stats_out[(b * 16 + g0 + gi) * 2] = st[gi][0]; stats_out[(b * 16 + g0 + gi) * 2 + 1] = st[gi][1]; }
    }
  }
  __syncthreads();
}
// forward:  y = relu?((z - mean) * rstd * gamma + beta (+ res))                       (absmax of y into `amax`)
// backward: z <- rstd * (gamma * g - S1 / n - zhat * S2 / n), zhat = (z - mean) rstd  (absmax of dz into `amax`)
template <bool BWD>
__global__ __launch_bounds__(256) void gn_apply_kernel(float* __restrict__ z, int ldz, const float* __restrict__ g, int ldg,
                                                        float* __restrict__ stats, const float2* __restrict__ partial, double inv_n, float eps,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float* __restrict__ res, int ldres, float* __restrict__ y, int ldy,
                                                        int P, int C, int relu, GnGeom gm, unsigned* __restrict__ amax,
                                                        uint8_t* __restrict__ m8, int ldm8) {
  __shared__ float st[16][2];
  const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y, col0 = blockIdx.z * gm.ncol;
  const int cg = C >> 4;
  const int g0 = col0 * 4 / cg;
  gn_finish_groups(partial, gm.chunks, b, g0, gm.ncol * 4 / cg, inv_n, eps, BWD, BWD ? nullptr : stats, st, z, ldz, P, cg);
  const int col = tid % gm.ncol, row = tid / gm.ncol;
  const bool act = row < gm.rows;
  const int c = (col0 + col) * 4;
  const int p0 = chunk * gm.per;
  int p1 = p0 + gm.per;
  if (p1 > P) p1 = P;
  unsigned am = 0;
  if (act) {
    // forward: y = (z - mu) * ka + kc;  backward: dz = g * ka - (k1 + zhat * k2), zhat = (z - mu) * rs
    float ka[4], mu[4], rs[4], kc[4], k2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gl = (c + j) / cg - g0, bg = b * 16 + g0 + gl;
      if (BWD) { mu[j] = stats[bg * 2]; rs[j] = stats[bg * 2 + 1]; kc[j] = rs[j] * st[gl][0]; k2[j] = rs[j] * st[gl][1]; }
      else { mu[j] = st[gl][0]; rs[j] = st[gl][1]; kc[j] = beta[c + j]; k2[j] = 0.f; }
      ka[j] = rs[j] * gamma[c + j];
    }
    float* zp = z + (size_t)b * P * ldz + c;
    const float* gp = BWD ? g + (size_t)b * P * ldg + c : nullptr;
    const float* rp = (!BWD && res) ? res + (size_t)b * P * ldres + c : nullptr;
    float* yp = BWD ? nullptr : y + (size_t)b * P * ldy + c;
    auto one = [&](const float4& zv, const float4& xv) -> float4 {      // xv: g (backward) or the residual (forward)
      float4 o;
      const float zz[4] = {zv.x, zv.y, zv.z, zv.w}, xx[4] = {xv.x, xv.y, xv.z, xv.w};
      float oo[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (BWD) oo[j] = xx[j] * ka[j] - (kc[j] + ((zz[j] - mu[j]) * rs[j]) * k2[j]);
        else {
          oo[j] = (zz[j] - mu[j]) * ka[j] + kc[j] + xx[j];
          if (relu) oo[j] = fmaxf(oo[j], 0.f);
        }
      }
      o = make_float4(oo[0], oo[1], oo[2], oo[3]);
      return o;
    };
    int p = p0 + row;
    for (; p + (GN_UNROLL - 1) * gm.rows < p1; p += GN_UNROLL * gm.rows) {
      float4 zv[GN_UNROLL], xv[GN_UNROLL];
#pragma unroll
      for (int u = 0; u < GN_UNROLL; ++u) {
        const size_t pp = (size_t)(p + u * gm.rows);
        zv[u] = *reinterpret_cast<const float4*>(zp + pp * ldz);
        if (BWD) xv[u] = *reinterpret_cast<const float4*>(gp + pp * ldg);
        else xv[u] = rp ? *reinterpret_cast<const float4*>(rp + pp * ldres) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < GN_UNROLL; ++u) {
        const size_t pp = (size_t)(p + u * gm.rows);
        const float4 o = one(zv[u], xv[u]);
        am = amax_f4(am, o);
        if (BWD) *reinterpret_cast<float4*>(zp + pp * ldz) = o;
        else {
          *reinterpret_cast<float4*>(yp + pp * ldy) = o;
          if (m8) m8[((size_t)b * P + pp) * ldm8 + (c >> 2)] = relu_bits(o);
        }
      }
    }
    for (; p < p1; p += gm.rows) {
      const float4 zv = *reinterpret_cast<const float4*>(zp + (size_t)p * ldz);
      float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (BWD) xv = *reinterpret_cast<const float4*>(gp + (size_t)p * ldg);
      else if (rp) xv = *reinterpret_cast<const float4*>(rp + (size_t)p * ldres);
      const float4 o = one(zv, xv);
      am = amax_f4(am, o);
      if (BWD) *reinterpret_cast<float4*>(zp + (size_t)p * ldz) = o;
      else {
        *reinterpret_cast<float4*>(yp + (size_t)p * ldy) = o;
        if (m8) m8[((size_t)b * P + p) * ldm8 + (c >> 2)] = relu_bits(o);
      }
    }
  }
  if (amax) amax_block_commit(am, amax);
}
int gn_partial_floats(int B) { return B * 16 * GN_MAX_CHUNKS * 2; }
void launch_gn_forward(const float* z, int ldz, const float* gamma, const float* beta, const float* res, int ldres,
                       float* y, int ldy, float* stats, float* partial, int B, int P, int C, float eps, int relu,
                       hipStream_t s, unsigned* amax_y, uint8_t* m8, int ldm8) {
  const GnGeom gm = gn_geom(B, P, C);
  const dim3 grid(gm.chunks, B, gm.colblocks);
  const double inv_n = 1.0 / ((double)P * (C / 16));
  hipLaunchKernelGGL((gn_stats_kernel<false>), grid, dim3(256), 0, s, z, ldz, nullptr, 0, nullptr, nullptr, (float2*)partial, P, C, gm);
  hipLaunchKernelGGL((gn_apply_kernel<false>), grid, dim3(256), 0, s, const_cast<float*>(z), ldz, nullptr, 0, stats, (const float2*)partial,
                     inv_n, eps, gamma, beta, res, ldres, y, ldy, P, C, relu, gm, amax_y, relu ? m8 : nullptr, ldm8);
}
void launch_gn_backward(float* z, int ldz, const float* g, int ldg, const float* gamma, const float* stats,
                        float* partial, int B, int P, int C, hipStream_t s, unsigned* amax_dz) {
  const GnGeom gm = gn_geom(B, P, C);
  const dim3 grid(gm.chunks, B, gm.colblocks);
  const double inv_n = 1.0 / ((double)P * (C / 16));
  hipLaunchKernelGGL((gn_stats_kernel<true>), grid, dim3(256), 0, s, z, ldz, g, ldg, gamma, stats, (float2*)partial, P, C, gm);
  hipLaunchKernelGGL((gn_apply_kernel<true>), grid, dim3(256), 0, s, z, ldz, g, ldg, const_cast<float*>(stats), (const float2*)partial, inv_n,
                     0.f, gamma, nullptr, nullptr, 0, nullptr, 0, P, C, 0, gm, amax_dz, nullptr, 0);
}
}  // namespace eosvos

// ---- the device losses and their gradients (launch_loss): BCE with logits (mean), dice / BCE+dice, class-balanced BCE ----
// One `template <bool VOID>` kernel family per loss.  VOID = true is the loss with a void label: a pixel with t == ign is in
// no sum and no count and its gradient is +0; its logit is selected away, never multiplied by 0 (it may be NaN / inf); the
// valid pixels are counted per block (integers, summed in a fixed order) and |V| takes the place of n.  VOID = false compiles
// the select, the count and the |V| == 0 results out: it reads no count buffer and V = n.  Grids, per-thread accumulation order
// and expressions are shared, so a map without a void pixel gives the bits of the plain launch.
// Every kind is partial -> final -> grad, the scalars of `final` staying on the device, but plain BCE: its 1 / n is known on
// the host, so the first pass writes the gradient too.  Scratch layout: LOSS_SCAL, LOSS_CNT (kernels.h).
namespace eosvos {
// |V| from the per-block counts, valid in every thread
__device__ __forceinline__ long valid_total(const int* __restrict__ cnt, int nb, int* shi) {
  long c = 0;                                     // (a block counts < 2^31 pixels; the total may not fit an int)
  for (int i = threadIdx.x; i < nb; i += 256) c += cnt[i];
  const int lo = block_sum_i((int)(c & 0xffff), shi), hi = block_sum_i((int)(c >> 16), shi);
  return ((long)hi << 16) + lo;
}
// (bce_value / bce_grad: loss_expr.h, shared with bootstrap_kernels.hip)
// VOID = false: dx = dL/dx with the host's inv_n = 1 / n
template <bool VOID>
__global__ __launch_bounds__(256) void bce_partial_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                           float* __restrict__ dx, float* __restrict__ partial,
                                                           int* __restrict__ cnt, long n, float inv_n, float ign) {
  __shared__ float sh[4];
  __shared__ int shi[4];
  float s = 0.f;
  int c = 0;
  GRID_STRIDE(i, n) {
    const float xv = x[i], tv = t[i];
    const bool ok = !VOID || tv != ign;
    const float e = expf(-fabsf(xv));
    const float v = bce_value(xv, tv, e);
    s = ok ? s + v : s;
    c += ok ? 1 : 0;
    if constexpr (!VOID) dx[i] = bce_grad(xv, tv, e, inv_n);
  }
  s = block_sum_256(s, sh);
  if constexpr (VOID) c = block_sum_i(c, shi);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = s;
    if constexpr (VOID) cnt[blockIdx.x] = c;
  }
}
// VOID: scal = {loss, 1 / |V|} (0 for an empty V)
template <bool VOID>
__global__ __launch_bounds__(256) void bce_final_kernel(const float* __restrict__ partial, const int* __restrict__ cnt,
                                                         float* __restrict__ loss, float* __restrict__ scal, int nb,
                                                         float inv_n) {
  __shared__ float sh[4];
  __shared__ int shi[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) s += partial[i];
  s = block_sum_256(s, sh);
  if constexpr (VOID) {
    const long V = valid_total(cnt, nb, shi);
    if (threadIdx.x == 0) {
      const float inv = V > 0 ? 1.0f / (float)V : 0.f;
      loss[0] = V > 0 ? s * inv : 0.f;
      scal[0] = loss[0]; scal[1] = inv;
    }
  } else if (threadIdx.x == 0) {
    loss[0] = s * inv_n;
  }
}
// the third pass of BCE with a void label
__global__ void bce_grad_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ scal,
                                float* __restrict__ dx, long n, float ign) {
  const float inv_n = scal[1];
  GRID_STRIDE(i, n) {
    const float xv = x[i], tv = t[i];
    const float e = expf(-fabsf(xv));
    const float g = bce_grad(xv, tv, e, inv_n);
    dx[i] = tv != ign ? g : 0.f;
  }
}
// dice / BCE+dice (loss_dice.py:4-40, helper_func.py:43-54), batch_average=True
// stage 1: per-block partials {sum p*y, sum p, sum y, sum bce}; stage 2: scalars; stage 3: dlogits
template <bool VOID>
__global__ __launch_bounds__(256) void dice_partial_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                            float4* __restrict__ partial, int* __restrict__ cnt, long n,
                                                            float ign) {
  __shared__ float sh[4];
  __shared__ int shi[4];
  float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
  int k = 0;
  GRID_STRIDE(i, n) {
    const float xv = x[i], tv = t[i];
    const bool ok = !VOID || tv != ign;
    const float e = expf(-fabsf(xv));
    const float p = xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    const float v = fmaxf(xv, 0.f) - xv * tv + log1pf(e);
    a = ok ? a + p * tv : a; b = ok ? b + p : b; c = ok ? c + tv : c;
    d = ok ? d + v : d;
    k += ok ? 1 : 0;
  }
  a = block_sum_256(a, sh); b = block_sum_256(b, sh); c = block_sum_256(c, sh); d = block_sum_256(d, sh);
  if constexpr (VOID) k = block_sum_i(k, shi);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = make_float4(a, b, c, d);
    if constexpr (VOID) cnt[blockIdx.x] = k;
  }
}
// scal = {loss, c_y, c_1, bce_w}:  dL/dx = bce_w*(p - y) + (c_y*y + c_1)*p*(1-p)
// VOID: |V| in the place of n; an empty V gives num = D = 1: dice = 0, -log(1 - 0) = 0, and no BCE term
template <bool VOID>
__global__ __launch_bounds__(256) void dice_final_kernel(const float4* __restrict__ partial, const int* __restrict__ cnt,
                                                          int nb, long n, int kind, float* __restrict__ loss,
                                                          float* __restrict__ scal) {
  __shared__ double sh[4][4];
  __shared__ int shi[4];
  double a = 0, b = 0, c = 0, d = 0;
  for (int i = threadIdx.x; i < nb; i += 256) { const float4 v = partial[i]; a += v.x; b += v.y; c += v.z; d += v.w; }
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); c += __shfl_xor(c, o, 64); d += __shfl_xor(d, o, 64); }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[w][0] = a; sh[w][1] = b; sh[w][2] = c; sh[w][3] = d; }
  long V = n;
  if constexpr (VOID) V = valid_total(cnt, nb, shi);   // (its barriers also publish sh)
  else __syncthreads();
  if (threadIdx.x == 0) {
    double I = 0, Sp = 0, Sy = 0, Sb = 0;
    for (int k = 0; k < 4; ++k) { I += sh[k][0]; Sp += sh[k][1]; Sy += sh[k][2]; Sb += sh[k][3]; }
    const double num = 2.0 * I + 1.0, D = Sp + Sy + 1.0;
    const double dice = 1.0 - num / D;
    const bool any = !VOID || V > 0;
    if (kind == 1) {            // dice:  dL/dp = -(2y*D - num)/D^2
      loss[0] = (float)dice;
      scal[1] = (float)(-2.0 / D); scal[2] = (float)(num / (D * D)); scal[3] = 0.f;
    } else {                    // BCE - log(1 - dice) = BCE - log(num/D):  dL/dp = -2y/num + 1/D
      loss[0] = any ? (float)(Sb / (double)V - log(num / D)) : 0.f;
      scal[1] = (float)(-2.0 / num); scal[2] = (float)(1.0 / D); scal[3] = any ? (float)(1.0 / (double)V) : 0.f;
    }
    scal[0] = loss[0];
  }
}
template <bool VOID>
__global__ void dice_grad_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ scal,
                                 float* __restrict__ dx, long n, float ign) {
  const float cy = scal[1], c1 = scal[2], bw = scal[3];
  GRID_STRIDE(i, n) {
    const float xv = x[i], tv = t[i];
    const float e = expf(-fabsf(xv));
    const float p = xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    dx[i] = (!VOID || tv != ign) ? bw * (p - tv) + (cy * tv + c1) * p * (1.f - p) : 0.f;
  }
}
// class-balanced cross entropy (loss_ce.py:15-60, batch_average = size_average = True):
//   labels = gt >= .5;  L = (N_neg * sum_pos bce + N_pos * sum_neg bce) / N^2
// VOID (loss_ce.py:42-53): N_pos, N_neg and the two sums run over V, num_total = |V|; the two trailing divisions (`:55`,
// `:58`) stay those of the tensor's full shape, n:  L = (N_neg * S_pos + N_pos * S_neg) / (|V| * n)
template <bool VOID>
__global__ __launch_bounds__(256) void cbce_partial_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                            float4* __restrict__ partial, int* __restrict__ cnt, long n,
                                                            float ign) {
  __shared__ float sh[4];
  __shared__ int shi[4];
  float a = 0.f, b = 0.f, c = 0.f;
  int k = 0;
  GRID_STRIDE(i, n) {
    const float xv = x[i], tv = t[i];
    const bool ok = !VOID || tv != ign;
    const float l = tv >= 0.5f ? 1.f : 0.f;
    const float v = fmaxf(xv, 0.f) - xv * l + log1pf(expf(-fabsf(xv)));
    a = ok ? a + l : a; b = ok ? b + l * v : b; c = ok ? c + (1.f - l) * v : c;
    k += ok ? 1 : 0;
  }
  a = block_sum_256(a, sh); b = block_sum_256(b, sh); c = block_sum_256(c, sh);
  if constexpr (VOID) k = block_sum_i(k, shi);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = make_float4(a, b, c, 0.f);
    if constexpr (VOID) cnt[blockIdx.x] = k;
  }
}
template <bool VOID>
__global__ __launch_bounds__(256) void cbce_final_kernel(const float4* __restrict__ partial, const int* __restrict__ cnt,
                                                          int nb, long n, float* __restrict__ loss,
                                                          float* __restrict__ scal) {
  __shared__ double sh[4][3];
  __shared__ int shi[4];
  double a = 0, b = 0, c = 0;
  for (int i = threadIdx.x; i < nb; i += 256) { const float4 v = partial[i]; a += v.x; b += v.y; c += v.z; }
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); c += __shfl_xor(c, o, 64); }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[w][0] = a; sh[w][1] = b; sh[w][2] = c; }
  long V = n;
  if constexpr (VOID) V = valid_total(cnt, nb, shi);   // (its barriers also publish sh)
  else __syncthreads();
  if (threadIdx.x == 0) {
    double Np = 0, Sp = 0, Sn = 0;
    for (int k = 0; k < 4; ++k) { Np += sh[k][0]; Sp += sh[k][1]; Sn += sh[k][2]; }
    const double N = (double)n, T = (double)V, Nn = T - Np;
    const bool any = !VOID || V > 0;
    loss[0] = any ? (float)((Nn * Sp + Np * Sn) / (T * N)) : 0.f;
    scal[0] = loss[0];
    scal[1] = any ? (float)(Nn / (T * N)) : 0.f; scal[2] = any ? (float)(Np / (T * N)) : 0.f;
  }
}
template <bool VOID>
__global__ void cbce_grad_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ scal,
                                 float* __restrict__ dx, long n, float ign) {
  const float wp = scal[1], wn = scal[2];
  GRID_STRIDE(i, n) {
    const float xv = x[i], tv = t[i];
    const bool pos = tv >= 0.5f;
    const float e = expf(-fabsf(xv));
    const float p = xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    const float g = pos ? wp * (p - 1.f) : wn * p;
    dx[i] = (!VOID || tv != ign) ? g : 0.f;
  }
}
template <bool VOID>
static void loss_launches(int kind, const float* logits, const float* gt, float* dlogits, float* loss, float* partial, long n,
                          float ign, hipStream_t s) {
  float* scal = partial + LOSS_SCAL;
  int* cnt = (int*)(partial + LOSS_CNT);
  const int nb = grid_for(n, 256, LOSS_BLOCKS);
  const dim3 one(1), block(256), part(nb), all(grid_for(n, 256));
  if (kind == 0) {
    const float inv_n = 1.0f / (float)n;
    hipLaunchKernelGGL((bce_partial_kernel<VOID>), part, block, 0, s, logits, gt, dlogits, partial, cnt, n, inv_n, ign);
    hipLaunchKernelGGL((bce_final_kernel<VOID>), one, block, 0, s, partial, cnt, loss, scal, nb, inv_n);
    if (VOID) hipLaunchKernelGGL(bce_grad_kernel, all, block, 0, s, logits, gt, scal, dlogits, n, ign);
  } else if (kind == 3) {
    hipLaunchKernelGGL((cbce_partial_kernel<VOID>), part, block, 0, s, logits, gt, (float4*)partial, cnt, n, ign);
    hipLaunchKernelGGL((cbce_final_kernel<VOID>), one, block, 0, s, (const float4*)partial, cnt, nb, n, loss, scal);
    hipLaunchKernelGGL((cbce_grad_kernel<VOID>), all, block, 0, s, logits, gt, scal, dlogits, n, ign);
  } else {
    hipLaunchKernelGGL((dice_partial_kernel<VOID>), part, block, 0, s, logits, gt, (float4*)partial, cnt, n, ign);
    hipLaunchKernelGGL((dice_final_kernel<VOID>), one, block, 0, s, (const float4*)partial, cnt, nb, n, kind, loss, scal);
    hipLaunchKernelGGL((dice_grad_kernel<VOID>), all, block, 0, s, logits, gt, scal, dlogits, n, ign);
  }
}
void launch_loss(int kind, const float* logits, const float* gt, float* dlogits, float* loss, float* partial, int64_t n,
                 const float* ignore, hipStream_t s) {
  if (ignore) loss_launches<true>(kind, logits, gt, dlogits, loss, partial, (long)n, *ignore, s);
  else loss_launches<false>(kind, logits, gt, dlogits, loss, partial, (long)n, 0.f, s);
}

// ---- weighted sums of the device losses (launch_loss_sum; the rule: include/eosvos.h at eosvos_set_loss_sum) ----------
// acc = w0 * x0, then acc = acc + wi * xi in spelled order, every product and every sum rounded on its own.  hipcc contracts
// a + w * b into one fused multiply-add by default, and the __fmul_rn / __fadd_rn family does not stop it (inline functions
// of a header compiled under that default, fused after inlining: the assembly showed v_fmac / v_pk_fma), so the expressions
// are plain operators under the pragma, as in lucid_kernels.hip.
template <int NT>
struct LossSumTerms { const float* d[NT]; float w[NT]; };
template <int NT>
__device__ __forceinline__ float loss_sum_of(const float (&x)[NT], const float (&w)[NT]) {
#pragma clang fp contract(off)
  float acc = w[0] * x[0];
#pragma unroll
  for (int t = 1; t < NT; ++t) {
    const float p = w[t] * x[t];
    acc = acc + p;
  }
  return acc;
}
// One streaming pass over the NT gradient slices: 16-byte loads and stores while `vec` (every pointer 16-byte aligned), the
// n mod 4 tail -- or, with an unaligned caller pointer, everything -- by single elements.  The first workgroup forms the
// loss value from the NT term values and copies those, unweighted, to `terms`.
template <int NT>
__global__ __launch_bounds__(256) void loss_sum_kernel(const LossSumTerms<NT> a, const float* __restrict__ vals,
                                                        float* __restrict__ out, float* __restrict__ loss,
                                                        float* __restrict__ terms, long n, int vec) {
  const long n4 = vec ? n >> 2 : 0;
  GRID_STRIDE(i, n4) {
    float4 v[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) v[t] = reinterpret_cast<const float4*>(a.d[t])[i];
    float x[NT], y[NT], z[NT], w[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { x[t] = v[t].x; y[t] = v[t].y; z[t] = v[t].z; w[t] = v[t].w; }
    reinterpret_cast<float4*>(out)[i] =
        make_float4(loss_sum_of<NT>(x, a.w), loss_sum_of<NT>(y, a.w), loss_sum_of<NT>(z, a.w), loss_sum_of<NT>(w, a.w));
  }
  for (long i = 4 * n4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float x[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) x[t] = a.d[t][i];
    out[i] = loss_sum_of<NT>(x, a.w);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float x[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) terms[t] = x[t] = vals[t];
    *loss = loss_sum_of<NT>(x, a.w);
  }
}
template <int NT>
static void loss_sum_launch(const float* const* grads, const float* weights, const float* vals, float* out, float* loss,
                            float* terms, long n, hipStream_t s) {
  LossSumTerms<NT> a;
  bool vec = ((uintptr_t)out & 15) == 0;
  for (int t = 0; t < NT; ++t) {
    a.d[t] = grads[t];
    a.w[t] = weights[t];
    vec = vec && ((uintptr_t)grads[t] & 15) == 0;
  }
  hipLaunchKernelGGL((loss_sum_kernel<NT>), dim3(grid_for(vec ? (n + 3) / 4 : n, 256, 2048)), dim3(256), 0, s, a, vals, out,
                     loss, terms, n, vec ? 1 : 0);
}
void launch_loss_sum(int n_terms, const float* const* grads, const float* weights, const float* vals, float* out, float* loss,
                     float* terms, int64_t n, hipStream_t s) {
  switch (n_terms) {
    case 1: loss_sum_launch<1>(grads, weights, vals, out, loss, terms, (long)n, s); break;
    case 2: loss_sum_launch<2>(grads, weights, vals, out, loss, terms, (long)n, s); break;
    case 3: loss_sum_launch<3>(grads, weights, vals, out, loss, terms, (long)n, s); break;
    default: loss_sum_launch<4>(grads, weights, vals, out, loss, terms, (long)n, s); break;
  }
}

// ---- pseudo-label targets of online adaptation with an uncertainty band -----------------------------------------------
// targets = 1 where p >= hi, 0 where p < lo, `ign` between (a NaN probability is void); n_pos[frame] += the frame's count
// of 1s: summed over the wave, one integer atomic per wave (integer adds commute: the counts do not depend on arrival order)
__global__ __launch_bounds__(256) void propagation_targets_kernel(const float* __restrict__ probs, float* __restrict__ targets,
                                                                   int* __restrict__ n_pos, long n_pix, float lo, float hi,
                                                                   float ign) {
  const long f0 = (long)blockIdx.y * n_pix;
  int c = 0;
  GRID_STRIDE(i, n_pix) {
    const float p = probs[f0 + i];
    const bool pos = p >= hi;
    targets[f0 + i] = pos ? 1.f : (p < lo ? 0.f : ign);
    c += pos ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(n_pos + blockIdx.y, c);
}
void launch_propagation_targets(const float* probs, float* targets, int* n_pos, int n_frames, int64_t n_pix, float lo, float hi,
                                float ignore, hipStream_t s) {
  hipLaunchKernelGGL(propagation_targets_kernel, dim3(grid_for(n_pix, 256, 1024), n_frames), dim3(256), 0, s, probs, targets,
                     n_pos, (long)n_pix, lo, hi, ignore);
}
}  // namespace eosvos

// ---- device-side data augmentation: cv2.warpAffine restated (custom_transforms.py:41-51) -----------------
// RandomScaleNRotate warps the frame with cv2.INTER_CUBIC and the label with cv2.INTER_NEAREST, border 0,
// canvas size unchanged; RandomHorizontalFlip mirrors the source first (cv2.flip, `:202-211`).  OpenCV's
// warpAffine (imgproc/imgwarp.cpp, 4.1) computes the source coordinates in 10-bit fixed point from integer
// tables adelta/bdelta (per column) and X0/Y0 (per row), built in double; the kernel evaluates the same entries with the
// same roundings, so the coordinates here are bit-identical to the restated algorithm; cubic taps use the
// a = -0.75 kernel sampled at 1/32 pixel (INTER_BITS = 5), weights = cy[k1]*cx[k2] in float.
namespace eosvos {
// The fixed-point tables of cv::warpAffine, entry by entry in the kernel (the inverted matrix travels by value, so a
// launch carries everything it reads: no table buffer a later call could overwrite while this one is still queued).
// Same double expressions as the host form, (M0 * x) * 1024 and (M1 * y + M2) * 1024, each operation rounded on its own
// (no fused multiply-add), then round-half-even to int like lrint.
// (`warp_fix` is in kernels.h: lucid_compose_kernel evaluates the same entries.)
struct WarpMat { double m[6]; int round_delta; };
__global__ __launch_bounds__(256) void warp_affine_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           int C, int H, int W, const WarpMat wm, const float* __restrict__ ctab,
                                                           int cubic, int flip, int* __restrict__ nonzero) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  int cnt = 0;
  if (x < W) {
    const long hw = (long)H * W;
    const int Xf = warp_fix(wm.m[1], y, wm.m[2], wm.round_delta) + warp_fix(wm.m[0], x);
    const int Yf = warp_fix(wm.m[4], y, wm.m[5], wm.round_delta) + warp_fix(wm.m[3], x);
    if (!cubic) {
      const int sx = Xf >> 10, sy = Yf >> 10;
      const bool in = (unsigned)sx < (unsigned)W && (unsigned)sy < (unsigned)H;
      const int ux = flip ? W - 1 - sx : sx;
      for (int c = 0; c < C; ++c) {
        const float v = in ? src[c * hw + (long)sy * W + ux] : 0.f;
        dst[c * hw + (long)y * W + x] = v;
        cnt += v != 0.f;
      }
    } else {
      const int X = Xf >> 5, Y = Yf >> 5;
      const int sx = (X >> 5) - 1, sy = (Y >> 5) - 1;
      const float* cx = ctab + (X & 31) * 4;
      const float* cy = ctab + (Y & 31) * 4;
      const bool interior = (unsigned)sx < (unsigned)(W - 3 > 0 ? W - 3 : 0) && (unsigned)sy < (unsigned)(H - 3 > 0 ? H - 3 : 0);
      const bool centre_out = (unsigned)(sx + 1) >= (unsigned)W || (unsigned)(sy + 1) >= (unsigned)H;
      for (int c = 0; c < C; ++c) {
        const float* S = src + c * hw;
        float sum = 0.f;
        if (interior) {
          // remapBicubic's interior order: one 4-term expression per row, rows accumulated
          // Every product goes through an opaque register so that the compiler keeps the 16 taps in scalar fp32
          // instructions.  Left alone it pairs the separately loaded taps into v_pk_mul_f32 / v_pk_fma_f32 operands, and
          // on MI355X that form of this kernel lost the odd tap of a pair in lanes 48..63 of a wave whenever waves of the
          // bf16x6 conv kernels (another engine's, on another stream) shared the SIMD -- 20-30 % of 96x160 warps had such
          // a 16-pixel run, none in 300 runs with scalar instructions (tools/debug/concurrent_victims2.py,
          // tests/test_augment.py::test_cubic_warp_is_stable_beside_another_engine).
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float* R = S + (long)(sy + i) * W;
            float r = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int ux = flip ? W - 1 - (sx + j) : sx + j;
              float t = R[ux] * (cy[i] * cx[j]);
              asm volatile("" : "+v"(t));
              r = j == 0 ? t : r + t;
              asm volatile("" : "+v"(r));
            }
            sum = i == 0 ? r : sum + r;
          }
        } else if (!centre_out) {
          // border branch: taps outside the image contribute the constant 0, tap-by-tap accumulation
          for (int i = 0; i < 4; ++i) {
            const int yy = sy + i;
            if ((unsigned)yy >= (unsigned)H) continue;
            for (int j = 0; j < 4; ++j) {
              const int xx = sx + j;
              if ((unsigned)xx >= (unsigned)W) continue;
              const int ux = flip ? W - 1 - xx : xx;
              sum += S[(long)yy * W + ux] * (cy[i] * cx[j]);
            }
          }
        }
        dst[c * hw + (long)y * W + x] = sum;
        cnt += sum != 0.f;
      }
    }
  }
  if (nonzero) {
    cnt = (int)wave_sum((float)cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(nonzero, cnt);
  }
}
void launch_warp_affine(const float* src, float* dst, int C, int H, int W, const double* inv_matrix /*6*/, int round_delta,
                        const float* ctab, int cubic, int flip, int* nonzero, hipStream_t s) {
  WarpMat wm;
  for (int i = 0; i < 6; ++i) wm.m[i] = inv_matrix[i];
  wm.round_delta = round_delta;
  hipLaunchKernelGGL(warp_affine_kernel, dim3((W + 255) / 256, H), dim3(256), 0, s, src, dst, C, H, W, wm, ctab, cubic, flip,
                     nonzero);
}
}  // namespace eosvos

// ---- Winograd F(m x m, 3x3) transform passes of the 3x3 / stride-1 convs: one kernel family for the two tile
// sizes m = TM = 2 and 4:  Y = A^T [ (G w G^T) (.) (B^T d B) ] A per TM x TM output tile and (cin, cout) pair.  With
// NP = TM + 2 and U = G w G^T:
//   forward          V = B^T d B (input), M[p] = V[p] U[p] (batched GEMM, conv_kernels.hip), y = epilogue(A^T M A) (output)
//   data gradient    dM = A dY A^T (grad), dV[p] = dM[p] (a U[p])^T (batched GEMM), dX = mask(B dV B^T, overlap-added)
//   weight gradient  dU[p] = sum_tiles dM[p][tile][cout] * V[p][tile][cin] (wgrad_kernel, the NP*NP positions as "taps"),
//                    dW = G^T dU G (wgrad finish)
// V / dM / M / dV are stored plane by plane ([p][tile][channel], prow >= ntile rows per plane, padded to the GEMM tile so
// that a row tile never straddles planes).  F(2,3): 16 positions, 4 MACs per output instead of 9; F(4,3): 36 positions,
// 2.25 MACs, transform-domain tensors 0.56x the F(2,3) size, interpolation points 0, +-1, +-2, inf (Lavin & Gray); fp32
// rounding error of one conv ~2e-6 rms of the output scale (direct fp32: 1e-7, F(2,3): 3e-7) -- far inside the 1e-3
// logit tolerance.  Stride 1, pad = dilation only.
// The transforms are driven by the constexpr matrices of WinoMat<TM>: zero entries are skipped at compile time, every
// other entry is one fmaf, in the order of the matrix row (for F(2,3), whose entries are 0, +-1 and +-1/2, that is the
// plain sum / difference chain).  Two F(2,3) kernels are explicit specialisations because their summation order is not
// the separable one of the template: wino_wgrad_finish_kernel<2> and wino_dgrad_output_kernel<2> (see there).
namespace eosvos {
// BT, G, AT of both sizes; tests/test_winograd_math.py parses them from this file and checks the Winograd identities
template <int TM> struct WinoMat;
template <> struct WinoMat<2> {
  static __device__ constexpr float BT[4][4] = {{1, 0, -1, 0}, {0, 1, 1, 0}, {0, -1, 1, 0}, {0, 1, 0, -1}};
  static __device__ constexpr float G[4][3] = {{1, 0, 0}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0, 0, 1}};
  static __device__ constexpr float AT[2][4] = {{1, 1, 1, 0}, {0, 1, -1, -1}};
};
template <> struct WinoMat<4> {
  static __device__ constexpr float BT[6][6] = {{4, 0, -5, 0, 1, 0}, {0, -4, -4, 1, 1, 0}, {0, 4, -4, -1, 1, 0},
                                                {0, -2, -1, 2, 1, 0}, {0, 2, -1, -2, 1, 0}, {0, 4, 0, -5, 0, 1}};
  static __device__ constexpr float G[6][3] = {{0.25f, 0, 0}, {-1.f / 6, -1.f / 6, -1.f / 6}, {-1.f / 6, 1.f / 6, -1.f / 6},
                                               {1.f / 24, 1.f / 12, 1.f / 6}, {1.f / 24, -1.f / 12, 1.f / 6}, {0, 0, 1}};
  static __device__ constexpr float AT[4][6] = {{1, 1, 1, 1, 1, 0}, {0, 1, -1, 2, -2, 0}, {0, 1, 1, 4, 4, 0}, {0, 1, -1, 8, -8, 1}};
};
__device__ __forceinline__ void fma4(float4& acc, float c, const float4& v) {
  acc.x = fmaf(c, v.x, acc.x); acc.y = fmaf(c, v.y, acc.y); acc.z = fmaf(c, v.z, acc.z); acc.w = fmaf(c, v.w, acc.w);
}
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 scaled4(float s, const float4& v) { return make_float4(s * v.x, s * v.y, s * v.z, s * v.w); }

// element e of a transform pass = (tile, 4 channels); tile = (image b, sy, sx, ty, tx): th x tw tiles of TM x TM outputs
// per sub-grid of a dilated conv (dil * dil interleaved sub-grids, each an ordinary 3x3 convolution; dil = 1: the image)
struct WinoTile { int c4; long tile; int tx, ty, sx, sy, b; };
__device__ __forceinline__ WinoTile wino_tile(long e, int C4, int th, int tw, int dil) {
  WinoTile t;
  t.c4 = (int)(e % C4);
  t.tile = e / C4;
  t.tx = (int)(t.tile % tw); t.ty = (int)((t.tile / tw) % th);
  t.sx = (int)((t.tile / ((long)tw * th)) % dil); t.sy = (int)((t.tile / ((long)tw * th * dil)) % dil);
  t.b = (int)(t.tile / ((long)tw * th * dil * dil));
  return t;
}

// V[p][tile][c] = B^T d B from X (NHWC, ld ldx), d = NP x NP patch rows TM*ty-1 .. TM*ty+TM, cols likewise (zero outside)
template <int TM>
__global__ __launch_bounds__(256) void wino_input_kernel(const float* __restrict__ x, int ldx, int C, int B, int H, int W,
                                                          int th, int tw, int dil, long prow, float* __restrict__ V, unsigned* __restrict__ amax) {
  using Mt = WinoMat<TM>;
  constexpr int NP = TM + 2;
  const int C4 = C >> 2;
  const long n = (long)B * dil * dil * th * tw * C4;
  unsigned am = 0;
  GRID_STRIDE(e, n) {
    const WinoTile t = wino_tile(e, C4, th, tw, dil);
    float4 d[NP][NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int yy = t.sy + dil * (TM * t.ty - 1 + i);
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int xx = t.sx + dil * (TM * t.tx - 1 + j);
        d[i][j] = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
                      ? *reinterpret_cast<const float4*>(x + (((long)t.b * H + yy) * W + xx) * ldx + t.c4 * 4)
                      : zero4();
      }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {         // columns: d[:, j] <- B^T d[:, j]
      float4 c[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        c[i] = zero4();
#pragma unroll
        for (int a = 0; a < NP; ++a)
          if (Mt::BT[i][a] != 0.f) fma4(c[i], Mt::BT[i][a], d[a][j]);
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) d[i][j] = c[i];
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {         // rows: V[i, :] = B^T applied along the row
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        float4 v = zero4();
#pragma unroll
        for (int bb = 0; bb < NP; ++bb)
          if (Mt::BT[j][bb] != 0.f) fma4(v, Mt::BT[j][bb], d[i][bb]);
        am = amax_f4(am, v);
        *reinterpret_cast<float4*>(V + ((long)(i * NP + j) * prow + t.tile) * C + t.c4 * 4) = v;
      }
    }
  }
  if (amax) amax_block_commit(am, amax);
}
// dM[p][tile][c] = A dY A^T from dY (NHWC, ld ldg): the tile's TM x TM outputs (zero outside), A = AT^T
template <int TM>
__global__ __launch_bounds__(256) void wino_grad_kernel(const float* __restrict__ g, int ldg, int C, int B, int H, int W,
                                                         int th, int tw, int dil, long prow, float* __restrict__ M, unsigned* __restrict__ amax) {
  using Mt = WinoMat<TM>;
  constexpr int NP = TM + 2;
  const int C4 = C >> 2;
  const long n = (long)B * dil * dil * th * tw * C4;
  unsigned am = 0;
  GRID_STRIDE(e, n) {
    const WinoTile tl = wino_tile(e, C4, th, tw, dil);
    float4 d[TM][TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const int yy = tl.sy + dil * (TM * tl.ty + i), xx = tl.sx + dil * (TM * tl.tx + j);
        d[i][j] = (yy < H && xx < W) ? *reinterpret_cast<const float4*>(g + (((long)tl.b * H + yy) * W + xx) * ldg + tl.c4 * 4)
                                     : zero4();
      }
    float4 t[NP][TM];                      // t = A d : t[a][j] = sum_r AT[r][a] d[r][j]
#pragma unroll
    for (int a = 0; a < NP; ++a)
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        t[a][j] = zero4();
#pragma unroll
        for (int r = 0; r < TM; ++r)
          if (Mt::AT[r][a] != 0.f) fma4(t[a][j], Mt::AT[r][a], d[r][j]);
      }
#pragma unroll
    for (int a = 0; a < NP; ++a)
#pragma unroll
      for (int bb = 0; bb < NP; ++bb) {    // dM[a][bb] = sum_r t[a][r] AT[r][bb]
        float4 v = zero4();
#pragma unroll
        for (int r = 0; r < TM; ++r)
          if (Mt::AT[r][bb] != 0.f) fma4(v, Mt::AT[r][bb], t[a][r]);
        am = amax_f4(am, v);
        *reinterpret_cast<float4*>(M + ((long)(a * NP + bb) * prow + tl.tile) * C + tl.c4 * 4) = v;
      }
  }
  if (amax) amax_block_commit(am, amax);
}
// U[p][cout][cin] = G w G^T from W[cout][3x3][cin]; Us (optional) = rowscale[cout] * U, the copy the data gradient
// multiplies with (the frozen-norm scale a[cout] folded in)
template <int TM>
__global__ __launch_bounds__(256) void wino_weight_kernel(const float* __restrict__ w, int Cout, int Cin,
                                                           const float* __restrict__ rowscale, float* __restrict__ U,
                                                           float* __restrict__ Us, unsigned* __restrict__ amax_u, unsigned* __restrict__ amax_us) {
  using Mt = WinoMat<TM>;
  constexpr int NP = TM + 2;
  const int C4 = Cin >> 2;
  const long n = (long)Cout * C4;
  unsigned am = 0, ams = 0;
  GRID_STRIDE(e, n) {
    const int c4 = (int)(e % C4), co = (int)(e / C4);
    const float rs = rowscale ? rowscale[co] : 1.f;
    float4 g[3][3];
#pragma unroll
    for (int t = 0; t < 9; ++t) g[t / 3][t % 3] = *reinterpret_cast<const float4*>(w + ((size_t)co * 9 + t) * Cin + c4 * 4);
    float4 t[NP][3];
#pragma unroll
    for (int a = 0; a < NP; ++a)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        t[a][j] = zero4();
#pragma unroll
        for (int r = 0; r < 3; ++r)
          if (Mt::G[a][r] != 0.f) fma4(t[a][j], Mt::G[a][r], g[r][j]);
      }
    const size_t ps = (size_t)Cout * Cin;
#pragma unroll
    for (int a = 0; a < NP; ++a)
#pragma unroll
      for (int bb = 0; bb < NP; ++bb) {
        float4 v = zero4();
#pragma unroll
        for (int r = 0; r < 3; ++r)
          if (Mt::G[bb][r] != 0.f) fma4(v, Mt::G[bb][r], t[a][r]);
        am = amax_f4(am, v);
        ams = amax_f4(ams, scaled4(rs, v));
        *reinterpret_cast<float4*>(U + (size_t)(a * NP + bb) * ps + (size_t)co * Cin + c4 * 4) = v;
        if (Us) *reinterpret_cast<float4*>(Us + (size_t)(a * NP + bb) * ps + (size_t)co * Cin + c4 * 4) = scaled4(rs, v);
      }
  }
  if (amax_u) amax_block_commit(am, amax_u);
  if (amax_us) amax_block_commit(ams, amax_us);
}
// y (NHWC, ld ldy) = relu?(scale * (A^T M A) + bias) from M[p][tile][c], TM x TM outputs per tile
template <int TM>
__global__ __launch_bounds__(256) void wino_output_kernel(const float* __restrict__ M, long prow, int C, int B, int H, int W,
                                                           int th, int tw, int dil, const float* __restrict__ scale,
                                                           const float* __restrict__ bias, int relu, float* __restrict__ y,
                                                           int ldy, unsigned* __restrict__ amax, uint8_t* __restrict__ mask8_out, int ldm8) {
  using Mt = WinoMat<TM>;
  constexpr int NP = TM + 2;
  const int C4 = C >> 2;
  const long n = (long)B * dil * dil * th * tw * C4;
  unsigned am = 0;
  GRID_STRIDE(e, n) {
    const WinoTile tl = wino_tile(e, C4, th, tw, dil);
    float4 t[TM][NP];                      // t = A^T m, streamed over the rows a of m
#pragma unroll
    for (int r = 0; r < TM; ++r)
#pragma unroll
      for (int j = 0; j < NP; ++j) t[r][j] = zero4();
#pragma unroll
    for (int a = 0; a < NP; ++a)
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const float4 m = *reinterpret_cast<const float4*>(M + ((long)(a * NP + j) * prow + tl.tile) * C + tl.c4 * 4);
#pragma unroll
        for (int r = 0; r < TM; ++r)
          if (Mt::AT[r][a] != 0.f) fma4(t[r][j], Mt::AT[r][a], m);
      }
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), bi = zero4();
    if (scale) sc = *reinterpret_cast<const float4*>(scale + tl.c4 * 4);
    if (bias) bi = *reinterpret_cast<const float4*>(bias + tl.c4 * 4);
#pragma unroll
    for (int r = 0; r < TM; ++r) {
      const int yy = tl.sy + dil * (TM * tl.ty + r);
      if (yy >= H) continue;
#pragma unroll
      for (int q = 0; q < TM; ++q) {
        const int xx = tl.sx + dil * (TM * tl.tx + q);
        if (xx >= W) continue;
        float4 v = zero4();
#pragma unroll
        for (int j = 0; j < NP; ++j)
          if (Mt::AT[q][j] != 0.f) fma4(v, Mt::AT[q][j], t[r][j]);
        if (scale) { v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w; }
        if (bias) { v.x += bi.x; v.y += bi.y; v.z += bi.z; v.w += bi.w; }
        if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        am = amax_f4(am, v);
        *reinterpret_cast<float4*>(y + (((long)tl.b * H + yy) * W + xx) * ldy + tl.c4 * 4) = v;
        if (mask8_out) mask8_out[(((long)tl.b * H + yy) * W + xx) * ldm8 + tl.c4] = relu_bits(v);
      }
    }
  }
  if (amax) amax_block_commit(am, amax);
}
// dW[cout][3x3][cin] = G^T (sum_z dU_z[cout][NP x NP][cin]) G.  One thread per (cout, cin): the decoder convs have only
// 256 x 304 of them, and a float4-per-thread version (64 workgroups of long dependent load chains) ran at 2 TB/s.
template <int TM> constexpr int wino_finish_cin_per_thread = 1;      // input channels one thread finishes (the launcher's grid)
template <int TM>
__global__ __launch_bounds__(256) void wino_wgrad_finish_kernel(const float* __restrict__ ws, int splits, int Cout, int Cin,
                                                                 float* __restrict__ dst) {
  using Mt = WinoMat<TM>;
  constexpr int NP = TM + 2;
  const long n = (long)Cout * Cin;
  GRID_STRIDE(e, n) {
    const int ci = (int)(e % Cin), co = (int)(e / Cin);
    float t[3][NP];                        // t = G^T u, streamed over the rows a of u (each summed over the splits)
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int j = 0; j < NP; ++j) t[r][j] = 0.f;
#pragma unroll
    for (int a = 0; a < NP; ++a) {
      float u[NP];                         // one row of dU, its NP loads per split in flight together
#pragma unroll
      for (int j = 0; j < NP; ++j) u[j] = 0.f;
      for (int z = 0; z < splits; ++z) {
        float v[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) v[j] = ws[(((size_t)z * Cout + co) * (NP * NP) + (a * NP + j)) * Cin + ci];
#pragma unroll
        for (int j = 0; j < NP; ++j) u[j] += v[j];
      }
#pragma unroll
      for (int j = 0; j < NP; ++j)
#pragma unroll
        for (int r = 0; r < 3; ++r)
          if (Mt::G[a][r] != 0.f) t[r][j] = fmaf(Mt::G[a][r], u[j], t[r][j]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < NP; ++j)
          if (Mt::G[j][q] != 0.f) v = fmaf(Mt::G[j][q], t[r][j], v);
        dst[((size_t)co * 9 + r * 3 + q) * Cin + ci] = v;
      }
  }
}
// F(2,3) keeps its own association: (u0 + .5(u1+u2), .5(u1-u2), .5(u1+u2) + u3) with the sum u1+u2 shared by two rows,
// which no traversal order of the fmaf chain above reproduces; its results must not move.  float4 per thread (Cin / 4).
__device__ __forceinline__ void wino2_gt(const float4& u0, const float4& u1, const float4& u2, const float4& u3, float4& r0, float4& r1, float4& r2) {
  const float4 s12 = make_float4(u1.x + u2.x, u1.y + u2.y, u1.z + u2.z, u1.w + u2.w);
  const float4 d12 = make_float4(u1.x - u2.x, u1.y - u2.y, u1.z - u2.z, u1.w - u2.w);
  r0 = make_float4(u0.x + 0.5f * s12.x, u0.y + 0.5f * s12.y, u0.z + 0.5f * s12.z, u0.w + 0.5f * s12.w);
  r1 = scaled4(0.5f, d12);
  r2 = make_float4(0.5f * s12.x + u3.x, 0.5f * s12.y + u3.y, 0.5f * s12.z + u3.z, 0.5f * s12.w + u3.w);
}
template <> constexpr int wino_finish_cin_per_thread<2> = 4;
template <>
__global__ __launch_bounds__(256) void wino_wgrad_finish_kernel<2>(const float* __restrict__ ws, int splits, int Cout, int Cin,
                                                                    float* __restrict__ dst) {
  static_assert(wino_finish_cin_per_thread<2> == 4, "this kernel finishes one float4 of input channels per thread");
  const int C4 = Cin >> 2;
  const long n = (long)Cout * C4;
  GRID_STRIDE(e, n) {
    const int c4 = (int)(e % C4), co = (int)(e / C4);
    float4 u[4][4];
#pragma unroll
    for (int p = 0; p < 16; ++p) u[p >> 2][p & 3] = zero4();
    for (int z = 0; z < splits; ++z) {
      const float* sp = ws + ((size_t)z * Cout + co) * 16 * Cin + c4 * 4;
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        const float4 v = *reinterpret_cast<const float4*>(sp + (size_t)p * Cin);
        float4& a = u[p >> 2][p & 3];
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
      }
    }
    float4 t[3][4];                        // t = G^T u (3x4); then w = t G (3x3), the same combination on columns
#pragma unroll
    for (int j = 0; j < 4; ++j) wino2_gt(u[0][j], u[1][j], u[2][j], u[3][j], t[0][j], t[1][j], t[2][j]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      float4 w0, w1, w2;
      wino2_gt(t[i][0], t[i][1], t[i][2], t[i][3], w0, w1, w2);
      float* o = dst + ((size_t)co * 9 + i * 3) * Cin + c4 * 4;
      *reinterpret_cast<float4*>(o) = w0;
      *reinterpret_cast<float4*>(o + Cin) = w1;
      *reinterpret_cast<float4*>(o + 2 * Cin) = w2;
    }
  }
}
// dX (NHWC, ld ldgx) = mask?(accum + overlap-add of B dV B^T), gather form, no atomics: deterministic.  One thread per
// TM x TM pixel block (= tile position) and 4 channels.  Block (k, l) takes patch rows i = 1..TM of tile k, i = NP-1 of
// tile k-1 (its row 0) and i = 0 of tile k+1 (its row TM-1); columns likewise.  B[i][a] = BT[a][i].
template <int TM>
__global__ __launch_bounds__(256) void wino_dgrad_output_kernel(const float* __restrict__ dV, long prow, int C, int B, int H,
                                                                 int W, int th, int tw, int dil,
                                                                 const uint8_t* __restrict__ mask8, int ldm8, int mask_c0,
                                                                 int accum, float* __restrict__ gx, int ldgx, unsigned* __restrict__ amax) {
  using Mt = WinoMat<TM>;
  constexpr int NP = TM + 2;
  const int C4 = C >> 2;
  const long n = (long)B * dil * dil * th * tw * C4;
  unsigned am = 0;
  GRID_STRIDE(e, n) {
    const WinoTile blk = wino_tile(e, C4, th, tw, dil);      // the block's own tile: k = ty, l = tx
    const int c4 = blk.c4, sx = blk.sx, sy = blk.sy, b = blk.b;
    float4 acc[TM][TM];
#pragma unroll
    for (int r = 0; r < TM; ++r)
#pragma unroll
      for (int q = 0; q < TM; ++q) acc[r][q] = zero4();
#pragma unroll
    for (int dk = -1; dk <= 1; ++dk) {
      const int ty = blk.ty + dk;
      if ((unsigned)ty >= (unsigned)th) continue;
#pragma unroll
      for (int dl = -1; dl <= 1; ++dl) {
        const int tx = blk.tx + dl;
        if ((unsigned)tx >= (unsigned)tw) continue;
        const long tile = ((((long)b * dil + sy) * dil + sx) * th + ty) * tw + tx;
        // patch rows of this tile that land in the block: dk = -1 -> {NP-1}, 0 -> {1..TM}, +1 -> {0}; output row r(i)
        const int ni = dk == 0 ? TM : 1, nj = dl == 0 ? TM : 1;
        // t[ii][bb] = sum_a B[i][a] dV[a][bb]   for the needed i, streamed over a
        float4 t[TM][NP];
#pragma unroll
        for (int ii = 0; ii < TM; ++ii)
#pragma unroll
          for (int bb = 0; bb < NP; ++bb) t[ii][bb] = zero4();
#pragma unroll
        for (int a = 0; a < NP; ++a) {
          // is row a needed by any of the i rows?  (i = NP-1: a = NP-1 only; i = 0: a = 0 only; centre: every a)
          if (dk < 0 && a != NP - 1) continue;
          if (dk > 0 && a != 0) continue;
#pragma unroll
          for (int bb = 0; bb < NP; ++bb) {
            if (dl < 0 && bb != NP - 1) continue;
            if (dl > 0 && bb != 0) continue;
            const float4 v = *reinterpret_cast<const float4*>(dV + ((long)(a * NP + bb) * prow + tile) * C + c4 * 4);
#pragma unroll
            for (int ii = 0; ii < TM; ++ii) {
              if (ii >= ni) continue;
              const int i = dk < 0 ? NP - 1 : (dk > 0 ? 0 : 1 + ii);
              if (Mt::BT[a][i] != 0.f) fma4(t[ii][bb], Mt::BT[a][i], v);
            }
          }
        }
#pragma unroll
        for (int ii = 0; ii < TM; ++ii) {
          if (ii >= ni) continue;
          const int r = dk < 0 ? 0 : (dk > 0 ? TM - 1 : ii);
#pragma unroll
          for (int jj = 0; jj < TM; ++jj) {
            if (jj >= nj) continue;
            const int j = dl < 0 ? NP - 1 : (dl > 0 ? 0 : 1 + jj);
            const int q = dl < 0 ? 0 : (dl > 0 ? TM - 1 : jj);
#pragma unroll
            for (int bb = 0; bb < NP; ++bb) {
              if (dl < 0 && bb != NP - 1) continue;
              if (dl > 0 && bb != 0) continue;
              if (Mt::BT[bb][j] != 0.f) fma4(acc[r][q], Mt::BT[bb][j], t[ii][bb]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < TM; ++r) {
      const int yy = sy + dil * (TM * blk.ty + r);
      if (yy >= H) continue;
#pragma unroll
      for (int q = 0; q < TM; ++q) {
        const int xx = sx + dil * (TM * blk.tx + q);
        if (xx >= W) continue;
        const long pix = ((long)b * H + yy) * W + xx;
        float4 v = acc[r][q];
        if (accum) {                       // several branches feed this gradient (ASPP): add, then mask, like the GEMM epilogue
          const float4 o = *reinterpret_cast<const float4*>(gx + pix * ldgx + c4 * 4);
          v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
        }
        if (mask8 && c4 * 4 >= mask_c0) relu_mask8(v, mask8[pix * ldm8 + c4]);
        am = amax_f4(am, v);
        *reinterpret_cast<float4*>(gx + pix * ldgx + c4 * 4) = v;
      }
    }
  }
  if (amax) amax_block_commit(am, amax);
}
// F(2,3) keeps its own association: each (tile, i, j) term sum_a sum_bb B[i][a] B[j][bb] dV[a][bb] is summed in ONE chain
// and then added to the block's accumulator, not in the two separable stages above; its results must not move.
template <>
__global__ __launch_bounds__(256) void wino_dgrad_output_kernel<2>(const float* __restrict__ dV, long prow, int C, int B, int H,
                                                                    int W, int th, int tw, int dil,
                                                                    const uint8_t* __restrict__ mask8, int ldm8, int mask_c0,
                                                                    int accum, float* __restrict__ gx, int ldgx, unsigned* __restrict__ amax) {
  using Mt = WinoMat<2>;
  const int C4 = C >> 2;
  const long n = (long)B * dil * dil * th * tw * C4;
  unsigned am = 0;
  GRID_STRIDE(e, n) {
    const WinoTile blk = wino_tile(e, C4, th, tw, dil);
    const int c4 = blk.c4, sx = blk.sx, sy = blk.sy, b = blk.b;
    float4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i >> 1][i & 1] = zero4();
#pragma unroll
    for (int dk = -1; dk <= 1; ++dk) {
      const int ty = blk.ty + dk;
      if ((unsigned)ty >= (unsigned)th) continue;
#pragma unroll
      for (int dl = -1; dl <= 1; ++dl) {
        const int tx = blk.tx + dl;
        if ((unsigned)tx >= (unsigned)tw) continue;
        const long tile = ((((long)b * dil + sy) * dil + sx) * th + ty) * tw + tx;
        // rows of B needed from this tile: dk = -1 -> {3}; dk = 0 -> {1, 2}; dk = +1 -> {0}; columns likewise with dl
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {
          const int i = dk < 0 ? 3 : (dk > 0 ? 0 : 1 + ii);
          if (dk != 0 && ii == 1) continue;
          const int r = dk < 0 ? 0 : (dk > 0 ? 1 : ii);              // output row inside the block
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            const int j = dl < 0 ? 3 : (dl > 0 ? 0 : 1 + jj);
            if (dl != 0 && jj == 1) continue;
            const int q = dl < 0 ? 0 : (dl > 0 ? 1 : jj);            // output column inside the block
            float4 sum = zero4();
#pragma unroll
            for (int a = 0; a < 4; ++a) {
              if (Mt::BT[a][i] == 0.f) continue;
#pragma unroll
              for (int bb = 0; bb < 4; ++bb) {
                if (Mt::BT[bb][j] == 0.f) continue;
                const float4 v = *reinterpret_cast<const float4*>(dV + ((long)(a * 4 + bb) * prow + tile) * C + c4 * 4);
                const float wgt = Mt::BT[a][i] * Mt::BT[bb][j];
                sum.x += wgt * v.x; sum.y += wgt * v.y; sum.z += wgt * v.z; sum.w += wgt * v.w;
              }
            }
            acc[r][q].x += sum.x; acc[r][q].y += sum.y; acc[r][q].z += sum.z; acc[r][q].w += sum.w;
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int yy = sy + dil * (2 * blk.ty + r);
      if (yy >= H) continue;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int xx = sx + dil * (2 * blk.tx + q);
        if (xx >= W) continue;
        const long pix = ((long)b * H + yy) * W + xx;
        float4 v = acc[r][q];
        if (accum) {
          const float4 o = *reinterpret_cast<const float4*>(gx + pix * ldgx + c4 * 4);
          v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
        }
        if (mask8 && c4 * 4 >= mask_c0) relu_mask8(v, mask8[pix * ldm8 + c4]);
        am = amax_f4(am, v);
        *reinterpret_cast<float4*>(gx + pix * ldgx + c4 * 4) = v;
      }
    }
  }
  if (amax) amax_block_commit(am, amax);
}

// ---- launchers: tm = 2 or 4 (WinoGeom::tm) selects the instantiation --------------------------------------------------
#define WINO_LAUNCH(kernel, grid, s, ...)                                                              \
  do {                                                                                                 \
    assert(tm == 2 || tm == 4);                                                                        \
    if (tm == 4) hipLaunchKernelGGL(kernel<4>, dim3(grid), dim3(256), 0, s, __VA_ARGS__);              \
    else hipLaunchKernelGGL(kernel<2>, dim3(grid), dim3(256), 0, s, __VA_ARGS__);                      \
  } while (0)
void launch_wino_input(int tm, const float* x, int ldx, int C, int B, int H, int W, int th, int tw, int dil, long prow, float* V,
                       hipStream_t s, unsigned* amax) {
  const long n = (long)B * dil * dil * th * tw * (C / 4);
  WINO_LAUNCH(wino_input_kernel, grid_for(n, 256, 8192), s, x, ldx, C, B, H, W, th, tw, dil, prow, V, amax);
}
void launch_wino_grad(int tm, const float* g, int ldg, int C, int B, int H, int W, int th, int tw, int dil, long prow, float* M,
                      hipStream_t s, unsigned* amax) {
  const long n = (long)B * dil * dil * th * tw * (C / 4);
  WINO_LAUNCH(wino_grad_kernel, grid_for(n, 256, 8192), s, g, ldg, C, B, H, W, th, tw, dil, prow, M, amax);
}
void launch_wino_weight(int tm, const float* w, int Cout, int Cin, const float* rowscale, float* U, float* Us, hipStream_t s,
                        unsigned* amax_u, unsigned* amax_us) {
  const long n = (long)Cout * (Cin / 4);
  WINO_LAUNCH(wino_weight_kernel, grid_for(n, 256), s, w, Cout, Cin, rowscale, U, Us, amax_u, amax_us);
}
void launch_wino_output(int tm, const float* M, long prow, int C, int B, int H, int W, int th, int tw, int dil, const float* scale,
                        const float* bias, int relu, float* y, int ldy, hipStream_t s, unsigned* amax, uint8_t* mask8_out, int ldm8) {
  const long n = (long)B * dil * dil * th * tw * (C / 4);
  WINO_LAUNCH(wino_output_kernel, grid_for(n, 256, 8192), s, M, prow, C, B, H, W, th, tw, dil, scale, bias, relu, y, ldy, amax,
              relu ? mask8_out : nullptr, ldm8);
}
void launch_wino_wgrad_finish(int tm, const float* ws, int splits, int Cout, int Cin, float* dst, hipStream_t s) {
  const long n = (long)Cout * (Cin / (tm == 4 ? wino_finish_cin_per_thread<4> : wino_finish_cin_per_thread<2>));
  WINO_LAUNCH(wino_wgrad_finish_kernel, grid_for(n, 256), s, ws, splits, Cout, Cin, dst);
}
void launch_wino_dgrad_output(int tm, const float* dV, long prow, int C, int B, int H, int W, int th, int tw, int dil,
                              const uint8_t* mask8, int ldm8, int mask_c0, int accum, float* gx, int ldgx, hipStream_t s,
                              unsigned* amax) {
  const long n = (long)B * dil * dil * th * tw * (C / 4);
  WINO_LAUNCH(wino_dgrad_output_kernel, grid_for(n, 256, 8192), s, dV, prow, C, B, H, W, th, tw, dil, mask8, ldm8, mask_c0, accum,
              gx, ldgx, amax);
}
#undef WINO_LAUNCH
}  // namespace eosvos
