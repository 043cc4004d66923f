// Image-aware pairwise (Potts) loss on a dilated (2r+1)^2 window, for gfx950: the relaxation p_i (1 - p_j) of the Potts model
// under a Gaussian position / colour kernel (Tang et al., ECCV 2018; the local-window form of Obukhov et al., 2019).  The rule
// is stated in include/eosvos.h (EOSVOS_LOSS_POTTS) and restated in numpy by eosvos_amd/potts.py (loss_host).
//
//   potts_stencil_kernel  one launch over 32 x 8 pixel tiles: S, M per pixel, the unscaled gradient, one partial of E and Z per tile
//   potts_finish_kernel   one workgroup: the partials in a fixed order -> the loss and the per-image 1 / (Z * images)
//   potts_scale_kernel    one streaming pass: gradient *= its image's scale
//
// potts_stencil_kernel: the staging idiom of crf_kernels.hip.  A workgroup of 256 threads owns a 32 x 8 tile, one pixel per
// thread, and stages the three colour planes and p = sigmoid(z) of the tile with its halo of r*d pixels in LDS once;
// positions outside the frame are staged as 0 and their taps are switched off by the same bounds test, so they are in neither
// S nor M.  Every thread walks the (2r+1)^2 - 1 offsets of its pixel: one exp per tap, the position factor from a table that
// travels by value.  A wave covers two rows of 32 consecutive pixels: its ds_read_b32 of one offset hits 32 consecutive banks
// per half wave.  LDS: 4 * (8 + 2h) * (32 + 2h) floats + 8, h = r*d <= 16: 40 KB at the largest halo, 10.6 KB at the default
// r 3, d 2.  The frame comes through an accessor (the engine's padded NHWC copy, or a planar NCHW caller tensor): one kernel
// body, the same arithmetic, the same bits.  E and Z: a wave sum by shuffles, the four waves through LDS in wave order, one
// partial per workgroup; no atomics, so two runs give the same bits.  Every word of the partials and scales that a launch
// reads is written by the launch before it: nothing depends on what the scratch held.
#include "kernels.h"

#include <math.h>

namespace eosvos {
namespace {
constexpr int POTTS_TX = 32, POTTS_TY = 8;

// the engine's copy of the last forward's frames: fp32 [image][H + 2 pad][W + 2 pad][3]
struct PottsPadded {
  const float* p;
  int Hp, Wp, pad;
  __device__ __forceinline__ float operator()(int b, int c, int y, int x) const {
    return p[(((long)b * Hp + y + pad) * Wp + x + pad) * 3 + c];
  }
};
// a caller tensor: fp32 [image][3][H][W]
struct PottsPlanar {
  const float* p;
  long n_pix;
  int W;
  __device__ __forceinline__ float operator()(int b, int c, int y, int x) const {
    return p[((long)b * 3 + c) * n_pix + (long)y * W + x];
  }
};

// sigmoid(|z|) and sigmoid(-|z|) from one exp, without a cancellation; a NaN stays a NaN
__device__ __forceinline__ void potts_sigmoid(float z, float& hi, float& lo) {
  const float e = expf(-fabsf(z));
  hi = 1.f / (1.f + e);
  lo = e / (1.f + e);
}

// the sum over the workgroup's 256 threads in a fixed order, valid in thread 0: lanes by shuffles, the waves in wave order
__device__ __forceinline__ float potts_block_sum(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// grid (ceil(W / 32), ceil(H / 8), images), block 256.  partial: [image][2][tiles] (E, then Z); grad may be null
template <class Frame>
__global__ __launch_bounds__(256) void potts_stencil_kernel(Frame img, const float* __restrict__ logits, float* __restrict__ grad,
                                                             float* __restrict__ partial, int H, int W, int r, int d, float inv_2s2,
                                                             PottsTable tab) {
  extern __shared__ __align__(16) float potts_lds[];
  const int h = r * d, TW = POTTS_TX + 2 * h, TH = POTTS_TY + 2 * h, tile = TW * TH;
  float* s_img = potts_lds;                // [3][TH][TW]
  float* s_p = potts_lds + 3 * tile;       // [TH][TW]
  float* s_red = potts_lds + 4 * tile;     // [2][4]
  const long n_pix = (long)H * W;
  const int f = blockIdx.z;
  logits += (long)f * n_pix;
  const int x0 = (int)blockIdx.x * POTTS_TX - h, y0 = (int)blockIdx.y * POTTS_TY - h;
  const int lx = threadIdx.x & (POTTS_TX - 1), ly = threadIdx.x >> 5;
  const int gx = x0 + h + lx, gy = y0 + h + ly;
  const bool live = gx < W && gy < H;
  const int side = 2 * r + 1;

  for (int i = threadIdx.x; i < tile; i += 256) {
    const int ty = i / TW, tx = i - ty * TW;
    const int sy = y0 + ty, sx = x0 + tx;
    const bool in = (unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W;
    float pr = 0.f;
    if (in) {
      float hi, lo;
      const float z = logits[(long)sy * W + sx];
      potts_sigmoid(z, hi, lo);
      pr = z >= 0.f ? hi : (z < 0.f ? lo : z);      // (a NaN logit: p is that NaN)
    }
    s_p[i] = pr;
#pragma unroll
    for (int c = 0; c < 3; ++c) s_img[c * tile + i] = in ? img(f, c, sy, sx) : 0.f;
  }
  __syncthreads();

  const int centre = (ly + h) * TW + lx + h;
  const float cr = s_img[centre], cg = s_img[tile + centre], cb = s_img[2 * tile + centre];
  float S = 0.f, M = 0.f;
  for (int dy = -r; dy <= r; ++dy) {
    const bool iny = (unsigned)(gy + dy * d) < (unsigned)H;
    const int row = centre + dy * d * TW;
    const int k0 = (dy + r) * side + r;
    for (int dx = -r; dx <= r; ++dx) {
      if ((dy | dx) == 0) continue;
      const int o = row + dx * d;
      const bool in = iny && (unsigned)(gx + dx * d) < (unsigned)W;
      const float er = cr - s_img[o], eg = cg - s_img[tile + o], eb = cb - s_img[2 * tile + o];
      const float k = in ? tab.w[k0 + dx] * expf(-(er * er + eg * eg + eb * eb) * inv_2s2) : 0.f;
      S += k;
      M += k * s_p[o];
    }
  }
  float e = 0.f, zz = 0.f;
  if (live) {
    const long pix = (long)gy * W + gx;
    if (grad) {
      float hi, lo;
      potts_sigmoid(logits[pix], hi, lo);
      grad[(long)f * n_pix + pix] = (S - 2.f * M) * (hi * lo);       // p (1 - p) = hi * lo
    }
    e = s_p[centre] * (S - M);
    zz = S;
  }
  e = potts_block_sum(e, s_red);
  zz = potts_block_sum(zz, s_red + 4);
  if (threadIdx.x == 0) {
    const long tiles = (long)gridDim.x * gridDim.y, t = (long)blockIdx.y * gridDim.x + blockIdx.x;
    partial[((long)f * 2) * tiles + t] = e;
    partial[((long)f * 2 + 1) * tiles + t] = zz;
  }
}

// grid 1, block 256.  Image after image: thread t adds the partials t, t + 256, ..., then the workgroup's fixed-order sum.
// loss = the mean over the images of E / Z (0 where Z is 0); scale[image] = 1 / (Z * images), 0 where Z is 0
__global__ __launch_bounds__(256) void potts_finish_kernel(const float* __restrict__ partial, int tiles, int images,
                                                            float* __restrict__ loss, float* __restrict__ scale) {
  __shared__ float red[8];
  float total = 0.f;
  for (int m = 0; m < images; ++m) {
    const float* pe = partial + (size_t)m * 2 * tiles;
    const float* pz = pe + tiles;
    float e = 0.f, z = 0.f;
    for (int b = threadIdx.x; b < tiles; b += 256) {
      e += pe[b];
      z += pz[b];
    }
    e = potts_block_sum(e, red);
    z = potts_block_sum(z, red + 4);
    if (threadIdx.x == 0) {
      total += z == 0.f ? 0.f : e / z;
      scale[m] = z == 0.f ? 0.f : 1.f / (z * (float)images);
    }
    __syncthreads();                       // the slots are free for the next image
  }
  if (threadIdx.x == 0) *loss = total / (float)images;
}

// grid (ceil(n_pix / 256), images), block 256
__global__ __launch_bounds__(256) void potts_scale_kernel(float* __restrict__ grad, const float* __restrict__ scale, long n_pix) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pix) return;
  grad[(long)blockIdx.y * n_pix + i] *= scale[blockIdx.y];
}
// ... over float4 (n4 = n_pix / 4 per image)
__global__ __launch_bounds__(256) void potts_scale4_kernel(float4* __restrict__ grad, const float* __restrict__ scale, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float s = scale[blockIdx.y];
  float4 g = grad[(long)blockIdx.y * n4 + i];
  g.x *= s; g.y *= s; g.z *= s; g.w *= s;
  grad[(long)blockIdx.y * n4 + i] = g;
}

inline int potts_tiles(int H, int W) { return ((W + POTTS_TX - 1) / POTTS_TX) * ((H + POTTS_TY - 1) / POTTS_TY); }
}  // namespace

int64_t potts_scratch_floats(int H, int W, int images) { return (int64_t)images * (2 * (int64_t)potts_tiles(H, W) + 1); }

void potts_fill_table(PottsTable& tab, int r, int d, float sigma_xy) {
  const int side = 2 * r + 1;
  const double is = 1.0 / (2.0 * (double)sigma_xy * (double)sigma_xy);
  for (int i = 0; i < CRF_MAX_SIDE * CRF_MAX_SIDE; ++i) tab.w[i] = 0.f;
  for (int dy = -r; dy <= r; ++dy)
    for (int dx = -r; dx <= r; ++dx) {
      const double d2 = (double)(dy * d) * (dy * d) + (double)(dx * d) * (dx * d);
      tab.w[(dy + r) * side + dx + r] = (float)exp(-d2 * is);
    }
}

void launch_potts(const float* logits, const float* frames, int pad, float* dlogits, float* loss, float* scratch, int H, int W,
                  int images, int r, int d, float sigma_xy, float sigma_rgb, hipStream_t s) {
  PottsTable tab;
  potts_fill_table(tab, r, d, sigma_xy);
  const int h = r * d, tiles = potts_tiles(H, W);
  const size_t lds = ((size_t)4 * (POTTS_TX + 2 * h) * (POTTS_TY + 2 * h) + 8) * sizeof(float);
  const dim3 grid((W + POTTS_TX - 1) / POTTS_TX, (H + POTTS_TY - 1) / POTTS_TY, images);
  const float inv_2s2 = (float)(1.0 / (2.0 * (double)sigma_rgb * (double)sigma_rgb));
  const long n_pix = (long)H * W;
  float* partial = scratch;
  float* scale = scratch + (size_t)images * 2 * tiles;
  if (pad)
    hipLaunchKernelGGL(potts_stencil_kernel<PottsPadded>, grid, dim3(256), lds, s, PottsPadded{frames, H + 2 * pad, W + 2 * pad, pad},
                       logits, dlogits, partial, H, W, r, d, inv_2s2, tab);
  else
    hipLaunchKernelGGL(potts_stencil_kernel<PottsPlanar>, grid, dim3(256), lds, s, PottsPlanar{frames, n_pix, W}, logits, dlogits,
                       partial, H, W, r, d, inv_2s2, tab);
  hipLaunchKernelGGL(potts_finish_kernel, dim3(1), dim3(256), 0, s, partial, tiles, images, loss, scale);
  if (!dlogits) return;
  if (n_pix % 4 == 0 && ((uintptr_t)dlogits & 15) == 0)
    hipLaunchKernelGGL(potts_scale4_kernel, dim3((unsigned)((n_pix / 4 + 255) / 256), images), dim3(256), 0, s, (float4*)dlogits, scale,
                       n_pix / 4);
  else
    hipLaunchKernelGGL(potts_scale_kernel, dim3((unsigned)((n_pix + 255) / 256), images), dim3(256), 0, s, dlogits, scale, n_pix);
}
}  // namespace eosvos
