// Soft boundary-F loss (Bokhovkin & Burnaev 2019) + gradient for gfx950: 1 - F of max-pool boundary maps, per image.
//
// For one image of H x W pixels, z the logits, y the targets, V the valid (non-void) pixels; every window is square, centred,
// clipped to the frame and ranges over valid pixels only (a valid pixel is always in its own windows):
//   q = sigmoid(-z) (the sign branch of loss_expr.h, never 1 - sigmoid(z)),  h = 1 - y
//   pb(i) = max_{N1(i)} q - q(i),   gb(i) = max_{N1(i)} h - h(i)            N1: 3 x 3;  both 0 at void pixels
//   pe(i) = max_{Nr(i)} pb,         ge(i) = max_{Nr(i)} gb                  Nr: (2r+1)^2; both 0 at void pixels
//   Sp = sum_V pb + eps, Sg = sum_V gb + eps, P = sum_V pb ge / Sp, R = sum_V pe gb / Sg, BF = 2PR / (P + R + eps), eps = 1e-7
//   image loss = 1 - BF (0 for an image without a valid pixel);  loss = the mean over the images
// Among equal maxima the first in row-major order is the arg-max (a1 of q in N1, ar of pb in Nr); with B images
//   G_pb(j) = -[dBF/dP (ge(j) - P) / Sp + dBF/dR / Sg * sum_{i: ar(i) = j} gb(i)]
//   G_q(k)  = sum_{i: a1(i) = k} G_pb(i) - G_pb(k),     dL/dz(k) = -sigmoid(z_k) q_k G_q(k) / B, exactly 0 at void pixels.
//
// Launches (one stream, every dependency a kernel boundary; blockIdx.y = image, 256 threads = 4 waves of 64, grid-stride):
//   q      q per pixel from a double exp, -inf at void pixels: the sentinel every later window test uses
//   edge   pb, gb, the 4-bit code of a1 (15 at void pixels); per-block fp64 partials of sum pb, sum gb and |V|
//   row    the (2r+1) row maxima of pb (over valid pixels, with the offset of the first) and of gb
//   col    the column maxima of the row maxima: ge, ar (rows first, then columns: exactly the row-major tie rule), and the
//          partials of sum pb ge and sum pe gb; pe is not stored
//   final  one workgroup: the partials in a fixed order, P, R, the loss and the coefficients of G_pb per image
//   gpb    G_pb by gather: pixel j scans Nr(j) for the pixels whose ar is j; a window row whose gb row maximum is 0 holds
//          none and is skipped, so only the band around the target's contour does any work
//   grad   G_q by a 9-neighbour gather in row-major order, dL/dz
// No atomics at all, every sum in a fixed order, nothing read before this call wrote it: two evaluations are bit-identical.
// The neighbour reads go through L1 / L2 (a pixel's window overlaps its neighbours'), no LDS tile is kept.
#include "kernels.h"

namespace eosvos {
namespace {

constexpr int BF_THREADS = 256;
constexpr int BF_PARTS = 5;                      // per image and block: sum pb, sum gb, |V|, sum pb ge, sum pe gb
constexpr int BF_COEF = 4;                       // per image: P, dBF/dP / Sp, dBF/dR / Sg, (unused)
constexpr double BF_EPS = 1e-7;

struct BfScratch {
  double* partial;                               // [images][BF_PARTS][BOUNDARY_BLOCKS]
  float *coef, *q, *pb, *gb, *rpb, *rgb, *ge, *gpb;
  int* ar;
  unsigned char *a1, *rarg;
};
inline BfScratch bf_carve(float* scratch, int images, int64_t n) {
  BfScratch S;
  S.partial = (double*)scratch;                                  // (hipMalloc alignment keeps the fp64 words aligned)
  S.coef = (float*)(S.partial + (int64_t)images * BF_PARTS * BOUNDARY_BLOCKS);
  S.q = S.coef + (int64_t)images * BF_COEF;
  S.pb = S.q + n; S.gb = S.pb + n; S.rpb = S.gb + n; S.rgb = S.rpb + n; S.ge = S.rgb + n; S.gpb = S.ge + n;
  S.ar = (int*)(S.gpb + n);
  S.a1 = (unsigned char*)(S.ar + n);
  S.rarg = S.a1 + n;
  return S;
}

#define BF_PIXELS(i, n) for (long i = (long)blockIdx.x * BF_THREADS + threadIdx.x; i < (n); i += (long)gridDim.x * BF_THREADS)

// fp64 sum over the 256 threads in a fixed order, valid in thread 0
__device__ __forceinline__ double bf_block_sum(double v, double* sh /*4*/) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// sigmoid(-z) and sigmoid(z) with the branch on the sign of z; the exponential in double, so both round once
__device__ __forceinline__ void bf_sigmoids(float z, float& q, float& sig) {
  const double e = exp(-fabs((double)z));
  const double a = 1.0 / (1.0 + e), b = e / (1.0 + e);
  q = (float)(z >= 0.f ? b : a);
  sig = (float)(z >= 0.f ? a : b);
}

__global__ __launch_bounds__(BF_THREADS) void boundary_q_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                                float* __restrict__ q, long P, int has_ign, float ign) {
  const long o = (long)blockIdx.y * P;
  BF_PIXELS(i, P) {
    float qv, sig;
    bf_sigmoids(z[o + i], qv, sig);
    q[o + i] = (has_ign && y[o + i] == ign) ? -INFINITY : qv;      // selected: a void logit may be NaN / inf
  }
}

__global__ __launch_bounds__(BF_THREADS) void boundary_edge_kernel(const float* __restrict__ q, const float* __restrict__ y,
                                                                   float* __restrict__ pb, float* __restrict__ gb,
                                                                   unsigned char* __restrict__ a1, double* __restrict__ partial,
                                                                   int H, int W) {
  __shared__ double sh[4];
  const long P = (long)H * W, o = (long)blockIdx.y * P;
  double s_pb = 0.0, s_gb = 0.0, s_n = 0.0;
  BF_PIXELS(i, P) {
    const int yy = (int)(i / W), xx = (int)(i - (long)yy * W);
    const float qc = q[o + i];
    float pv = 0.f, gv = 0.f;
    int code = 15;
    if (qc != -INFINITY) {                       // valid (a NaN q is a valid pixel)
      float m = -INFINITY, hm = -INFINITY;
      code = 4;
      for (int dy = -1; dy <= 1; ++dy) {
        const int y2 = yy + dy;
        if (y2 < 0 || y2 >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
          const int x2 = xx + dx;
          if (x2 < 0 || x2 >= W) continue;
          const long j = o + (long)y2 * W + x2;
          const float qn = q[j];
          if (qn == -INFINITY) continue;         // void
          if (qn > m) { m = qn; code = (dy + 1) * 3 + (dx + 1); }
          hm = fmaxf(hm, 1.f - y[j]);
        }
      }
      pv = m - qc;                               // NaN where q(i) is NaN: the sums, and with them the loss, turn NaN
      gv = hm - (1.f - y[o + i]);
      s_pb += (double)pv; s_gb += (double)gv; s_n += 1.0;
    }
    pb[o + i] = pv; gb[o + i] = gv; a1[o + i] = (unsigned char)code;
  }
  double* pp = partial + (long)blockIdx.y * BF_PARTS * BOUNDARY_BLOCKS + blockIdx.x;
  const double a = bf_block_sum(s_pb, sh), b = bf_block_sum(s_gb, sh), c = bf_block_sum(s_n, sh);
  if (threadIdx.x == 0) { pp[0] = a; pp[BOUNDARY_BLOCKS] = b; pp[2 * BOUNDARY_BLOCKS] = c; }
}

// every pixel, void ones too (a column window passes through them): rpb = the maximum of pb over the valid pixels of the row
// window (-inf when it holds none), rarg = the offset + r of the first one that reaches it; rgb = the maximum of gb (gb is 0 at
// void pixels and >= 0 elsewhere, so no validity test is needed for a value)
__global__ __launch_bounds__(BF_THREADS) void boundary_row_kernel(const float* __restrict__ q, const float* __restrict__ pb,
                                                                  const float* __restrict__ gb, float* __restrict__ rpb,
                                                                  float* __restrict__ rgb, unsigned char* __restrict__ rarg,
                                                                  int H, int W, int r) {
  const long P = (long)H * W, o = (long)blockIdx.y * P;
  BF_PIXELS(i, P) {
    const int yy = (int)(i / W), xx = (int)(i - (long)yy * W);
    const int x0 = xx - r < 0 ? 0 : xx - r, x1 = xx + r >= W ? W - 1 : xx + r;
    const long row = o + (long)yy * W;
    float m = -INFINITY, g = 0.f;
    int arg = r;
    for (int x2 = x0; x2 <= x1; ++x2) {
      const float v = pb[row + x2];
      if (q[row + x2] != -INFINITY && v > m) { m = v; arg = x2 - xx + r; }
      g = fmaxf(g, gb[row + x2]);
    }
    rpb[o + i] = m; rgb[o + i] = g; rarg[o + i] = (unsigned char)arg;
  }
}

__global__ __launch_bounds__(BF_THREADS) void boundary_col_kernel(const float* __restrict__ q, const float* __restrict__ pb,
                                                                  const float* __restrict__ gb, const float* __restrict__ rpb,
                                                                  const float* __restrict__ rgb,
                                                                  const unsigned char* __restrict__ rarg, float* __restrict__ ge,
                                                                  int* __restrict__ ar, double* __restrict__ partial, int H, int W,
                                                                  int r) {
  __shared__ double sh[4];
  const long P = (long)H * W, o = (long)blockIdx.y * P;
  double s_p = 0.0, s_r = 0.0;
  BF_PIXELS(i, P) {
    const int yy = (int)(i / W), xx = (int)(i - (long)yy * W);
    float gev = 0.f;
    int arg = -1;
    if (q[o + i] != -INFINITY) {
      const int y0 = yy - r < 0 ? 0 : yy - r, y1 = yy + r >= H ? H - 1 : yy + r;
      float m = -INFINITY;
      arg = (int)i;                              // (kept only when every pb of the window is NaN)
      for (int y2 = y0; y2 <= y1; ++y2) {
        const long j = o + (long)y2 * W + xx;
        const float v = rpb[j];
        if (v > m) { m = v; arg = y2 * W + xx + (int)rarg[j] - r; }
        gev = fmaxf(gev, rgb[j]);
      }
      s_p += (double)pb[o + i] * (double)gev;
      s_r += (double)m * (double)gb[o + i];
    }
    ge[o + i] = gev; ar[o + i] = arg;
  }
  double* pp = partial + (long)blockIdx.y * BF_PARTS * BOUNDARY_BLOCKS + blockIdx.x;
  const double a = bf_block_sum(s_p, sh), b = bf_block_sum(s_r, sh);
  if (threadIdx.x == 0) { pp[3 * BOUNDARY_BLOCKS] = a; pp[4 * BOUNDARY_BLOCKS] = b; }
}

// one workgroup.  `add`: the loss already holds the cross-entropy term of the combined kind.
__global__ __launch_bounds__(BF_THREADS) void boundary_final_kernel(const double* __restrict__ partial, float* __restrict__ coef,
                                                                    float* __restrict__ loss, int images, int nb, int add) {
  __shared__ double sh[4];
  double tot = 0.0;
  for (int img = 0; img < images; ++img) {
    double s[BF_PARTS];
    for (int k = 0; k < BF_PARTS; ++k) {
      const double* pp = partial + ((long)img * BF_PARTS + k) * BOUNDARY_BLOCKS;
      double a = 0.0;
      for (int b = threadIdx.x; b < nb; b += BF_THREADS) a += pp[b];
      s[k] = bf_block_sum(a, sh);
    }
    if (threadIdx.x == 0) {
      float* c = coef + img * BF_COEF;
      if (s[2] > 0.0) {
        const double Sp = s[0] + BF_EPS, Sg = s[1] + BF_EPS, Pv = s[3] / Sp, Rv = s[4] / Sg, d = Pv + Rv + BF_EPS;
        tot += 1.0 - 2.0 * Pv * Rv / d;
        c[0] = (float)Pv;
        c[1] = (float)(2.0 * Rv * (Rv + BF_EPS) / (d * d) / Sp);
        c[2] = (float)(2.0 * Pv * (Pv + BF_EPS) / (d * d) / Sg);
      } else {                                   // no valid pixel: loss 0, gradient 0
        c[0] = 0.f; c[1] = 0.f; c[2] = 0.f;
      }
      c[3] = 0.f;
    }
  }
  if (threadIdx.x == 0) {
    const float v = (float)(tot / (double)images);
    loss[0] = add ? loss[0] + v : v;
  }
}

__global__ __launch_bounds__(BF_THREADS) void boundary_gpb_kernel(const float* __restrict__ q, const float* __restrict__ gb,
                                                                  const float* __restrict__ rgb, const float* __restrict__ ge,
                                                                  const int* __restrict__ ar, const float* __restrict__ coef,
                                                                  float* __restrict__ gpb, int H, int W, int r) {
  const long P = (long)H * W, o = (long)blockIdx.y * P;
  const float* c = coef + blockIdx.y * BF_COEF;
  const float Pv = c[0], cP = c[1], cR = c[2];
  BF_PIXELS(i, P) {
    float out = 0.f;
    if (q[o + i] != -INFINITY) {
      const float gev = ge[o + i];
      float s = 0.f;
      if (gev != 0.f) {                          // otherwise gb is 0 in the whole window
        const int yy = (int)(i / W), xx = (int)(i - (long)yy * W);
        const int y0 = yy - r < 0 ? 0 : yy - r, y1 = yy + r >= H ? H - 1 : yy + r;
        const int x0 = xx - r < 0 ? 0 : xx - r, x1 = xx + r >= W ? W - 1 : xx + r;
        for (int y2 = y0; y2 <= y1; ++y2) {
          const long row = o + (long)y2 * W;
          if (rgb[row + xx] == 0.f) continue;    // gb is 0 on this row of the window
          for (int x2 = x0; x2 <= x1; ++x2) {
            const float g = gb[row + x2];
            if (g != 0.f && ar[row + x2] == (int)i) s += g;
          }
        }
      }
      out = -(cP * (gev - Pv) + cR * s);
    }
    gpb[o + i] = out;
  }
}

// `add`: dz already holds the cross-entropy gradient of the combined kind (exactly 0 at void pixels)
__global__ __launch_bounds__(BF_THREADS) void boundary_grad_kernel(const float* __restrict__ z, const float* __restrict__ q,
                                                                   const float* __restrict__ gpb,
                                                                   const unsigned char* __restrict__ a1, float* __restrict__ dz,
                                                                   int H, int W, float images, int add) {
  const long P = (long)H * W, o = (long)blockIdx.y * P;
  BF_PIXELS(i, P) {
    float out = 0.f;
    if (q[o + i] != -INFINITY) {
      const int yy = (int)(i / W), xx = (int)(i - (long)yy * W);
      float s = 0.f;
      for (int dy = -1; dy <= 1; ++dy) {
        const int y2 = yy + dy;
        if (y2 < 0 || y2 >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
          const int x2 = xx + dx;
          if (x2 < 0 || x2 >= W) continue;
          const long j = o + (long)y2 * W + x2;
          if ((int)a1[j] == (1 - dy) * 3 + (1 - dx)) s += gpb[j];      // the arg-max of j's 3 x 3 window is this pixel
        }
      }
      const float Gq = s - gpb[o + i];
      float qv, sig;
      bf_sigmoids(z[o + i], qv, sig);
      out = -(sig * qv) * Gq / images;
      if (add) out += dz[o + i];
    }
    dz[o + i] = out;
  }
}
}  // namespace

int64_t boundary_scratch_floats(int64_t n_total, int max_images) {
  // 8 words per pixel (q, pb, gb, two row maxima, ge, G_pb, ar) + 2 bytes (a1, the row offset), the partials, the coefficients
  return n_total * 8 + (n_total * 2 + 3) / 4 + (int64_t)max_images * (2 * BF_PARTS * BOUNDARY_BLOCKS + BF_COEF) + 16;
}

void launch_boundary_f(const float* logits, const float* gt, float* dlogits, float* loss, float* scratch, int H, int W, int images,
                       int radius, int add, const float* ignore, hipStream_t s) {
  const int64_t P = (int64_t)H * W;
  const BfScratch S = bf_carve(scratch, images, P * images);
  int64_t nbl = (P + BF_THREADS - 1) / BF_THREADS;
  const int nb = (int)(nbl > BOUNDARY_BLOCKS ? BOUNDARY_BLOCKS : nbl);
  const dim3 grid(nb, images), block(BF_THREADS);
  hipLaunchKernelGGL(boundary_q_kernel, grid, block, 0, s, logits, gt, S.q, (long)P, ignore ? 1 : 0, ignore ? *ignore : 0.f);
  hipLaunchKernelGGL(boundary_edge_kernel, grid, block, 0, s, S.q, gt, S.pb, S.gb, S.a1, S.partial, H, W);
  hipLaunchKernelGGL(boundary_row_kernel, grid, block, 0, s, S.q, S.pb, S.gb, S.rpb, S.rgb, S.rarg, H, W, radius);
  hipLaunchKernelGGL(boundary_col_kernel, grid, block, 0, s, S.q, S.pb, S.gb, S.rpb, S.rgb, S.rarg, S.ge, S.ar, S.partial, H, W,
                     radius);
  hipLaunchKernelGGL(boundary_final_kernel, dim3(1), block, 0, s, S.partial, S.coef, loss, images, nb, add);
  hipLaunchKernelGGL(boundary_gpb_kernel, grid, block, 0, s, S.q, S.gb, S.rgb, S.ge, S.ar, S.coef, S.gpb, H, W, radius);
  hipLaunchKernelGGL(boundary_grad_kernel, grid, block, 0, s, logits, S.q, S.gpb, S.a1, dlogits, H, W, (float)images, add);
}

}  // namespace eosvos
