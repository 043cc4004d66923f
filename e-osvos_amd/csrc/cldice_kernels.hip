// Soft centreline Dice (clDice, Shit et al., CVPR 2021) + gradient for gfx950: 1 - the harmonic mean of how much of each map's
// soft skeleton lies inside the other map, per image.  The soft skeleton comes from iterated min / max pooling.
//
// For one image of H x W pixels, z the logits, y the targets, V the valid (non-void) pixels, p = sigmoid(z) (the sign branch of
// loss_expr.h); every window is clipped to the frame and ranges over valid pixels only.  With x_0 = x (p, or y), depth k:
//   v_j(i) = the first minimum of x_j over (up, centre, down),  h_j(i) = the first minimum over (left, centre, right)
//   x_{j+1}(i) = min(v_j, h_j),  o_j(i) = the first maximum of x_{j+1} over 3 x 3 in row-major order,  d_j = max(x_j - o_j, 0)
//   S(x) = 1 - prod_{j = 0 .. k} (1 - d_j), the product in ascending j, every factor and product rounded on its own (no fma)
//   Tp = (sum_V S(p) y + 1) / (sum_V S(p) + 1),  Ts = (sum_V S(y) p + 1) / (sum_V S(y) + 1),  image loss = 1 - 2 Tp Ts / (Tp + Ts)
//   (0 for an image without a valid pixel);  loss = the mean over the images
// The gradient follows the selections: a window routes to its first extremum, min(v, h) to v's pixel if v < h, to h's if
// h < v, half to each if v = h.  With Bq = sum_V S(p) + 1, Sy = sum_V S(y) + 1, cP = -2 Ts^2 / (Tp + Ts)^2, cS = -2 Tp^2 / (Tp + Ts)^2:
//   g_S(i) = cP / Bq (y_i - Tp),  Gd_j(i) = [d_j(i) > 0] g_S(i) prod_{m != j} (1 - d_m(i))     (ascending m, no fma)
//   T_{k+1}(q) = -sum_{i in N3x3(q), arg o_k(i) = q} Gd_k(i)
//   T_j(q) = Gd_j(q) + sum_{i in cross(q)} w_j(i -> q) T_{j+1}(i) - [j >= 1] sum_{i in N3x3(q), arg o_{j-1}(i) = q} Gd_{j-1}(i)
//   dL/dz = (T_0 + cS / Sy S(y)) p (1 - p) / images, exactly +0 at void pixels;  S(y) carries no gradient
// both gathers in row-major order of i, the cross first; w in {0, 1/2, 1} from the erosion's routing.
//
// Launches (one stream, every dependency a kernel boundary; blockIdx.y = image, 256 threads = 4 waves of 64, grid-stride):
//   p       p and y per pixel, -inf at void pixels: the sentinel every later window test uses
//   erode   per level: x_{j+1} of both chains, the routing of p's (2 + 2 + 2 bits of the level's 16-bit code)
//   dilate  per level: o_j, d_j of p's chain (fp32) with its arg (4 bits), the running product of y's chain, S(y) at the last
//   sum     S(p) from the d_j, per-block fp64 partials of the four sums and |V|
//   final   one workgroup: the partials in a fixed order, the loss, Tp and the two coefficients per image
//   gd      Gd_j over d_j in place, all levels of a pixel by one thread (its d_j staged in LDS, 17 x 256 words)
//   back    T_{k+1}, then one launch per level j = k .. 0 (cross gather, 3 x 3 gather, Gd_j); the last writes dL/dz
// 3 k + 8 launches.  No atomics at all, every sum in a fixed order, nothing read before this call wrote it: two evaluations are
// bit-identical.  The neighbour reads go through L1 / L2 (a pixel's window overlaps its neighbours'), no LDS tile is kept.
#include "kernels.h"

namespace eosvos {
namespace {

constexpr int CD_THREADS = 256;
constexpr int CD_PARTS = 5;                      // per image and block: sum S(p) y, sum S(p), sum S(y) p, sum S(y), |V|
constexpr int CD_COEF = 4;                       // per image: Tp, cP / Bq, cS / Sy, (unused)
constexpr int CD_LEVELS = CLDICE_MAX_DEPTH + 1;
// the 16-bit code of a pixel and level: bits 0-1 the vertical arg (0 up, 1 centre, 2 down), 2-3 the horizontal arg (0 left,
// 1 centre, 2 right), 4-5 which of v / h / both won (0 / 1 / 2), 6-9 the arg of the 3 x 3 maximum (row-major), 10 void
constexpr unsigned CD_VOID = 0x3u | 0xCu | (15u << 6) | (1u << 10);     // args no gather ever looks for

struct CdScratch {
  double* partial;                               // [images][CD_PARTS][CLDICE_BLOCKS]
  float *coef, *p, *sy, *xa, *xb, *ta, *tb, *d;  // d: [level][images][H][W]
  unsigned short* code;                          // [level][images][H][W]
};
inline CdScratch cd_carve(float* scratch, int images, int64_t n, int levels) {
  CdScratch S;
  S.partial = (double*)scratch;                                  // (the allocation's alignment keeps the fp64 words aligned)
  S.coef = (float*)(S.partial + (int64_t)images * CD_PARTS * CLDICE_BLOCKS);
  S.p = S.coef + (int64_t)images * CD_COEF;
  S.sy = S.p + n; S.xa = S.sy + n; S.xb = S.xa + n; S.ta = S.xb + n; S.tb = S.ta + n; S.d = S.tb + n;
  S.code = (unsigned short*)(S.d + n * levels);
  return S;
}

// an image has at most 4096 x 4096 pixels: 32-bit pixel indices (and a 32-bit division for the row), 64-bit offsets of the image
#define CD_PIXELS(i, n) for (int i = blockIdx.x * CD_THREADS + threadIdx.x; i < (n); i += gridDim.x * CD_THREADS)

// fp64 sum over the 256 threads in a fixed order, valid in thread 0
__device__ __forceinline__ double cd_block_sum(double v, double* sh /*4*/) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// u (1 - d) and 1 - u, every difference and product rounded on its own.  hipcc contracts a * b - c into one fused multiply-add by
// default and the __fmul_rn / __fsub_rn family does not stop it (misc_kernels.hip at loss_sum_of), so these are plain operators
// under the pragma.
__device__ __forceinline__ float cd_times_1m(float u, float d) {
#pragma clang fp contract(off)
  const float f = 1.f - d;
  return u * f;
}
__device__ __forceinline__ float cd_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float cd_1m(float u) {
#pragma clang fp contract(off)
  return 1.f - u;
}

// sigmoid(z) and sigmoid(-z) with the branch on the sign of z (loss_expr.h: bce_grad)
__device__ __forceinline__ void cd_sigmoids(float z, float& p, float& q) {
  const float e = expf(-fabsf(z));
  const float a = 1.f / (1.f + e), b = e / (1.f + e);
  p = z >= 0.f ? a : b;
  q = z >= 0.f ? b : a;
}

// x = the map (the logits' sigmoid with `logits`) and, where yx is not null, yx = the targets; -inf where the target (the map
// itself without one) is the void label
__global__ __launch_bounds__(CD_THREADS) void cldice_p_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                              float* __restrict__ x, float* __restrict__ yx, int P, int logits,
                                                              int has_ign, float ign) {
  const long o = (long)blockIdx.y * P;
  CD_PIXELS(i, P) {
    const float zv = z[o + i], yv = y ? y[o + i] : zv;
    const bool dead = has_ign && yv == ign;
    float p = zv, q;
    if (logits) cd_sigmoids(zv, p, q);
    x[o + i] = dead ? -INFINITY : p;                               // selected: a void logit may be NaN / inf
    if (yx) yx[o + i] = dead ? -INFINITY : yv;
  }
}

// the first minimum of x over the valid pixels at i - step, i, i + step (those with lo / hi); arg 1 = the centre
__device__ __forceinline__ float cd_min3(const float* __restrict__ x, long i, long step, bool lo, bool hi, int& arg) {
  float m = INFINITY;
  arg = 1;
  if (lo) { const float v = x[i - step]; if (v != -INFINITY && v < m) { m = v; arg = 0; } }
  { const float v = x[i]; if (v < m) { m = v; arg = 1; } }
  if (hi) { const float v = x[i + step]; if (v != -INFINITY && v < m) { m = v; arg = 2; } }
  return m;
}

// one erosion of chain A (xa -> xb, its routing to `code` unless that is null) and, unless ya is null, of chain B (ya -> yb)
__global__ __launch_bounds__(CD_THREADS) void cldice_erode_kernel(const float* __restrict__ xa, float* __restrict__ xb,
                                                                  const float* __restrict__ ya, float* __restrict__ yb,
                                                                  unsigned short* __restrict__ code, int H, int W) {
  const int P = H * W;
  const long o = (long)blockIdx.y * P;
  CD_PIXELS(i, P) {
    const int yy = (int)((unsigned)i / (unsigned)W), xx = i - yy * W;
    const long g = o + i;
    float nx = -INFINITY, ny = -INFINITY;
    unsigned c = CD_VOID;
    if (xa[g] != -INFINITY) {                    // valid (a NaN is a valid pixel)
      const bool up = yy > 0, down = yy + 1 < H, left = xx > 0, right = xx + 1 < W;
      int av, ah;
      const float v = cd_min3(xa, g, W, up, down, av), h = cd_min3(xa, g, 1, left, right, ah);
      const unsigned which = v < h ? 0u : h < v ? 1u : 2u;
      nx = which == 1u ? h : v;
      c = (unsigned)av | ((unsigned)ah << 2) | (which << 4);
      if (ya) {
        int a0, a1;
        const float vy = cd_min3(ya, g, W, up, down, a0), hy = cd_min3(ya, g, 1, left, right, a1);
        ny = hy < vy ? hy : vy;
      }
    }
    xb[g] = nx;
    if (ya) yb[g] = ny;
    if (code) code[g] = (unsigned short)c;
  }
}

// the first maximum of x over the valid pixels of the 3 x 3 window in row-major order (void pixels hold -inf and never win)
__device__ __forceinline__ float cd_max9(const float* __restrict__ x, long o, int yy, int xx, int H, int W, int& arg) {
  float m = -INFINITY;
  arg = 4;
  for (int dy = -1; dy <= 1; ++dy) {
    const int y2 = yy + dy;
    if (y2 < 0 || y2 >= H) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int x2 = xx + dx;
      if (x2 < 0 || x2 >= W) continue;
      const float v = x[o + (long)y2 * W + x2];
      if (v > m) { m = v; arg = (dy + 1) * 3 + (dx + 1); }
    }
  }
  return m;
}

// the dilation and increment of one level.  Chain A: x_j = xa, x_{j+1} = xb; d_j to `d` and the arg into `code` (both may be
// null), the running product into ua (may be null).  Chain B (ya null: none): the running product into ub.  `first`: the
// products start at 1; `last`: the product planes receive S = 1 - u (0 at void pixels) instead.
__global__ __launch_bounds__(CD_THREADS) void cldice_dilate_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                                   const float* __restrict__ ya, const float* __restrict__ yb,
                                                                   float* __restrict__ d, unsigned short* __restrict__ code,
                                                                   float* __restrict__ ua, float* __restrict__ ub, int H, int W,
                                                                   int first, int last) {
  const int P = H * W;
  const long o = (long)blockIdx.y * P;
  CD_PIXELS(i, P) {
    const int yy = (int)((unsigned)i / (unsigned)W), xx = i - yy * W;
    const long g = o + i;
    const bool valid = xa[g] != -INFINITY;
    float dv = 0.f, dyv = 0.f;
    if (valid) {
      int ad;
      const float t = xa[g] - cd_max9(xb, o, yy, xx, H, W, ad);
      dv = t > 0.f ? t : 0.f;
      if (code) code[g] = (unsigned short)((unsigned)code[g] | ((unsigned)ad << 6));
      if (ya) {
        int a0;
        const float ty = ya[g] - cd_max9(yb, o, yy, xx, H, W, a0);
        dyv = ty > 0.f ? ty : 0.f;
      }
    }
    if (d) d[g] = dv;
    if (ua) {
      const float u = cd_times_1m(first ? 1.f : ua[g], dv);
      ua[g] = last ? (valid ? cd_1m(u) : 0.f) : u;
    }
    if (ya) {
      const float u = cd_times_1m(first ? 1.f : ub[g], dyv);
      ub[g] = last ? (valid ? cd_1m(u) : 0.f) : u;
    }
  }
}

__global__ __launch_bounds__(CD_THREADS) void cldice_sum_kernel(const float* __restrict__ p, const float* __restrict__ y,
                                                                const float* __restrict__ d, const float* __restrict__ sy,
                                                                double* __restrict__ partial, int P, long n_total, int levels) {
  __shared__ double sh[4];
  const long o = (long)blockIdx.y * P;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, sn = 0.0;
  CD_PIXELS(i, P) {
    const long g = o + i;
    const float pv = p[g];
    if (pv != -INFINITY) {
      float u = 1.f;
      for (int j = 0; j < levels; ++j) u = cd_times_1m(u, d[(long)j * n_total + g]);
      const double sp = (double)cd_1m(u), syv = (double)sy[g];
      s0 += sp * (double)y[g]; s1 += sp; s2 += syv * (double)pv; s3 += syv; sn += 1.0;     // a NaN p reaches s2 whatever S(y) is
    }
  }
  double* pp = partial + (long)blockIdx.y * CD_PARTS * CLDICE_BLOCKS + blockIdx.x;
  const double a = cd_block_sum(s0, sh), b = cd_block_sum(s1, sh), c = cd_block_sum(s2, sh), e = cd_block_sum(s3, sh),
               f = cd_block_sum(sn, sh);
  if (threadIdx.x == 0) {
    pp[0] = a; pp[CLDICE_BLOCKS] = b; pp[2 * CLDICE_BLOCKS] = c; pp[3 * CLDICE_BLOCKS] = e; pp[4 * CLDICE_BLOCKS] = f;
  }
}

// one workgroup
__global__ __launch_bounds__(CD_THREADS) void cldice_final_kernel(const double* __restrict__ partial, float* __restrict__ coef,
                                                                  float* __restrict__ loss, int images, int nb) {
  __shared__ double sh[4];
  double tot = 0.0;
  for (int img = 0; img < images; ++img) {
    double s[CD_PARTS];
    for (int k = 0; k < CD_PARTS; ++k) {
      const double* pp = partial + ((long)img * CD_PARTS + k) * CLDICE_BLOCKS;
      double a = 0.0;
      for (int b = threadIdx.x; b < nb; b += CD_THREADS) a += pp[b];
      s[k] = cd_block_sum(a, sh);
    }
    if (threadIdx.x == 0) {
      float* c = coef + img * CD_COEF;
      if (s[4] > 0.0) {
        const double Bq = s[1] + 1.0, Sy = s[3] + 1.0, Tp = (s[0] + 1.0) / Bq, Ts = (s[2] + 1.0) / Sy, den = Tp + Ts;
        tot += 1.0 - 2.0 * Tp * Ts / den;
        c[0] = (float)Tp;
        c[1] = (float)(-2.0 * Ts * Ts / (den * den) / Bq);
        c[2] = (float)(-2.0 * Tp * Tp / (den * den) / Sy);
      } else {                                   // no valid pixel: loss 0, gradient 0
        c[0] = 0.f; c[1] = 0.f; c[2] = 0.f;
      }
      c[3] = 0.f;
    }
  }
  if (threadIdx.x == 0) loss[0] = (float)(tot / (double)images);
}

// Gd_j over d_j in place.  A thread stages its pixel's d_j in its own LDS column (no thread reads another's: no barrier).
__global__ __launch_bounds__(CD_THREADS) void cldice_gd_kernel(const float* __restrict__ p, const float* __restrict__ y,
                                                               float* __restrict__ d, const float* __restrict__ coef, int P,
                                                               long n_total, int levels) {
  __shared__ float dl[CD_LEVELS][CD_THREADS];
  const long o = (long)blockIdx.y * P;
  const float Tp = coef[blockIdx.y * CD_COEF], c1 = coef[blockIdx.y * CD_COEF + 1];
  CD_PIXELS(i, P) {
    const long g = o + i;
    if (p[g] == -INFINITY) continue;             // void: every d_j is 0 already, which is its Gd_j
    const float gs = c1 * (y[g] - Tp);
    for (int j = 0; j < levels; ++j) dl[j][threadIdx.x] = d[(long)j * n_total + g];
    for (int j = 0; j < levels; ++j) {
      float out = 0.f;
      if (dl[j][threadIdx.x] > 0.f) {
        float e = 1.f;
        for (int m = 0; m < levels; ++m)
          if (m != j) e = cd_times_1m(e, dl[m][threadIdx.x]);
        out = cd_mul(gs, e);
      }
      d[(long)j * n_total + g] = out;
    }
  }
}

// One level of the backward pass: T_j = Gd_j (gd; null: 0) + the cross gather of T_{j+1} (tin; null: none) through the routing
// of level j (code) - the 3 x 3 gather of Gd_{j-1} (gdm; null: none) through the args of level j - 1 (codem).  T_{k+1} is the
// launch with the 3 x 3 gather of level k alone.  With dz (the launch of level 0) the result is dL/dz instead of tout.
__global__ __launch_bounds__(CD_THREADS) void cldice_back_kernel(const float* __restrict__ tin, float* __restrict__ tout,
                                                                 const float* __restrict__ gd, const float* __restrict__ gdm,
                                                                 const unsigned short* __restrict__ code,
                                                                 const unsigned short* __restrict__ codem,
                                                                 const float* __restrict__ z, const float* __restrict__ sy,
                                                                 const float* __restrict__ coef, float* __restrict__ dz, int H,
                                                                 int W, float images) {
  const int P = H * W;
  const long o = (long)blockIdx.y * P;
  const float c2 = coef[blockIdx.y * CD_COEF + 2];
  CD_PIXELS(i, P) {
    const int yy = (int)((unsigned)i / (unsigned)W), xx = i - yy * W;
    const long g = o + i;
    float out = 0.f;
    if (!(((unsigned)code[g] >> 10) & 1u)) {
      float a = gd ? gd[g] : 0.f;
      if (tin) {                                 // up, left, centre, right, down: the pixels whose windows hold this one
        if (yy > 0) { const unsigned c = code[g - W]; a += ((c & 3u) == 2u ? ((c >> 4 & 3u) == 0u ? 1.f : (c >> 4 & 3u) == 2u ? 0.5f : 0.f) : 0.f) * tin[g - W]; }
        if (xx > 0) { const unsigned c = code[g - 1]; a += ((c >> 2 & 3u) == 2u ? ((c >> 4 & 3u) == 1u ? 1.f : (c >> 4 & 3u) == 2u ? 0.5f : 0.f) : 0.f) * tin[g - 1]; }
        {
          const unsigned c = code[g], which = c >> 4 & 3u;
          const float wv = (c & 3u) == 1u ? (which == 0u ? 1.f : which == 2u ? 0.5f : 0.f) : 0.f;
          const float wh = (c >> 2 & 3u) == 1u ? (which == 1u ? 1.f : which == 2u ? 0.5f : 0.f) : 0.f;
          a += (wv + wh) * tin[g];
        }
        if (xx + 1 < W) { const unsigned c = code[g + 1]; a += ((c >> 2 & 3u) == 0u ? ((c >> 4 & 3u) == 1u ? 1.f : (c >> 4 & 3u) == 2u ? 0.5f : 0.f) : 0.f) * tin[g + 1]; }
        if (yy + 1 < H) { const unsigned c = code[g + W]; a += ((c & 3u) == 0u ? ((c >> 4 & 3u) == 0u ? 1.f : (c >> 4 & 3u) == 2u ? 0.5f : 0.f) : 0.f) * tin[g + W]; }
      }
      if (gdm) {
        for (int dy = -1; dy <= 1; ++dy) {
          const int y2 = yy + dy;
          if (y2 < 0 || y2 >= H) continue;
          for (int dx = -1; dx <= 1; ++dx) {
            const int x2 = xx + dx;
            if (x2 < 0 || x2 >= W) continue;
            const long j = o + (long)y2 * W + x2;
            a -= ((unsigned)codem[j] >> 6 & 15u) == (unsigned)((1 - dy) * 3 + (1 - dx)) ? gdm[j] : 0.f;   // j's maximum is this pixel
          }
        }
      }
      out = a;
      if (dz) {
        float pv, qv;
        cd_sigmoids(z[g], pv, qv);
        out = (a + c2 * sy[g]) * (pv * qv) / images;
      }
    }
    if (dz) dz[g] = out; else tout[g] = out;
  }
}

inline dim3 cd_grid(int64_t P, int images, int& nb) {
  const int64_t nbl = (P + CD_THREADS - 1) / CD_THREADS;
  nb = (int)(nbl > CLDICE_BLOCKS ? CLDICE_BLOCKS : nbl);
  return dim3(nb, images);
}
}  // namespace

int64_t cldice_scratch_floats(int64_t n_total, int max_images, int depth) {
  // per pixel 6 planes (p, S(y), two of x, two of T) and per level d_j and the 16-bit code; the partials, the coefficients
  const int64_t levels = depth + 1;
  return n_total * (6 + levels) + (n_total * levels * 2 + 3) / 4 + (int64_t)max_images * (2 * CD_PARTS * CLDICE_BLOCKS + CD_COEF) + 16;
}

void launch_cldice(const float* logits, const float* gt, float* dlogits, float* loss, float* scratch, int H, int W, int images,
                   int depth, const float* ignore, hipStream_t s) {
  const int64_t P = (int64_t)H * W, n = P * images;
  const int levels = depth + 1;
  const CdScratch S = cd_carve(scratch, images, n, levels);
  int nb;
  const dim3 grid = cd_grid(P, images, nb), block(CD_THREADS);
  hipLaunchKernelGGL(cldice_p_kernel, grid, block, 0, s, logits, gt, S.p, S.ta, (int)P, 1, ignore ? 1 : 0, ignore ? *ignore : 0.f);
  const float *xa = S.p, *ya = S.ta;
  float *xb = S.xa, *yb = S.tb;
  for (int j = 0; j < levels; ++j) {
    hipLaunchKernelGGL(cldice_erode_kernel, grid, block, 0, s, xa, xb, ya, yb, S.code + (int64_t)j * n, H, W);
    hipLaunchKernelGGL(cldice_dilate_kernel, grid, block, 0, s, xa, (const float*)xb, ya, (const float*)yb, S.d + (int64_t)j * n,
                       S.code + (int64_t)j * n, (float*)nullptr, S.sy, H, W, j == 0 ? 1 : 0, j == depth ? 1 : 0);
    float* const nx = j == 0 ? S.xb : (float*)xa;      // p stays; afterwards the two x planes and the two T planes alternate
    float* const ny = (float*)ya;
    xa = xb; ya = yb; xb = nx; yb = ny;
  }
  hipLaunchKernelGGL(cldice_sum_kernel, grid, block, 0, s, (const float*)S.p, gt, (const float*)S.d, (const float*)S.sy, S.partial,
                     (int)P, (long)n, levels);
  hipLaunchKernelGGL(cldice_final_kernel, dim3(1), block, 0, s, (const double*)S.partial, S.coef, loss, images, nb);
  if (!dlogits) return;
  hipLaunchKernelGGL(cldice_gd_kernel, grid, block, 0, s, (const float*)S.p, gt, S.d, (const float*)S.coef, (int)P, (long)n, levels);
  const float* const nof = nullptr;
  const unsigned short* const noc = nullptr;
  float *tin = S.ta, *tout = S.tb;
  hipLaunchKernelGGL(cldice_back_kernel, grid, block, 0, s, nof, tin, nof, (const float*)(S.d + (int64_t)depth * n),
                     (const unsigned short*)S.code, (const unsigned short*)(S.code + (int64_t)depth * n), nof, nof,
                     (const float*)S.coef, (float*)nullptr, H, W, (float)images);
  for (int j = depth; j >= 0; --j) {
    hipLaunchKernelGGL(cldice_back_kernel, grid, block, 0, s, (const float*)tin, tout, (const float*)(S.d + (int64_t)j * n),
                       j ? (const float*)(S.d + (int64_t)(j - 1) * n) : nof, (const unsigned short*)(S.code + (int64_t)j * n),
                       j ? (const unsigned short*)(S.code + (int64_t)(j - 1) * n) : noc, logits, (const float*)S.sy,
                       (const float*)S.coef, j ? (float*)nullptr : dlogits, H, W, (float)images);
    float* const t = tin; tin = tout; tout = t;
  }
}

int64_t cldice_skeleton_scratch_floats(int64_t n_total) { return 2 * n_total; }

void launch_cldice_skeleton(const float* maps, const float* masks, float* out, float* scratch, int H, int W, int images, int depth,
                            const float* ignore, hipStream_t s) {
  const int64_t P = (int64_t)H * W, n = P * images;
  int nb;
  const dim3 grid = cd_grid(P, images, nb), block(CD_THREADS);
  float *xa = scratch, *xb = scratch + n;
  const float* const nof = nullptr;
  hipLaunchKernelGGL(cldice_p_kernel, grid, block, 0, s, maps, masks, xa, (float*)nullptr, (int)P, 0, ignore ? 1 : 0,
                     ignore ? *ignore : 0.f);
  for (int j = 0; j <= depth; ++j) {
    hipLaunchKernelGGL(cldice_erode_kernel, grid, block, 0, s, (const float*)xa, xb, nof, (float*)nullptr, (unsigned short*)nullptr, H, W);
    hipLaunchKernelGGL(cldice_dilate_kernel, grid, block, 0, s, (const float*)xa, (const float*)xb, nof, nof, (float*)nullptr,
                       (unsigned short*)nullptr, out, (float*)nullptr, H, W, j == 0 ? 1 : 0, j == depth ? 1 : 0);
    float* const t = xa; xa = xb; xb = t;
  }
}

}  // namespace eosvos
