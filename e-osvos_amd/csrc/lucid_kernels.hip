// Lucid first-frame synthesis for the one-shot fine-tune, for gfx950: the background plate of the annotated frame (the
// object cut out and the hole filled from a push-pull pyramid) and the composition of a batch's synthesised samples (plate
// and object moved independently and put together again).  The rules are stated in include/eosvos.h (eosvos_lucid_plate,
// eosvos_lucid_compose) and restated in numpy by eosvos_amd/lucid.py (plate_host, compose_host).
//
//   lucid_rowhit_kernel   one thread per pixel: is a mask pixel within `dilate` columns in this row?  (The Chebyshev ball is a
//                         square, so the hole is a row pass followed by a column pass.)
//   lucid_level0_kernel   the column pass over the row hits: known = !hole; plate = known ? frame : 0, k0 = known.
//   lucid_push_kernel     level l -> l + 1: one thread per parent, k = OR of the children inside the level, v = the sum of the
//                         known children in the order (0,0) (0,1) (1,0) (1,1) divided by their number.
//   lucid_pull_kernel     level l + 1 -> l: one thread per pixel of level l, unknown pixels only, the 1/4 - 3/4 bilinear sample
//                         of the completed level above with clamped taps.  It reads level l + 1 and writes level l: no launch
//                         reads what it writes.
//   lucid_compose_kernel  one thread per output pixel, rows of 256, the sample in the grid's third dimension.  The samples'
//                         matrices travel by value (LucidParams), so a queued launch owns everything it reads.
// Every level is written in full by every call (level 0 and the pushes write each element, the pulls only overwrite), so the
// result does not depend on what the scratch held.  fp32 with every operation rounded on its own (no contraction), in the
// order of the numpy twin; no float atomics; the count is an integer sum.  One writer per element, no cooperative launch, no
// workgroup waits for another.  Vector stores only.
#include "kernels.h"

// Every fp32 operation below is rounded on its own, in the order of the numpy twin: no multiply-add is fused.  The pragma
// governs the expressions written in this file, which is why they are plain operators and not the __fmul_rn family
// (inline functions of a header compiled under the default, which the compiler still fuses after inlining).
#pragma clang fp contract(off)

namespace eosvos {
namespace {
// grid (ceil(W / 256), H), block 256
__global__ __launch_bounds__(256) void lucid_rowhit_kernel(const float* __restrict__ mask, int H, int W, int d,
                                                            uint8_t* __restrict__ hit) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const float* r = mask + (long)y * W;
  const int lo = max(x - d, 0), hi = min(x + d, W - 1);
  int h = 0;
  for (int i = lo; i <= hi; ++i) h |= r[i] != 0.f;
  hit[(long)y * W + x] = (uint8_t)h;
}

__global__ __launch_bounds__(256) void lucid_level0_kernel(const float* __restrict__ frame, const uint8_t* __restrict__ hit, int C,
                                                            int H, int W, int d, float* __restrict__ plate,
                                                            uint8_t* __restrict__ k0) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const int lo = max(y - d, 0), hi = min(y + d, H - 1);
  int h = 0;
  for (int i = lo; i <= hi; ++i) h |= hit[(long)i * W + x];
  const long hw = (long)H * W, o = (long)y * W + x;
  k0[o] = h ? 0 : 1;
  for (int c = 0; c < C; ++c) plate[c * hw + o] = h ? 0.f : frame[c * hw + o];
}

// grid (ceil(Wn / 256), Hn): level (Hl, Wl) -> its parent (Hn, Wn) = (ceil(Hl / 2), ceil(Wl / 2))
__global__ __launch_bounds__(256) void lucid_push_kernel(const float* __restrict__ v, const uint8_t* __restrict__ k, int C, int Hl,
                                                          int Wl, float* __restrict__ vn, uint8_t* __restrict__ kn, int Hn, int Wn) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= Wn) return;
  bool kk[4];
  long at[4];
  int n = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int yy = 2 * y + (t >> 1), xx = 2 * x + (t & 1);
    const bool in = yy < Hl && xx < Wl;
    at[t] = in ? (long)yy * Wl + xx : 0;
    kk[t] = in && k[at[t]] != 0;
    n += kk[t];
  }
  const long pl = (long)Hl * Wl, pn = (long)Hn * Wn, o = (long)y * Wn + x;
  kn[o] = n ? 1 : 0;
  for (int c = 0; c < C; ++c) {
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (kk[t]) sum = sum + v[c * pl + at[t]];
    vn[c * pn + o] = n ? __fdiv_rn(sum, (float)n) : 0.f;
  }
}

// grid (ceil(Wl / 256), Hl): the unknown pixels of level (Hl, Wl) from the completed level (Hn, Wn) above
__global__ __launch_bounds__(256) void lucid_pull_kernel(float* __restrict__ v, const uint8_t* __restrict__ k, int C, int Hl, int Wl,
                                                          const float* __restrict__ vn, int Hn, int Wn) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= Wl) return;
  const long o = (long)y * Wl + x;
  if (k[o]) return;
  // (y + 0.5) / 2 - 0.5 = y / 2 - 0.25: floor (y - 1) >> 1, fraction 3/4 for even y and 1/4 for odd y
  const int ya = (y - 1) >> 1, xa = (x - 1) >> 1;
  const float ly = (y & 1) ? 0.25f : 0.75f, lx = (x & 1) ? 0.25f : 0.75f, hy = 1.f - ly, hx = 1.f - lx;
  const int y0 = min(max(ya, 0), Hn - 1), y1 = min(max(ya + 1, 0), Hn - 1);
  const int x0 = min(max(xa, 0), Wn - 1), x1 = min(max(xa + 1, 0), Wn - 1);
  const long pl = (long)Hl * Wl, pn = (long)Hn * Wn;
  // (not vectorised over the channels: that pairs separately loaded taps into v_pk_mul_f32 / v_pk_add_f32 operands, the form
  // the Makefile's -fno-slp-vectorize keeps out of this library)
#pragma clang loop vectorize(disable) interleave(disable)
  for (int c = 0; c < C; ++c) {
    const float* s = vn + c * pn;
    const float top = hx * s[(long)y0 * Wn + x0] + lx * s[(long)y0 * Wn + x1];
    const float bot = hx * s[(long)y1 * Wn + x0] + lx * s[(long)y1 * Wn + x1];
    v[c * pl + o] = hy * top + ly * bot;
  }
}

struct LucidSample { double bi[6], oi[6]; int flip, pad; };
struct LucidParams { LucidSample s[LUCID_MAX_SAMPLES]; };

// the bicubic sample with its 4 x 4 taps at (sy .. sy + 3, sx .. sx + 3): taps outside the plane are 0, tap-by-tap
// accumulation, weights cy[i] * cx[j] in float as the warp kernel's
__device__ __forceinline__ float lucid_cubic(const float* __restrict__ S, int H, int W, int sy, int sx, const float* __restrict__ cy,
                                             const float* __restrict__ cx) {
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int yy = sy + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xx = sx + j;
      const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
      const float t = in ? S[(long)yy * W + xx] * (cy[i] * cx[j]) : 0.f;
      sum = sum + t;
    }
  }
  return sum;
}

// grid (ceil(W / 256), H, samples), block 256.  No thread leaves before the wave sum.
__global__ __launch_bounds__(256) void lucid_compose_kernel(const float* __restrict__ frame, const float* __restrict__ mask,
                                                             const float* __restrict__ plate, int C, int H, int W,
                                                             const LucidParams prm, const float* __restrict__ ctab,
                                                             float* __restrict__ images, float* __restrict__ labels,
                                                             int* __restrict__ counts) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, s = blockIdx.z;
  int lab = 0;
  if (x < W) {
    const LucidSample& p = prm.s[s];
    const long hw = (long)H * W, o = (long)y * W + x;
    const int xm = p.flip ? W - 1 - x : x;
    const int rd = 16;                                    // the interpolating round_delta of warp_affine_kernel
    const int Xo = (warp_fix(p.oi[1], y, p.oi[2], rd) + warp_fix(p.oi[0], xm)) >> 5;
    const int Yo = (warp_fix(p.oi[4], y, p.oi[5], rd) + warp_fix(p.oi[3], xm)) >> 5;
    const int Xb = (warp_fix(p.bi[1], y, p.bi[2], rd) + warp_fix(p.bi[0], xm)) >> 5;
    const int Yb = (warp_fix(p.bi[4], y, p.bi[5], rd) + warp_fix(p.bi[3], xm)) >> 5;
    const int ox = Xo >> 5, oy = Yo >> 5, fx = Xo & 31, fy = Yo & 31;
    int A = 0;                                            // coverage in 1/1024
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int yy = oy + i, xx = ox + j;
        const bool on = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W && mask[(long)yy * W + xx] != 0.f;
        A += on ? (i ? fy : 32 - fy) * (j ? fx : 32 - fx) : 0;
      }
    }
    lab = A >= 512;
    labels[(long)s * hw + o] = lab ? 1.f : 0.f;
    const float alpha = (float)A * (1.f / 1024.f);        // exact
    const float* bcx = ctab + (Xb & 31) * 4;
    const float* bcy = ctab + (Yb & 31) * 4;
    const float* ocx = ctab + fx * 4;
    const float* ocy = ctab + fy * 4;
    for (int c = 0; c < C; ++c) {
      float v = A == 1024 ? 0.f : lucid_cubic(plate + c * hw, H, W, (Yb >> 5) - 1, (Xb >> 5) - 1, bcy, bcx);
      if (A > 0) {
        const float ob = lucid_cubic(frame + c * hw, H, W, oy - 1, ox - 1, ocy, ocx);
        v = A == 1024 ? ob : v + alpha * (ob - v);
      }
      images[((long)s * C + c) * hw + o] = v;
    }
  }
  lab = wave_sum_i(lab);
  if ((threadIdx.x & 63) == 0 && lab) atomicAdd(counts + s, lab);
}
}  // namespace

// levels from H x W down to 1 x 1: at most 13 for sides <= 4096
static int lucid_levels(int H, int W) {
  int n = 1;
  while (H > 1 || W > 1) { H = (H + 1) / 2; W = (W + 1) / 2; ++n; }
  return n;
}

void lucid_scratch(int C, int H, int W, size_t* floats, size_t* bytes) {
  size_t px = 0;
  for (int h = H, w = W; h > 1 || w > 1;) { h = (h + 1) / 2; w = (w + 1) / 2; px += (size_t)h * w; }
  *floats = (size_t)C * px;
  *bytes = 2 * (size_t)H * W + px;
}

void launch_lucid_plate(const float* frame, const float* mask, int C, int H, int W, int dilate, float* plate, float* vbuf,
                        uint8_t* kbuf, hipStream_t s) {
  uint8_t* hit = kbuf;                                    // [H][W] row hits, then k of level 0, then k of the levels above
  uint8_t* k0 = kbuf + (size_t)H * W;
  hipLaunchKernelGGL(lucid_rowhit_kernel, dim3((W + 255) / 256, H), dim3(256), 0, s, mask, H, W, dilate, hit);
  hipLaunchKernelGGL(lucid_level0_kernel, dim3((W + 255) / 256, H), dim3(256), 0, s, frame, hit, C, H, W, dilate, plate, k0);
  const int n = lucid_levels(H, W);
  float* v[16];
  uint8_t* k[16];
  int hs[16], ws[16];
  v[0] = plate; k[0] = k0; hs[0] = H; ws[0] = W;
  float* vp = vbuf;
  uint8_t* kp = k0 + (size_t)H * W;
  for (int l = 1; l < n; ++l) {
    hs[l] = (hs[l - 1] + 1) / 2; ws[l] = (ws[l - 1] + 1) / 2;
    v[l] = vp; k[l] = kp;
    vp += (size_t)C * hs[l] * ws[l];
    kp += (size_t)hs[l] * ws[l];
    hipLaunchKernelGGL(lucid_push_kernel, dim3((ws[l] + 255) / 256, hs[l]), dim3(256), 0, s, v[l - 1], k[l - 1], C, hs[l - 1],
                       ws[l - 1], v[l], k[l], hs[l], ws[l]);
  }
  for (int l = n - 2; l >= 0; --l)
    hipLaunchKernelGGL(lucid_pull_kernel, dim3((ws[l] + 255) / 256, hs[l]), dim3(256), 0, s, v[l], k[l], C, hs[l], ws[l], v[l + 1],
                       hs[l + 1], ws[l + 1]);
}

void launch_lucid_compose(const float* frame, const float* mask, const float* plate, int C, int H, int W, int n_samples,
                          const int* flips, const double* matrices, const float* ctab, float* images, float* labels, int* counts,
                          hipStream_t s) {
  LucidParams prm = {};
  for (int i = 0; i < n_samples; ++i) {
    for (int j = 0; j < 6; ++j) {
      prm.s[i].bi[j] = matrices[i * 12 + j];
      prm.s[i].oi[j] = matrices[i * 12 + 6 + j];
    }
    prm.s[i].flip = flips[i] != 0;
  }
  hipLaunchKernelGGL(lucid_compose_kernel, dim3((W + 255) / 256, H, n_samples), dim3(256), 0, s, frame, mask, plate, C, H, W, prm, ctab,
                     images, labels, counts);
}
}  // namespace eosvos
