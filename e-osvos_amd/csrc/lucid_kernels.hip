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
//   lucid_layers_kernel   the same launch shape for the layered samples (eosvos_lucid_compose_layers): up to 8 layers per sample,
//                         each a label of the id map moved by its own matrix, composed back to front; the coordinate, coverage
//                         and bicubic code is the compose kernel's (lucid_coords, lucid_coverage, lucid_cubic).
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

// rule 6: the source coordinates of output pixel (y, xm) under the inverse matrix m, 5 fractional bits
__device__ __forceinline__ void lucid_coords(const double* m, int y, int xm, int& X, int& Y) {
  const int rd = 16;                                      // the interpolating round_delta of warp_affine_kernel
  X = (warp_fix(m[1], y, m[2], rd) + warp_fix(m[0], xm)) >> 5;
  Y = (warp_fix(m[4], y, m[5], rd) + warp_fix(m[3], xm)) >> 5;
}

// rule 7: the coverage in 1/1024 of the 2 x 2 bilinear taps at (oy + i, ox + j) with the fractions (fy, fx) in 1/32; on(index)
// is the tap predicate, asked only inside the frame
template <class On>
__device__ __forceinline__ int lucid_coverage(int H, int W, int oy, int ox, int fy, int fx, On on) {
  int A = 0;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int yy = oy + i, xx = ox + j;
      const bool hit = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W && on((long)yy * W + xx);
      A += hit ? (i ? fy : 32 - fy) * (j ? fx : 32 - fx) : 0;
    }
  }
  return A;
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
    int Xo, Yo, Xb, Yb;
    lucid_coords(p.oi, y, xm, Xo, Yo);
    lucid_coords(p.bi, y, xm, Xb, Yb);
    const int ox = Xo >> 5, oy = Yo >> 5, fx = Xo & 31, fy = Yo & 31;
    const int A = lucid_coverage(H, W, oy, ox, fy, fx, [&](long at) { return mask[at] != 0.f; });   // coverage in 1/1024
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

// The layered samples (rules L2-L5 of include/eosvos.h): per sample the inverse background matrix and up to LUCID_MAX_LAYERS
// inverse layer matrices, back to front, each with the id its layer carries in `ids`.
struct LucidLayerSample { double bi[6], oi[LUCID_MAX_LAYERS][6]; int flip, n_layers; uint8_t id[LUCID_MAX_LAYERS]; };
struct LucidLayerParams { LucidLayerSample s[LUCID_LAYERS_MAX_SAMPLES]; };
// HIP passes at most 4 KB of kernel arguments; the pointers and sizes beside the samples take 88 bytes
static_assert(sizeof(LucidLayerParams) + 128 <= 4096, "LucidLayerParams must fit the kernel-argument segment: lower LUCID_LAYERS_MAX_SAMPLES");

// layer k's coverage at output pixel (y, xm), with its coordinates
__device__ __forceinline__ int lucid_layer_coverage(const LucidLayerSample& p, int k, const uint8_t* __restrict__ ids, int H, int W,
                                                    int y, int xm, int& Xo, int& Yo) {
  lucid_coords(p.oi[k], y, xm, Xo, Yo);
  const int id = p.id[k];
  return lucid_coverage(H, W, Yo >> 5, Xo >> 5, Yo & 31, Xo & 31, [&](long at) { return ids[at] == id; });
}

// grid (ceil(W / 256), H, samples), block 256.  No thread leaves before the wave sums.  Two walks over the sample's layers, both
// uniform in k (the matrices are scalar loads): the first takes the coverages alone -- the visible layer, the front-most opaque
// one and which layers touch the pixel at all --, the second samples the frame for the touching layers from the opaque one
// upwards, four channels at a time.  What lies under an opaque layer is overwritten by rule L4 and never computed.
__global__ __launch_bounds__(256) void lucid_layers_kernel(const float* __restrict__ frame, const uint8_t* __restrict__ ids,
                                                            const float* __restrict__ plate, int C, int H, int W,
                                                            const LucidLayerParams prm, int target_id,
                                                            const float* __restrict__ ctab, float* __restrict__ images,
                                                            float* __restrict__ labels, uint8_t* __restrict__ ids_out,
                                                            int* __restrict__ counts) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, s = blockIdx.z;
  const LucidLayerSample& p = prm.s[s];
  const int L = p.n_layers;
  int top = -1;                                           // the visible layer: the largest k with A_k >= 512
  if (x < W) {
    const long hw = (long)H * W, o = (long)y * W + x;
    const int xm = p.flip ? W - 1 - x : x;
    int opaque = -1;                                      // the largest k with A_k == 1024
    unsigned touch = 0;                                   // bit k: A_k > 0
    for (int k = 0; k < L; ++k) {
      int Xo, Yo;
      const int A = lucid_layer_coverage(p, k, ids, H, W, y, xm, Xo, Yo);
      top = A >= 512 ? k : top;
      opaque = A == 1024 ? k : opaque;
      touch |= (A > 0 ? 1u : 0u) << k;
    }
    const int id_top = top >= 0 ? p.id[top] : 0;
    labels[(long)s * hw + o] = id_top == target_id ? 1.f : 0.f;
    if (ids_out) ids_out[(long)s * hw + o] = (uint8_t)id_top;
    int Xb, Yb;
    lucid_coords(p.bi, y, xm, Xb, Yb);
    const float* bcx = ctab + (Xb & 31) * 4;
    const float* bcy = ctab + (Yb & 31) * 4;
    for (int c0 = 0; c0 < C; c0 += 4) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[j] = opaque < 0 && c0 + j < C ? lucid_cubic(plate + (c0 + j) * hw, H, W, (Yb >> 5) - 1, (Xb >> 5) - 1, bcy, bcx) : 0.f;
      for (int k = max(opaque, 0); k < L; ++k) {
        if (!((touch >> k) & 1)) continue;
        int Xo, Yo;
        const int A = lucid_layer_coverage(p, k, ids, H, W, y, xm, Xo, Yo);
        const float alpha = (float)A * (1.f / 1024.f);    // exact
        const float* ocx = ctab + (Xo & 31) * 4;
        const float* ocy = ctab + (Yo & 31) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (c0 + j < C) {
            const float ob = lucid_cubic(frame + (c0 + j) * hw, H, W, (Yo >> 5) - 1, (Xo >> 5) - 1, ocy, ocx);
            v[j] = A == 1024 ? ob : v[j] + alpha * (ob - v[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < C) images[((long)s * C + c0 + j) * hw + o] = v[j];
    }
  }
  for (int k = 0; k < L; ++k) {                           // one wave sum and at most one integer atomic per layer
    const int n = wave_sum_i(top == k);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(counts + s * LUCID_MAX_LAYERS + k, n);
  }
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
void launch_lucid_layers(const float* frame, const uint8_t* ids, const float* plate, int C, int H, int W, int n_samples,
                         const int* flips, const int* n_layers, const uint8_t* layer_ids, const double* matrices, int target_id,
                         const float* ctab, float* images, float* labels, uint8_t* ids_out, int* counts, hipStream_t s) {
  LucidLayerParams prm = {};
  for (int i = 0; i < n_samples; ++i) {
    LucidLayerSample& p = prm.s[i];
    const double* m = matrices + (size_t)i * (1 + LUCID_MAX_LAYERS) * 6;
    for (int j = 0; j < 6; ++j) p.bi[j] = m[j];
    for (int k = 0; k < n_layers[i]; ++k) {
      for (int j = 0; j < 6; ++j) p.oi[k][j] = m[(1 + k) * 6 + j];
      p.id[k] = layer_ids[i * LUCID_MAX_LAYERS + k];
    }
    p.flip = flips[i] != 0;
    p.n_layers = n_layers[i];
  }
  hipLaunchKernelGGL(lucid_layers_kernel, dim3((W + 255) / 256, H, n_samples), dim3(256), 0, s, frame, ids, plate, C, H, W, prm,
                     target_id, ctab, images, labels, ids_out, counts);
}
}  // namespace eosvos
