// Locally connected dense CRF (mean field on a dilated (2r+1)^2 window; the "ConvCRF" restriction of Kraehenbuehl-Koltun)
// over the per-object probabilities of a frame, for gfx950.  The model is stated in include/eosvos.h (eosvos_crf_labels)
// and restated in torch by eosvos_amd/crf.py (refine_host).
//
//   crf_prepare_kernel   one thread per pixel: clamp, unary U = -log q0, Q^0 = q0; with T = 0 the label decision
//   crf_iter_kernel      one launch per mean-field iteration; the last one also takes the label decision
//
// crf_iter_kernel: a workgroup of 256 threads owns a 32 x 8 pixel tile, one pixel per thread.  It stages the three colour
// planes of the tile with its halo of r*d pixels in LDS once, then the Q planes of LC labels at a time; every thread walks
// the (2r+1)^2 - 1 offsets of its pixel, computes the (label-independent) appearance kernel once per neighbour and applies
// it to the LC labels in registers.  Positions outside the frame are staged as 0 (they add nothing to a message) and are
// left out of the two position-only normalisers, which the same walk accumulates.  A wave covers two rows of 32 consecutive
// pixels, so its ds_read_b32 of one offset hits 32 consecutive banks per half wave: no bank conflict at any row pitch.
// LDS: (3 + LC) * (8 + 2h) * (32 + 2h) floats, h = r*d <= 16: 40 KB at the default r 5, d 2 with LC = 4 (three workgroups per
// CU); LC drops to 3 at h >= 15 to stay under 64 KB.
// More than LC labels: the chunks' logits go to the output planes, the softmax is finished by two more passes of the thread
// over its own pixel (maximum, then sum, then normalise) -- the plain three-step softmax, so the number of chunks does not
// change the arithmetic of a label.  One writer per element, a fixed summation order: two calls give the same bits.
#include "kernels.h"

#include <math.h>

namespace eosvos {
namespace {
constexpr int CRF_TX = 32, CRF_TY = 8;

__device__ __forceinline__ float crf_clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }   // keeps a NaN

// probs [frames][n_obj][n_pix] -> q0 / u [frames][n_obj + 1][n_pix] (either may be null), labels [frames][n_pix] (may be null)
__global__ __launch_bounds__(256) void crf_prepare_kernel(const float* __restrict__ probs, int n_obj, long n_pix, long total,
                                                           float* __restrict__ q0, float* __restrict__ u,
                                                           uint8_t* __restrict__ labels) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const long f = i / n_pix, p = i - f * n_pix;
    const float* pr = probs + f * n_obj * n_pix + p;
    if (labels) {                        // T = 0: merge_labels_kernel's rule on the probabilities as they are
      float best = pr[0];
      int arg = 0;
      for (int o = 1; o < n_obj; ++o) {
        const float v = pr[(long)o * n_pix];
        if (v > best) { best = v; arg = o; }
      }
      labels[i] = best < 0.5f ? 0 : (uint8_t)(arg + 1);
    }
    if (!q0) continue;
    float m = crf_clamp01(pr[0]);
    for (int o = 1; o < n_obj; ++o) {
      const float v = crf_clamp01(pr[(long)o * n_pix]);
      m = (v > m || v != v) ? v : m;
    }
    float s0 = 1.f - m;
    s0 = s0 < 1e-5f ? 1e-5f : s0;
    float sum = s0;
    for (int o = 0; o < n_obj; ++o) {
      const float v = crf_clamp01(pr[(long)o * n_pix]);
      sum += v < 1e-5f ? 1e-5f : v;
    }
    const long base = f * (n_obj + 1) * n_pix + p;
    for (int l = 0; l <= n_obj; ++l) {
      float s = l == 0 ? s0 : crf_clamp01(pr[(long)(l - 1) * n_pix]);
      s = s < 1e-5f ? 1e-5f : s;
      const float q = s / sum;
      q0[base + (long)l * n_pix] = q;
      if (u) u[base + (long)l * n_pix] = -logf(q);
    }
  }
}

template <int LC>
__global__ __launch_bounds__(256) void crf_iter_kernel(const float* __restrict__ img, const float* __restrict__ unary,
                                                        const float* __restrict__ qin, float* __restrict__ qout,
                                                        uint8_t* __restrict__ labels, int n_lab, int H, int W, int r, int d,
                                                        float w_a, float w_s, float inv_2tb2, CrfTables tab) {
  extern __shared__ __align__(16) float crf_lds[];
  const int h = r * d, TW = CRF_TX + 2 * h, TH = CRF_TY + 2 * h, tile = TW * TH;
  float* s_img = crf_lds;                  // [3][TH][TW]
  float* s_q = crf_lds + 3 * tile;         // [LC][TH][TW]
  const long n_pix = (long)H * W;
  const int f = blockIdx.z;
  img += (long)f * 3 * n_pix;
  unary += (long)f * n_lab * n_pix;
  qin += (long)f * n_lab * n_pix;
  qout += (long)f * n_lab * n_pix;
  const int x0 = (int)blockIdx.x * CRF_TX - h, y0 = (int)blockIdx.y * CRF_TY - h;
  const int lx = threadIdx.x & (CRF_TX - 1), ly = threadIdx.x >> 5;
  const int gx = x0 + h + lx, gy = y0 + h + ly;
  const bool live = gx < W && gy < H;
  const long pix = (long)gy * W + gx;
  const int side = 2 * r + 1;

  for (int i = threadIdx.x; i < tile; i += 256) {
    const int ty = i / TW, tx = i - ty * TW;
    const int sy = y0 + ty, sx = x0 + tx;
    const bool in = (unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W;
    const long sp = (long)sy * W + sx;
#pragma unroll
    for (int c = 0; c < 3; ++c) s_img[c * tile + i] = in ? img[c * n_pix + sp] : 0.f;
  }
  const int centre = (ly + h) * TW + lx + h;
  float run_max = -INFINITY;               // more than one chunk: the pixel's largest logit so far
  const int chunks = (n_lab + LC - 1) / LC;
  float logit[LC];
  for (int c0 = 0; c0 < n_lab; c0 += LC) {
    __syncthreads();                       // the image tile is staged / the previous chunk's walk is over
    for (int i = threadIdx.x; i < tile; i += 256) {
      const int ty = i / TW, tx = i - ty * TW;
      const int sy = y0 + ty, sx = x0 + tx;
      const bool in = (unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W;
      const long sp = (long)sy * W + sx;
#pragma unroll
      for (int l = 0; l < LC; ++l) s_q[l * tile + i] = (in && c0 + l < n_lab) ? qin[(long)(c0 + l) * n_pix + sp] : 0.f;
    }
    __syncthreads();
    const float cr = s_img[centre], cg = s_img[tile + centre], cb = s_img[2 * tile + centre];
    float acc_a[LC], acc_s[LC], na = 0.f, ns = 0.f;
#pragma unroll
    for (int l = 0; l < LC; ++l) acc_a[l] = acc_s[l] = 0.f;
    for (int dy = -r; dy <= r; ++dy) {
      const bool iny = (unsigned)(gy + dy * d) < (unsigned)H;
      const int row = centre + dy * d * TW;
      const int k0 = (dy + r) * side + r;
      for (int dx = -r; dx <= r; ++dx) {
        if ((dy | dx) == 0) continue;
        const int o = row + dx * d;
        const float pa = tab.wa[k0 + dx], ps = tab.ws[k0 + dx];
        const bool in = iny && (unsigned)(gx + dx * d) < (unsigned)W;
        na += in ? pa : 0.f;
        ns += in ? ps : 0.f;
        const float er = cr - s_img[o], eg = cg - s_img[tile + o], eb = cb - s_img[2 * tile + o];
        const float ka = pa * expf(-(er * er + eg * eg + eb * eb) * inv_2tb2);
#pragma unroll
        for (int l = 0; l < LC; ++l) {
          const float q = s_q[l * tile + o];
          acc_a[l] += ka * q;
          acc_s[l] += ps * q;
        }
      }
    }
    if (live) {
#pragma unroll
      for (int l = 0; l < LC; ++l) {
        if (c0 + l < n_lab) {
          const float msg = w_a * (na > 0.f ? acc_a[l] / na : 0.f) + w_s * (ns > 0.f ? acc_s[l] / ns : 0.f);
          logit[l] = msg - unary[(long)(c0 + l) * n_pix + pix];
          if (chunks > 1) {
            qout[(long)(c0 + l) * n_pix + pix] = logit[l];
            run_max = (logit[l] > run_max || logit[l] != logit[l]) ? logit[l] : run_max;
          }
        }
      }
    }
  }
  if (!live) return;
  float q_bg = 0.f, best = -INFINITY;
  int arg = 0;
  if (chunks == 1) {
    float mx = logit[0];
#pragma unroll
    for (int l = 1; l < LC; ++l)
      if (l < n_lab) mx = (logit[l] > mx || logit[l] != logit[l]) ? logit[l] : mx;
    float sum = 0.f;
#pragma unroll
    for (int l = 0; l < LC; ++l)
      if (l < n_lab) { logit[l] = expf(logit[l] - mx); sum += logit[l]; }
#pragma unroll
    for (int l = 0; l < LC; ++l)
      if (l < n_lab) {
        const float q = logit[l] / sum;
        qout[(long)l * n_pix + pix] = q;
        if (l == 0) q_bg = q;
        else if (q > best) { best = q; arg = l; }
      }
  } else {                                 // the thread reads back what it wrote itself
    float sum = 0.f;
    for (int l = 0; l < n_lab; ++l) sum += expf(qout[(long)l * n_pix + pix] - run_max);
    for (int l = 0; l < n_lab; ++l) {
      const float q = expf(qout[(long)l * n_pix + pix] - run_max) / sum;
      qout[(long)l * n_pix + pix] = q;
      if (l == 0) q_bg = q;
      else if (q > best) { best = q; arg = l; }
    }
  }
  if (labels) labels[(long)f * n_pix + pix] = q_bg > best ? 0 : (uint8_t)(arg ? arg : 1);
}

inline int crf_label_chunk(int r, int d) {
  const int h = r * d;
  return (size_t)7 * (CRF_TX + 2 * h) * (CRF_TY + 2 * h) * sizeof(float) <= 65536 ? 4 : 3;
}
}  // namespace

void launch_crf_prepare(const float* probs, int n_frames, int n_obj, int64_t n_pix, float* q0, float* u, uint8_t* labels,
                        hipStream_t s) {
  const long total = (long)n_frames * n_pix;
  const long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(crf_prepare_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, probs, n_obj,
                     (long)n_pix, total, q0, u, labels);
}

void launch_crf_iteration(const float* images, const float* unary, const float* q_in, float* q_out, uint8_t* labels,
                          int n_frames, int n_lab, int H, int W, int r, int d, float w_a, float w_s, float theta_beta,
                          const CrfTables& tab, hipStream_t s) {
  const int h = r * d, lc = crf_label_chunk(r, d);
  const size_t lds = (size_t)(3 + lc) * (CRF_TX + 2 * h) * (CRF_TY + 2 * h) * sizeof(float);
  const dim3 grid((W + CRF_TX - 1) / CRF_TX, (H + CRF_TY - 1) / CRF_TY, n_frames);
  const float inv_2tb2 = (float)(1.0 / (2.0 * (double)theta_beta * (double)theta_beta));
  if (lc == 4)
    hipLaunchKernelGGL(crf_iter_kernel<4>, grid, dim3(256), lds, s, images, unary, q_in, q_out, labels, n_lab, H, W, r, d, w_a,
                       w_s, inv_2tb2, tab);
  else
    hipLaunchKernelGGL(crf_iter_kernel<3>, grid, dim3(256), lds, s, images, unary, q_in, q_out, labels, n_lab, H, W, r, d, w_a,
                       w_s, inv_2tb2, tab);
}

void crf_fill_tables(CrfTables& tab, int r, int d, float theta_alpha, float theta_gamma) {
  const int side = 2 * r + 1;
  const double ia = 1.0 / (2.0 * (double)theta_alpha * (double)theta_alpha), ig = 1.0 / (2.0 * (double)theta_gamma * (double)theta_gamma);
  for (int i = 0; i < CRF_MAX_SIDE * CRF_MAX_SIDE; ++i) tab.wa[i] = tab.ws[i] = 0.f;
  for (int dy = -r; dy <= r; ++dy)
    for (int dx = -r; dx <= r; ++dx) {
      const double d2 = (double)(dy * d) * (dy * d) + (double)(dx * d) * (dx * d);
      tab.wa[(dy + r) * side + dx + r] = (float)exp(-d2 * ia);
      tab.ws[(dy + r) * side + dx + r] = (float)exp(-d2 * ig);
    }
}
}  // namespace eosvos
