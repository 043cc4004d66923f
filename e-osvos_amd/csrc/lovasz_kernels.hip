// Lovasz hinge (Jaccard hinge) loss + gradient for gfx950 -- networks/loss_lovasz.py:78-111.
//
// For one set of pixels:  g = (t >= .5), s = 2g - 1, e = 1 - x*s;  rank the errors in descending order (ties by ascending
// pixel index, the order of a stable sort);  with G = sum g and c1_k / c0_k the inclusive counts of g = 1 / g = 0 among
// ranks 0..k:  I_k = G - c1_k,  U_k = G + c0_k,  w_k = J_k - J_{k-1} with J_k = 1 - I_k / U_k;  loss = sum_k max(e_k, 0) w_k,
// dL/dx_i = -s_i w_rank(i) where e_i > 0.  The increments are formed from the integer counts without cancellation:
//   g_k = 1:  w_k = 1 / U_k          g_k = 0:  w_k = I_k / (U_{k-1} U_k) = I_k / ((U_k - 1) U_k)          w_0 = 1 / U_0
//
// Pipeline (one stream, no host round trip, no workgroup waits for another: every dependency is a kernel boundary):
//   prep      e per pixel; per-tile counts of e > 0, of g, and a non-finite flag; dlogits <- 0
//             (with a void label, `ignore=` of loss_lovasz.py:114-126: a pixel with t == ignore is dropped here and in compact,
//             so the segment sizes below count valid pixels only; size 0 is legal and gives loss 0)
//   compact   the pixels with e > 0 only, in index order, as (key = ~bits(e), value = index << 1 | g).  Pixels with e <= 0
//             rank last and change no higher rank's counts, so they never enter the sort.
//   4 x (hist, scan, scatter)   stable LSD radix sort, 8-bit digits, segmented by image.  The rank of an element within its
//             digit is computed (wave ballots, per-wave LDS counters, prefix over waves and tiles), never raced for.
//   bits      per-tile count of g = 1 in sorted order
//   weights   inclusive scan of the label bits -> c1, c0 -> w_k; gradient scattered to dlogits[index]; loss partials
//   final     partials summed in a fixed order (fp64), mean over the images
// Every count is an integer (< 2^31 elements per call); the weights and the loss terms are formed in fp64 and rounded once.
#include "kernels.h"

namespace eosvos {
namespace {

constexpr int LV_THREADS = 256;
constexpr int LV_ITEMS = 8;                      // 64-element rows per wave
constexpr int LV_WSPAN = 64 * LV_ITEMS;          // contiguous elements owned by one wave
constexpr int LV_TILE = 4 * LV_WSPAN;            // elements per workgroup
constexpr int LV_SCAN_THREADS = 1024;

// per-tile words {e > 0 count, g count, non-finite flag, g = 1 count in sorted order}; per-segment words {M, G, non-finite, -}
constexpr int LV_TINFO = 4, LV_SINFO = 4;

struct LvScratch {
  unsigned *key[2], *val[2];
  int *hist, *tinfo, *sinfo;
  double* partial;
};
inline int64_t lv_tiles(int64_t seg_len) { return (seg_len + LV_TILE - 1) / LV_TILE; }
inline LvScratch lv_carve(float* scratch, int64_t n_total, int64_t tiles, int segs) {
  LvScratch L;
  unsigned* p = (unsigned*)scratch;
  const int64_t n2 = (n_total + 1) / 2 * 2;      // keep the fp64 partials 8-byte aligned
  L.key[0] = p; p += n2;
  L.val[0] = p; p += n2;
  L.key[1] = p; p += n2;
  L.val[1] = p; p += n2;
  L.partial = (double*)p; p += 2 * tiles;
  L.hist = (int*)p; p += 256 * tiles;
  L.tinfo = (int*)p; p += LV_TINFO * tiles;
  L.sinfo = (int*)p;
  return L;
}

__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }
// fp64 sum over the 256 threads in a fixed order, valid in every thread
__device__ __forceinline__ double block_sum_d(double v, double* sh /*4*/) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ __forceinline__ float lv_error(float x, float t, int& g) {
  g = t >= 0.5f ? 1 : 0;
  return 1.0f - (g ? x : -x);                   // x * (+-1) is exact: one rounding, as torch's fp32 evaluation
}
// lanes of the wave that are `valid` and hold the same 8-bit digit as this lane
__device__ __forceinline__ unsigned long long digit_peers(unsigned digit, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const unsigned long long v = __ballot((digit >> b) & 1u);
    m &= ((digit >> b) & 1u) ? v : ~v;
  }
  return m;
}

// element i of the segment handled by (wave, row j, lane) of tile `tile`: waves own contiguous spans, so index order is
// (wave, row, lane) order
__device__ __forceinline__ long lv_elem(int tile, int j) {
  return (long)tile * LV_TILE + (threadIdx.x >> 6) * LV_WSPAN + j * 64 + (threadIdx.x & 63);
}

// VOID: a pixel with t == ign is dropped here and in the compaction (flatten_binary_scores, loss_lovasz.py:114-126): it counts
// neither as e > 0 nor as foreground, its logit may be non-finite, and dlogits stays the +0 written below.  VOID = false never
// reads `ign`.
template <bool VOID>
__global__ __launch_bounds__(LV_THREADS) void lovasz_prep_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                 float* __restrict__ dx, int* __restrict__ tinfo, long seg_len,
                                                                 int tps, float ign) {
  __shared__ int sh[4];
  const int seg = blockIdx.x / tps, tile = blockIdx.x % tps;
  const long seg0 = (long)seg * seg_len;
  int m = 0, G = 0, nf = 0;
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const long i = lv_elem(tile, j);
    if (i < seg_len) {
      const float xv = x[seg0 + i], tv = t[seg0 + i];
      int g;
      const float e = lv_error(xv, tv, g);
      dx[seg0 + i] = 0.f;
      if (VOID && tv == ign) continue;
      m += e > 0.f ? 1 : 0;
      G += g;
      nf |= (__float_as_uint(xv) & 0x7f800000u) == 0x7f800000u ? 1 : 0;
    }
  }
  m = block_sum_i(m, sh);
  G = block_sum_i(G, sh);
  nf = block_sum_i(nf, sh);
  if (threadIdx.x == 0) {
    int* ti = tinfo + (long)blockIdx.x * LV_TINFO;
    ti[0] = m; ti[1] = G; ti[2] = nf ? 1 : 0; ti[3] = 0;
  }
}

// VOID: as in prep, a pixel with t == ign is left out of the compaction.
template <bool VOID>
__global__ __launch_bounds__(LV_THREADS) void lovasz_compact_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                    const int* __restrict__ tinfo, int* __restrict__ sinfo,
                                                                    unsigned* __restrict__ keys, unsigned* __restrict__ vals,
                                                                    long seg_len, int tps, float ign) {
  __shared__ int sh[4];
  __shared__ int wtot[4];
  const int seg = blockIdx.x / tps, tile = blockIdx.x % tps;
  const int w = threadIdx.x >> 6;
  const long seg0 = (long)seg * seg_len;
  // this tile's first output slot = e > 0 count of the segment's earlier tiles; tile 0 also publishes the segment totals
  int pre = 0, M = 0, G = 0, nf = 0;
  for (int tt = threadIdx.x; tt < tps; tt += LV_THREADS) {
    const int* ti = tinfo + ((long)seg * tps + tt) * LV_TINFO;
    const int m = ti[0];
    M += m;
    pre += tt < tile ? m : 0;
    G += ti[1];
    nf += ti[2];
  }
  pre = block_sum_i(pre, sh);
  if (tile == 0) {
    M = block_sum_i(M, sh);
    G = block_sum_i(G, sh);
    nf = block_sum_i(nf, sh);
    if (threadIdx.x == 0) {
      int* si = sinfo + seg * LV_SINFO;
      si[0] = M; si[1] = G; si[2] = nf ? 1 : 0; si[3] = 0;
    }
  }
  float e[LV_ITEMS];
  int g[LV_ITEMS];
  unsigned long long bal[LV_ITEMS];
  int total = 0;
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const long i = lv_elem(tile, j);
    e[j] = 0.f; g[j] = 0;
    if (i < seg_len) {
      const float tv = t[seg0 + i];
      e[j] = lv_error(x[seg0 + i], tv, g[j]);
      if (VOID && tv == ign) e[j] = 0.f;           // a select: ranks with the e <= 0 pixels, i.e. never enters the sort
    }
    bal[j] = __ballot(e[j] > 0.f);               // (a NaN error compares false: it ranks with the e <= 0 pixels)
    total += __popcll(bal[j]);
  }
  if ((threadIdx.x & 63) == 0) wtot[w] = total;
  __syncthreads();
  long run = pre;
  for (int ww = 0; ww < w; ++ww) run += wtot[ww];
  const unsigned long long below = lanes_below();
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const long dst = run + __popcll(bal[j] & below);
    if (e[j] > 0.f && dst < seg_len) {
      keys[seg0 + dst] = ~__float_as_uint(e[j]);  // unsigned ascending on the key = error descending
      vals[seg0 + dst] = ((unsigned)(seg0 + lv_elem(tile, j)) << 1) | (unsigned)g[j];
    }
    run += __popcll(bal[j]);
  }
}

__global__ __launch_bounds__(LV_THREADS) void lovasz_hist_kernel(const unsigned* __restrict__ keys, const int* __restrict__ sinfo,
                                                                 int* __restrict__ hist, long seg_len, int tps, int shift) {
  __shared__ int h[4][256];
  const int seg = blockIdx.x / tps, tile = blockIdx.x % tps;
  const long M = sinfo[seg * LV_SINFO];
  if ((long)tile * LV_TILE >= M) return;
  const int w = threadIdx.x >> 6;
  const long seg0 = (long)seg * seg_len;
#pragma unroll
  for (int q = 0; q < 4; ++q) h[q][threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long below = lanes_below();
  unsigned key[LV_ITEMS];
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) key[j] = lv_elem(tile, j) < M ? keys[seg0 + lv_elem(tile, j)] : 0xffffffffu;
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const bool valid = lv_elem(tile, j) < M;
    const unsigned d = (key[j] >> shift) & 255u;
    const unsigned long long peers = digit_peers(d, valid);
    if (valid && (peers & below) == 0) atomicAdd(&h[w][d], __popcll(peers));     // one lane per digit, a counter row per wave
  }
  __syncthreads();
  hist[(long)blockIdx.x * 256 + threadIdx.x] = (h[0][threadIdx.x] + h[1][threadIdx.x]) + (h[2][threadIdx.x] + h[3][threadIdx.x]);
}

// hist[tile][digit] -> first output slot of (digit, tile) within the segment: digit-major, tile-minor exclusive scan
__global__ __launch_bounds__(LV_SCAN_THREADS) void lovasz_scan_kernel(int* __restrict__ hist, const int* __restrict__ sinfo,
                                                                      int tps) {
  __shared__ int part[4][256];
  __shared__ int wsum[4];
  const int seg = blockIdx.x;
  const long M = sinfo[seg * LV_SINFO];
  const int nt = (int)((M + LV_TILE - 1) / LV_TILE);
  if (nt == 0) return;
  const int d = threadIdx.x & 255, grp = threadIdx.x >> 8;
  const int per = (nt + 3) / 4;
  const int a = min(nt, grp * per), b = min(nt, a + per);
  int* h = hist + (long)seg * tps * 256;
  int sum = 0;
  for (int t = a; t < b; ++t) sum += h[(long)t * 256 + d];
  part[grp][d] = sum;
  __syncthreads();
  const int tot = (part[0][d] + part[1][d]) + (part[2][d] + part[3][d]);
  int incl = tot;                                 // inclusive scan over the 64 digits of this wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if ((threadIdx.x & 63) >= o) incl += up;
  }
  if (grp == 0 && (threadIdx.x & 63) == 63) wsum[d >> 6] = incl;
  __syncthreads();
  int run = incl - tot;
  for (int ww = 0; ww < (d >> 6); ++ww) run += wsum[ww];
  for (int gg = 0; gg < grp; ++gg) run += part[gg][d];
  for (int t = a; t < b; ++t) {
    const int v = h[(long)t * 256 + d];
    h[(long)t * 256 + d] = run;
    run += v;
  }
}

__global__ __launch_bounds__(LV_THREADS) void lovasz_scatter_kernel(const unsigned* __restrict__ kin, const unsigned* __restrict__ vin,
                                                                    unsigned* __restrict__ kout, unsigned* __restrict__ vout,
                                                                    const int* __restrict__ sinfo, const int* __restrict__ offs,
                                                                    long seg_len, int tps, int shift) {
  __shared__ int wc[4][256];
  const int seg = blockIdx.x / tps, tile = blockIdx.x % tps;
  const long M = sinfo[seg * LV_SINFO];
  if ((long)tile * LV_TILE >= M) return;
  const int w = threadIdx.x >> 6;
  const long seg0 = (long)seg * seg_len;
#pragma unroll
  for (int q = 0; q < 4; ++q) wc[q][threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long below = lanes_below();
  unsigned key[LV_ITEMS];
  int pos[LV_ITEMS];
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) key[j] = lv_elem(tile, j) < M ? kin[seg0 + lv_elem(tile, j)] : 0xffffffffu;
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const bool valid = lv_elem(tile, j) < M;
    const unsigned d = (key[j] >> shift) & 255u;
    const unsigned long long peers = digit_peers(d, valid);
    // the first peer advances this wave's running count of the digit (only this wave touches the row) and hands the
    // count of the rows before this one to the others
    int prior = 0;
    if (valid && (peers & below) == 0) prior = atomicAdd(&wc[w][d], __popcll(peers));
    prior = __shfl(prior, (__ffsll((long long)peers) - 1) & 63, 64);
    pos[j] = prior + __popcll(peers & below);
  }
  __syncthreads();
  {   // counts -> first slot of (digit, wave): the tile's scanned offset, then the waves in order
    const int d = threadIdx.x;
    int run = offs[(long)blockIdx.x * 256 + d];
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const int c = wc[ww][d];
      wc[ww][d] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const long i = lv_elem(tile, j);
    if (i < M) {
      const long dst = (long)wc[w][(key[j] >> shift) & 255u] + pos[j];
      if (dst >= 0 && dst < M) {
        kout[seg0 + dst] = key[j];
        vout[seg0 + dst] = vin[seg0 + i];
      }
    }
  }
}

__global__ __launch_bounds__(LV_THREADS) void lovasz_bits_kernel(const unsigned* __restrict__ vals, const int* __restrict__ sinfo,
                                                                 int* __restrict__ tinfo, long seg_len, int tps) {
  __shared__ int sh[4];
  const int seg = blockIdx.x / tps, tile = blockIdx.x % tps;
  const long M = sinfo[seg * LV_SINFO];
  if ((long)tile * LV_TILE >= M) return;
  const long seg0 = (long)seg * seg_len;
  int c = 0;
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const long i = lv_elem(tile, j);
    if (i < M) c += (int)(vals[seg0 + i] & 1u);
  }
  c = block_sum_i(c, sh);
  if (threadIdx.x == 0) tinfo[(long)blockIdx.x * LV_TINFO + 3] = c;
}

__global__ __launch_bounds__(LV_THREADS) void lovasz_weights_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals,
                                                                    const int* __restrict__ sinfo, const int* __restrict__ tinfo,
                                                                    float* __restrict__ dx, double* __restrict__ partial,
                                                                    long seg_len, int tps, long n_total, double scale) {
  __shared__ int sh[4];
  __shared__ int wtot[4];
  __shared__ double shd[4];
  const int seg = blockIdx.x / tps, tile = blockIdx.x % tps;
  const long M = sinfo[seg * LV_SINFO];
  if ((long)tile * LV_TILE >= M) return;
  const long G = sinfo[seg * LV_SINFO + 1];
  const int w = threadIdx.x >> 6;
  const long seg0 = (long)seg * seg_len;
  int c1base = 0;                                // g = 1 among the ranks before this tile
  for (int tt = threadIdx.x; tt < tile; tt += LV_THREADS) c1base += tinfo[((long)seg * tps + tt) * LV_TINFO + 3];
  c1base = block_sum_i(c1base, sh);
  unsigned key[LV_ITEMS], val[LV_ITEMS];
  unsigned long long bal[LV_ITEMS];
  int total = 0;
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const long i = lv_elem(tile, j);
    key[j] = 0; val[j] = 0;
    if (i < M) { key[j] = keys[seg0 + i]; val[j] = vals[seg0 + i]; }
    bal[j] = __ballot(val[j] & 1u);
    total += __popcll(bal[j]);
  }
  if ((threadIdx.x & 63) == 0) wtot[w] = total;
  __syncthreads();
  long run = c1base;
  for (int ww = 0; ww < w; ++ww) run += wtot[ww];
  const unsigned long long upto = lanes_below() | (1ull << (threadIdx.x & 63));
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const long k = lv_elem(tile, j);             // rank within the segment
    if (k < M) {
      const int g = (int)(val[j] & 1u);
      const long c1 = run + __popcll(bal[j] & upto);
      const long c0 = k + 1 - c1;
      const long I = G - c1, U = G + c0;         // U >= 1
      const double wk = (g || k == 0) ? 1.0 / (double)U : (double)I / ((double)(U - 1) * (double)U);
      acc += (double)__uint_as_float(~key[j]) * wk;
      const long idx = (long)(val[j] >> 1);
      if (idx < n_total) dx[idx] = (float)((g ? -wk : wk) * scale);
    }
    run += __popcll(bal[j]);
  }
  acc = block_sum_d(acc, shd);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(LV_THREADS) void lovasz_final_kernel(const double* __restrict__ partial, const int* __restrict__ sinfo,
                                                                  float* __restrict__ loss, int segs, int tps) {
  __shared__ double shd[4];
  double tot = 0.0;
  int nf = 0;
  for (int seg = 0; seg < segs; ++seg) {
    const long M = sinfo[seg * LV_SINFO];
    const int nt = (int)((M + LV_TILE - 1) / LV_TILE);
    nf |= sinfo[seg * LV_SINFO + 2];
    double a = 0.0;
    for (int t = threadIdx.x; t < nt; t += LV_THREADS) a += partial[(long)seg * tps + t];
    tot += block_sum_d(a, shd);
  }
  // a non-finite logit makes the loss NaN whatever its rank (the meta loop skips such a task)
  if (threadIdx.x == 0) loss[0] = nf ? __uint_as_float(0x7fc00000u) : (float)(tot / (double)segs);
}

}  // namespace

int64_t lovasz_scratch_floats(int64_t n_total, int max_images) {
  const int64_t tiles = n_total / LV_TILE + max_images + 1;      // >= images * ceil(n_per_image / tile) for every split of n_total
  return 4 * ((n_total + 1) / 2 * 2) + tiles * (2 + 256 + LV_TINFO) + (int64_t)LV_SINFO * max_images + 16;
}

namespace {
template <bool VOID>
void lovasz_launches(const float* logits, const float* gt, float* dlogits, float* loss, float* scratch, int64_t n_per_image,
                     int images, int flat, float ign, hipStream_t s) {
  const int segs = flat ? 1 : images;
  const int64_t n_total = n_per_image * images;
  const long seg_len = (long)(flat ? n_total : n_per_image);
  const int tps = (int)lv_tiles(seg_len);
  const int nb = segs * tps;
  const LvScratch L = lv_carve(scratch, n_total, nb, segs);
  const dim3 grid(nb), block(LV_THREADS);
  hipLaunchKernelGGL((lovasz_prep_kernel<VOID>), grid, block, 0, s, logits, gt, dlogits, L.tinfo, seg_len, tps, ign);
  hipLaunchKernelGGL((lovasz_compact_kernel<VOID>), grid, block, 0, s, logits, gt, L.tinfo, L.sinfo, L.key[0], L.val[0], seg_len,
                     tps, ign);
  for (int pass = 0; pass < 4; ++pass) {           // (the key's top bit is always set: 31 significant bits, four 8-bit digits)
    const int in = pass & 1, out = in ^ 1;
    hipLaunchKernelGGL(lovasz_hist_kernel, grid, block, 0, s, L.key[in], L.sinfo, L.hist, seg_len, tps, 8 * pass);
    hipLaunchKernelGGL(lovasz_scan_kernel, dim3(segs), dim3(LV_SCAN_THREADS), 0, s, L.hist, L.sinfo, tps);
    hipLaunchKernelGGL(lovasz_scatter_kernel, grid, block, 0, s, L.key[in], L.val[in], L.key[out], L.val[out], L.sinfo, L.hist,
                       seg_len, tps, 8 * pass);
  }
  hipLaunchKernelGGL(lovasz_bits_kernel, grid, block, 0, s, L.val[0], L.sinfo, L.tinfo, seg_len, tps);
  hipLaunchKernelGGL(lovasz_weights_kernel, grid, block, 0, s, L.key[0], L.val[0], L.sinfo, L.tinfo, dlogits, L.partial, seg_len,
                     tps, (long)n_total, 1.0 / (double)segs);
  hipLaunchKernelGGL(lovasz_final_kernel, dim3(1), block, 0, s, L.partial, L.sinfo, loss, segs, tps);
}
}  // namespace

void launch_lovasz(const float* logits, const float* gt, float* dlogits, float* loss, float* scratch, int64_t n_per_image,
                   int images, int flat, const float* ignore, hipStream_t s) {
  if (ignore) lovasz_launches<true>(logits, gt, dlogits, loss, scratch, n_per_image, images, flat, *ignore, s);
  else lovasz_launches<false>(logits, gt, dlogits, loss, scratch, n_per_image, images, flat, 0.f, s);
}

}  // namespace eosvos
