// SLIC superpixels of uint8 frames in integers (the gSLIC scheme) and the superpixel vote that snaps the merged label maps to
// them, for gfx950.  The rules are stated in include/eosvos.h (eosvos_superpixels, eosvos_snap_labels) and restated in numpy
// by eosvos_amd/snap.py (superpixels_host, snap_host).
//
// A frame of H x W pixels has gy x gx = ceil(H / S) x ceil(W / S) cells and one cluster per cell, id = cy * gx + cx.  Per
// frame: centres [K][5] (y, x, R, G, B), sums [K][6] (n and the sums of y, x, R, G, B), ids [H * W], and for the vote
// votes [K][n_obj + 1].
//   slic_init_kernel      one launch: the centres start at the cell centres, with the colour of that pixel
//   slic_assign_kernel<0> one launch per iteration but the last: a workgroup owns a 64 x 16 pixel tile, holds the centres of
//                         the cells its tile touches +-1 in LDS, gives every pixel the nearest of its (up to) nine candidates and
//                         adds (1, y, x, R, G, B) to that cluster's LDS accumulators; at the end one global atomic per
//                         non-zero accumulator word
//   slic_finish_kernel    one launch per iteration but the last: new centres from the sums, sums zeroed
//   slic_assign_kernel<1> the last iteration of eosvos_superpixels: writes the ids, accumulates nothing
//   slic_assign_kernel<2> the last iteration of eosvos_snap_labels: writes the ids and counts the votes -- in LDS where the
//                         tile's slice of the table fits, else one global atomic per wave and distinct (cluster, label)
//   slic_apply_kernel     the winner and the share rule per cluster of the tile, then the pixels
// LDS bound: a tile spans at most 63 / S + 2 cell columns and 15 / S + 2 cell rows, +-1 on each side gives at most
// (63 / S + 4) * (15 / S + 4) <= 19 * 7 = 133 clusters for S >= 4 (SLIC_MAXC): 133 * (5 + 6) words = 5852 bytes.
// Integer arithmetic and integer atomics only: sums and counts do not depend on arrival order, the result is exact.  No
// launch is cooperative, no workgroup waits for another; the bound of every loop is stated at the loop.
// D of the assignment fits unsigned 32 bits: the colour part is <= 3 * 255^2 * 64^2 = 799 027 200; a centre is a mean of pixels
// of cells within +-1 of its own and a pixel only meets clusters within +-1 of its home cell, so |dy|, |dx| < 3 S <= 192 and the
// position part is <= 64^2 * 2 * 191^2 < 3.0e8.  A sum is <= (3 * 64)^2 pixels * 4095 < 1.6e8, and 2 * sum + n fits as well.
#include "kernels.h"

namespace eosvos {
namespace {
constexpr int SLIC_TW = 64, SLIC_TH = 16;     // tile: one wave-wide row segment x 16 rows, 4 rows per wave
constexpr int SLIC_MAXC = 19 * 7;             // clusters a tile can meet (S >= 4), see above
constexpr int SLIC_VOTE_LDS = 2048;           // words of LDS for a tile's slice of the vote table (8 KB)

typedef unsigned long long u64;

// The cells a tile's pixels can be assigned to: those its pixels lie in, +-1, clipped to the grid.  Uniform per workgroup.
struct SlicTile {
  int cy_lo, cx_lo, ncy, ncx;
  __device__ __forceinline__ int count() const { return ncy * ncx; }
  __device__ __forceinline__ int id(int local, int gx) const { return (cy_lo + local / ncx) * gx + cx_lo + local % ncx; }
};

__device__ __forceinline__ SlicTile slic_tile(int H, int W, int S, int gy, int gx) {
  const int x0 = (int)blockIdx.x * SLIC_TW, y0 = (int)blockIdx.y * SLIC_TH;
  const int x1 = min(x0 + SLIC_TW - 1, W - 1), y1 = min(y0 + SLIC_TH - 1, H - 1);
  SlicTile t;
  t.cx_lo = max(x0 / S - 1, 0);
  t.cy_lo = max(y0 / S - 1, 0);
  t.ncx = min(x1 / S + 1, gx - 1) - t.cx_lo + 1;
  t.ncy = min(y1 / S + 1, gy - 1) - t.cy_lo + 1;
  return t;
}

// grid (ceil(K / 256), frames), block 256
__global__ __launch_bounds__(256) void slic_init_kernel(const uint8_t* __restrict__ rgb, int H, int W, int S, int gx, int K,
                                                         int* __restrict__ centres) {
  const int k = (int)(blockIdx.x * 256u + threadIdx.x);
  if (k >= K) return;
  const size_t plane = (size_t)H * W;
  rgb += (size_t)blockIdx.y * 3 * plane;
  int* c = centres + ((size_t)blockIdx.y * K + k) * 5;
  const int cy = k / gx, cx = k - cy * gx;
  const int y = min(cy * S + S / 2, H - 1), x = min(cx * S + S / 2, W - 1);
  const size_t p = (size_t)y * W + x;
  c[0] = y;
  c[1] = x;
  c[2] = rgb[p];
  c[3] = rgb[plane + p];
  c[4] = rgb[2 * plane + p];
}

// grid (ceil(W / 64), ceil(H / 16), frames), block 256.  MODE 0: accumulate into sums (zeroed by the caller / the finish
// launch); 1: write ids; 2: write ids and count votes (zeroed by the caller).  No thread leaves before the end: the barriers
// and, in mode 2, the ballots see whole workgroups / waves.
template <int MODE>
__global__ __launch_bounds__(256) void slic_assign_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ labels,
                                                           int H, int W, int S, int m, int gy, int gx, int n_obj,
                                                           const int* __restrict__ centres, unsigned* __restrict__ sums,
                                                           int* __restrict__ ids, unsigned* __restrict__ votes) {
  __shared__ int s_cen[SLIC_MAXC * 5];
  __shared__ unsigned s_acc[MODE == 0 ? SLIC_MAXC * 6 : 1];
  __shared__ unsigned s_vote[MODE == 2 ? SLIC_VOTE_LDS : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = gy * gx, nl = n_obj + 1;
  const size_t plane = (size_t)H * W, f = blockIdx.z;
  rgb += f * 3 * plane;
  centres += f * K * 5;
  const SlicTile t = slic_tile(H, W, S, gy, gx);
  const int nc = t.count();                                      // <= SLIC_MAXC
  const bool vote_lds = MODE == 2 && nc * nl <= SLIC_VOTE_LDS;
  for (int i = tid; i < nc * 5; i += 256) {                      // <= 665 words: <= 3 passes
    const int local = i / 5;
    s_cen[i] = centres[(size_t)t.id(local, gx) * 5 + (i - local * 5)];
  }
  if (MODE == 0)
    for (int i = tid; i < nc * 6; i += 256) s_acc[i] = 0;        // <= 798 words: <= 4 passes
  if (vote_lds)
    for (int i = tid; i < nc * nl; i += 256) s_vote[i] = 0;      // <= 2048 words: <= 8 passes
  __syncthreads();
  const int x = (int)blockIdx.x * SLIC_TW + lane, hx = x / S;
  const unsigned S2 = (unsigned)(S * S), m2 = (unsigned)(m * m);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = (int)blockIdx.y * SLIC_TH + wave + 4 * k;
    const bool in = x < W && y < H;
    int best_local = 0;
    if (in) {
      const size_t p = (size_t)y * W + x;
      const int R = rgb[p], G = rgb[plane + p], B = rgb[2 * plane + p];
      const int hy = y / S;
      unsigned best = 0xffffffffu;                               // D < 2^32 - 1: the first candidate always takes it
      // the candidates in ascending id order, a strict `<`: ties go to the smaller id.  9 passes.
      for (int dy = -1; dy <= 1; ++dy) {
        const int cy = hy + dy;
        if (cy < 0 || cy >= gy) continue;
        for (int dx = -1; dx <= 1; ++dx) {
          const int cx = hx + dx;
          if (cx < 0 || cx >= gx) continue;
          const int local = (cy - t.cy_lo) * t.ncx + (cx - t.cx_lo);
          const int* c = s_cen + local * 5;
          const int ey = y - c[0], ex = x - c[1], er = R - c[2], eg = G - c[3], eb = B - c[4];
          const unsigned D = (unsigned)(er * er + eg * eg + eb * eb) * S2 + m2 * (unsigned)(ey * ey + ex * ex);
          if (D < best) { best = D; best_local = local; }
        }
      }
      if (MODE == 0) {
        unsigned* a = s_acc + best_local * 6;
        atomicAdd(a + 0, 1u);
        atomicAdd(a + 1, (unsigned)y);
        atomicAdd(a + 2, (unsigned)x);
        atomicAdd(a + 3, (unsigned)R);
        atomicAdd(a + 4, (unsigned)G);
        atomicAdd(a + 5, (unsigned)B);
      } else {
        ids[f * plane + p] = t.id(best_local, gx);
      }
    }
    if (MODE == 2) {
      const int L = in ? labels[f * plane + (size_t)y * W + x] : 256;
      const bool voter = L <= n_obj;
      if (vote_lds) {
        if (voter) atomicAdd(s_vote + best_local * nl + L, 1u);
      } else {
        // one global atomic per (wave, distinct (cluster, label)).  Loop bound: every pass clears at least the bit it took
        // the key from: <= 64 passes.
        const int key = best_local * 256 + L;
        u64 rem = __ballot(voter);
        while (rem) {
          const int k0 = __shfl(key, __ffsll((long long)rem) - 1);
          const u64 mine = __ballot(voter && key == k0);
          rem &= ~mine;
          if (lane == __ffsll((long long)mine) - 1)
            atomicAdd(votes + (f * K + (size_t)t.id(k0 >> 8, gx)) * nl + (k0 & 255), (unsigned)__popcll(mine));
        }
      }
    }
  }
  if (MODE == 0 || vote_lds) __syncthreads();
  if (MODE == 0) {
    for (int i = tid; i < nc * 6; i += 256) {                    // <= 4 passes; one global atomic per non-zero word
      const unsigned v = s_acc[i];
      const int local = i / 6;
      if (v) atomicAdd(sums + (f * K + (size_t)t.id(local, gx)) * 6 + (i - local * 6), v);
    }
  }
  if (vote_lds) {
    for (int i = tid; i < nc * nl; i += 256) {                   // <= 8 passes; one global atomic per non-zero word
      const unsigned v = s_vote[i];
      const int local = i / nl;
      if (v) atomicAdd(votes + (f * K + (size_t)t.id(local, gx)) * nl + (i - local * nl), v);
    }
  }
}

// grid (ceil(K / 256), frames), block 256.  A cluster without pixels keeps its centre.
__global__ __launch_bounds__(256) void slic_finish_kernel(int K, int* __restrict__ centres, unsigned* __restrict__ sums) {
  const int k = (int)(blockIdx.x * 256u + threadIdx.x);
  if (k >= K) return;
  unsigned* s = sums + ((size_t)blockIdx.y * K + k) * 6;
  int* c = centres + ((size_t)blockIdx.y * K + k) * 5;
  const unsigned n = s[0];
  s[0] = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    if (n) c[j] = (int)((2u * s[1 + j] + n) / (2u * n));         // round half up
    s[1 + j] = 0;
  }
}

// grid (ceil(W / 64), ceil(H / 16), frames), block 256.  keep_all: the frames are copied unchanged.  changed [frame]: zeroed
// by the caller; one LDS add per wave, one global atomic per workgroup.  No thread leaves before the end.
__global__ __launch_bounds__(256) void slic_apply_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ ids,
                                                          const unsigned* __restrict__ votes, int keep_all, int H, int W, int S,
                                                          int gy, int gx, int n_obj, unsigned q16, uint8_t* __restrict__ out,
                                                          u64* __restrict__ changed) {
  __shared__ int s_dec[SLIC_MAXC];             // per cluster of the tile: the label its voters take, -1: they are copied
  __shared__ unsigned s_changed;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = gy * gx, nl = n_obj + 1;
  const size_t plane = (size_t)H * W, f = blockIdx.z;
  const SlicTile t = slic_tile(H, W, S, gy, gx);
  if (tid == 0) s_changed = 0;
  if (!keep_all && tid < t.count()) {          // count() <= SLIC_MAXC < 256: one thread per cluster
    const unsigned* v = votes + (f * K + (size_t)t.id(tid, gx)) * nl;
    unsigned n_c = 0, top = 0;
    int w = 0;
    for (int l = 0; l < nl; ++l) {             // <= 256 labels; a strict `>`: ties go to the smaller label
      const unsigned c = v[l];
      n_c += c;
      if (c > top) { top = c; w = l; }
    }
    s_dec[tid] = (n_c > 0 && (u64)top * 65536ull >= (u64)q16 * (u64)n_c) ? w : -1;
  }
  __syncthreads();
  const int x = (int)blockIdx.x * SLIC_TW + lane;
  unsigned moved = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = (int)blockIdx.y * SLIC_TH + wave + 4 * k;
    bool diff = false;
    if (x < W && y < H) {
      const size_t p = f * plane + (size_t)y * W + x;
      const int L = labels[p];
      int v = L;
      if (!keep_all && L <= n_obj) {
        const int id = ids[p];
        const int ly = id / gx - t.cy_lo, lx = id % gx - t.cx_lo;
        if (ly >= 0 && ly < t.ncy && lx >= 0 && lx < t.ncx) {    // always: the id is one of the pixel's candidates
          const int w = s_dec[ly * t.ncx + lx];
          if (w >= 0) v = w;
        }
      }
      out[p] = (uint8_t)v;
      diff = v != L;
    }
    moved += (unsigned)__popcll(__ballot(diff));
  }
  if (lane == 0 && moved) atomicAdd(&s_changed, moved);
  __syncthreads();
  if (tid == 0 && s_changed) atomicAdd(changed + f, (u64)s_changed);
}

dim3 slic_tiles(int n_frames, int H, int W) { return dim3((W + SLIC_TW - 1) / SLIC_TW, (H + SLIC_TH - 1) / SLIC_TH, n_frames); }
}  // namespace

void launch_slic_init(const uint8_t* rgb, int n_frames, int H, int W, int S, int* centres, hipStream_t s) {
  const int gy = (H + S - 1) / S, gx = (W + S - 1) / S, K = gy * gx;
  hipLaunchKernelGGL(slic_init_kernel, dim3((K + 255) / 256, n_frames), dim3(256), 0, s, rgb, H, W, S, gx, K, centres);
}

void launch_slic_iterate(const uint8_t* rgb, int n_frames, int H, int W, int S, int m, int* centres, unsigned* sums, hipStream_t s) {
  const int gy = (H + S - 1) / S, gx = (W + S - 1) / S, K = gy * gx;
  hipLaunchKernelGGL(slic_assign_kernel<0>, slic_tiles(n_frames, H, W), dim3(256), 0, s, rgb, (const uint8_t*)nullptr, H, W, S, m, gy, gx,
                     0, (const int*)centres, sums, (int*)nullptr, (unsigned*)nullptr);
  hipLaunchKernelGGL(slic_finish_kernel, dim3((K + 255) / 256, n_frames), dim3(256), 0, s, K, centres, sums);
}

void launch_slic_last(const uint8_t* rgb, const uint8_t* labels, int n_frames, int H, int W, int S, int m, int n_obj,
                      const int* centres, int* ids, unsigned* votes, hipStream_t s) {
  const int gy = (H + S - 1) / S, gx = (W + S - 1) / S;
  if (labels)
    hipLaunchKernelGGL(slic_assign_kernel<2>, slic_tiles(n_frames, H, W), dim3(256), 0, s, rgb, labels, H, W, S, m, gy, gx, n_obj,
                       centres, (unsigned*)nullptr, ids, votes);
  else
    hipLaunchKernelGGL(slic_assign_kernel<1>, slic_tiles(n_frames, H, W), dim3(256), 0, s, rgb, labels, H, W, S, m, gy, gx, 0, centres,
                       (unsigned*)nullptr, ids, (unsigned*)nullptr);
}

void launch_slic_apply(const uint8_t* labels, const int* ids, const unsigned* votes, int keep_all, int n_frames, int H, int W,
                       int S, int n_obj, unsigned q16, uint8_t* out, unsigned long long* changed, hipStream_t s) {
  const int gy = (H + S - 1) / S, gx = (W + S - 1) / S;
  hipLaunchKernelGGL(slic_apply_kernel, slic_tiles(n_frames, H, W), dim3(256), 0, s, labels, ids, votes, keep_all, H, W, S, gy, gx, n_obj,
                     q16, out, changed);
}
}  // namespace eosvos
