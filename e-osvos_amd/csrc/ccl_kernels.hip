// Connected components of uint8 label maps and the component filter of the evaluation (small / non-dominant / ungated
// components are zeroed), for gfx950.  The rules are stated in include/eosvos.h (eosvos_label_components,
// eosvos_filter_components) and restated in numpy by eosvos_amd/components.py (label_host, filter_host).
//
// Labelling is a union-find over frame-local pixel indices p = y * W + x with the invariant  parent[p] <= p  at all times:
// every value ever stored in slot p is p itself or a smaller index.  So `find` walks strictly downward and ends, the root of
// a tree is its smallest index, and once all unions are done  id = 1 + root  is the 1 + min(y * W + x) of the component.
//   ccl_tile_kernel     one workgroup per 64 x 16 tile, one wave per row: run starts from the __ballot word of "same label as
//                       the left neighbour", the rows joined by a union-find in LDS; writes parent[p] = global index of the
//                       tile-local root and tarea[p] = pixel count of the tile-local root (0 where p is no tile-local root)
//   ccl_seam_kernel     pixels on tile borders are united with their neighbours across the border (atomicMin on parent)
//   ccl_flatten_kernel  every pixel resolves its root (parent is read-only here) and writes the id map; every tile-local root
//                       adds its count to area[root]: one atomic per (tile, tile-local root), never one per pixel
// and, for the filter, per frame in ascending order (one launch for all frames when the gate is off: nothing then depends on
// the frame before):
//   ccl_presence_kernel which labels a map R contains (pres[o] = 1)
//   ccl_gate_kernel     cand[root] = 1 for every component with a pixel within Chebyshev distance g of a pixel of R with its label
//   ccl_best_kernel     best[o] = max over the candidates of (area << 32) | ~id : the largest area, ties to the smallest id
//   ccl_apply_kernel    the three area rules; writes the filtered map, the labels it contains (the next frame's `pres`) and the
//                       number of pixels zeroed
// No launch is cooperative, no workgroup waits for another, no loop's exit depends on another workgroup's progress: other
// workgroups can only LOWER a parent slot, and every loop below makes progress by reading a strictly smaller index than
// before.  The bound of every loop is stated at the loop.  All sums, maxima and flags are integers: arrival order cannot
// change a result.
#include "kernels.h"

namespace eosvos {
namespace {
constexpr int CCL_TW = 64, CCL_TH = 16;      // tile: one wave-wide row segment x 16 rows, 4 rows per wave
constexpr int CCL_TILE = CCL_TW * CCL_TH;

typedef unsigned long long u64;

// ---- union-find primitives --------------------------------------------------------------------------------------------
// Loop bound: the index read strictly decreases (parent[i] <= i, and the loop goes on only where parent[i] != i), so at
// most i + 1 <= 1024 steps in a tile (LDS) and at most H * W < 2^24 steps in a frame (global), whatever other threads store.
__device__ __forceinline__ int ccl_find(const int* parent, int i) {
  for (;;) {
    const int p = __atomic_load_n(parent + i, __ATOMIC_RELAXED);
    if (p == i) return i;
    i = p;
  }
}

// The atomicMin form of union.  Loop bound: a retry happens only when the atomicMin found the larger root's slot already
// lowered (old < hi), and it continues from old: max(a, b) or the other index strictly decreases, so a + b strictly
// decreases with every retry -- at most a + b < 2 * H * W retries (2048 in a tile), each with two bounded finds.  Another
// thread's stores can only make `old` smaller, never send the loop back up.
__device__ __forceinline__ void ccl_union(int* parent, int a, int b) {
  for (;;) {
    a = ccl_find(parent, a);
    b = ccl_find(parent, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicMin(parent + hi, lo);
    if (old == hi) return;                   // hi was a root and now hangs under lo
    a = old;                                 // old < hi: somebody hooked hi first; unite what it hangs under with lo
    b = lo;
  }
}

// OR of the word shifted towards higher pixels by 0..k (lo = the word of lower pixels) / towards lower pixels by 0..k (hi = the
// word of higher pixels); bit j of a word is pixel 64 * word + j.  k <= 63.  (The shift-or of metrics_kernels.hip.)
// Loop bound: cov at least doubles or reaches k + 1: at most 7 steps.
__device__ __forceinline__ u64 ccl_spread(u64 lo, u64 c, u64 hi, int k) {
  unsigned __int128 up = ((unsigned __int128)c << 64) | lo;
  unsigned __int128 dn = ((unsigned __int128)hi << 64) | c;
  for (int cov = 1; cov <= k;) {
    const int s = cov < k + 1 - cov ? cov : k + 1 - cov;
    up |= up << s;
    dn |= dn >> s;
    cov += s;
  }
  return (u64)(up >> 64) | (u64)dn;
}

// ---- labelling --------------------------------------------------------------------------------------------------------
// grid (ceil(W / 64), ceil(H / 16), frames), block 256
__global__ __launch_bounds__(256) void ccl_tile_kernel(const uint8_t* __restrict__ labels, int H, int W, int conn8,
                                                        int* __restrict__ parent, int* __restrict__ tarea) {
  __shared__ int s_par[CCL_TILE];
  __shared__ int s_cnt[CCL_TILE];
  __shared__ uint8_t s_lab[CCL_TILE];
  __shared__ u64 s_same[CCL_TH];             // per row: bit x = pixel x continues the run of pixel x - 1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t plane = (size_t)H * W;
  labels += blockIdx.z * plane;
  parent += blockIdx.z * plane;
  tarea += blockIdx.z * plane;
  const int x = (int)blockIdx.x * CCL_TW + lane, y0 = (int)blockIdx.y * CCL_TH;
  int lab[4], root[4];
  u64 same[4];
  // 1. rows: every pixel points at the start of its run
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = wave + 4 * k, y = y0 + r;
    const int L = (x < W && y < H) ? labels[(size_t)y * W + x] : 0;          // 0 outside the frame: joins nothing
    const int left = __shfl_up(L, 1);
    const u64 m = __ballot(lane > 0 && L != 0 && L == left);
    const u64 upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);               // bits 0 .. lane
    const int start = 63 - __clzll((long long)(~m & upto));                  // bit 0 of ~m is always set
    lab[k] = L;
    same[k] = m;
    s_lab[r * CCL_TW + lane] = (uint8_t)L;
    s_par[r * CCL_TW + lane] = r * CCL_TW + start;
    s_cnt[r * CCL_TW + lane] = 0;
    if (lane == 0) s_same[r] = m;
  }
  __syncthreads();
  // 2. columns: a run meets the runs of the row above.  Two runs that share a column share the leftmost such column, which is
  // the start of one of them, so only those pixels unite upward; a corner neighbour matters only where the pixel above differs
  // (else it is in that pixel's run).
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = wave + 4 * k, i = r * CCL_TW + lane, L = lab[k];
    if (r == 0 || L == 0) continue;
    if (s_lab[i - CCL_TW] == L) {
      if (!((same[k] >> lane) & 1) || !((s_same[r - 1] >> lane) & 1)) ccl_union(s_par, i, i - CCL_TW);
    } else if (conn8) {
      if (lane > 0 && s_lab[i - CCL_TW - 1] == L) ccl_union(s_par, i, i - CCL_TW - 1);
      if (lane < 63 && s_lab[i - CCL_TW + 1] == L) ccl_union(s_par, i, i - CCL_TW + 1);
    }
  }
  __syncthreads();
  // 3. roots (the forest is read-only from here) and their pixel counts: one LDS add per run
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = wave + 4 * k, i = r * CCL_TW + lane;
    root[k] = ccl_find(s_par, i);
    if (lab[k] != 0 && !((same[k] >> lane) & 1)) {                            // the start of a run of an object label
      const u64 later = lane == 63 ? 0ull : (~same[k] & ~((2ull << lane) - 1));   // starts after this lane (background pixels are starts)
      const int end = later ? __ffsll((long long)later) - 1 : 64;
      atomicAdd(s_cnt + root[k], end - lane);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = wave + 4 * k, i = r * CCL_TW + lane, y = y0 + r;
    if (x >= W || y >= H) continue;
    const int rr = root[k] >> 6, rl = root[k] & 63;
    const size_t p = (size_t)y * W + x;
    parent[p] = (y0 + rr) * W + (int)blockIdx.x * CCL_TW + rl;                // row-major in the tile and in the frame: <= p
    tarea[p] = (lab[k] != 0 && root[k] == i) ? s_cnt[i] : 0;
  }
}

// grid (ceil(H * W / 256), frames), block 256.  Pixels whose neighbour to the left / above / at an upper corner lies in another tile.
__global__ __launch_bounds__(256) void ccl_seam_kernel(const uint8_t* __restrict__ labels, int H, int W, int conn8,
                                                        int* __restrict__ parent) {
  const int n_pix = H * W;
  const int p = (int)(blockIdx.x * 256u + threadIdx.x);
  if (p >= n_pix) return;
  const int y = p / W, x = p - y * W;
  const bool col0 = (x & (CCL_TW - 1)) == 0, col63 = (x & (CCL_TW - 1)) == CCL_TW - 1, row0 = (y & (CCL_TH - 1)) == 0;
  if (!(col0 || row0 || (conn8 && col63))) return;
  labels += (size_t)blockIdx.y * n_pix;
  parent += (size_t)blockIdx.y * n_pix;
  const int L = labels[p];
  if (L == 0) return;
  if (col0 && x > 0 && labels[p - 1] == L) ccl_union(parent, p, p - 1);
  if (y == 0) return;
  if (row0 && labels[p - W] == L) ccl_union(parent, p, p - W);
  if (!conn8) return;
  if ((col0 || row0) && x > 0 && labels[p - W - 1] == L) ccl_union(parent, p, p - W - 1);
  if ((col63 || row0) && x + 1 < W && labels[p - W + 1] == L) ccl_union(parent, p, p - W + 1);
}

// grid (ceil(H * W / 256), frames), block 256.  area: zeroed by the caller.
__global__ __launch_bounds__(256) void ccl_flatten_kernel(const uint8_t* __restrict__ labels, int n_pix, const int* __restrict__ parent,
                                                           const int* __restrict__ tarea, int* __restrict__ ids, int* __restrict__ area) {
  const int p = (int)(blockIdx.x * 256u + threadIdx.x);
  if (p >= n_pix) return;
  const size_t base = (size_t)blockIdx.y * n_pix;
  if (labels[base + p] == 0) { ids[base + p] = 0; return; }
  const int root = ccl_find(parent + base, p);
  ids[base + p] = root + 1;
  if (area) {
    const int a = tarea[base + p];
    if (a) atomicAdd(area + base + root, a);
  }
}

// ---- filter -----------------------------------------------------------------------------------------------------------
// grid (ceil(H * W / 256)), block 256.  pres[256]: zeroed by the caller.  Every writer stores the same 1.
__global__ __launch_bounds__(256) void ccl_presence_kernel(const uint8_t* __restrict__ map, int n_pix, uint8_t* __restrict__ pres) {
  const int p = (int)(blockIdx.x * 256u + threadIdx.x);
  if (p >= n_pix) return;
  const int v = map[p];
  if (v && !pres[v]) pres[v] = 1;
}

// grid (ceil(W / 64), ceil(H / 4)), block 256: one wave per 64-pixel word of a row of `labels`.  R: the filtered map of the
// frame before, pres: the labels it contains.  cand: zeroed by the caller; every writer stores the same 1.
__global__ __launch_bounds__(256) void ccl_gate_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ R,
                                                        const uint8_t* __restrict__ pres, const int* __restrict__ ids, int H, int W,
                                                        int g, uint8_t* __restrict__ cand) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = (W + 63) / 64, w = blockIdx.x;
  const int y = (int)blockIdx.y * 4 + wave;
  if (y >= H) return;                        // the whole wave
  const int ya = max(0, y - g), yb = min(H - 1, y + g);
  const int x = w * 64 + lane;
  const bool in = x < W;
  const int L = in ? labels[(size_t)y * W + x] : 0;
  u64 rem = __ballot(L != 0);
  while (rem) {                              // the distinct labels of the word: every pass clears at least one bit, <= 64 passes
    const int o = __shfl(L, __ffsll((long long)rem) - 1);
    const u64 mine = __ballot(L == o);
    rem &= ~mine;
    if (!pres[o]) continue;                  // the gate is inactive for this label (wave-uniform)
    u64 lo = 0, c = 0, hi = 0;
    for (int yy = ya; yy <= yb; ++yy) {      // <= 2 g + 1 <= 127 rows
      const uint8_t* row = R + (size_t)yy * W;
      c |= __ballot(in && row[x] == o);
      if (w > 0) lo |= __ballot(row[x - 64] == o);
      if (w + 1 < nw) hi |= __ballot(x + 64 < W && row[x + 64] == o);
    }
    const u64 near = ccl_spread(lo, c, hi, g);
    if (((near & mine) >> lane) & 1) {
      const int root = ids[(size_t)y * W + x] - 1;
      if (!cand[root]) cand[root] = 1;
    }
  }
}

// A component of label o is a candidate when the gate is inactive for o or its root is flagged.
__device__ __forceinline__ bool ccl_candidate(const uint8_t* pres, const uint8_t* cand, int o, int root) {
  return pres == nullptr || !pres[o] || cand[root];
}

// grid (ceil(H * W / 256), frames), block 256.  best [frames][256]: zeroed by the caller.  pres: null when the gate is off or
// there is no frame before (only then may frames > 1).  One atomic per component at most; the plain read first spares the
// atomic where a larger key has arrived already (the maximum only grows).
__global__ __launch_bounds__(256) void ccl_best_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ ids,
                                                        const int* __restrict__ area, const uint8_t* __restrict__ pres,
                                                        const uint8_t* __restrict__ cand, int n_pix, u64* __restrict__ best) {
  const int p = (int)(blockIdx.x * 256u + threadIdx.x);
  if (p >= n_pix) return;
  const size_t base = (size_t)blockIdx.y * n_pix;
  if (ids[base + p] != p + 1) return;        // not the root of a component
  const int o = labels[base + p];
  if (!ccl_candidate(pres, cand + base, o, p)) return;
  const u64 key = ((u64)(unsigned)area[base + p] << 32) | (unsigned)~(unsigned)(p + 1);
  u64* slot = best + (size_t)blockIdx.y * 256 + o;
  if (__atomic_load_n(slot, __ATOMIC_RELAXED) < key) atomicMax(slot, key);
}

// grid (ceil(H * W / 256), frames), block 256.  keep_all: the frames are copied unchanged; pres_out [frames][256] and
// removed [frames]: zeroed by the caller.
__global__ __launch_bounds__(256) void ccl_apply_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ ids,
                                                         const int* __restrict__ area, const uint8_t* __restrict__ pres,
                                                         const uint8_t* __restrict__ cand, const u64* __restrict__ best,
                                                         int keep_all, int n_pix, int min_area, unsigned rel_q16,
                                                         int largest_only, uint8_t* __restrict__ out, uint8_t* __restrict__ pres_out,
                                                         u64* __restrict__ removed) {
  __shared__ unsigned s_removed;
  if (threadIdx.x == 0) s_removed = 0;
  __syncthreads();
  const int p = (int)(blockIdx.x * 256u + threadIdx.x);
  const int f = blockIdx.y;
  const size_t base = (size_t)f * n_pix;
  bool zeroed = false;
  if (p < n_pix) {
    const int o = labels[base + p];
    int v = o;
    if (o != 0 && !keep_all) {
      const int id = ids[base + p], root = id - 1;
      const u64 b = best[(size_t)f * 256 + o];
      const u64 A = (u64)(unsigned)area[base + root], amax = b >> 32;
      const unsigned best_id = ~(unsigned)b;
      const bool kept = ccl_candidate(pres, cand + base, o, root) && A >= (u64)min_area && A * 65536ull >= (u64)rel_q16 * amax &&
                        (!largest_only || (A == amax && (unsigned)id == best_id));
      if (!kept) { v = 0; zeroed = true; }
    }
    out[base + p] = (uint8_t)v;
    if (v && !pres_out[(size_t)f * 256 + v]) pres_out[(size_t)f * 256 + v] = 1;
  }
  const u64 z = __ballot(zeroed);
  if ((threadIdx.x & 63) == 0 && z) atomicAdd(&s_removed, (unsigned)__popcll(z));
  __syncthreads();
  if (threadIdx.x == 0 && s_removed) atomicAdd(removed + f, (u64)s_removed);
}
}  // namespace

void launch_ccl_label(const uint8_t* labels, int n_frames, int H, int W, int connectivity, int* parent, int* tarea, int* ids,
                      int* area, hipStream_t s) {
  const int conn8 = connectivity == 8, n_pix = H * W;
  const dim3 per_pixel((n_pix + 255) / 256, n_frames);
  hipLaunchKernelGGL(ccl_tile_kernel, dim3((W + CCL_TW - 1) / CCL_TW, (H + CCL_TH - 1) / CCL_TH, n_frames), dim3(256), 0, s,
                     labels, H, W, conn8, parent, tarea);
  hipLaunchKernelGGL(ccl_seam_kernel, per_pixel, dim3(256), 0, s, labels, H, W, conn8, parent);
  hipLaunchKernelGGL(ccl_flatten_kernel, per_pixel, dim3(256), 0, s, labels, n_pix, (const int*)parent, (const int*)tarea, ids, area);
}

void launch_ccl_presence(const uint8_t* map, int n_pix, uint8_t* pres, hipStream_t s) {
  hipLaunchKernelGGL(ccl_presence_kernel, dim3((n_pix + 255) / 256), dim3(256), 0, s, map, n_pix, pres);
}

void launch_ccl_gate(const uint8_t* labels, const uint8_t* R, const uint8_t* pres, const int* ids, int H, int W, int gate,
                     uint8_t* cand, hipStream_t s) {
  hipLaunchKernelGGL(ccl_gate_kernel, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, s, labels, R, pres, ids, H, W, gate, cand);
}

void launch_ccl_filter(const uint8_t* labels, const int* ids, const int* area, const uint8_t* pres, const uint8_t* cand,
                       int keep_all, int n_frames, int n_pix, int min_area, unsigned rel_q16, int largest_only,
                       unsigned long long* best, uint8_t* out, uint8_t* pres_out, unsigned long long* removed, hipStream_t s) {
  const dim3 grid((n_pix + 255) / 256, n_frames);
  if (!keep_all) hipLaunchKernelGGL(ccl_best_kernel, grid, dim3(256), 0, s, labels, ids, area, pres, cand, n_pix, best);
  hipLaunchKernelGGL(ccl_apply_kernel, grid, dim3(256), 0, s, labels, ids, area, pres, cand, (const u64*)best, keep_all, n_pix, min_area,
                     rel_q16, largest_only, out, pres_out, removed);
}
}  // namespace eosvos
