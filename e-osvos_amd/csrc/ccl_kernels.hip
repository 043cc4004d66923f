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
// and, for the hole filler (eosvos_fill_holes, eosvos_amd/holes.py: fill_host), the same three labelling kernels over the ZERO
// pixels under the dual connectivity, then
//   hole_scan_kernel    every zero pixel merges its border flag and its non-zero neighbours into its root's record; the frame's
//                       label histogram
//   hole_overlap_kernel per frame, only with the previous-frame rule: how many pixels of a candidate hole were its label in R
//   hole_apply_kernel   the size and overlap rules; writes the filled map, the labels it contains and the pixels filled
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
// ZERO: the hole filler's labelling of the BACKGROUND -- a pixel counts as label 1 where the map holds 0 and as background where
// it holds an object label; the three kernels are otherwise the same code, and the <false> instances are the ones they were.
template <bool ZERO>
__device__ __forceinline__ int ccl_value(int raw) { return ZERO ? (raw == 0 ? 1 : 0) : raw; }

// grid (ceil(W / 64), ceil(H / 16), frames), block 256
template <bool ZERO>
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
    const int L = (x < W && y < H) ? ccl_value<ZERO>(labels[(size_t)y * W + x]) : 0;   // 0 outside the frame: joins nothing
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
template <bool ZERO>
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
  const int L = ccl_value<ZERO>(labels[p]);
  if (L == 0) return;
  if (col0 && x > 0 && ccl_value<ZERO>(labels[p - 1]) == L) ccl_union(parent, p, p - 1);
  if (y == 0) return;
  if (row0 && ccl_value<ZERO>(labels[p - W]) == L) ccl_union(parent, p, p - W);
  if (!conn8) return;
  if ((col0 || row0) && x > 0 && ccl_value<ZERO>(labels[p - W - 1]) == L) ccl_union(parent, p, p - W - 1);
  if ((col63 || row0) && x + 1 < W && ccl_value<ZERO>(labels[p - W + 1]) == L) ccl_union(parent, p, p - W + 1);
}

// grid (ceil(H * W / 256), frames), block 256.  area: zeroed by the caller.
template <bool ZERO>
__global__ __launch_bounds__(256) void ccl_flatten_kernel(const uint8_t* __restrict__ labels, int n_pix, const int* __restrict__ parent,
                                                           const int* __restrict__ tarea, int* __restrict__ ids, int* __restrict__ area) {
  const int p = (int)(blockIdx.x * 256u + threadIdx.x);
  if (p >= n_pix) return;
  const size_t base = (size_t)blockIdx.y * n_pix;
  if (ccl_value<ZERO>(labels[base + p]) == 0) { ids[base + p] = 0; return; }
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

// ---- hole filling (eosvos_fill_holes; the rules: include/eosvos.h, the numpy twin: eosvos_amd/holes.py) ------------------
// The background is labelled by the three kernels above in their ZERO form under the dual connectivity; ids[p] - 1 is then the
// root of a zero pixel's background component and area[root] its pixel count A.  Per root one 32-bit record:
//   bit 16       a pixel of the component lies on the frame border
//   bits 8..15   255 - the smallest non-zero neighbour label seen
//   bits 0..7    the largest non-zero neighbour label seen (0: none yet)
// All three fields only grow, and merging two records is the field-wise maximum.  A record is DEAD once the border bit is set or
// the two labels differ: the component is then no candidate whatever else arrives, and nobody stores to it any more.
constexpr unsigned HOLE_BORDER = 1u << 16;

__device__ __forceinline__ unsigned hole_merge(unsigned a, unsigned b) {
  const unsigned hi = max(a & 0xffu, b & 0xffu), lo = max(a & 0xff00u, b & 0xff00u);
  return ((a | b) & HOLE_BORDER) | lo | hi;
}
__device__ __forceinline__ unsigned hole_word(int label) { return ((255u - (unsigned)label) << 8) | (unsigned)label; }   // label != 0
__device__ __forceinline__ bool hole_dead(unsigned r) {
  return (r & HOLE_BORDER) || ((r & 0xffu) && 255u - ((r >> 8) & 0xffu) != (r & 0xffu));
}
// the label a finished record makes its component a candidate for; 0: none (border, several labels)
__device__ __forceinline__ int hole_label(unsigned r) { return hole_dead(r) ? 0 : (int)(r & 0xffu); }

// Merges v into *slot.  The plain read first spares the atomic where the stored record is dead or already dominates v (both are
// monotone, so a stale read can only cost a spared atomic, never a result).  Loop bound: a retry happens only when another
// thread's compare-and-swap changed the word in between; a live word has seen at most one label, so it changes at most twice
// (first label; border bit or second label, after which it is dead and nobody stores): at most 3 passes.  A retry is another
// thread's completed store, never a wait for one.
__device__ __forceinline__ void hole_update(unsigned* slot, unsigned v) {
  unsigned cur = __atomic_load_n(slot, __ATOMIC_RELAXED);
  for (;;) {
    if (hole_dead(cur)) return;
    const unsigned nw = hole_merge(cur, v);
    if (nw == cur) return;
    const unsigned old = atomicCAS(slot, cur, nw);
    if (old == cur) return;
    cur = old;
  }
}

__device__ __forceinline__ bool hole_size_ok(int A, unsigned S, int max_area, unsigned rel_q16) {
  return A <= max_area && (u64)(unsigned)A * 65536ull <= (u64)rel_q16 * (u64)S;
}

// (a) grid (ceil(H * W / 256), frames), block 256.  rec [frame][H * W] and hist [frame][256]: zeroed by the caller.  Every zero
// pixel merges its border flag and its non-zero neighbours (under the background's connectivity, bg8) into its root's record;
// every non-zero pixel counts in the frame's label histogram (S of the size rule).  No thread leaves before the end: the
// ballots and shuffles below see whole waves.
__global__ __launch_bounds__(256) void hole_scan_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ ids, int H, int W,
                                                         int bg8, unsigned* __restrict__ rec, unsigned* __restrict__ hist) {
  __shared__ unsigned s_hist[256];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const int n_pix = H * W, lane = threadIdx.x & 63;
  const int p = (int)(blockIdx.x * 256u + threadIdx.x);
  const size_t base = (size_t)blockIdx.y * n_pix;
  labels += base;
  int L = -1, root = -1;
  unsigned c = 0;
  if (p < n_pix) {
    L = labels[p];
    if (L == 0) {
      const int y = p / W, x = p - y * W;
      root = ids[base + p] - 1;
      if (x == 0 || y == 0 || x == W - 1 || y == H - 1) c = HOLE_BORDER;
      const bool l = x > 0, r = x + 1 < W, u = y > 0, d = y + 1 < H;      // every read below is inside the frame
      int v;
      if (l && (v = labels[p - 1])) c = hole_merge(c, hole_word(v));
      if (r && (v = labels[p + 1])) c = hole_merge(c, hole_word(v));
      if (u && (v = labels[p - W])) c = hole_merge(c, hole_word(v));
      if (d && (v = labels[p + W])) c = hole_merge(c, hole_word(v));
      if (bg8) {
        if (u && l && (v = labels[p - W - 1])) c = hole_merge(c, hole_word(v));
        if (u && r && (v = labels[p - W + 1])) c = hole_merge(c, hole_word(v));
        if (d && l && (v = labels[p + W - 1])) c = hole_merge(c, hole_word(v));
        if (d && r && (v = labels[p + W + 1])) c = hole_merge(c, hole_word(v));
      }
    }
  }
  // histogram: one LDS add per (wave, distinct label), not one per pixel -- an object fills whole waves with one label.
  // Loop bound: every pass clears at least the bit it took the label from: <= 64 passes.
  u64 rem = __ballot(L > 0);
  while (rem) {
    const int o = __shfl(L, __ffsll((long long)rem) - 1);
    const u64 mine = __ballot(L == o);
    rem &= ~mine;
    if (lane == 0) atomicAdd(s_hist + o, (unsigned)__popcll(mine));
  }
  // records: lanes whose root's record is dead or dominates their word already drop out on a plain read -- almost every pixel
  // of the "outside" component, whose record dies with the first border pixel that arrives; the rest go one atomic per
  // (wave, distinct root), the lanes of a root merged by a butterfly first.  Loop bound: as above, <= 64 passes of 6 shuffles.
  bool todo = root >= 0 && c != 0;
  if (todo) {
    const unsigned cur = __atomic_load_n(rec + base + root, __ATOMIC_RELAXED);
    if (hole_dead(cur) || hole_merge(cur, c) == cur) todo = false;
  }
  rem = __ballot(todo);
  while (rem) {
    const int r0 = __shfl(root, __ffsll((long long)rem) - 1);
    const bool mine = todo && root == r0;
    const u64 m = __ballot(mine);
    rem &= ~m;
    unsigned v = mine ? c : 0u;
#pragma unroll
    for (int sft = 32; sft; sft >>= 1) v = hole_merge(v, (unsigned)__shfl_xor((int)v, sft));
    if (lane == __ffsll((long long)m) - 1) hole_update(rec + base + r0, v);
  }
  __syncthreads();
  const unsigned h = s_hist[threadIdx.x];                                // one global atomic per (workgroup, label present in it)
  if (h) atomicAdd(hist + (size_t)blockIdx.y * 256 + threadIdx.x, h);
}

// (b) one frame; grid (ceil(H * W / 256)), block 256.  Launched only where the previous-frame rule can be active (overlap_q16 > 0
// and R exists).  cnt [H * W]: zeroed by the caller; cnt[root] = C, the pixels p of the hole with R[p] == o, for the holes that
// are candidates of a label o that R contains (pres) and that pass the size rule -- the others are never read.  One atomic per
// (wave, distinct root) with the wave's count: a hole receives one add per wave it has a pixel in, not one per pixel.
// Loop bound: every pass clears at least one bit: <= 64 passes.
__global__ __launch_bounds__(256) void hole_overlap_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ R,
                                                            const uint8_t* __restrict__ pres, const int* __restrict__ ids,
                                                            const int* __restrict__ area, const unsigned* __restrict__ rec,
                                                            const unsigned* __restrict__ hist, int n_pix, int max_area,
                                                            unsigned rel_q16, unsigned* __restrict__ cnt) {
  const int p = (int)(blockIdx.x * 256u + threadIdx.x), lane = threadIdx.x & 63;
  int root = -1;
  bool hit = false;
  if (p < n_pix && labels[p] == 0) {
    root = ids[p] - 1;
    const int o = hole_label(rec[root]);
    hit = o != 0 && pres[o] && R[p] == o && hole_size_ok(area[root], hist[o], max_area, rel_q16);
  }
  u64 rem = __ballot(hit);
  while (rem) {
    const int r0 = __shfl(root, __ffsll((long long)rem) - 1);
    const u64 m = __ballot(hit && root == r0);
    rem &= ~m;
    if (lane == __ffsll((long long)m) - 1) atomicAdd(cnt + r0, (unsigned)__popcll(m));
  }
}

// (c) grid (ceil(H * W / 256), frames), block 256.  pres: the labels R contains, null where the previous-frame rule is inactive
// for every label (overlap_q16 == 0 or no R; only then may frames > 1).  keep_all: the frames are copied unchanged.  pres_out
// [frame][256] and filled [frame]: zeroed by the caller.  Pixels filled: one LDS add per wave, one global atomic per workgroup.
__global__ __launch_bounds__(256) void hole_apply_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ ids,
                                                          const int* __restrict__ area, const unsigned* __restrict__ rec,
                                                          const unsigned* __restrict__ hist, const unsigned* __restrict__ cnt,
                                                          const uint8_t* __restrict__ pres, int keep_all, int n_pix, int max_area,
                                                          unsigned rel_q16, unsigned overlap_q16, uint8_t* __restrict__ out,
                                                          uint8_t* __restrict__ pres_out, u64* __restrict__ filled) {
  __shared__ unsigned s_filled;
  if (threadIdx.x == 0) s_filled = 0;
  __syncthreads();
  const int p = (int)(blockIdx.x * 256u + threadIdx.x);
  const int f = blockIdx.y;
  const size_t base = (size_t)f * n_pix;
  bool fill = false;
  if (p < n_pix) {
    int v = labels[base + p];
    if (v == 0 && !keep_all) {
      const int root = ids[base + p] - 1;
      const int o = hole_label(rec[base + root]);
      if (o != 0) {
        const int A = area[base + root];
        bool ok = hole_size_ok(A, hist[(size_t)f * 256 + o], max_area, rel_q16);
        if (ok && pres != nullptr && pres[o])
          ok = (u64)cnt[base + root] * 65536ull >= (u64)overlap_q16 * (u64)(unsigned)A;
        if (ok) { v = o; fill = true; }
      }
    }
    out[base + p] = (uint8_t)v;
    if (v && !pres_out[(size_t)f * 256 + v]) pres_out[(size_t)f * 256 + v] = 1;
  }
  const u64 z = __ballot(fill);
  if ((threadIdx.x & 63) == 0 && z) atomicAdd(&s_filled, (unsigned)__popcll(z));
  __syncthreads();
  if (threadIdx.x == 0 && s_filled) atomicAdd(filled + f, (u64)s_filled);
}
}  // namespace

template <bool ZERO>
static void ccl_label(const uint8_t* labels, int n_frames, int H, int W, int connectivity, int* parent, int* tarea, int* ids,
                      int* area, hipStream_t s) {
  const int conn8 = connectivity == 8, n_pix = H * W;
  const dim3 per_pixel((n_pix + 255) / 256, n_frames);
  hipLaunchKernelGGL(ccl_tile_kernel<ZERO>, dim3((W + CCL_TW - 1) / CCL_TW, (H + CCL_TH - 1) / CCL_TH, n_frames), dim3(256), 0, s,
                     labels, H, W, conn8, parent, tarea);
  hipLaunchKernelGGL(ccl_seam_kernel<ZERO>, per_pixel, dim3(256), 0, s, labels, H, W, conn8, parent);
  hipLaunchKernelGGL(ccl_flatten_kernel<ZERO>, per_pixel, dim3(256), 0, s, labels, n_pix, (const int*)parent, (const int*)tarea, ids, area);
}

void launch_ccl_label(const uint8_t* labels, int n_frames, int H, int W, int connectivity, int* parent, int* tarea, int* ids,
                      int* area, hipStream_t s) {
  ccl_label<false>(labels, n_frames, H, W, connectivity, parent, tarea, ids, area, s);
}

void launch_ccl_label_zero(const uint8_t* labels, int n_frames, int H, int W, int connectivity, int* parent, int* tarea, int* ids,
                           int* area, hipStream_t s) {
  ccl_label<true>(labels, n_frames, H, W, connectivity, parent, tarea, ids, area, s);
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

void launch_hole_scan(const uint8_t* labels, const int* ids, int n_frames, int H, int W, int connectivity, unsigned* rec,
                      unsigned* hist, hipStream_t s) {
  hipLaunchKernelGGL(hole_scan_kernel, dim3((H * W + 255) / 256, n_frames), dim3(256), 0, s, labels, ids, H, W,
                     connectivity == 4 ? 1 : 0, rec, hist);       // objects 4-connected: the background is 8-connected
}

void launch_hole_overlap(const uint8_t* labels, const uint8_t* R, const uint8_t* pres, const int* ids, const int* area,
                         const unsigned* rec, const unsigned* hist, int n_pix, int max_area, unsigned rel_q16, unsigned* cnt,
                         hipStream_t s) {
  hipLaunchKernelGGL(hole_overlap_kernel, dim3((n_pix + 255) / 256), dim3(256), 0, s, labels, R, pres, ids, area, rec, hist, n_pix,
                     max_area, rel_q16, cnt);
}

void launch_hole_apply(const uint8_t* labels, const int* ids, const int* area, const unsigned* rec, const unsigned* hist,
                       const unsigned* cnt, const uint8_t* pres, int keep_all, int n_frames, int n_pix, int max_area,
                       unsigned rel_q16, unsigned overlap_q16, uint8_t* out, uint8_t* pres_out, unsigned long long* filled,
                       hipStream_t s) {
  hipLaunchKernelGGL(hole_apply_kernel, dim3((n_pix + 255) / 256, n_frames), dim3(256), 0, s, labels, ids, area, rec, hist, cnt, pres,
                     keep_all, n_pix, max_area, rel_q16, overlap_q16, out, pres_out, filled);
}
}  // namespace eosvos
