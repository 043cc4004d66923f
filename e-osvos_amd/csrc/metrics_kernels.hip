// DAVIS-2017 region / contour counts on the device (the reference's evaluation: evaluate.py:345-359 -> eval_davis_seq,
// helper_func.py:444-458, which runs the `davis` package's J and F measures per sequence and object).
//
// The kernels produce integer counts only; every ratio and statistic is computed on the host in float64 (data.py).
// Per (frame f, object o), with P = (pred == o), G = (gt == o) and label values above n_obj belonging to no object:
//   inter = |P & G|, union = |P | G|                                     (J = inter / union, 1 if union = 0)
//   n_fg = |bmap(P)|, n_gt = |bmap(G)|
//   fg_match = |bmap(P) & dilate(bmap(G))|, gt_match = |bmap(G) & dilate(bmap(P))|
// bmap(S) is the `davis` package's seg2bmap: b = S^E | S^Sd | S^SE with E, Sd, SE = S shifted one pixel from the right,
// below and below-right (zero-filled); on the last row b = S^E, on the last column b = S^Sd, and b = 0 at the corner.
// dilate(.) is a binary dilation by the disk {dx^2 + dy^2 <= r^2}, everything outside the frame being 0.
//
// Launch A (davis_bmap_kernel): one wave per image row; for every object the boundary bits of P and G are formed
// 64 pixels at a time with __ballot and stored bit-packed ([f][o][y][word], ceil(W/64) words per row), and inter /
// union / n_fg / n_gt are popcounted.  Launch B (davis_match_kernel): one wave per row, one lane per 64-bit word
// (W <= 4096): the other map's rows y-r .. y+r are dilated horizontally by floor(sqrt(r^2 - dy^2)) (a shift-or over the
// word and its two neighbours, enough for r <= 63), OR-ed together, AND-ed with this map's row and popcounted.
// Counts are integers, so the order of the atomic sums does not matter.
#include "kernels.h"

namespace eosvos {

namespace {
constexpr int DAVIS_WAVES = 4;           // waves per workgroup
constexpr int DAVIS_ROWS = 16;           // image rows per workgroup (4 per wave)

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// OR of the word shifted towards higher pixels by 0..k (lo = the word of lower pixels) / towards lower pixels by 0..k
// (hi = the word of higher pixels); bit j of a word is pixel 64 * word + j.  k <= 63.
__device__ __forceinline__ unsigned long long spread(unsigned long long lo, unsigned long long c, unsigned long long hi, int k) {
  unsigned __int128 up = ((unsigned __int128)c << 64) | lo;
  unsigned __int128 dn = ((unsigned __int128)hi << 64) | c;
  for (int cov = 1; cov <= k;) {          // shifts 0 .. cov-1 are covered
    const int s = cov < k + 1 - cov ? cov : k + 1 - cov;
    up |= up << s;
    dn |= dn >> s;
    cov += s;
  }
  return (unsigned long long)(up >> 64) | (unsigned long long)dn;
}
}  // namespace

// grid (ceil(H / DAVIS_ROWS), frames), block 64 * DAVIS_WAVES; lds: 4 * n_obj unsigned
__global__ __launch_bounds__(64 * DAVIS_WAVES) void davis_bmap_kernel(
    const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int H, int W, int nw, int n_obj,
    unsigned long long* __restrict__ bmp, unsigned long long* __restrict__ bmg, long long* __restrict__ counts) {
  extern __shared__ unsigned sacc[];     // [n_obj][4]: inter, union, n_fg, n_gt of this workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.y;
  for (int i = threadIdx.x; i < 4 * n_obj; i += blockDim.x) sacc[i] = 0;
  __syncthreads();
  const size_t plane = (size_t)H * W;
  const uint8_t* P = pred + (size_t)f * plane;
  const uint8_t* G = gt + (size_t)f * plane;
  const int y_end = min(H, (int)(blockIdx.x + 1) * DAVIS_ROWS);
  for (int y = blockIdx.x * DAVIS_ROWS + wave; y < y_end; y += DAVIS_WAVES) {
    const bool last_row = y == H - 1;
    const uint8_t* p0 = P + (size_t)y * W;
    const uint8_t* g0 = G + (size_t)y * W;
    for (int w = 0; w < nw; ++w) {
      const int x = w * 64 + lane;
      const bool in = x < W, right = x + 1 < W, last_col = x == W - 1;
      // 0 is never an object id, so it stands for "outside the frame"
      const int ps = in ? p0[x] : 0, pe = right ? p0[x + 1] : 0;
      const int pd = in && !last_row ? p0[x + W] : 0, pse = right && !last_row ? p0[x + W + 1] : 0;
      const int gs = in ? g0[x] : 0, ge = right ? g0[x + 1] : 0;
      const int gd = in && !last_row ? g0[x + W] : 0, gse = right && !last_row ? g0[x + W + 1] : 0;
      for (int o = 1; o <= n_obj; ++o) {
        const bool S = ps == o, E = pe == o, D = pd == o, SE = pse == o;
        const bool T = gs == o, TE = ge == o, TD = gd == o, TSE = gse == o;
        bool bp, bg;
        if (last_row && last_col) {
          bp = bg = false;
        } else if (last_row) {
          bp = S != E; bg = T != TE;
        } else if (last_col) {
          bp = S != D; bg = T != TD;
        } else {
          bp = (S != E) || (S != D) || (S != SE);
          bg = (T != TE) || (T != TD) || (T != TSE);
        }
        const unsigned long long wp = __ballot(bp), wg = __ballot(bg);
        const unsigned long long wi = __ballot(S && T), wu = __ballot(S || T);
        if (lane == 0) {
          const size_t row = (((size_t)f * n_obj + (o - 1)) * H + y) * nw + w;
          bmp[row] = wp;
          bmg[row] = wg;
          unsigned* a = sacc + 4 * (o - 1);
          if (wi) atomicAdd(a + 0, (unsigned)__popcll(wi));
          if (wu) atomicAdd(a + 1, (unsigned)__popcll(wu));
          if (wp) atomicAdd(a + 2, (unsigned)__popcll(wp));
          if (wg) atomicAdd(a + 3, (unsigned)__popcll(wg));
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * n_obj; i += blockDim.x)
    if (sacc[i]) atomicAdd((unsigned long long*)(counts + ((size_t)f * n_obj + i / 4) * 6 + i % 4), (unsigned long long)sacc[i]);
}

// grid (ceil(H / DAVIS_ROWS), n_obj, frames), block 64 * DAVIS_WAVES
__global__ __launch_bounds__(64 * DAVIS_WAVES) void davis_match_kernel(
    const unsigned long long* __restrict__ bmp, const unsigned long long* __restrict__ bmg, int H, int nw, int n_obj, int r,
    long long* __restrict__ counts) {
  __shared__ unsigned long long sm[DAVIS_WAVES][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int o = blockIdx.y, f = blockIdx.z;
  const size_t base = ((size_t)f * n_obj + o) * H * nw;
  const unsigned long long* BP = bmp + base;
  const unsigned long long* BG = bmg + base;
  const bool in = lane < nw;
  unsigned long long fg = 0, gm = 0;      // per lane: |P & dil(G)|, |G & dil(P)| of this wave's rows
  const int y_end = min(H, (int)(blockIdx.x + 1) * DAVIS_ROWS);
  for (int y = blockIdx.x * DAVIS_ROWS + wave; y < y_end; y += DAVIS_WAVES) {
    const unsigned long long p = in ? BP[(size_t)y * nw + lane] : 0, g = in ? BG[(size_t)y * nw + lane] : 0;
    if (__ballot((p | g) != 0) == 0) continue;       // no boundary pixel of either map on this row
    unsigned long long dp = 0, dg = 0;
    const int y0 = max(0, y - r), y1 = min(H - 1, y + r);
    for (int yy = y0; yy <= y1; ++yy) {
      const int dy = yy - y, q = r * r - dy * dy;
      int k = (int)sqrtf((float)q);
      while (k * k > q) --k;
      while ((k + 1) * (k + 1) <= q) ++k;
      const unsigned long long cp = in ? BP[(size_t)yy * nw + lane] : 0, cg = in ? BG[(size_t)yy * nw + lane] : 0;
      const unsigned long long lp = __shfl_up(cp, 1), hp = __shfl_down(cp, 1);
      const unsigned long long lg = __shfl_up(cg, 1), hg = __shfl_down(cg, 1);
      dp |= spread(lane > 0 ? lp : 0, cp, lane < 63 ? hp : 0, k);
      dg |= spread(lane > 0 ? lg : 0, cg, lane < 63 ? hg : 0, k);
    }
    fg += (unsigned long long)__popcll(p & dg);
    gm += (unsigned long long)__popcll(g & dp);
  }
  fg = wave_sum(fg);
  gm = wave_sum(gm);
  if (lane == 0) { sm[wave][0] = fg; sm[wave][1] = gm; }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long t = 0;
    for (int i = 0; i < DAVIS_WAVES; ++i) t += sm[i][threadIdx.x];
    if (t) atomicAdd((unsigned long long*)(counts + ((size_t)f * n_obj + o) * 6 + 4 + threadIdx.x), t);
  }
}

void launch_davis_counts(const uint8_t* pred, const uint8_t* gt, int frames, int H, int W, int n_obj, int r,
                         unsigned long long* bmp, unsigned long long* bmg, int64_t* counts, hipStream_t s) {
  const int nw = (W + 63) / 64;
  const unsigned rb = (unsigned)((H + DAVIS_ROWS - 1) / DAVIS_ROWS);
  hipLaunchKernelGGL(davis_bmap_kernel, dim3(rb, frames), dim3(64 * DAVIS_WAVES), 4 * n_obj * sizeof(unsigned), s,
                     pred, gt, H, W, nw, n_obj, bmp, bmg, (long long*)counts);
  hipLaunchKernelGGL(davis_match_kernel, dim3(rb, n_obj, frames), dim3(64 * DAVIS_WAVES), 0, s,
                     bmp, bmg, H, nw, n_obj, r, (long long*)counts);
}

}  // namespace eosvos
