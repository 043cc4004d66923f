// Block motion between consecutive uint8 frames by exhaustive matching on 8-bit luma, and the warp of label maps by the
// vectors, for gfx950.  The rules are stated in include/eosvos.h (eosvos_block_motion, eosvos_warp_labels) and restated in
// numpy by eosvos_amd/motion.py (vectors_host, warp_host).
//
// Luma planes live in engine scratch: plane p is [H][LS] bytes with LS = W rounded up to 4 (the padding columns are 0), so
// that every row starts on a word and a word of a row never straddles two rows.  Plane 0 is the frame before the call's
// first (prev_rgb), plane 1 + f frame f.
//   motion_luma_kernel       one launch: one thread per word of the planes, Y = (77 R + 150 G + 29 B + 128) >> 8
//   motion_search_kernel<B>  one launch: a workgroup owns a tile of 32 x 64 pixels = (32 / B) x (64 / B) blocks.  It stages the
//                            tile of Y_f (32 rows x 16 words) and the window of Y_{f-1} that the tile's candidates can reach
//                            in LDS: rows tile_y0 - R .. tile_y0 + 31 + R, columns from tile_x0 - Rp on with Rp = R rounded
//                            up to 4, 64 + 2 Rp + 4 bytes = at most 33 words a row, at most 96 rows; outside the frame the
//                            window holds 0.  Each of the four waves takes blocks in turn.  A lane takes a work item
//                            (dy, g): the four candidates (dy, dx) with dx = -Rp + 4 g + 0..3.  Window origin, block origin and
//                            4 g are multiples of 4, so the 8 bytes a packed quad-SAD needs are two ALIGNED words of a window
//                            row: per 4 bytes of a block row one v_qsad_pk_u16_u8 adds the four candidates' sums to four
//                            16-bit lanes (16 * 16 * 255 = 65280 fits).  A block cut by the right border (bw < B) takes the
//                            same words through v_alignbyte_b32 and a masked v_sad_u8 per candidate.  Candidates that
//                            leave the frame or the radius get the key ~0; every read stays inside the staged window
//                            whether the candidate is valid or not (bounds at the loops).  The wave reduces the 64-bit key
//                            cost << 26 | (dy^2 + dx^2) << 14 | (dy + 32) << 7 | (dx + 32) by an integer min; lane 0 writes
//                            the vector.
//   motion_warp_kernel       one launch: out(y, x) = lab(y + dy, x + dx), the read clamped to the frame
// Integer arithmetic only, no atomics: the result does not depend on any order.  No launch is cooperative, no workgroup waits
// for another; the bound of every loop is stated at the loop.  Vector stores only.
#include "kernels.h"

namespace eosvos {
namespace {
constexpr int MOT_TH = 32, MOT_TW = 64;                   // the tile of pixels a workgroup owns
constexpr int MOT_RMAX = 32;                              // the largest radius
constexpr int MOT_PW = (MOT_TW + 2 * MOT_RMAX + 4) / 4;   // 33 words: the stride of a window row (odd: rows shift banks)
constexpr int MOT_PH = MOT_TH + 2 * MOT_RMAX;             // 96 window rows at most
constexpr int MOT_CW = MOT_TW / 4;                        // 16 words per row of the current tile

typedef unsigned long long u64;

// grid (ceil(H * LW / 256), planes), block 256.  Plane blockIdx.y + first; plane 0 reads prev_rgb, plane p > 0 frame p - 1.
__global__ __launch_bounds__(256) void motion_luma_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ prev_rgb,
                                                           int first, int H, int W, int LW, unsigned* __restrict__ luma) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);   // H * LW <= 4096 * 1024 words
  if (i >= H * LW) return;
  const int p = first + (int)blockIdx.y;
  const size_t plane = (size_t)H * W;
  const uint8_t* src = p == 0 ? prev_rgb : rgb + (size_t)(p - 1) * 3 * plane;
  const int y = i / LW, xw = i - y * LW;
  unsigned word = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = 4 * xw + k;
    if (x < W) {
      const size_t q = (size_t)y * W + x;
      const unsigned v = (77u * src[q] + 150u * src[plane + q] + 29u * src[2 * plane + q] + 128u) >> 8;
      word |= v << (8 * k);
    }
  }
  luma[(size_t)p * H * LW + i] = word;
}

// grid (ceil(W / 64), ceil(H / 32), frames), block 256.  Frame first + blockIdx.z of the call: Y_f is plane f + 1, Y_{f-1} plane
// f.  No thread leaves before the wave reductions: the shuffles see whole waves.
template <int B>
__global__ __launch_bounds__(256) void motion_search_kernel(const unsigned* __restrict__ luma, int first, int H, int W, int LW, int R,
                                                             int bias, int by, int bx, int8_t* __restrict__ mv) {
  __shared__ unsigned s_prev[MOT_PH * MOT_PW];            // 12672 bytes
  __shared__ unsigned s_cur[MOT_TH * MOT_CW];             // 2048 bytes
  constexpr int TBX = MOT_TW / B, NBLK = (MOT_TH / B) * TBX, BWORDS = B / 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = first + (int)blockIdx.z;
  const size_t pwords = (size_t)H * LW;
  const unsigned* cur = luma + (size_t)(f + 1) * pwords;
  const unsigned* ref = luma + (size_t)f * pwords;
  const int tile_x0 = (int)blockIdx.x * MOT_TW, tile_y0 = (int)blockIdx.y * MOT_TH;
  const int Rp = (R + 3) & ~3;                            // <= 32
  const int oy = tile_y0 - R, oxw = (tile_x0 - Rp) / 4;   // the window's first row and first word column (a multiple of 4 pixels)
  const int nrows = MOT_TH + 2 * R;                       // <= 96
  const int pw = (MOT_TW + 2 * Rp + 4) / 4;               // words staged per window row, <= 33
  for (int i = tid; i < nrows * pw; i += 256) {           // <= 3168 words: <= 13 passes
    const int r = i / pw, c = i - r * pw;
    const int gy = oy + r, gw = oxw + c;
    s_prev[r * MOT_PW + c] = (gy >= 0 && gy < H && gw >= 0 && gw < LW) ? ref[(size_t)gy * LW + gw] : 0u;
  }
  for (int i = tid; i < MOT_TH * MOT_CW; i += 256) {      // 512 words: 2 passes
    const int r = i / MOT_CW, c = i - r * MOT_CW;
    const int gy = tile_y0 + r, gw = tile_x0 / 4 + c;
    s_cur[i] = (gy < H && gw < LW) ? cur[(size_t)gy * LW + gw] : 0u;
  }
  __syncthreads();
  const int G = Rp / 2 + 1;                               // groups of four dx: -Rp, -Rp + 4, .., Rp; <= 17
  const int items = (2 * R + 1) * G;                      // <= 65 * 17 = 1105
  for (int b = wave; b < NBLK; b += 4) {                  // NBLK = 8 or 32: 2 or 8 passes; everything about b is wave-uniform
    const int lby = b / TBX, lbx = b - lby * TBX;
    const int y0 = tile_y0 + lby * B, x0 = tile_x0 + lbx * B;
    if (y0 >= H || x0 >= W) continue;                     // no such block in this frame
    const int bh = min(B, H - y0), bw = min(B, W - x0);
    const int extra = bias * bh * bw;                     // <= 255 * 256
    const unsigned* crow = s_cur + lby * B * MOT_CW + lbx * BWORDS;
    u64 best = ~0ull;
    for (int base = 0; base < items; base += 64) {        // <= 18 passes
      const int want = base + lane;
      const int it = min(want, items - 1);                // lanes past the end repeat the last item and discard it
      const int dyi = it / G, g = it - dyi * G;           // dyi = dy + R in [0, 2 R], g in [0, G)
      // window row of block row r: y0 + dy + r - oy = lby * B + dyi + r <= 31 + 2 R < nrows; window word of block word c:
      // (x0 - Rp + 4 g + 4 c) / 4 - oxw = lbx * B / 4 + g + c, and one more for the quad: <= 16 + Rp / 2 = pw - 1
      const unsigned* prow = s_prev + (lby * B + dyi) * MOT_PW + lbx * BWORDS + g;
      unsigned cost[4];
      if (bw == B) {
        u64 acc = 0;
        for (int r = 0; r < bh; ++r) {                    // <= B rows
          const unsigned* p = prow + r * MOT_PW;
          const unsigned* c = crow + r * MOT_CW;
          unsigned lo = p[0];
#pragma unroll
          for (int k = 0; k < BWORDS; ++k) {
            const unsigned hi = p[k + 1];
            acc = __builtin_amdgcn_qsad_pk_u16_u8(((u64)hi << 32) | lo, c[k], acc);
            lo = hi;
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) cost[k] = (unsigned)(acc >> (16 * k)) & 0xffffu;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) cost[k] = 0;
        for (int r = 0; r < bh; ++r) {                    // <= B rows
          const unsigned* p = prow + r * MOT_PW;
          const unsigned* c = crow + r * MOT_CW;
          unsigned lo = p[0];
#pragma unroll
          for (int k = 0; k < BWORDS; ++k) {
            const unsigned hi = p[k + 1];
            const int nb = bw - 4 * k;                    // the block's bytes in this word
            const unsigned m = nb >= 4 ? 0xffffffffu : nb <= 0 ? 0u : (1u << (8 * nb)) - 1u;
            const unsigned a = c[k] & m;
            cost[0] = __builtin_amdgcn_sad_u8(lo & m, a, cost[0]);
            cost[1] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, 1) & m, a, cost[1]);
            cost[2] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, 2) & m, a, cost[2]);
            cost[3] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, 3) & m, a, cost[3]);
            lo = hi;
          }
        }
      }
      const int dy = dyi - R;
      const bool row_ok = want < items && y0 + dy >= 0 && y0 + bh + dy <= H;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int dx = -Rp + 4 * g + k;
        const bool ok = row_ok && dx >= -R && dx <= R && x0 + dx >= 0 && x0 + bw + dx <= W;
        const u64 c = (u64)(cost[k] + ((dy | dx) ? (unsigned)extra : 0u));
        const u64 key = (c << 26) | ((u64)(dy * dy + dx * dx) << 14) | ((u64)(dy + 32) << 7) | (u64)(dx + 32);
        if (ok && key < best) best = key;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {              // 6 steps: the wave's minimum in every lane
      const u64 other = __shfl_xor(best, off);
      best = other < best ? other : best;
    }
    if (lane == 0) {                                      // (0, 0) is always valid: best is a key
      int8_t* out = mv + (((size_t)f * by + (y0 / B)) * bx + (x0 / B)) * 2;
      out[0] = (int8_t)((int)((best >> 7) & 127) - 32);
      out[1] = (int8_t)((int)(best & 127) - 32);
    }
  }
}

// grid (ceil(W / 64), ceil(H / 16), frames), block 256: one wave-wide row segment, 4 rows per wave.
__global__ __launch_bounds__(256) void motion_warp_kernel(const uint8_t* __restrict__ labels, const int8_t* __restrict__ mv, int H, int W,
                                                           int B, int by, int bx, uint8_t* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t f = blockIdx.z, plane = (size_t)H * W;
  const int x = (int)blockIdx.x * 64 + lane;
  if (x >= W) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = (int)blockIdx.y * 16 + wave + 4 * k;
    if (y >= H) continue;
    const int8_t* d = mv + ((f * by + (y / B)) * bx + (x / B)) * 2;
    const int sy = min(max(y + (int)d[0], 0), H - 1), sx = min(max(x + (int)d[1], 0), W - 1);
    out[f * plane + (size_t)y * W + x] = labels[f * plane + (size_t)sy * W + sx];
  }
}
}  // namespace

void launch_motion_luma(const uint8_t* rgb, const uint8_t* prev_rgb, int n_frames, int H, int W, unsigned* luma, hipStream_t s) {
  const int LW = (W + 3) / 4, first = prev_rgb ? 0 : 1;
  hipLaunchKernelGGL(motion_luma_kernel, dim3((H * LW + 255) / 256, n_frames + 1 - first), dim3(256), 0, s, rgb, prev_rgb, first, H, W,
                     LW, luma);
}

void launch_motion_search(const unsigned* luma, int first, int n_frames, int H, int W, int block, int radius, int bias, int8_t* mv,
                          hipStream_t s) {
  if (first >= n_frames) return;
  const int LW = (W + 3) / 4, by = (H + block - 1) / block, bx = (W + block - 1) / block;
  const dim3 grid((W + MOT_TW - 1) / MOT_TW, (H + MOT_TH - 1) / MOT_TH, n_frames - first);
  if (block == 8)
    hipLaunchKernelGGL(motion_search_kernel<8>, grid, dim3(256), 0, s, luma, first, H, W, LW, radius, bias, by, bx, mv);
  else
    hipLaunchKernelGGL(motion_search_kernel<16>, grid, dim3(256), 0, s, luma, first, H, W, LW, radius, bias, by, bx, mv);
}

void launch_motion_warp(const uint8_t* labels, const int8_t* mv, int n_frames, int H, int W, int block, uint8_t* out, hipStream_t s) {
  const int by = (H + block - 1) / block, bx = (W + block - 1) / block;
  hipLaunchKernelGGL(motion_warp_kernel, dim3((W + 63) / 64, (H + 15) / 16, n_frames), dim3(256), 0, s, labels, mv, H, W, block, by, bx, out);
}
}  // namespace eosvos
