// Implicit-GEMM convolution kernels for gfx950 (MI355X) on the fp32 matrix cores.
//
// All three conv passes of the fine-tuning step (forward, data gradient, weight
// gradient) are dense fp32 contractions; on CDNA4 the fp32 MFMA
// (v_mfma_f32_32x32x2_f32) runs at the fp32 vector peak but needs one VGPR per operand
// per lane and leaves the VALU free for address generation and the fused epilogues, so
// every contraction here is tiled for it: 128 x {128,64} output tile per 256-thread
// workgroup, four 64-lane waves in a 2x2 arrangement, each wave owning a
// 64 x {64,32} sub-tile = 2 x {2,1} accumulators of 32x32 (f32x16 per lane).
// Operands are gathered global -> registers -> LDS (double buffered, one barrier per
// 32-deep K step, next tile's loads in flight behind the current tile's MFMAs); LDS rows
// are padded by one 16-byte access so the ds_read_b128 fragment reads are conflict free.
//
// NHWC activations make the K dimension (input channels of one filter tap) contiguous for
// the gathered operand, so no im2col buffer is ever materialised and 1x1, 3x3, dilated
// and strided convolutions (and their data gradients, through the fractional-stride
// gather) are the same kernel.  The same kernels also run the batched GEMMs of the
// Winograd-domain convolutions (ConvArgs::plane_rows, WgradArgs::*_tap_stride; transforms
// in misc_kernels.hip, selection in engine.cpp wino_on()).
#include "kernels.h"
#include "conv_tile.h"

#include <stdlib.h>
#include <string.h>

#include <type_traits>
#include <vector>

namespace eosvos {

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define EOSVOS_BK 32
#define EOSVOS_EB 4   // epilogue rows whose global operands are requested together
#define EOSVOS_EB128 EOSVOS_EB      // rows per batch in the 128-wide kernels (their accumulators are dead here: registers to spare)
#define EOSVOS_OCC 2
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// Work decomposition ("stream-K"): the launch has nwg workgroups (<= 2 per CU, all resident);
// the tiles x K-steps work units are dealt out in equal contiguous runs of `per` units, so a
// workgroup walks through a few whole tiles plus at most one partial tile at each end of its
// run.  Whole tiles get the fused epilogue directly; partial tiles are parked as raw fp32
// slabs (ws[wg][0|1][BM][BN]) and conv_fixup_kernel sums them in workgroup order
// (deterministic) and applies the epilogue.  This removes the 59-78 % wave-quantisation loss
// a tile-per-workgroup grid has on 256 CUs for this network's shapes.
// DEEP != 0: half the LDS and a smaller register budget so that 3 workgroups fit a CU -- 3 waves per SIMD keep
// the MFMA pipe busier on long-K, many-tile launches (decoder 3x3: +3-5 %) but lose on short or small ones, so
// conv_plan selects it per launch (ConvArgs::deep).  DEEP = 1: one LDS stage of K = 32 (two barriers per K
// step); DEEP = 2: two stages of K = 16, for channel counts that are not a multiple of 32 (304: no padded step).
#define EOSVOS_BK_DEEP 16
#define EOSVOS_DEEP_TILES 1024
template <int BN, bool KMAJOR, int DEEP = 0>
__global__ __launch_bounds__(256, DEEP ? 3 : EOSVOS_OCC) void conv_igemm_kernel(const ConvArgs p) {
  constexpr int BM = 128, BK = DEEP == 2 ? EOSVOS_BK_DEEP : EOSVOS_BK;
  constexpr int LDA = BK + 4;
  constexpr int LDB = KMAJOR ? BN + 4 : BK + 4;
  constexpr int A_EL = BM * LDA;
  constexpr int B_EL = KMAJOR ? BK * LDB : BN * LDB;
  constexpr int STAGE = A_EL + B_EL;
  constexpr int LDC = BN + 4;
  constexpr int NBUF = DEEP == 1 ? 1 : 2;
  constexpr int EPASS = (BM * LDC <= NBUF * STAGE) ? 1 : 2;      // C-tile staging passes
  constexpr int EROWS = BM / EPASS;
  static_assert(EROWS * LDC <= NBUF * STAGE, "epilogue staging must fit the operand buffers");
  __shared__ __attribute__((aligned(16))) float smem[NBUF * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;

  const int T = p.KH * p.KW;
  const int chunks = (p.Kc + BK - 1) / BK;
  const int ksteps = T * chunks;
  const int nt = (p.N + BN - 1) / BN;
  const int tiles = ((p.M + BM - 1) / BM) * nt;
  // tprefix != null: per-tile list of the K steps that can contribute (filter taps that fall wholly
  // into the padding for every pixel of the tile are dropped -- dilated 3x3 convs on the 30x54 map);
  // units are then counted in that compacted space
  const long U = p.tprefix ? (long)p.tprefix[tiles] : (long)tiles * ksteps;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  // data-parallel part: dp_q whole tiles per workgroup; stream-K part: `per` units of the rest
  const long sk0 = (long)p.dp_q * gridDim.x * ksteps;
  const long u_begin = sk0 + (long)bid * p.per;
  long u_end = u_begin + p.per;
  if (u_end > U) u_end = U;
  int dp_i = 0;

  constexpr int AF4 = BK / 4, AROWS = 256 / AF4, APASS = BM / AROWS;   // 8, 32, 4
  const int a_c4 = tid % AF4, a_r = tid / AF4;
  constexpr int BF4 = KMAJOR ? BN / 4 : BK / 4;
  constexpr int BROWS = 256 / BF4;
  constexpr int BPASS = (KMAJOR ? BK : BN) / BROWS;
  const int b_c4 = tid % BF4, b_r = tid / BF4;
  const int up = 1 << p.upshift;
  constexpr int TN = BN / 64;
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, (long)p.B * p.Hi * p.Wi * p.ldx * 4);
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, (p.plane_rows ? (long)p.nplanes : 1L) * p.wN * T * p.wK * 4);

  for (long u = u_begin;;) {
    int tile, ks_begin, ks_end = ksteps;
    const bool dp = dp_i < p.dp_q;
    if (dp) {
      tile = dp_i * (int)gridDim.x + bid;      // neighbouring workgroups (one XCD) work on neighbouring tiles at the same time: shared operand rows meet in L2
      ks_begin = 0;
      ++dp_i;
      if (tile >= tiles) continue;
    } else if (u < u_end) {
      if (p.tprefix) {
        int lo = 0, hi = tiles - 1;                 // last tile with tprefix[tile] <= u
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if ((long)p.tprefix[mid] <= u) lo = mid; else hi = mid - 1;
        }
        tile = lo;
        ks_begin = (int)(u - p.tprefix[tile]);
        ks_end = p.tprefix[tile + 1] - p.tprefix[tile];
      } else {
        tile = (int)(u / ksteps);
        ks_begin = (int)(u - (long)tile * ksteps);
      }
      if ((long)ks_end - ks_begin > u_end - u) ks_end = ks_begin + (int)(u_end - u);
    } else {
      break;
    }
    const int ks_total = p.tprefix ? p.tprefix[tile + 1] - p.tprefix[tile] : ksteps;
    // valid taps of this tile packed 4 bits each (tap-major K order inside a tile)
    unsigned long long tappack = 0x876543210ULL;
    if (p.tprefix) {
      const int mask = p.tmask[tile];
      tappack = 0;
      int nv = 0;
      for (int t2 = 0; t2 < T; ++t2)
        if ((mask >> t2) & 1) { tappack |= (unsigned long long)t2 << (4 * nv); ++nv; }
    }
    const int m0 = (tile / nt) * BM, n0 = (tile % nt) * BN;

    int a_sy0[APASS], a_sx0[APASS], a_img[APASS];
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
      int m = m0 + a_r + i * AROWS;
      if (m < p.M) {
        if (p.par) m = conv_par_pixel(p.B, p.Ho, p.Wo, m);
        const int hw = p.Ho * p.Wo;
        const int b = m / hw, rem = m - b * hw;
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        a_sy0[i] = oy * p.mul + p.off0;
        a_sx0[i] = ox * p.mul + p.off0;
        a_img[i] = b * p.Hi * p.Wi;
      } else {
        a_sy0[i] = -(1 << 28);
        a_sx0[i] = 0;
        a_img[i] = 0;
      }
    }
    float4 ra[APASS], rb[BPASS];
    // Gather offsets (in floats, without the channel-chunk term) are cached per filter tap
    // and re-derived only when the tap changes; loads are buffer loads whose hardware range
    // check returns 0 for the deliberately out-of-range offset of padded / masked elements,
    // so the K loop carries no divergent branches and ~10x less address arithmetic.
    constexpr unsigned OOB = 0x80000000u;
    int a_off[APASS];
    int b_off[BPASS];   // weight offset without the (tap, chunk) term, or -1
    const int wplane = p.plane_rows ? (m0 / p.plane_rows) * (int)p.w_plane : 0;     // batched GEMM: this tile's weights
#pragma unroll
    for (int i = 0; i < BPASS; ++i) {
      if (KMAJOR) {
        const int n = n0 + b_c4 * 4;
        b_off[i] = n < p.N ? wplane + (b_r + i * BROWS) * T * p.wK + n : -1;
      } else {
        const int n = n0 + b_r + i * BROWS;
        b_off[i] = n < p.N ? wplane + n * T * p.wK + b_c4 * 4 : -1;
      }
    }
    int cur_tap = -1;
    auto load_tiles = [&](int ks) {
      const int vt = ks / chunks;
      const int c0 = (ks - vt * chunks) * BK;
      const int tap = p.tprefix ? (int)((tappack >> (4 * vt)) & 15) : vt;
      if (tap != cur_tap) {          // wave-uniform
        cur_tap = tap;
        const int ky = tap / p.KW, kx = tap - ky * p.KW;
        const int dy = ky * p.kstep, dx = kx * p.kstep;
#pragma unroll
        for (int i = 0; i < APASS; ++i) {
          const int sy = a_sy0[i] + dy, sx = a_sx0[i] + dx;
          bool ok = sy >= 0 && sx >= 0 && ((sy | sx) & (up - 1)) == 0;
          const int iy = sy >> p.upshift, ix = sx >> p.upshift;
          ok = ok && iy < p.Hi && ix < p.Wi;
          a_off[i] = ok ? (a_img[i] + iy * p.Wi + ix) * p.ldx + a_c4 * 4 : -1;
        }
      }
      const bool cok = (c0 + a_c4 * 4) < p.Kc;
      float4 ks4 = make_float4(1.f, 1.f, 1.f, 1.f);
      if (KMAJOR && p.kscale && cok) ks4 = ldg4(p.kscale + c0 + a_c4 * 4);
#pragma unroll
      for (int i = 0; i < APASS; ++i) {
        const unsigned off = (cok && a_off[i] >= 0) ? (unsigned)(a_off[i] + c0) * 4u : OOB;
        float4 v = bufld4(rx, off);
        if (KMAJOR) { v.x *= ks4.x; v.y *= ks4.y; v.z *= ks4.z; v.w *= ks4.w; }
        ra[i] = v;
      }
#pragma unroll
      for (int i = 0; i < BPASS; ++i) {
        unsigned off;
        if (KMAJOR) {
          const int k = c0 + b_r + i * BROWS;
          off = (b_off[i] >= 0 && k < p.Kc) ? (unsigned)(b_off[i] + (c0 * T + tap) * p.wK) * 4u : OOB;
        } else {
          const int k = c0 + b_c4 * 4;
          off = (b_off[i] >= 0 && k < p.Kc) ? (unsigned)(b_off[i] + tap * p.wK + c0) * 4u : OOB;
        }
        rb[i] = bufld4(rw, off);
      }
    };
    auto store_tiles = [&](int buf) {
      float* As = smem + buf * STAGE;
      float* Bs = As + A_EL;
#pragma unroll
      for (int i = 0; i < APASS; ++i)
        *reinterpret_cast<float4*>(As + (a_r + i * AROWS) * LDA + a_c4 * 4) = ra[i];
#pragma unroll
      for (int i = 0; i < BPASS; ++i)
        *reinterpret_cast<float4*>(Bs + (b_r + i * BROWS) * LDB + b_c4 * 4) = rb[i];
    };

    f32x16 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    load_tiles(ks_begin);
    __syncthreads();            // previous segment's epilogue reads of smem are done
    store_tiles(0);
    __syncthreads();

    for (int ks = ks_begin; ks < ks_end; ++ks) {
      const int buf = NBUF == 2 ? (ks - ks_begin) & 1 : 0;
      const bool more = (ks + 1) < ks_end;
      if (more) load_tiles(ks + 1);          // global loads in flight behind the MFMAs below
      const float* As = smem + buf * STAGE;
      const float* Bs = As + A_EL;
#pragma unroll
      for (int kk = 0; kk < BK / 8; ++kk) {
        float4 a4[2];
        float bv[TN][4];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
          a4[tm] = *reinterpret_cast<const float4*>(As + (wm * 64 + tm * 32 + r) * LDA + kk * 8 + h * 4);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          if (KMAJOR) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              bv[tn][j] = Bs[(kk * 8 + h * 4 + j) * LDB + wn * (BN / 2) + tn * 32 + r];
          } else {
            const float4 t = *reinterpret_cast<const float4*>(Bs + (wn * (BN / 2) + tn * 32 + r) * LDB + kk * 8 + h * 4);
            bv[tn][0] = t.x; bv[tn][1] = t.y; bv[tn][2] = t.z; bv[tn][3] = t.w;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int tm = 0; tm < 2; ++tm) {
            const float av = j == 0 ? a4[tm].x : j == 1 ? a4[tm].y : j == 2 ? a4[tm].z : a4[tm].w;
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = MFMA32(av, bv[tn][j], acc[tm][tn]);
          }
        }
      }
      if (NBUF == 1) __syncthreads();         // every wave is done reading the single stage
      if (more) store_tiles(NBUF == 2 ? buf ^ 1 : 0);
      __syncthreads();
    }

    // ---- epilogue: accumulators -> LDS tile -> full-row float4 stores ------------------------
    // With a short BK the operand buffers are smaller than the C tile: it is then staged in two
    // passes of 64 rows (pass ep holds the tm == ep half of every wave's rows).
    float* Cs = smem;
    const bool full = (ks_begin == 0 && ks_end == ks_total);
    constexpr int CF4 = BN / 4, CROWS = 256 / CF4;
    const int c_c4 = tid % CF4, c_r = tid / CF4;
    const int n = n0 + c_c4 * 4;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), bi = make_float4(0.f, 0.f, 0.f, 0.f);
    if (full && n < p.N) {
      if (p.scale) sc = ldg4(p.scale + n);
      if (p.bias) bi = ldg4(p.bias + n);
    }
    const bool use_mask8 = p.mask8 && n >= p.mask_c0;
    const bool write_m8 = p.mask8_out && p.relu;
#pragma unroll
    for (int ep = 0; ep < EPASS; ++ep) {
      if (ep) __syncthreads();
#pragma unroll
      for (int tm = 0; tm < 2; ++tm) {
        if (EPASS == 2 && tm != ep) continue;
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
          for (int e = 0; e < 16; ++e)
            Cs[((EPASS == 1 ? wm * 64 + tm * 32 : wm * 32) + (e & 3) + 8 * (e >> 2) + 4 * h) * LDC + wn * (BN / 2) +
               tn * 32 + r] = acc[tm][tn][e];
      }
      __syncthreads();
      // staged row lr of this pass is tile row trow(lr)
      auto trow = [&](int lr) { return EPASS == 1 ? lr : ((lr >> 5) << 6) + (ep << 5) + (lr & 31); };
      if (full) {
        if (n < p.N) {
          // All global operands of a batch of rows are requested before any is consumed: the epilogue of
          // the short-K layers is latency bound, and one dependent load per row left the HBM pipe empty.
          constexpr int NIT = EROWS / CROWS, EB = DEEP == 1 ? 1 : (DEEP == 2 ? 2 : EOSVOS_EB);
#pragma unroll
          for (int it0 = 0; it0 < NIT; it0 += EB) {
            size_t md[EB];
            bool ok[EB];
            float4 rs[EB], ac[EB];
            unsigned mk8[EB];                 // ReLU mask bits of the row's 4 channels
#pragma unroll
            for (int j = 0; j < EB; ++j) {
              const int m = m0 + trow(c_r + (it0 + j) * CROWS);
              ok[j] = m < p.M;
              md[j] = dst_pixel(p, ok[j] ? m : p.M - 1);
            }
            if (p.res) {
#pragma unroll
              for (int j = 0; j < EB; ++j) rs[j] = ldg4(p.res + md[j] * p.ldres + n);
            }
            if (p.accum) {
#pragma unroll
              for (int j = 0; j < EB; ++j) ac[j] = ldg4(p.y + md[j] * p.ldy + n);
            }
            if (use_mask8) {
#pragma unroll
              for (int j = 0; j < EB; ++j) mk8[j] = p.mask8[md[j] * p.ldm8 + (n >> 2)];
            }
#pragma unroll
            for (int j = 0; j < EB; ++j) {
              float4 v = *reinterpret_cast<const float4*>(Cs + (c_r + (it0 + j) * CROWS) * LDC + c_c4 * 4);
              if (p.scale) { v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w; }
              if (p.bias) { v.x += bi.x; v.y += bi.y; v.z += bi.z; v.w += bi.w; }
              if (p.res) { v.x += rs[j].x; v.y += rs[j].y; v.z += rs[j].z; v.w += rs[j].w; }
              if (p.accum) { v.x += ac[j].x; v.y += ac[j].y; v.z += ac[j].z; v.w += ac[j].w; }
              if (p.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
              if (use_mask8) relu_mask8(v, mk8[j]);
              if (ok[j]) {
                *reinterpret_cast<float4*>(p.y + md[j] * p.ldy + n) = v;
                if (write_m8) p.mask8_out[md[j] * p.ldm8_out + (n >> 2)] = relu_bits(v);
              }
            }
          }
        }
      } else {
        float* slab = p.ws + ((size_t)bid * 2 + (u == u_begin ? 0 : 1)) * (BM * BN);
#pragma unroll 4
        for (int lr = c_r; lr < EROWS; lr += CROWS)
          *reinterpret_cast<float4*>(slab + trow(lr) * BN + c_c4 * 4) =
              *reinterpret_cast<const float4*>(Cs + lr * LDC + c_c4 * 4);
      }
    }
    if (!dp) u += ks_end - ks_begin;
  }
}

// Sum the parked partial tiles in workgroup order and apply the fused epilogue.
template <int BN>
__global__ __launch_bounds__(256) void conv_fixup_kernel(const ConvArgs p) {
  constexpr int BM = 128;
  const int BK = p.deep == 2 ? EOSVOS_BK_DEEP : EOSVOS_BK;
  const int T = p.KH * p.KW;
  const int ksteps = T * ((p.Kc + BK - 1) / BK);
  const int nt = (p.N + BN - 1) / BN;
  const int tile = p.dp_q * p.nwg + blockIdx.x;
  const long sk0 = (long)p.dp_q * p.nwg * ksteps;
  const long a = p.tprefix ? (long)p.tprefix[tile] : (long)tile * ksteps;
  const long b = p.tprefix ? (long)p.tprefix[tile + 1] : a + ksteps;
  // contributors: stream-K -- the workgroups g0..g1 whose unit runs touch the tile; split-K -- workgroups c * tiles + tile
  const int tiles_all = ((p.M + BM - 1) / BM) * nt;
  int g0 = 0, g1 = p.splitk - 1;
  if (p.splitk == 0) {
    g0 = (int)((a - sk0) / p.per); g1 = (int)((b - 1 - sk0) / p.per);
    if (g0 == g1) return;                       // computed whole by one workgroup
  }
  const int m0 = (tile / nt) * BM, n0 = (tile % nt) * BN;
  constexpr int CF4 = BN / 4, CROWS = 256 / CF4;
  const int c_c4 = threadIdx.x % CF4, c_r = threadIdx.x / CF4;
  const bool act = n0 + c_c4 * 4 < p.N;          // threads past the last column only take part in the absmax reduction
  const int n = act ? n0 + c_c4 * 4 : n0;
  // blockIdx.y selects one eighth of the tile's rows (more, shorter workgroups: the sum is latency
  // bound); every global operand of the thread's rows is requested before the first is consumed
  constexpr int RPB = BM / 8 / CROWS;          // rows per thread: 2 (BN = 128) or 1 (BN = 64)
  float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), bi = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p.scale) sc = ldg4(p.scale + n);
  if (p.bias) bi = ldg4(p.bias + n);
  const float y2s = p.y2 ? *p.y2_sc : 0.f;       // requested with the other operands, consumed after the slab sums
  const bool use_mask8 = p.mask8 && n >= p.mask_c0;
  size_t md[RPB];
  unsigned mk8[RPB];
  bool ok[RPB];
  int rows[RPB];
  float4 rs[RPB], ac[RPB], sum[RPB];
#pragma unroll
  for (int j = 0; j < RPB; ++j) {
    rows[j] = blockIdx.y * (BM / 8) + c_r + j * CROWS;
    const int m = m0 + rows[j];
    ok[j] = act && m < p.M;
    md[j] = dst_pixel(p, ok[j] ? m : p.M - 1);
    sum[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.res) rs[j] = ldg4(p.res + md[j] * p.ldres + n);
    if (p.accum) ac[j] = ldg4(p.y + md[j] * p.ldy + n);
    if (use_mask8) mk8[j] = p.mask8[md[j] * p.ldm8 + (n >> 2)];
  }
  for (int g = g0; g <= g1; g += 4) {
    float4 t[4][RPB];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gc = g + i <= g1 ? g + i : g1;
      const int gi = p.splitk ? gc * tiles_all + tile : gc;
      const int slot = (p.splitk || sk0 + (long)gi * p.per >= a) ? 0 : 1;
#pragma unroll
      for (int j = 0; j < RPB; ++j)
        t[i][j] = ldg4(p.ws + ((size_t)gi * 2 + slot) * (BM * BN) + rows[j] * BN + c_c4 * 4);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (g + i > g1) break;
#pragma unroll
      for (int j = 0; j < RPB; ++j) { sum[j].x += t[i][j].x; sum[j].y += t[i][j].y; sum[j].z += t[i][j].z; sum[j].w += t[i][j].w; }
    }
  }
  unsigned ymax = 0;
#pragma unroll
  for (int j = 0; j < RPB; ++j) {
    if (!ok[j]) continue;
    float4 v = sum[j];
    if (p.scale) { v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w; }
    if (p.bias) { v.x += bi.x; v.y += bi.y; v.z += bi.z; v.w += bi.w; }
    if (p.res) { v.x += rs[j].x; v.y += rs[j].y; v.z += rs[j].z; v.w += rs[j].w; }
    if (p.accum) { v.x += ac[j].x; v.y += ac[j].y; v.z += ac[j].z; v.w += ac[j].w; }
    if (p.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    if (use_mask8) relu_mask8(v, mk8[j]);
    *reinterpret_cast<float4*>(p.y + md[j] * p.ldy + n) = v;
    if (p.mask8_out && p.relu) p.mask8_out[md[j] * p.ldm8_out + (n >> 2)] = relu_bits(v);
    if (p.y2) pair_store4(p.y2, md[j], p.ldy, n, v, y2s);
    ymax = amax_f4(ymax, v);
  }
  if (p.amax_y) amax_block_commit(ymax, p.amax_y);
}

// Tile width in N.  128 x 64 tiles (half the bytes of every parked partial tile, twice the tiles, 1.5x the LDS reads per
// MFMA) pay for launches that have few tiles AND a short K: per-layer A/B in the f16x3 mode (tools/layer_times.py,
// profiles/r03_bn64_layer_times.txt) -- the 1x1 convs of layer2-4 / ASPP at batch 1 gain 5-30 %, long-K 3x3 convs and
// everything with >= 256 tiles lose.  Batch 1 only: at batch 3 the same rule makes the two-stream iteration 1.4 % slower
// (9.97 -> 10.12 ms) although the single-stream per-layer times predict a small gain; batch 1: 5.46 -> 5.33 ms.
int conv_bn(const ConvArgs& a) {
  if (a.nseg > 0) return 128;                     // the K-concatenated kernel exists for 128-wide tiles only
  if (a.N <= 64) return 64;
  constexpr long kMaxTiles = 256, kMaxKSteps = 16;      // (K steps: 40 until the streaming kernels took the short-K launches; re-measured: 4.55 -> 4.50 ms)
  if (a.B == 1 && conv_mfma_mode() == 2 && !a.plane_rows) {
    const long tiles = (long)((a.M + 127) / 128) * ((a.N + 127) / 128);
    const long ksteps = (long)a.KH * a.KW * ((a.Kc + 31) / 32);
    if (tiles < kMaxTiles && ksteps <= kMaxKSteps) return 64;
  }
  return 128;
}

// Host: per-tile compacted K-step prefix and valid-tap masks (dilated unit-stride gathers; stride-2 data
// gradients in parity-major row order).
// Returns the total number of valid K steps.  prefix has tiles+1 entries, mask tiles entries.
long conv_build_tap_table(const ConvArgs& a, std::vector<int>& prefix, std::vector<int>& mask) {
  const int bn = conv_bn(a);
  const int T = a.KH * a.KW;
  const int chunks = (a.Kc + EOSVOS_BK - 1) / EOSVOS_BK;
  const int nt = (a.N + bn - 1) / bn, mt = (a.M + 127) / 128;
  prefix.assign((size_t)mt * nt + 1, 0);
  mask.assign((size_t)mt * nt, 0);
  long total = 0;
  const int up = 1 << a.upshift;
  for (int tm = 0; tm < mt; ++tm) {
    int mk = 0;
    for (int mr = tm * 128; mr < a.M && mr < tm * 128 + 128; ++mr) {
      const int m = a.par ? conv_par_pixel(a.B, a.Ho, a.Wo, mr) : mr;
      const int hw = a.Ho * a.Wo, rem = m % hw;
      const int oy = rem / a.Wo, ox = rem % a.Wo;
      for (int t2 = 0; t2 < T; ++t2) {
        const int ky = t2 / a.KW, kx = t2 % a.KW;
        const int sy = oy * a.mul + a.off0 + ky * a.kstep, sx = ox * a.mul + a.off0 + kx * a.kstep;
        if (sy >= 0 && sx >= 0 && sy % up == 0 && sx % up == 0 && sy / up < a.Hi && sx / up < a.Wi) mk |= 1 << t2;
      }
    }
    int nv = 0;
    for (int t2 = 0; t2 < T; ++t2) nv += (mk >> t2) & 1;
    for (int tn = 0; tn < nt; ++tn) {
      const size_t tile = (size_t)tm * nt + tn;
      prefix[tile] = (int)total;
      mask[tile] = mk;
      total += (long)nv * chunks;
    }
  }
  prefix.back() = (int)total;
  return total;
}

// K-concatenated data gradient: global tap ids (segment-major, then ky, kx), per-tile lists of the taps that reach the
// image for at least one pixel of the tile, K-step prefix (every segment has the same Kc = a.Kc reduction channels).
long conv_build_multi_table(const ConvArgs& a, const ConvSegHost* segs, int nseg, std::vector<int>& prefix,
                            std::vector<unsigned char>& taplist, std::vector<ConvTap>& taps) {
  const int chunks = (a.Kc + EOSVOS_BK - 1) / EOSVOS_BK;
  const int nt = (a.N + 127) / 128, mt = (a.M + 127) / 128;
  taps.clear();
  for (int g = 0; g < nseg; ++g) {
    const ConvSegHost& sg = segs[g];
    const int T = sg.k * sg.k;
    for (int ky = 0; ky < sg.k; ++ky)
      for (int kx = 0; kx < sg.k; ++kx) {
        ConvTap t;
        t.dy = sg.pad - ky * sg.dil; t.dx = sg.pad - kx * sg.dil;
        t.xoff = sg.xoff;
        t.wbase = (int)(sg.woff + (long)(ky * sg.k + kx) * a.wK);
        t.wrow = T * a.wK;
        t.ksoff = sg.ksoff; t.seg = g; t.pad_ = 0;
        taps.push_back(t);
      }
  }
  prefix.assign((size_t)mt * nt + 1, 0);
  taplist.assign((size_t)mt * nt * 32, 0);
  long total = 0;
  for (int tm = 0; tm < mt; ++tm) {
    std::vector<unsigned char> keep;
    for (size_t id = 0; id < taps.size(); ++id) {
      bool any = false;
      for (int m = tm * 128; m < a.M && m < tm * 128 + 128 && !any; ++m) {
        const int hw = a.Ho * a.Wo, rem = m % hw;
        const int sy = rem / a.Wo + taps[id].dy, sx = rem % a.Wo + taps[id].dx;
        any = sy >= 0 && sx >= 0 && sy < a.Hi && sx < a.Wi;
      }
      if (any) keep.push_back((unsigned char)id);
    }
    for (int tn = 0; tn < nt; ++tn) {
      const size_t tile = (size_t)tm * nt + tn;
      prefix[tile] = (int)total;
      for (size_t k = 0; k < keep.size() && k < 32; ++k) taplist[tile * 32 + k] = keep[k];
      total += (long)keep.size() * chunks;
    }
  }
  prefix.back() = (int)total;
  return total;
}
bool conv_multi_supported() { return conv_mfma_mode() >= 1; }


// ---------------------------------------------------------------------------------------
// fp32 contraction on the bf16 matrix cores ("bf16x6").
//
// The fp32 MFMA runs at 1/16 of the bf16 MFMA rate on CDNA4, so every operand is split into three bf16 pieces,
// a = hi + mid + lo (each piece = the top 16 bits of the running remainder: 3 x 8 significand bits cover the 24-bit
// significand, so the split is exact; the remainders are exact fp32 subtractions), and a*b is accumulated from the
// six partial products
//   hi*hi + hi*mid + mid*hi + mid*mid + hi*lo + lo*hi      (v_mfma_f32_32x32x16_bf16, fp32 accumulate);
// the dropped mid*lo, lo*mid, lo*lo terms are <= 2^-24 relative, i.e. below one fp32 rounding of the product.
// bf16 x bf16 products are exact in fp32.  Measured against fp64 (tools/probes/bf16x6_probe.cpp): error relative to
// sum|a*b| 1.4e-7 (the fp32 MFMA: 2.0e-7), at 1.45-1.6x the fp32-MFMA rate of the same tile structure.
// Six 32-cycle MFMAs replace eight 64-cycle ones per 16 k of a 32x32 tile: 2.67x the fp32 matrix peak.
//
// Tile: 128 x {128,64} x 32 per 256-thread workgroup (2x2 waves, 64 x {64,32} per wave), 2 workgroups per CU.
// Operands are gathered global -> registers (fp32, prefetched behind the MFMAs) -> split -> one LDS stage of
// [piece][row][32 k] bf16 rows.  The products run on v_mfma_f32_16x16x32_bf16 (one ds_read_b128 = the 8 k of a lane's
// k slot; a fragment = 16 rows x all 32 k of the stage): on random data the chip holds a higher clock under this shape
// than under 32x32x16 at equal cycles per FLOP (MI355X_MICROARCH.md, DVFS give-back item 7; measured on this loop:
// +7-11 %, tools/probes/x6_shape_probe.cpp, profiles/r03_x6_shape_probe.txt), and s_setprio 1 around the MFMA block
// keeps the co-resident workgroup's split / LDS-store phase from delaying it (+4-6 % more).  Row pitch 96 bytes:
// conflict-free ds_read_b128 for the 16-row fragments (lane l reads row l % 16, 16-byte slot l / 16).
// K-major operands (the weights of the data gradient, both operands of the weight gradient) are transposed in
// registers while staging: a thread loads RPT consecutive k rows of 4 channels and writes one k-run per channel; their
// LDS rows are de-interleaved (row j*W/4 + c <-> channel 4c + j) -- the epilogue maps the MFMA tile coordinates back.
// ---------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
#define X6_ROWB 96

// Two fp32 values -> bf16 pieces, packed (e1 << 16 | e0): the truncated top 16 bits (one v_perm_b32; the 3-way split of
// a 24-bit significand is then exact).  Rounding to nearest even instead (v_cvt_pk_bf16_f32) was measured: same parity
// margins (profiles/r02_parity_margins.txt), 4 % slower step on the same box.
__device__ __forceinline__ unsigned x6_pack(float e0, float e1) {
  return __builtin_amdgcn_perm(__float_as_uint(e1), __float_as_uint(e0), 0x07060302u);
}
__device__ __forceinline__ float x6_lo(unsigned pk) { return __uint_as_float(pk << 16); }          // piece of e0 as fp32
__device__ __forceinline__ float x6_hi(unsigned pk) { return __uint_as_float(pk & 0xffff0000u); }  // piece of e1 as fp32
// four consecutive-k values -> the three pieces, 4 bf16 (8 bytes) each
__device__ __forceinline__ void x6_split4(float a, float b, float c, float d, uint2 out[3]) {
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    out[p].x = x6_pack(a, b);
    out[p].y = x6_pack(c, d);
    if (p < 2) { a -= x6_lo(out[p].x); b -= x6_hi(out[p].x); c -= x6_lo(out[p].y); d -= x6_hi(out[p].y); }
  }
}
__device__ __forceinline__ void x6_split2(float a, float b, unsigned out[3]) {
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    out[p] = x6_pack(a, b);
    if (p < 2) { a -= x6_lo(out[p]); b -= x6_hi(out[p]); }
  }
}
// ---- "f16x3": 2-way fp16 split, 3 partial products (NP = 2) ---------------------------------------------------------
// a * s = h0 + h1 + e with h0 = rn16(a * s), h1 = rn16(a * s - h0): |e| <= 1 ulp of the fp32 value while h1 is a normal
// fp16 number.  s is a power of two per operand TENSOR that puts the tensor's largest magnitude into [2^14, 2^15) (fp16
// overflows at 65504); elements below 2^-16 of that maximum start to lose relative precision (h1 goes subnormal: absolute
// error floor 2^-40 of the maximum -- the matrix cores keep fp16 subnormals).  The product drops h1a * h1b <= 2^-22 |ab|.
// Half the MFMAs, a third less LDS traffic than bf16x6; measured on the bare GEMM loop 238-276 TFLOP/s against 163-188 and
// a smaller error than bf16x6 on well-scaled data (tools/probes/f16x3_probe.cpp, profiles/r03_f16x3_probe.txt).
// The scale comes from the absmax slots the engine maintains (uint bit patterns of max|x|, atomicMax'ed by absmax_kernel
// or by the kernel that produced the tensor; finite values only).  NaN / inf elements become fp16 NaN / inf pieces and
// reach the outputs they contribute to as NaN, as in the bf16x6 mode.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
#define MFMA_F16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)
__device__ __forceinline__ unsigned h3_pack(float e0, float e1) {          // v_cvt_pk_f16_f32, round to nearest even
  f32x2v v = {e0, e1};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2v));
}
__device__ __forceinline__ f32x2v h3_unpack(unsigned w) { return __builtin_convertvector(__builtin_bit_cast(f16x2v, w), f32x2v); }
// scale 2^(141 - e) for a tensor whose absmax has the biased exponent e (largest magnitude -> [2^14, 2^15)), and 1 / scale.
// `amax2`: optional second factor of the staged values (the per-channel norm scale of the data gradient).
__device__ __forceinline__ float h3_scale(const unsigned* amax, const unsigned* amax2, float& inv) {
  float m = __uint_as_float(amax_read(amax));
  if (amax2) m *= __uint_as_float(amax_read(amax2));
  const int e = (int)((__float_as_uint(m) >> 23) & 0xffu);
  int f = 268 - e;
  f = f < 1 ? 1 : (f > 254 ? 254 : f);
  inv = __uint_as_float((unsigned)(254 - f) << 23);
  return __uint_as_float((unsigned)f << 23);
}
// the same from slot words already in registers (one word per lane < AMAX_SUB, 0 elsewhere): lets a kernel issue the slot
// loads together with its other prologue loads instead of one memory round trip per h3_scale call
__device__ __forceinline__ unsigned amax_issue(const unsigned* slot) {
  const int lane = threadIdx.x & 63;
  return (slot && lane < AMAX_SUB) ? slot[(size_t)lane * AMAX_ROW] : 0u;
}
__device__ __forceinline__ unsigned amax_wave_max(unsigned m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = (unsigned)__shfl_xor((int)m, o);
    m = m > t ? m : t;
  }
  return m;
}
__device__ __forceinline__ float h3_scale_bits(unsigned w1, bool two, unsigned w2, float& inv) {
  float m = __uint_as_float(amax_wave_max(w1));
  if (two) m *= __uint_as_float(amax_wave_max(w2));
  const int e = (int)((__float_as_uint(m) >> 23) & 0xffu);
  int f = 268 - e;
  f = f < 1 ? 1 : (f > 254 ? 254 : f);
  inv = __uint_as_float((unsigned)(254 - f) << 23);
  return __uint_as_float((unsigned)f << 23);
}
// The 2-way fp16 split of two values.  Writing both halves of each piece register in place with v_fma_mixlo / mixhi_f16
// (2 VALU instructions per value against 4) was measured with an A/B switch since removed: bit-identical pieces
// (tools/probes/mixsplit_probe.cpp) -- and slower, iteration 9.07 against 8.87 ms: the mix forms run at a lower rate.
__device__ __forceinline__ void h3_split_pair(float x0, float x1, float s, unsigned& hi, unsigned& lo) {
  const float a = x0 * s, b = x1 * s;
  hi = h3_pack(a, b);
  const f32x2v u = h3_unpack(hi);
  lo = h3_pack(a - u.x, b - u.y);
}
// four consecutive-k values -> NP pieces of 4 x 16 bit (8 bytes) each.  NP = 3: exact bf16 split (s unused); NP = 2: fp16.
template <int NP>
__device__ __forceinline__ void xs_split4(float a, float b, float c, float d, float s, uint2 (&out)[NP]) {
  if (NP == 3) {
    uint2 t[3];
    x6_split4(a, b, c, d, t);
#pragma unroll
    for (int p = 0; p < NP; ++p) out[p] = t[p];
  } else {
    h3_split_pair(a, b, s, out[0].x, out[NP - 1].x);
    h3_split_pair(c, d, s, out[0].y, out[NP - 1].y);
  }
}
template <int NP>
__device__ __forceinline__ void xs_split2(float a, float b, float s, unsigned (&out)[NP]) {
  if (NP == 3) {
    unsigned t[3];
    x6_split2(a, b, t);
#pragma unroll
    for (int p = 0; p < NP; ++p) out[p] = t[p];
  } else {
    h3_split_pair(a, b, s, out[0], out[NP - 1]);
  }
}
__device__ __forceinline__ float f4c(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
// LDS row of a K-major operand tile of width W <-> channel inside the tile
__device__ __forceinline__ int x6_row_chan(int R, int W) { return 4 * (R % (W / 4)) + R / (W / 4); }

// Staging maps.  Row-major operands: a thread stores 8 bytes (4 k) of one row per pass of 32 rows; the two rows of a
// 16-lane ds_write_b64 group lie 2 rows apart (192 B = 16 banks: disjoint bank halves at the 96-byte pitch).
__device__ __forceinline__ int x6_stage_row(int tid) {
  const int j = (tid >> 3) & 7;
  return ((tid >> 6) << 3) + ((j & 1) << 1) + ((j >> 1) & 1) + (j & 4);
}
// K-major operands, 128 channels wide (a thread owns 4 k x 4 channels): a 16-lane ds_write_b64 group = 4 consecutive
// LDS rows x 4 k runs (32 distinct banks); a wave's global load covers 256 contiguous bytes of each of 4 k rows.
__device__ __forceinline__ int x6_kmaj_c4_128(int tid) { return (tid & 3) | (((tid >> 4) & 3) << 2) | (((tid >> 6) & 1) << 4); }
__device__ __forceinline__ int x6_kmaj_kq_128(int tid) { return ((tid >> 2) & 3) | (((tid >> 7) & 1) << 2); }
// 64 channels wide (2 k x 4 channels, ds_write_b32): a 32-lane group = 4 consecutive rows x 8 k pairs
__device__ __forceinline__ int x6_kmaj_c4_64(int tid) { return (tid & 3) | (((tid >> 5) & 1) << 2) | (((tid >> 6) & 1) << 3); }
__device__ __forceinline__ int x6_kmaj_kq_64(int tid) { return ((tid >> 2) & 7) | (((tid >> 7) & 1) << 3); }

// one 32-deep K step of a wave's (16*TM) x (16*TN) tile: 6*TM*TN MFMAs.  Fragments are taken MB x 2 at a time:
// MB = TM reads every fragment once (3*(TM + TN) ds_read_b128); MB = 2 re-reads the B fragments per A pair
// (3*(TM + TN*TM/2) reads) and keeps only 12 fragments live -- for the conv kernels, whose gather state needs the registers.
template <int TM, int TN, int MB = TM, int NP = 3>
__device__ __forceinline__ void x6_mma_step(const unsigned char* As, const unsigned char* Bs, int a_rows, int b_rows, int a_row0,
                                            int b_row0, int r16, int q, f32x4 (&acc)[TM][TN]) {
#pragma unroll
  for (int hm = 0; hm < TM; hm += MB) {
    bf16x8 fa[MB][NP];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int t = 0; t < MB; ++t)
        fa[t][p] = *reinterpret_cast<const bf16x8*>(As + (p * a_rows + a_row0 + (hm + t) * 16 + r16) * X6_ROWB + q * 16);
    // the re-read of the B fragments must stay a re-read (a merged load would keep all of them live): opaque base
    unsigned boff = (unsigned)((b_row0 + r16) * X6_ROWB + q * 16);
    if (MB != TM) asm volatile("" : "+v"(boff));
#pragma unroll
    for (int hn = 0; hn < TN; hn += 2) {
      bf16x8 fb[2][NP];
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          fb[t][p] = *reinterpret_cast<const bf16x8*>(Bs + boff + (p * b_rows + (hn + t) * 16) * X6_ROWB);
#pragma unroll
      for (int tm = 0; tm < MB; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          f32x4 c = acc[hm + tm][hn + tn];
          if (NP == 3) {
            c = MFMA_BF16(fa[tm][NP - 1], fb[tn][0], c);            // smallest terms first
            c = MFMA_BF16(fa[tm][0], fb[tn][NP - 1], c);
            c = MFMA_BF16(fa[tm][1], fb[tn][1], c);
            c = MFMA_BF16(fa[tm][1], fb[tn][0], c);
            c = MFMA_BF16(fa[tm][0], fb[tn][1], c);
            c = MFMA_BF16(fa[tm][0], fb[tn][0], c);
          } else {
            c = MFMA_F16(__builtin_bit_cast(f16x8, fa[tm][1]), __builtin_bit_cast(f16x8, fb[tn][0]), c);
            c = MFMA_F16(__builtin_bit_cast(f16x8, fa[tm][0]), __builtin_bit_cast(f16x8, fb[tn][1]), c);
            c = MFMA_F16(__builtin_bit_cast(f16x8, fa[tm][0]), __builtin_bit_cast(f16x8, fb[tn][0]), c);
          }
          acc[hm + tm][hn + tn] = c;
        }
    }
  }
}

constexpr int xs_max(int a, int b) { return a > b ? a : b; }
// LDS of a conv workgroup: NP operand planes, or the C tile that the epilogue stages through the same bytes
template <int BN, int NP> constexpr int conv_xs_smem() { return xs_max(NP * (128 + BN) * X6_ROWB, 128 * (BN + 4) * 4); }
template <int BN, bool KMAJOR, int NP, bool MULTI = false>
__device__ __forceinline__ void conv_xs_body(const ConvArgs& p, unsigned char* smem) {
  constexpr int BM = 128, BK = 32;
  constexpr int A_BYTES = NP * BM * X6_ROWB;
  constexpr int LDC = BN + 4;
  unsigned char* const As = smem;
  unsigned char* const Bs = smem + A_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;              // fragment row / 16-byte k slot of this lane

  const int T = p.KH * p.KW;
  const int chunks = (p.Kc + BK - 1) / BK;
  const int ksteps = T * chunks;
  const int nt = (p.N + BN - 1) / BN;
  const int tiles = ((p.M + BM - 1) / BM) * nt;
  const long U = p.tprefix ? (long)p.tprefix[tiles] : (long)tiles * ksteps;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const long sk0 = (long)p.dp_q * gridDim.x * ksteps;
  const long u_begin = sk0 + (long)bid * p.per;
  long u_end = u_begin + p.per;
  if (u_end > U) u_end = U;
  int dp_i = 0;

  constexpr int APASS = BM / 32;                         // 8 float4 per 32-k row, 32 rows per pass
  const int a_c4 = tid & 7, a_r = x6_stage_row(tid);
  // B operand: rows of k (n-major weights, forward) staged like A; k-major weights (data gradient): a thread owns
  // RPT consecutive k rows x 4 columns
  constexpr int NQ = BN / 4, RPT = BN / 32;              // K-major: threads per k row, k rows per thread
  constexpr int BPASS = BN / 32;                         // = RPT: float4 loads per thread in both layouts
  const int b_c4 = a_c4, b_r = a_r;
  const int b_n4 = RPT == 4 ? x6_kmaj_c4_128(tid) : x6_kmaj_c4_64(tid);
  const int b_kq = RPT == 4 ? x6_kmaj_kq_128(tid) : x6_kmaj_kq_64(tid);
  const int up = 1 << p.upshift;
  constexpr int TN = BN / 32;                            // 16-column fragments per wave
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, (long)p.B * p.Hi * p.Wi * p.ldx * 4);
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, MULTI ? p.w_floats * 4 : (p.plane_rows ? (long)p.nplanes : 1L) * p.wN * T * p.wK * 4);
  float sa = 1.f, sb = 1.f, inv_ab = 1.f;
  // The slot words of all operands are requested together -- statement by statement the compiler waits for each load where
  // its reduction starts: one memory round trip per slot in front of the first tile -- and reduced only when the first tile's
  // operand loads are in flight as well (scales_late()).
  unsigned h3_ax = 0, h3_ak = 0, h3_aw = 0;
  bool h3_pending = false;
  if (NP == 2 && !MULTI) {
    h3_ax = amax_issue(p.amax_x); h3_ak = amax_issue(KMAJOR ? p.amax_ks : nullptr); h3_aw = amax_issue(p.amax_w);
    h3_pending = true;
  }
  auto scales_late = [&]() {
    if (h3_pending) {                                 // wave-uniform; true once per workgroup
      float ia, ib;
      sa = h3_scale_bits(h3_ax, KMAJOR && p.amax_ks, h3_ak, ia);
      sb = h3_scale_bits(h3_aw, false, 0u, ib);
      inv_ab = ia * ib;
      h3_pending = false;
    }
  };
  // K-concatenated launch: operand scales per segment (f16x3); the accumulators live in units of 1 / inv_ab of the segment
  // they were last added to and are rescaled (exact: powers of two) where the K loop enters the next one
  float seg_sa[4] = {1.f, 1.f, 1.f, 1.f}, seg_sb[4] = {1.f, 1.f, 1.f, 1.f}, seg_inv[4] = {1.f, 1.f, 1.f, 1.f};
  if (MULTI && NP == 2) {
    const unsigned ax = amax_issue(p.amax_x);
    unsigned ak[4], aw[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {                     // all slot words in flight together (else 8 serial round trips)
      ak[g] = amax_issue(g < p.nseg ? p.seg_amax_ks[g] : nullptr);
      aw[g] = amax_issue(g < p.nseg ? p.seg_amax_w[g] : nullptr);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (g >= p.nseg) break;
      float ia, ib;
      seg_sa[g] = h3_scale_bits(ax, p.seg_amax_ks[g] != nullptr, ak[g], ia);
      seg_sb[g] = h3_scale_bits(aw[g], false, 0u, ib);
      seg_inv[g] = ia * ib;
    }
  }
  auto pick4 = [](const float (&v)[4], int g) { return g == 0 ? v[0] : (g == 1 ? v[1] : (g == 2 ? v[2] : v[3])); };
  int seg_ld = 0, seg_acc = 0;   // segment of the operands in flight / of the accumulators' unit

  unsigned ymax = 0;           // f16x3: absmax of what this workgroup writes (-> p.amax_y)
  bool splitk_pending = p.splitk > 0;
  for (long u = u_begin;;) {
    int tile, ks_begin, ks_end = ksteps;
    const bool dp = dp_i < p.dp_q;
    if (dp) {
      // tap-table launch dealt out as whole tiles, longest first (p.torder); odd rounds run backwards so that the
      // workgroups with the longest first tile get the shortest second one
      const int idx = dp_i * (int)gridDim.x + ((p.torder && (dp_i & 1)) ? (int)gridDim.x - 1 - bid : bid);
      ks_begin = 0;
      ++dp_i;
      if (idx >= tiles) continue;
      tile = p.torder ? p.torder[idx] : idx;
      if (p.tprefix) ks_end = p.tprefix[tile + 1] - p.tprefix[tile];
    } else if (p.splitk > 0) {
      // uniform split-K, chunk-major: the workgroups of an XCD (consecutive bid) work on the SAME K chunk of neighbouring
      // tiles at the same time, so the weight slice of a chunk is fetched into the XCD's L2 once instead of once per workgroup
      if (!splitk_pending) break;
      splitk_pending = false;
      tile = bid % tiles;
      const int c = bid / tiles;
      const int n_t = p.tprefix ? p.tprefix[tile + 1] - p.tprefix[tile] : ksteps;
      ks_begin = (int)((long)c * n_t / p.splitk);
      ks_end = (int)((long)(c + 1) * n_t / p.splitk);
    } else if (u < u_end) {
      if (p.tprefix) {
        int lo = 0, hi = tiles - 1;
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if ((long)p.tprefix[mid] <= u) lo = mid; else hi = mid - 1;
        }
        tile = lo;
        ks_begin = (int)(u - p.tprefix[tile]);
        ks_end = p.tprefix[tile + 1] - p.tprefix[tile];
      } else {
        tile = (int)(u / ksteps);
        ks_begin = (int)(u - (long)tile * ksteps);
      }
      if ((long)ks_end - ks_begin > u_end - u) ks_end = ks_begin + (int)(u_end - u);
    } else {
      break;
    }
    const int ks_total = p.tprefix ? p.tprefix[tile + 1] - p.tprefix[tile] : ksteps;
    unsigned long long tappack = 0x876543210ULL;
    if (!MULTI && p.tprefix) {
      const int mask = p.tmask[tile];
      tappack = 0;
      int nv = 0;
      for (int t2 = 0; t2 < T; ++t2)
        if ((mask >> t2) & 1) { tappack |= (unsigned long long)t2 << (4 * nv); ++nv; }
    }
    const int m0 = (tile / nt) * BM, n0 = (tile % nt) * BN;

    int a_sy0[APASS], a_sx0[APASS], a_img[APASS];
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
      int m = m0 + a_r + i * 32;
      if (m < p.M) {
        if (p.par) m = conv_par_pixel(p.B, p.Ho, p.Wo, m);
        const int hw = p.Ho * p.Wo;
        const int b = m / hw, rem = m - b * hw;
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        a_sy0[i] = oy * p.mul + p.off0;
        a_sx0[i] = ox * p.mul + p.off0;
        a_img[i] = b * p.Hi * p.Wi;
      } else {
        a_sy0[i] = -(1 << 28);
        a_sx0[i] = 0;
        a_img[i] = 0;
      }
    }
    float4 ra[APASS], rb[BPASS];
    constexpr unsigned OOB = 0x80000000u;
    int a_off[APASS];
    int b_off[BPASS];
    const int wplane = p.plane_rows ? (m0 / p.plane_rows) * (int)p.w_plane : 0;
#pragma unroll
    for (int i = 0; i < BPASS; ++i) {
      if (KMAJOR) {
        const int n = n0 + b_n4 * 4;
        b_off[i] = n < p.N ? wplane + (b_kq * RPT + i) * T * p.wK + n : -1;
      } else {
        const int n = n0 + b_r + i * 32;
        b_off[i] = n < p.N ? wplane + n * T * p.wK + b_c4 * 4 : -1;
      }
    }
    int cur_tap = -1;
    int m_wrow = 0, m_ksoff = 0;     // K-concatenated launch: k-row pitch of the segment's weights, offset of its norm scale
    auto load_tiles = [&](int ks) {
      const int vt = ks / chunks;
      const int c0 = (ks - vt * chunks) * BK;
      const int tap = MULTI ? vt : (p.tprefix ? (int)((tappack >> (4 * vt)) & 15) : vt);
      if (tap != cur_tap) {          // wave-uniform
        cur_tap = tap;
        int dy, dx, xoff = 0;
        if (MULTI) {
          const int id = __builtin_amdgcn_readfirstlane((int)p.taplist[(size_t)tile * 32 + vt]);
          const ConvTap d = p.taps[id];
          dy = d.dy; dx = d.dx; xoff = d.xoff; m_wrow = d.wrow; m_ksoff = d.ksoff; seg_ld = d.seg;
          if (NP == 2) { sa = pick4(seg_sa, seg_ld); sb = pick4(seg_sb, seg_ld); }
#pragma unroll
          for (int i = 0; i < BPASS; ++i) {
            const int n = n0 + b_n4 * 4;
            b_off[i] = n < p.N ? d.wbase + (b_kq * RPT + i) * d.wrow + n : -1;
          }
        } else {
          const int ky = tap / p.KW, kx = tap - ky * p.KW;
          dy = ky * p.kstep; dx = kx * p.kstep;
        }
#pragma unroll
        for (int i = 0; i < APASS; ++i) {
          const int sy = a_sy0[i] + dy, sx = a_sx0[i] + dx;
          bool ok = sy >= 0 && sx >= 0 && ((sy | sx) & (up - 1)) == 0;
          const int iy = sy >> p.upshift, ix = sx >> p.upshift;
          ok = ok && iy < p.Hi && ix < p.Wi;
          a_off[i] = ok ? (a_img[i] + iy * p.Wi + ix) * p.ldx + a_c4 * 4 + xoff : -1;
        }
      }
      const bool cok = (c0 + a_c4 * 4) < p.Kc;
      float4 ks4 = make_float4(1.f, 1.f, 1.f, 1.f);
      if (KMAJOR && p.kscale && cok) ks4 = ldg4(p.kscale + (MULTI ? m_ksoff : 0) + c0 + a_c4 * 4);
#pragma unroll
      for (int i = 0; i < APASS; ++i) {
        const unsigned off = (cok && a_off[i] >= 0) ? (unsigned)(a_off[i] + c0) * 4u : OOB;
        float4 v = bufld4(rx, off);
        if (KMAJOR) { v.x *= ks4.x; v.y *= ks4.y; v.z *= ks4.z; v.w *= ks4.w; }
        ra[i] = v;
      }
#pragma unroll
      for (int i = 0; i < BPASS; ++i) {
        unsigned off;
        if (MULTI) {
          const int k = c0 + b_kq * RPT + i;
          off = (b_off[i] >= 0 && k < p.Kc) ? (unsigned)(b_off[i] + c0 * m_wrow) * 4u : OOB;
        } else if (KMAJOR) {
          const int k = c0 + b_kq * RPT + i;
          off = (b_off[i] >= 0 && k < p.Kc) ? (unsigned)(b_off[i] + (c0 * T + tap) * p.wK) * 4u : OOB;
        } else {
          const int k = c0 + b_c4 * 4;
          off = (b_off[i] >= 0 && k < p.Kc) ? (unsigned)(b_off[i] + tap * p.wK + c0) * 4u : OOB;
        }
        rb[i] = bufld4(rw, off);
      }
    };
    auto store_tiles = [&]() {
#pragma unroll
      for (int i = 0; i < APASS; ++i) {
        uint2 pc[NP];
        xs_split4<NP>(ra[i].x, ra[i].y, ra[i].z, ra[i].w, sa, pc);
#pragma unroll
        for (int q = 0; q < NP; ++q) *reinterpret_cast<uint2*>(As + (q * BM + a_r + i * 32) * X6_ROWB + a_c4 * 8) = pc[q];
      }
      if (!KMAJOR) {
#pragma unroll
        for (int i = 0; i < BPASS; ++i) {
          uint2 pc[NP];
          xs_split4<NP>(rb[i].x, rb[i].y, rb[i].z, rb[i].w, sb, pc);
#pragma unroll
          for (int q = 0; q < NP; ++q) *reinterpret_cast<uint2*>(Bs + (q * BN + b_r + i * 32) * X6_ROWB + b_c4 * 8) = pc[q];
        }
      } else if (RPT == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {            // column 4*n4 + j of the tile lives in LDS row j*NQ + n4
          uint2 pc[NP];
          xs_split4<NP>(f4c(rb[0], j), f4c(rb[1], j), f4c(rb[RPT == 4 ? 2 : 0], j), f4c(rb[RPT == 4 ? 3 : 0], j), sb, pc);
#pragma unroll
          for (int q = 0; q < NP; ++q) *reinterpret_cast<uint2*>(Bs + (q * BN + j * NQ + b_n4) * X6_ROWB + b_kq * 8) = pc[q];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          unsigned pc[NP];
          xs_split2<NP>(f4c(rb[0], j), f4c(rb[1], j), sb, pc);
#pragma unroll
          for (int q = 0; q < NP; ++q) *reinterpret_cast<unsigned*>(Bs + (q * BN + j * NQ + b_n4) * X6_ROWB + b_kq * 4) = pc[q];
        }
      }
    };

    constexpr int TM = 4;                                // 16-row fragments of a wave's 64 x (BN/2) tile
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

    load_tiles(ks_begin);
    scales_late();
    __syncthreads();            // previous segment's epilogue reads of smem are done
    store_tiles();
    __syncthreads();
    if (MULTI) seg_acc = seg_ld;

    for (int ks = ks_begin; ks < ks_end; ++ks) {
      const bool more = (ks + 1) < ks_end;
      if (more) load_tiles(ks + 1);          // global loads in flight behind the MFMAs below
      __builtin_amdgcn_s_setprio(1);
      x6_mma_step<TM, TN, ((BN == 128 && NP == 3) ? 2 : TM), NP>(As, Bs, BM, BN, wm * 64, wn * (BN / 2), fr, fq, acc);
      __builtin_amdgcn_s_setprio(0);
      __syncthreads();                       // every wave is done reading the stage
      if (more) store_tiles();
      if (MULTI && NP == 2 && more && seg_ld != seg_acc) {
        // the next K step belongs to another segment: its operands were staged under that segment's scales
        const float f = pick4(seg_inv, seg_acc) / pick4(seg_inv, seg_ld);      // power of two: exact
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][e] *= f;
        seg_acc = seg_ld;
      }
      __syncthreads();
    }
    if (MULTI && NP == 2) inv_ab = pick4(seg_inv, seg_acc);

    // ---- epilogue: accumulators -> LDS tile -> full-row float4 stores ------------------------
    float* Cs = reinterpret_cast<float*>(smem);
    const bool full = p.splitk == 0 && ks_begin == 0 && ks_end == ks_total;
    constexpr int CF4 = BN / 4, CROWS = 256 / CF4;
    const int c_c4 = tid % CF4, c_r = tid / CF4;
    const int n = n0 + c_c4 * 4;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), bi = make_float4(0.f, 0.f, 0.f, 0.f);
    if (full && n < p.N) {
      if (p.scale) sc = ldg4(p.scale + n);
      if (p.bias) bi = ldg4(p.bias + n);
    }
    const bool use_mask8 = p.mask8 && n >= p.mask_c0;
    const bool write_m8 = p.mask8_out && p.relu;
    const float y2s = (NP == 2 && p.y2) ? *p.y2_sc : 0.f;
    {
      // D of 16x16x32: lane (fr = column, fq) holds rows 4*fq .. 4*fq+3 of the fragment
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          const int Rb = wn * (BN / 2) + tn * 16 + fr;
          const int ncol = KMAJOR ? x6_row_chan(Rb, BN) : Rb;
#pragma unroll
          for (int e = 0; e < 4; ++e) Cs[(wm * 64 + tm * 16 + 4 * fq + e) * LDC + ncol] = NP == 2 ? acc[tm][tn][e] * inv_ab : acc[tm][tn][e];
        }
      __syncthreads();
      if (full) {
        if (n < p.N) {
          constexpr int NIT = BM / CROWS, EB = BN == 128 ? EOSVOS_EB128 : EOSVOS_EB;
          // the tensor added to the tile: the residual / skip gradient (res) or the destination's previous contents (accum).
          // One register set serves both; a launch with both (none in the network) reads the second one row by row.
          const float* const adp = p.res ? p.res : (p.accum ? p.y : nullptr);
          const int adld = p.res ? p.ldres : p.ldy;
          const bool both = p.res && p.accum;
#pragma unroll
          for (int it0 = 0; it0 < NIT; it0 += EB) {
            size_t md[EB];
            bool ok[EB];
            float4 ad[EB];
            unsigned mk8[EB];                 // ReLU mask bits of the row's 4 channels
#pragma unroll
            for (int j = 0; j < EB; ++j) {
              const int m = m0 + c_r + (it0 + j) * CROWS;
              ok[j] = m < p.M;
              md[j] = dst_pixel(p, ok[j] ? m : p.M - 1);
            }
            if (adp) {
#pragma unroll
              for (int j = 0; j < EB; ++j) ad[j] = ldg4(adp + md[j] * adld + n);
            }
            if (use_mask8) {
#pragma unroll
              for (int j = 0; j < EB; ++j) mk8[j] = p.mask8[md[j] * p.ldm8 + (n >> 2)];
            }
#pragma unroll
            for (int j = 0; j < EB; ++j) {
              float4 v = *reinterpret_cast<const float4*>(Cs + (c_r + (it0 + j) * CROWS) * LDC + c_c4 * 4);
              if (p.scale) { v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w; }
              if (p.bias) { v.x += bi.x; v.y += bi.y; v.z += bi.z; v.w += bi.w; }
              if (adp) { v.x += ad[j].x; v.y += ad[j].y; v.z += ad[j].z; v.w += ad[j].w; }
              if (both) { const float4 a2 = ldg4(p.y + md[j] * p.ldy + n); v.x += a2.x; v.y += a2.y; v.z += a2.z; v.w += a2.w; }
              if (p.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
              if (use_mask8) relu_mask8(v, mk8[j]);
              if (ok[j]) {
                *reinterpret_cast<float4*>(p.y + md[j] * p.ldy + n) = v;
                if (write_m8) p.mask8_out[md[j] * p.ldm8_out + (n >> 2)] = relu_bits(v);
                if (NP == 2 && p.y2) pair_store4(p.y2, md[j], p.ldy, n, v, y2s);
                if (NP == 2) ymax = amax_f4(ymax, v);
              }
            }
          }
        }
      } else {
        float* slab = p.ws + ((size_t)bid * 2 + (u == u_begin ? 0 : 1)) * (BM * BN);
#pragma unroll 4
        for (int lr = c_r; lr < BM; lr += CROWS)
          *reinterpret_cast<float4*>(slab + lr * BN + c_c4 * 4) = *reinterpret_cast<const float4*>(Cs + lr * LDC + c_c4 * 4);
      }
    }
    if (!dp) u += ks_end - ks_begin;
  }
  if (NP == 2 && p.amax_y) amax_block_commit(ymax, p.amax_y);
}

template <int BN, bool KMAJOR>
__global__ __launch_bounds__(256, 2) void conv_x6_kernel(const ConvArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[conv_xs_smem<BN, 3>()];
  conv_xs_body<BN, KMAJOR, 3>(p, smem);
}
#define EOSVOS_H3_OCC64 2       // workgroups per CU the 64-wide f16x3 kernels are compiled for (3 / 4 for short-K launches were tried)
template <int BN, bool KMAJOR>
__global__ __launch_bounds__(256, BN == 64 ? EOSVOS_H3_OCC64 : 2) void conv_h3_kernel(const ConvArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[conv_xs_smem<BN, 2>()];
  conv_xs_body<BN, KMAJOR, 2>(p, smem);
}
// K-concatenated data gradient (ConvArgs::nseg > 0): several convolutions' gradients into one destination
__global__ __launch_bounds__(256, 2) void conv_h3_multi_kernel(const ConvArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[conv_xs_smem<128, 2>()];
  conv_xs_body<128, true, 2, true>(p, smem);
}
__global__ __launch_bounds__(256, 2) void conv_x6_multi_kernel(const ConvArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[conv_xs_smem<128, 3>()];
  conv_xs_body<128, true, 3, true>(p, smem);
}

// ---------------------------------------------------------------------------------------
// Streaming kernel for the SHORT-K 1x1 stride-1 convolutions on the large maps (layer1 / layer2: K = 64 ... 256 reduction
// channels, tens of thousands of pixels), forward and data gradient, f16x3 mode.  These launches are HBM-bound -- a pixel's
// output row (+ residual) is 4-16x its input row -- and ran at 2-3.5 TB/s in the tiled kernel above: a 128 x 128 tile with
// 2-8 K steps spends most of its time in the fixed cost per tile (prologue, first operand latency, two barriers per K step,
// the LDS-staged epilogue), and neither deeper epilogue batches, more workgroups per CU nor narrower tiles changed that
// (DESIGN.md 5b, round 4).  Structure here (tools/probes/skinny_probe.cpp): a 512-thread workgroup keeps the WHOLE weight
// matrix of its column range (NC output channels x K) in LDS, split once into the two fp16 pieces; after that single barrier
// each wave streams strips of 16 pixels on its own: X fragments straight from global into registers (a lane's 8 k values are
// 32 contiguous bytes), split per wave, D = W_frag * X_frag^T on v_mfma_f32_16x16x32_f16, so that a lane ends up with 4
// CONSECUTIVE channels of one pixel: float4 residual / accumulate loads and output stores, one mask byte per lane, the next
// strip's activations in flight behind the current strip's MFMAs.  Measured: layer1 conv3 (64 -> 256, + residual) 60 -> 41 us,
// layer2 conv3 (128 -> 512) 43 -> 31 us, layer1 conv1 (256 -> 64) 35 -> 26 us.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void s1_split8(const float4& lo, const float4& hi, float s, uint4& h0, uint4& h1) {
  unsigned a[4], b[4];
  h3_split_pair(lo.x, lo.y, s, a[0], b[0]);
  h3_split_pair(lo.z, lo.w, s, a[1], b[1]);
  h3_split_pair(hi.x, hi.y, s, a[2], b[2]);
  h3_split_pair(hi.z, hi.w, s, a[3], b[3]);
  h0 = make_uint4(a[0], a[1], a[2], a[3]);
  h1 = make_uint4(b[0], b[1], b[2], b[3]);
}
// Row pitch (bytes) of a weight image whose rows are read as 16x16x32 fragments by ds_read_b128 (lane -> row fr = lane % 16,
// 16-byte slot fq = lane / 16): the instruction's four 16-lane groups mix slots -- {fr 0-3, 12-15 of slot 2g} with {fr 4-11
// of slot 2g + 1} and the reverse (MI355X_MICROARCH.md, LDS) --, so the pitch in 16-byte units must be 2 mod 4 for the 16
// lanes of a group to cover all 64 banks: pitch = 32 bytes mod 64.  With K * 2 + 16 (round-4 first version: 16 mod 64) every
// fragment read was a 2-way conflict (SQ_LDS_BANK_CONFLICT 42 % of the LDS cycles of conv3x3_stream_kernel) and the LDS, not
// the matrix cores, paced the K loop.
constexpr int frag_pitch(int row_bytes) { return row_bytes % 64 == 32 ? row_bytes : row_bytes + (96 - row_bytes % 64) % 64; }
#define EOSVOS_STREAM3X3_D 6       // K steps the activation ring of the 3x3 streaming kernel runs ahead (a divisor of 18)
#define EOSVOS_STREAM_OCC 1        // workgroups per CU the K <= 128 variants are compiled for (2: 128 VGPRs, 4 fragments per pass)
template <int K, int NC>
__global__ __launch_bounds__(512, (K <= 128 ? EOSVOS_STREAM_OCC : 1)) void conv1x1_stream_kernel(const ConvArgs p) {
  constexpr int WAVES = 8;
  constexpr int KS = (K + 31) / 32;                   // K steps of the 16x16x32 MFMA (K = 304: the last one is half empty)
  constexpr int PITCH = frag_pitch(K * 2);            // bytes per weight row of one piece (conflict-free fragment reads)
  constexpr int NF = NC / 16;                         // 16-channel fragments of the column range
  constexpr int FHM = (K >= 256 || EOSVOS_STREAM_OCC > 1) ? 4 : 8;
  constexpr int FH = NF < FHM ? NF : FHM;             // fragments per pass (4 accumulator registers each)
  // K = 512: a strip's activations are 128 registers per lane.  The K steps become the OUTER loop (all NF accumulators live),
  // a K step's activations are split right before its MFMAs and its registers are refilled with the next strip's at once.
  constexpr bool KOUT = K >= 304;
  // K = 304 (the decoder's concatenated input): the lanes of the last K step whose 8 values lie past K carry zero
  // activations and read their weights from the start of the row instead (finite values: 0 * w = 0)
  constexpr bool KTAIL = (K % 32) != 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char s1_smem[];      // [2 pieces][NC rows][PITCH] | scale[NC] bias[NC] kscale[K]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // Column range and rows of this workgroup.  Plain conv: blockIdx.y = range, the strips of all rows go round-robin over the
  // waves of the range's workgroups.  Batched GEMM (plane_rows != 0: the Winograd-domain products): a workgroup belongs to one
  // (plane, row chunk) group and one column range; the groups' workgroups of all ranges get ids 8 apart, i.e. the same XCD at
  // the same time, so that the rows they all read meet in that XCD's L2.
  int n0 = blockIdx.y * NC;
  long rbase = 0, rend = p.M;
  int sbeg = blockIdx.x * WAVES + wave, sstride = gridDim.x * WAVES;
  const float* wsrc = p.w;
  if (p.plane_rows) {
    const int ranges = p.N / NC, chunks = p.row_chunks;
    const int i = blockIdx.x, xcd = i & 7, j = i >> 3;
    const int g = (j / ranges) * 8 + xcd;
    if (g >= p.nplanes * chunks) return;
    const int plane = g / chunks, chunk = g % chunks;
    const long per = (((long)p.plane_rows + chunks - 1) / chunks + 15) / 16 * 16;
    n0 = (j % ranges) * NC;
    rbase = (long)plane * p.plane_rows + chunk * per;
    rend = rbase + per;
    if (rend > (long)(plane + 1) * p.plane_rows) rend = (long)(plane + 1) * p.plane_rows;
    sbeg = wave; sstride = WAVES;
    wsrc = p.w + (size_t)plane * p.w_plane;
  }
  // per-channel epilogue / staging factors live in LDS: a global load per fragment and strip would stall every epilogue pass
  float* const s_sc = reinterpret_cast<float*>(s1_smem + 2 * NC * PITCH);
  float* const s_bi = s_sc + NC;
  float* const s_ks = s_bi + NC;
  // Prologue: EVERY global load -- this thread's weights, the per-channel factors, the absmax slot words -- is issued before
  // the first one is consumed.  Written statement by statement (load, use, load, use ...) the compiler waits for each load
  // where it is used: six serial memory round trips in front of the weight pass, and one per granule inside it (15 us of
  // a 39 us launch, measured on a 16 x 16 map where the launch is nothing but its prologue).  The two weight layouts' passes
  // are kept apart down to their stores: sharing the split / store code lets the compiler merge the forward pass's float4
  // loads into the data gradient's eight strided scalar loads per granule.
  static_assert(NC <= WAVES * 64 && K <= WAVES * 64, "one factor per thread");
  const float f_sc = (p.scale && tid < NC) ? p.scale[n0 + tid] : 1.f;
  const float f_bi = (p.bias && tid < NC) ? p.bias[n0 + tid] : 0.f;
  const float f_ks = (p.kscale && tid < K) ? p.kscale[tid] : 1.f;
  const unsigned ax = amax_issue(p.amax_x), aks = amax_issue(p.kmajor ? p.amax_ks : nullptr), aw = amax_issue(p.amax_w);
  float sx = 1.f, sw = 1.f, inv = 1.f;
  auto scales = [&]() {                               // first consumer: called once the weight loads are in flight too
    if (tid < NC) { s_sc[tid] = f_sc; s_bi[tid] = f_bi; }
    if (tid < KS * 32) s_ks[tid] = f_ks;
    float ix, iw;
    sx = h3_scale_bits(ax, p.kmajor && p.amax_ks, aks, ix);
    sw = h3_scale_bits(aw, false, 0u, iw);
    inv = ix * iw;
  };
  {
    constexpr int GR = NC * (K / 8), IT = (GR + WAVES * 64 - 1) / (WAVES * 64);
    if (!p.kmajor) {                                  // forward: W[n][K], a row's k contiguous
      float4 raw[IT][2];
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int i = tid + it * WAVES * 64;
        const int r = (i < GR ? i : 0) / (K / 8), c8 = i % (K / 8);
        const float* src = wsrc + (size_t)(n0 + r) * p.wK + c8 * 8;
        raw[it][0] = ldg4(src);
        raw[it][1] = ldg4(src + 4);
      }
      scales();
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int i = tid + it * WAVES * 64;
        if (i < GR) {
          const int r = i / (K / 8), c8 = i % (K / 8);
          uint4 h0, h1;
          s1_split8(raw[it][0], raw[it][1], sw, h0, h1);
          *reinterpret_cast<uint4*>(s1_smem + r * PITCH + c8 * 16) = h0;
          *reinterpret_cast<uint4*>(s1_smem + NC * PITCH + r * PITCH + c8 * 16) = h1;
        }
      }
    } else {                                          // data gradient: W[k][N]: consecutive lanes read consecutive n of one k row
      float raw[IT][8];
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int i = tid + it * WAVES * 64;
        const int c8 = (i < GR ? i : 0) / NC, r = i % NC;
        const float* src = wsrc + (size_t)(c8 * 8) * p.wK + n0 + r;
#pragma unroll
        for (int j = 0; j < 8; ++j) raw[it][j] = src[(size_t)j * p.wK];
      }
      scales();
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int i = tid + it * WAVES * 64;
        if (i < GR) {
          const int c8 = i / NC, r = i % NC;
          uint4 h0, h1;
          s1_split8(make_float4(raw[it][0], raw[it][1], raw[it][2], raw[it][3]), make_float4(raw[it][4], raw[it][5], raw[it][6], raw[it][7]), sw, h0, h1);
          *reinterpret_cast<uint4*>(s1_smem + r * PITCH + c8 * 16) = h0;
          *reinterpret_cast<uint4*>(s1_smem + NC * PITCH + r * PITCH + c8 * 16) = h1;
        }
      }
    }
  }
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  const int nstrips = (int)((rend - rbase + 15) / 16);
  const int gw = sbeg, gstride = sstride;
  // the tensor added to the output: residual / skip gradient, or (accumulating data gradient) the destination's old contents
  const float* const adp = p.res ? p.res : (p.accum ? p.y : nullptr);
  const int adld = p.res ? p.ldres : p.ldy;
  const bool both = p.res && p.accum;
  float4 xr[KS][2];
  auto load_x = [&](int strip) {
    const long m = rbase + (long)strip * 16 + fr;
    const float* q = p.x + (size_t)(m < rend ? m : rend - 1) * p.ldx + fq * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (!KTAIL || ks * 32 + fq * 8 < K) {
        xr[ks][0] = ldg4(q + ks * 32);
        xr[ks][1] = ldg4(q + ks * 32 + 4);
      } else {
        xr[ks][0] = xr[ks][1] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  unsigned ymax = 0;
  int strip = gw;
  // (Requesting a strip's addend rows and mask bytes one strip ahead, together with its activations, was measured with an
  // A/B switch since removed: per launch +-10 % either way, the iteration 9.50 (ahead) vs 9.45 ms.)
  auto load_ad = [&](int st, float4 (&ad)[FH], unsigned (&mk)[FH], int half) {
    const long m = rbase + (long)st * 16 + fr;
    const size_t r = (size_t)(m < rend ? m : rend - 1);
    if (adp) {
#pragma unroll
      for (int f = 0; f < FH; ++f) ad[f] = ldg4(adp + r * adld + n0 + (half + f) * 16 + 4 * fq);
    }
    if (p.mask8) {
#pragma unroll
      for (int f = 0; f < FH; ++f) mk[f] = p.mask8[r * p.ldm8 + ((n0 + (half + f) * 16) >> 2) + fq];
    }
  };
  if (strip < nstrips) load_x(strip);
  // epilogue of one 16-channel fragment: scale / shift / addend / ReLU / mask, float4 store + mask byte, absmax
  auto finish = [&](const f32x4& a4, int f16, const float4& adv, unsigned mkv, size_t row, bool ok) {
    const int n = n0 + f16 * 16 + 4 * fq;
    float4 v = make_float4(a4[0] * inv, a4[1] * inv, a4[2] * inv, a4[3] * inv);
    if (p.scale) { const float4 s4 = *reinterpret_cast<const float4*>(s_sc + (n - n0)); v.x *= s4.x; v.y *= s4.y; v.z *= s4.z; v.w *= s4.w; }
    if (p.bias) { const float4 b4 = *reinterpret_cast<const float4*>(s_bi + (n - n0)); v.x += b4.x; v.y += b4.y; v.z += b4.z; v.w += b4.w; }
    if (adp) { v.x += adv.x; v.y += adv.y; v.z += adv.z; v.w += adv.w; }
    if (both) { const float4 a2 = ldg4(p.y + row * p.ldy + n); v.x += a2.x; v.y += a2.y; v.z += a2.z; v.w += a2.w; }
    if (p.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    if (p.mask8 && n >= p.mask_c0) relu_mask8(v, mkv);
    if (ok) {
      *reinterpret_cast<float4*>(p.y + row * p.ldy + n) = v;
      if (p.mask8_out && p.relu) p.mask8_out[row * p.ldm8_out + (n >> 2)] = relu_bits(v);
      ymax = amax_f4(ymax, v);
    }
  };
  if constexpr (KOUT) {
    for (; strip < nstrips; strip += gstride) {
      const int nxt = strip + gstride;
      const bool more = nxt < nstrips;
      const long mn = rbase + (long)nxt * 16 + fr;
      const float* qn = p.x + (size_t)(mn < rend ? mn : rend - 1) * p.ldx + fq * 8;
      const long m = rbase + (long)strip * 16 + fr;
      const bool ok = m < rend;
      const size_t row = (size_t)(ok ? m : rend - 1);
      f32x4 acc[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        float4 a = xr[ks][0], b = xr[ks][1];
        if (more && (!KTAIL || ks * 32 + fq * 8 < K)) {      // this K step's registers take the next strip's activations right away
          xr[ks][0] = ldg4(qn + ks * 32);
          xr[ks][1] = ldg4(qn + ks * 32 + 4);
        }
        if (p.kscale) {
          const float4 k0 = *reinterpret_cast<const float4*>(s_ks + ks * 32 + fq * 8), k1 = *reinterpret_cast<const float4*>(s_ks + ks * 32 + fq * 8 + 4);
          a.x *= k0.x; a.y *= k0.y; a.z *= k0.z; a.w *= k0.w;
          b.x *= k1.x; b.y *= k1.y; b.z *= k1.z; b.w *= k1.w;
        }
        uint4 x0, x1;
        s1_split8(a, b, sx, x0, x1);
        const int koffs = (!KTAIL || ks * 32 + fq * 8 < K) ? ks * 64 + fq * 16 : 0;
#pragma unroll
        for (int h0 = 0; h0 < NF; h0 += FH) {
          uint4 w0[FH], w1[FH];
#pragma unroll
          for (int f = 0; f < FH; ++f) {
            const unsigned char* wp = s1_smem + ((h0 + f) * 16 + fr) * PITCH + koffs;
            w0[f] = *reinterpret_cast<const uint4*>(wp);
            w1[f] = *reinterpret_cast<const uint4*>(wp + NC * PITCH);
          }
#pragma unroll
          for (int f = 0; f < FH; ++f) acc[h0 + f] = MFMA_F16(__builtin_bit_cast(f16x8, w1[f]), __builtin_bit_cast(f16x8, x0), acc[h0 + f]);
#pragma unroll
          for (int f = 0; f < FH; ++f) acc[h0 + f] = MFMA_F16(__builtin_bit_cast(f16x8, w0[f]), __builtin_bit_cast(f16x8, x1), acc[h0 + f]);
#pragma unroll
          for (int f = 0; f < FH; ++f) acc[h0 + f] = MFMA_F16(__builtin_bit_cast(f16x8, w0[f]), __builtin_bit_cast(f16x8, x0), acc[h0 + f]);
          __builtin_amdgcn_sched_barrier(0);          // (keeps later work from being hoisted: register pressure)
        }
      }
#pragma unroll 1
      for (int h0 = 0; h0 < NF; h0 += FH) {
        float4 ad[FH];
        unsigned mk[FH];
        load_ad(strip, ad, mk, h0);
#pragma unroll
        for (int f = 0; f < FH; ++f) finish(acc[h0 + f], h0 + f, ad[f], mk[f], row, ok);
      }
    }
  } else
  for (; strip < nstrips; strip += gstride) {
    uint4 x0[KS], x1[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (p.kscale) {                                 // data gradient: the frozen-norm scale of the conv, per reduction channel
        const float4 k0 = *reinterpret_cast<const float4*>(s_ks + ks * 32 + fq * 8), k1 = *reinterpret_cast<const float4*>(s_ks + ks * 32 + fq * 8 + 4);
        xr[ks][0].x *= k0.x; xr[ks][0].y *= k0.y; xr[ks][0].z *= k0.z; xr[ks][0].w *= k0.w;
        xr[ks][1].x *= k1.x; xr[ks][1].y *= k1.y; xr[ks][1].z *= k1.z; xr[ks][1].w *= k1.w;
      }
      s1_split8(xr[ks][0], xr[ks][1], sx, x0[ks], x1[ks]);
    }
    float4 ad[FH];
    unsigned mk[FH];
    const int nxt = strip + gstride;
    if (nxt < nstrips) load_x(nxt);                   // the next strip's operands in flight behind this strip's work
    const long m = rbase + (long)strip * 16 + fr;
    const bool ok = m < rend;
    const size_t row = (size_t)(ok ? m : rend - 1);
#pragma unroll 1
    for (int half = 0; half < NF; half += FH) {
      load_ad(strip, ad, mk, half);
      f32x4 acc[FH];
#pragma unroll
      for (int f = 0; f < FH; ++f) {
        acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const unsigned char* wp = s1_smem + ((half + f) * 16 + fr) * PITCH + ks * 64 + fq * 16;
          const uint4 w0 = *reinterpret_cast<const uint4*>(wp);
          const uint4 w1 = *reinterpret_cast<const uint4*>(wp + NC * PITCH);
          acc[f] = MFMA_F16(__builtin_bit_cast(f16x8, w1), __builtin_bit_cast(f16x8, x0[ks]), acc[f]);      // smallest terms first
          acc[f] = MFMA_F16(__builtin_bit_cast(f16x8, w0), __builtin_bit_cast(f16x8, x1[ks]), acc[f]);
          acc[f] = MFMA_F16(__builtin_bit_cast(f16x8, w0), __builtin_bit_cast(f16x8, x0[ks]), acc[f]);
        }
        __builtin_amdgcn_sched_barrier(0);            // (keeps later fragments' reads from being hoisted: register pressure)
      }
#pragma unroll
      for (int f = 0; f < FH; ++f) {
        finish(acc[f], half + f, ad[f], mk[f], row, ok);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  if (p.amax_y) amax_block_commit<8>(ymax, p.amax_y);
}
// ---------------------------------------------------------------------------------------
// The same structure for layer1's 3x3 convs (64 -> 64 channels, stride 1, 77 040 pixels at batch 3), forward and data gradient:
// all 9 x 64 x 64 weights live in LDS as their two fp16 pieces (147 KB), a wave streams strips of 16 output pixels through
// the 18 K steps (tap-major: K step = tap x 32 channels), the activations of the (dy, dx)-shifted pixel come straight from
// global memory (zero outside the map) through a ring of D K steps that runs ahead across strip boundaries.  In the tiled
// kernel these launches ran at 85-100 TFLOP/s (57 / 65 us): 64-wide tiles with 18 K steps, half the MFMA work per staged
// operand byte.
// ---------------------------------------------------------------------------------------
template <int KC, int NC, int D>
__global__ __launch_bounds__(512, 1) void conv3x3_stream_kernel(const ConvArgs p) {
  constexpr int WAVES = 8, T = 9;
  constexpr int K = T * KC, KS = K / 32, KPT = KC / 32;        // K steps per tap
  constexpr int PITCH = frag_pitch(K * 2);
  constexpr int NF = NC / 16;
  static_assert(KS % D == 0 && NF <= 4, "ring depth must divide the K steps; every fragment's accumulator stays live");
  extern __shared__ __attribute__((aligned(16))) unsigned char s3_smem[];      // [2 pieces][NC rows][PITCH] | scale[NC] bias[NC] kscale[KC]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* const s_sc = reinterpret_cast<float*>(s3_smem + 2 * NC * PITCH);
  float* const s_bi = s_sc + NC;
  float* const s_ks = s_bi + NC;
  // Prologue: EVERY global load -- the nine taps' weights of this thread, the per-channel factors, the absmax slot words --
  // is issued before the first one is consumed.  Written statement by statement (load, use, load, use ...) the compiler
  // waits for each load where it is used: six to fifteen serial memory round trips, 12-15 us of a 39 us launch.
  constexpr int GR = NC * (K / 8), IT = (GR + WAVES * 64 - 1) / (WAVES * 64);
  static_assert(NC <= WAVES * 64 && KC <= WAVES * 64, "one factor per thread");
  // (the two layouts' passes are kept apart down to their stores: sharing the split / store code let the compiler merge the
  // forward pass's float4 loads into the data gradient's eight strided scalar loads per granule -- 17 us instead of 3)
  const float f_sc = (p.scale && tid < NC) ? p.scale[tid] : 1.f;
  const float f_bi = (p.bias && tid < NC) ? p.bias[tid] : 0.f;
  const float f_ks = (p.kscale && tid < KC) ? p.kscale[tid] : 1.f;
  const unsigned ax = amax_issue(p.amax_x), aks = amax_issue(p.kmajor ? p.amax_ks : nullptr), aw = amax_issue(p.amax_w);
  float sx = 1.f, sw = 1.f, inv = 1.f;
  auto scales = [&]() {                               // first consumer of the prologue's loads: called once the weights' are in flight too
    if (tid < NC) { s_sc[tid] = f_sc; s_bi[tid] = f_bi; }
    if (tid < KC) s_ks[tid] = f_ks;
    float ix, iw;
    sx = h3_scale_bits(ax, p.kmajor && p.amax_ks, aks, ix);
    sw = h3_scale_bits(aw, false, 0u, iw);
    inv = ix * iw;
  };
  if (!p.kmajor) {                                    // forward: W[n][tap][c], a row's 9 * KC values contiguous; LDS row n holds k = tap * KC + c
    float4 raw[IT][2];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * WAVES * 64;
      const int r = i / (K / 8), c8 = i % (K / 8);
      const float* src = p.w + (size_t)(i < GR ? r : 0) * T * p.wK + c8 * 8;
      raw[it][0] = ldg4(src);
      raw[it][1] = ldg4(src + 4);
    }
    scales();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * WAVES * 64;
      if (i < GR) {
        const int r = i / (K / 8), c8 = i % (K / 8);
        uint4 h0, h1;
        s1_split8(raw[it][0], raw[it][1], sw, h0, h1);
        *reinterpret_cast<uint4*>(s3_smem + r * PITCH + c8 * 16) = h0;
        *reinterpret_cast<uint4*>(s3_smem + NC * PITCH + r * PITCH + c8 * 16) = h1;
      }
    }
  } else {                                            // data gradient: W[c][tap][n]: consecutive lanes read consecutive n
    float raw[IT][8];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * WAVES * 64;
      const int c8 = (i < GR ? i : 0) / NC, r = i % NC;
      const int tap = (c8 * 8) / KC, c0 = (c8 * 8) % KC;
      const float* src = p.w + ((size_t)c0 * T + tap) * p.wK + r;
      const size_t st = (size_t)T * p.wK;
#pragma unroll
      for (int j = 0; j < 8; ++j) raw[it][j] = src[j * st];
    }
    scales();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * WAVES * 64;
      if (i < GR) {
        const int c8 = i / NC, r = i % NC;
        uint4 h0, h1;
        s1_split8(make_float4(raw[it][0], raw[it][1], raw[it][2], raw[it][3]), make_float4(raw[it][4], raw[it][5], raw[it][6], raw[it][7]), sw, h0, h1);
        *reinterpret_cast<uint4*>(s3_smem + r * PITCH + c8 * 16) = h0;
        *reinterpret_cast<uint4*>(s3_smem + NC * PITCH + r * PITCH + c8 * 16) = h1;
      }
    }
  }
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  const int nstrips = (p.M + 15) / 16;
  const int gstride = gridDim.x * WAVES;
  const float* const adp = p.res ? p.res : (p.accum ? p.y : nullptr);
  const int adld = p.res ? p.ldres : p.ldy;
  const bool both = p.res && p.accum;
  const int hw = p.Ho * p.Wo;
  // a strip's lane state: source offset of the unshifted pixel and the validity of the three row / column shifts
  struct Pix { long base, centre; unsigned ok; };    // ok: bit ky = row shift ky valid, bit 3 + kx = column shift kx valid
  auto pix_of = [&](int strip) {
    int m = strip * 16 + fr;
    m = m < p.M ? m : p.M - 1;
    const int b = m / hw, rem = m - b * hw;
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    Pix q;
    q.base = (((long)b * p.Hi + oy + p.off0) * p.Wi + ox + p.off0) * p.ldx + fq * 8;
    q.centre = (((long)b * p.Hi + oy) * p.Wi + ox) * p.ldx + fq * 8;
    q.ok = 0;
#pragma unroll
    for (int k3 = 0; k3 < 3; ++k3) {
      const int sy = oy + p.off0 + k3 * p.kstep, sx2 = ox + p.off0 + k3 * p.kstep;
      if (sy >= 0 && sy < p.Hi) q.ok |= 1u << k3;
      if (sx2 >= 0 && sx2 < p.Wi) q.ok |= 8u << k3;
    }
    return q;
  };
  float4 ring[D][2];
  // Straight-line code: a shifted pixel outside the map is loaded from the unshifted one instead and zeroed where the ring
  // slot is consumed.  With a branch around the loads the compiler can no longer count the loads in flight and drains them
  // all (s_waitcnt vmcnt(0)) at every wrap of the ring: three exposed memory round trips per strip.
  auto tap_ok = [&](const Pix& q, int ks) {
    const int tap = ks / KPT, ky = tap / 3, kx = tap % 3;
    return ((q.ok >> ky) & (q.ok >> (3 + kx)) & 1u) != 0;
  };
  auto load_k = [&](const Pix& q, int ks, float4 (&dst)[2]) {      // ks: compile-time constant at every call site
    const int tap = ks / KPT, kin = ks % KPT, ky = tap / 3, kx = tap % 3;
    const long off = tap_ok(q, ks) ? q.base + ((long)ky * p.kstep * p.Wi + kx * p.kstep) * p.ldx : q.centre;
    const float* src = p.x + off + kin * 32;
    dst[0] = ldg4(src);
    dst[1] = ldg4(src + 4);
  };
  unsigned ymax = 0;
  int strip = blockIdx.x * WAVES + wave;
  Pix cur = pix_of(strip < nstrips ? strip : 0);
  if (strip < nstrips) {
#pragma unroll
    for (int d = 0; d < D; ++d) load_k(cur, d, ring[d]);
  }
  for (; strip < nstrips; strip += gstride) {
    const int nxt = strip + gstride;
    const bool more = nxt < nstrips;
    const Pix nx = pix_of(more ? nxt : strip);
    const int m = strip * 16 + fr;
    const bool ok = m < p.M;
    const size_t row = (size_t)(ok ? m : p.M - 1);
    f32x4 acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool border = __any(cur.ok != 0x3fu);          // wave-uniform
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      // the slot is split in place and refilled afterwards (a copy of its 8 registers per K step otherwise); only strips that
      // touch the border of the map pay for zeroing their outside taps
      float4& a = ring[ks % D][0];
      float4& b = ring[ks % D][1];
      if (border && !tap_ok(cur, ks)) a = b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p.kscale) {
        const int kin = ks % KPT;
        const float4 k0 = *reinterpret_cast<const float4*>(s_ks + kin * 32 + fq * 8), k1 = *reinterpret_cast<const float4*>(s_ks + kin * 32 + fq * 8 + 4);
        a.x *= k0.x; a.y *= k0.y; a.z *= k0.z; a.w *= k0.w;
        b.x *= k1.x; b.y *= k1.y; b.z *= k1.z; b.w *= k1.w;
      }
      uint4 x0, x1;
      s1_split8(a, b, sx, x0, x1);
      if (ks + D < KS) load_k(cur, ks + D, ring[ks % D]);          // the ring runs D K steps ahead, across the strip boundary
      else load_k(nx, ks + D - KS, ring[ks % D]);                  // (past the last strip: the strip's own pixels once more)
      // (reading the weight fragments one K step ahead of their MFMAs was measured: no difference, 9.00 vs 9.01 ms)
      uint4 w0[NF], w1[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const unsigned char* wp = s3_smem + (f * 16 + fr) * PITCH + ks * 64 + fq * 16;
        w0[f] = *reinterpret_cast<const uint4*>(wp);
        w1[f] = *reinterpret_cast<const uint4*>(wp + NC * PITCH);
      }
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = MFMA_F16(__builtin_bit_cast(f16x8, w1[f]), __builtin_bit_cast(f16x8, x0), acc[f]);
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = MFMA_F16(__builtin_bit_cast(f16x8, w0[f]), __builtin_bit_cast(f16x8, x1), acc[f]);
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = MFMA_F16(__builtin_bit_cast(f16x8, w0[f]), __builtin_bit_cast(f16x8, x0), acc[f]);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int n = f * 16 + 4 * fq;
      float4 v = make_float4(acc[f][0] * inv, acc[f][1] * inv, acc[f][2] * inv, acc[f][3] * inv);
      if (p.scale) { const float4 s4 = *reinterpret_cast<const float4*>(s_sc + n); v.x *= s4.x; v.y *= s4.y; v.z *= s4.z; v.w *= s4.w; }
      if (p.bias) { const float4 b4 = *reinterpret_cast<const float4*>(s_bi + n); v.x += b4.x; v.y += b4.y; v.z += b4.z; v.w += b4.w; }
      if (adp) { const float4 a4 = ldg4(adp + row * adld + n); v.x += a4.x; v.y += a4.y; v.z += a4.z; v.w += a4.w; }
      if (both) { const float4 a2 = ldg4(p.y + row * p.ldy + n); v.x += a2.x; v.y += a2.y; v.z += a2.z; v.w += a2.w; }
      if (p.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      if (p.mask8 && n >= p.mask_c0) relu_mask8(v, p.mask8[row * p.ldm8 + (n >> 2)]);
      if (ok) {
        *reinterpret_cast<float4*>(p.y + row * p.ldy + n) = v;
        if (p.mask8_out && p.relu) p.mask8_out[row * p.ldm8_out + (n >> 2)] = relu_bits(v);
        ymax = amax_f4(ymax, v);
      }
    }
    cur = nx;
  }
  if (p.amax_y) amax_block_commit<8>(ymax, p.amax_y);
}
static bool stream3x3_ok(const ConvArgs& a) {
  constexpr int min_m = 16384;
  if (conv_mfma_mode() != 2 || a.nseg > 0 || a.plane_rows || a.KH != 3 || a.KW != 3 || a.upshift || a.dst_up || a.par ||
      a.tprefix || a.mul != 1 || a.M < min_m)
    return false;
  if (a.Kc != 64 || a.N != 64 || a.wK != 64) return false;
  if ((a.mask_c0 & 15) || (a.ldx & 3) || (a.ldy & 3)) return false;
  if (a.Hi != a.Ho || a.Wi != a.Wo) return false;
  if (!(a.kstep == 1 || a.kstep == -1) || a.off0 != -a.kstep) return false;      // pad 1, dilation 1 (forward: -1 / +1, data gradient: +1 / -1)
  return true;
}
static void launch_stream3x3(const ConvArgs& a, hipStream_t s) {
  constexpr int KC = 64, NC = 64, D = EOSVOS_STREAM3X3_D;
  constexpr int lds = 2 * NC * frag_pitch(9 * KC * 2) + (2 * NC + KC) * 4;
  static bool attr = false;
  if (!attr) { (void)hipFuncSetAttribute((const void*)conv3x3_stream_kernel<KC, NC, D>, hipFuncAttributeMaxDynamicSharedMemorySize, lds); attr = true; }
  hipLaunchKernelGGL((conv3x3_stream_kernel<KC, NC, D>), dim3(256), dim3(512), lds, s, a);
}
// the launches the streaming kernel takes (f16x3 mode): 1x1, stride 1, K in {64, 128, 256}, whole column ranges, many pixels
static int stream1x1_nc(const ConvArgs& a) {
  // pixels from which on: 16 384 at batch 3 (below: +-0 in the iteration), 1 024 at batch 1 (layer2's 6 420 and layer3 / 4's
  // 1 620 pixels: 4.68 -> 4.65 ms; batch 3 8.86 -> 8.88 with the same rule)
  const int min_m = a.B == 1 && !a.plane_rows ? 1024 : 16384;
  if (conv_mfma_mode() != 2 || a.nseg > 0 || a.KH != 1 || a.KW != 1 || a.upshift || a.dst_up || a.par ||
      a.tprefix || a.mul != 1 || a.off0 != 0 || a.M < min_m)
    return 0;
  if (a.plane_rows) {
    // batched GEMMs of the Winograd-domain convs (decoder), K = 256: 128-channel column ranges (the rows are re-read by the
    // two ranges of a group from one XCD's L2), or the 48-channel tail of the 304-wide data gradient.  Measured at batch 3
    // (one stream): 139 -> 122 us forward, 149 / 153 -> 110 / 113 us data gradients, tail 64 -> 46 us; iteration 9.20 -> 9.07 ms.
    // 64-channel ranges (measured with an A/B switch since removed; they also take K = 304 in the 320 variant) are slower than
    // the tiled kernel: 4 x 36 workgroups per row chunk leave either 56 % of the CUs busy or a second round (195 / 232 us).
    if (a.mask8 || a.res || a.accum || a.scale || a.bias || a.relu || a.kscale || a.amax_y) return 0;
    if ((a.ldx & 3) || (a.ldy & 3) || (a.plane_rows & 15)) return 0;
    if (a.Kc != 256 && !(a.Kc == 304 && !a.kmajor)) return 0;
    if (a.N % 128 == 0) return 128;
    if (a.N % 64 == 0) return 64;
    if (a.N == 48 && a.Kc == 256) return 48;
    return 0;
  }
  if (a.Kc != 64 && a.Kc != 128 && a.Kc != 256 && a.Kc != 512) return 0;
  if ((a.mask_c0 & 15) || (a.ldx & 3) || (a.ldy & 3) || (a.N & 15)) return 0;
  if (a.Hi != a.Ho || a.Wi != a.Wo) return 0;
  if (a.Kc == 512) return a.N % 64 == 0 && a.N <= 128 ? 64 : 0;     // (weights of 64 channels x 512: 133 KB of LDS)
  if (a.N % 128 == 0) return 128;
  if (a.N == 64) return 64;
  if (a.N == 48 && a.Kc == 256) return 48;
  return 0;
}
template <int K, int NC>
static void launch_stream1x1(ConvArgs& a, hipStream_t s) {
  constexpr int lds = 2 * NC * frag_pitch(K * 2) + (2 * NC + (K + 31) / 32 * 32) * 4;
  static bool attr = false;
  if (!attr) { (void)hipFuncSetAttribute((const void*)conv1x1_stream_kernel<K, NC>, hipFuncAttributeMaxDynamicSharedMemorySize, lds); attr = true; }
  if (a.plane_rows) {
    // groups = planes x row chunks, each with one workgroup per column range; about `target` workgroups in all
    constexpr int target = 216;      // measured: 144 / 216 / 256
    const int ranges = a.N / NC;
    int chunks = (target + a.nplanes * ranges - 1) / (a.nplanes * ranges);
    const int max_chunks = a.plane_rows / 128 > 0 ? a.plane_rows / 128 : 1;      // >= one strip per wave
    chunks = chunks < 1 ? 1 : (chunks > max_chunks ? max_chunks : chunks);
    a.row_chunks = chunks;
    const int groups8 = (a.nplanes * chunks + 7) / 8 * 8;
    hipLaunchKernelGGL((conv1x1_stream_kernel<K, NC>), dim3(groups8 * ranges), dim3(512), lds, s, a);
    return;
  }
  // one workgroup per CU over all column ranges together (a workgroup's 8 waves take the strips of its range round-robin):
  // measured per shape with 128 / 256 / 512 / 1024 workgroups per range, 256 in all is the fastest or within 2 % of it
  constexpr int total = 256 * (K <= 128 ? EOSVOS_STREAM_OCC : 1);
  const int ranges = a.N / NC;
  const int wgs = total / ranges > 0 ? total / ranges : 1;
  hipLaunchKernelGGL((conv1x1_stream_kernel<K, NC>), dim3(wgs, ranges), dim3(512), lds, s, a);
}


// ---------------------------------------------------------------------------------------
// Stem (7x7 stride-2 conv, 3 -> 64, on the 3-pixel zero-padded NHWC3 frame) on the fp16 matrix cores, f16x3 mode.
// Same structure as the streaming 1x1 kernel: the whole 64 x 147 weight panel lives in LDS as its two fp16 pieces (split
// once per workgroup; its absmax is taken while it is staged), each wave streams strips of 16 output pixels, D = W_frag *
// patch_frag^T, so a lane ends with 4 consecutive channels of one pixel.  K order: 24 slots of 8 values, slot s = 3 ky + part
// holds floats [8 part, 8 part + 8) of the 21-float patch row ky (floats 21 ... 23 of a row belong to the next pixel -- or, for
// the last pixel of an odd x odd frame, lie past the frame in the allocation's zeroed 8-float tail; they meet zero weights
// AND are zeroed after the load: a stale value above 2 x the frame's absmax would become inf in fp16 and inf x 0 = NaN, which
// the ReLU turned into 0 -- round 5, the 1 x 97 x 163 guard trip; slots 21 ... 23 are not loaded): a lane's 8 k values are 32
// contiguous bytes of the frame, 8-byte aligned for even padded widths only (odd widths: 4-byte aligned dwordx2 loads).
// The VALU kernel (misc_kernels.hip) took 93 us at batch 3 -- 5.8 GFLOP of fp32 FMAs; the output (79 MB) bounds this one.
// ---------------------------------------------------------------------------------------
#define STEM_SLOTS 24
#define STEM_PITCH (STEM_SLOTS * 16 + 32)       // 32 mod 64: see frag_pitch
__global__ __launch_bounds__(512) void stem_fwd_h3_kernel(const float* __restrict__ xpad, const float* __restrict__ w,
                                                          const float* __restrict__ a, const float* __restrict__ bb,
                                                          float* __restrict__ y, int B, int H, int W, int Ho, int Wo,
                                                          const unsigned* __restrict__ amax_x) {
  __shared__ __attribute__((aligned(16))) unsigned char sw_[2 * 64 * STEM_PITCH];
  __shared__ float s_a[64], s_b[64];
  __shared__ unsigned s_red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // ---- weights: 64 rows x 24 slots, three slots per thread; absmax, then the split ----
  float wv[3][8];
  unsigned wm = 0;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int i = tid + q * 512, r = i / STEM_SLOTS, sl = i % STEM_SLOTS;
    const int ky = sl / 3, part = sl % 3;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int j = part * 8 + t;
      const float v = (sl < 21 && j < 21) ? w[r * 147 + ky * 21 + j] : 0.f;
      wv[q][t] = v;
      const unsigned b = amax_f1(v);
      wm = wm > b ? wm : b;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = (unsigned)__shfl_xor((int)wm, o);
    wm = wm > t ? wm : t;
  }
  if (lane == 0) s_red[wave] = wm;
  if (tid < 64) { s_a[tid] = a ? a[tid] : 1.f; s_b[tid] = bb ? bb[tid] : 0.f; }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) wm = wm > s_red[i] ? wm : s_red[i];
  float sw, iw;
  {
    const int e = (int)((wm >> 23) & 0xffu);
    int f = 268 - e;
    f = f < 1 ? 1 : (f > 254 ? 254 : f);
    iw = __uint_as_float((unsigned)(254 - f) << 23);
    sw = __uint_as_float((unsigned)f << 23);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int i = tid + q * 512, r = i / STEM_SLOTS, sl = i % STEM_SLOTS;
    uint4 h0, h1;
    s1_split8(make_float4(wv[q][0], wv[q][1], wv[q][2], wv[q][3]), make_float4(wv[q][4], wv[q][5], wv[q][6], wv[q][7]), sw, h0, h1);
    *reinterpret_cast<uint4*>(sw_ + r * STEM_PITCH + sl * 16) = h0;
    *reinterpret_cast<uint4*>(sw_ + 64 * STEM_PITCH + r * STEM_PITCH + sl * 16) = h1;
  }
  float ix;
  const float sx = h3_scale(amax_x, nullptr, ix);
  const float inv = ix * iw;
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  const int Wp = W + 6, Hp = H + 6;
  const long P = (long)B * Ho * Wo;
  const long nstrips = (P + 15) / 16;
  // this lane's slot of each K step: offset inside the frame relative to the pixel's patch origin; < 0: an empty slot
  int koff[6];
  int ktail = 0;                                  // bit ks: this lane's slot of K step ks is the third of a patch row
#pragma unroll
  for (int ks = 0; ks < 6; ++ks) {
    const int sl = ks * 4 + fq;
    koff[ks] = sl < 21 ? (sl / 3) * Wp * 3 + (sl % 3) * 8 : -1;
    if (sl < 21 && sl % 3 == 2) ktail |= 1 << ks;
  }
  float2 xr[6][4];
  auto load_x = [&](long strip) {
    long pp = strip * 16 + fr;
    pp = pp < P ? pp : P - 1;
    const int ox = (int)(pp % Wo), oy = (int)((pp / Wo) % Ho), b = (int)(pp / ((long)Wo * Ho));
    const float* base = xpad + (((long)b * Hp + oy * 2) * Wp + ox * 2) * 3;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
      if (koff[ks] >= 0) {
        const float2* q = reinterpret_cast<const float2*>(base + koff[ks]);
#pragma unroll
        for (int t = 0; t < 4; ++t) xr[ks][t] = q[t];
        if (ktail & (1 << ks)) { xr[ks][2].y = 0.f; xr[ks][3] = make_float2(0.f, 0.f); }      // floats 21 ... 23 of the patch row
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) xr[ks][t] = make_float2(0.f, 0.f);
      }
    }
  };
  const long gw = (long)blockIdx.x * 8 + wave, gstride = (long)gridDim.x * 8;
  long strip = gw;
  if (strip < nstrips) load_x(strip);
  for (; strip < nstrips; strip += gstride) {
    uint4 x0[6], x1[6];
#pragma unroll
    for (int ks = 0; ks < 6; ++ks)
      s1_split8(make_float4(xr[ks][0].x, xr[ks][0].y, xr[ks][1].x, xr[ks][1].y), make_float4(xr[ks][2].x, xr[ks][2].y, xr[ks][3].x, xr[ks][3].y),
                sx, x0[ks], x1[ks]);
    if (strip + gstride < nstrips) load_x(strip + gstride);
    const long pp = strip * 16 + fr;
    const bool ok = pp < P;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) {
        const unsigned char* wp = sw_ + (f * 16 + fr) * STEM_PITCH + ks * 64 + fq * 16;
        const uint4 w0 = *reinterpret_cast<const uint4*>(wp);
        const uint4 w1 = *reinterpret_cast<const uint4*>(wp + 64 * STEM_PITCH);
        acc = MFMA_F16(__builtin_bit_cast(f16x8, w1), __builtin_bit_cast(f16x8, x0[ks]), acc);
        acc = MFMA_F16(__builtin_bit_cast(f16x8, w0), __builtin_bit_cast(f16x8, x1[ks]), acc);
        acc = MFMA_F16(__builtin_bit_cast(f16x8, w0), __builtin_bit_cast(f16x8, x0[ks]), acc);
      }
      const int n = f * 16 + 4 * fq;
      float4 v = make_float4(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
      if (a) {
        const float4 a4 = *reinterpret_cast<const float4*>(s_a + n), b4 = *reinterpret_cast<const float4*>(s_b + n);
        v.x = fmaxf(v.x * a4.x + b4.x, 0.f); v.y = fmaxf(v.y * a4.y + b4.y, 0.f);
        v.z = fmaxf(v.z * a4.z + b4.z, 0.f); v.w = fmaxf(v.w * a4.w + b4.w, 0.f);
      }
      if (ok) *reinterpret_cast<float4*>(y + pp * 64 + n) = v;
      __builtin_amdgcn_sched_barrier(0);            // (keeps the next fragments' weight reads from being hoisted: registers)
    }
  }
}
void launch_stem_fwd_h3(const float* xpad, const float* w, const float* a, const float* b, float* y, int B, int H, int W, int Ho,
                        int Wo, const unsigned* amax_x, hipStream_t s) {
  hipLaunchKernelGGL(stem_fwd_h3_kernel, dim3(256), dim3(512), 0, s, xpad, w, a, b, y, B, H, W, Ho, Wo, amax_x);
}

// Stem weight gradient on the fp16 matrix cores (f16x3): dW[64][147] = sum_p G[p][64]^T * patch[p][147], one [64][147] slab
// per workgroup (a chunk of the output pixels), summed by the update kernel like every other layer's slabs.  Per 32-pixel K
// step: G rows come in as float4 (a thread owns 2 pixels x 4 channels and packs along the pixels), the 7 x 21 patch of every
// pixel by one thread per patch element, which walks the 32 pixels with scalar loads and owns their 64 contiguous bytes of
// its LDS row; wave w multiplies channels [16 w, 16 w + 16) with all ten 16-wide fragments of the (147 -> 160) patch rows.
__global__ __launch_bounds__(256, 2) void stem_wgrad_h3_kernel(const float* __restrict__ xpad, const float* __restrict__ g,
                                                               float* __restrict__ ws, int B, int H, int W, int Ho, int Wo,
                                                               int chunks, const unsigned* __restrict__ amax_g,
                                                               const unsigned* __restrict__ amax_x) {
  constexpr int KR = 160;                               // patch rows (147 padded to ten fragments)
  __shared__ __attribute__((aligned(16))) unsigned char As[2 * 64 * X6_ROWB];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[2 * KR * X6_ROWB];
  const long P = (long)B * Ho * Wo;
  const long per = ((P + chunks - 1) / chunks + 31) / 32 * 32;
  const long p0 = (long)blockIdx.x * per;
  long p1 = p0 + per;
  if (p1 > P) p1 = P;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int Wp = W + 6, Hp = H + 6;
  const int k = tid;                                    // B staging: one thread per patch element k
  const int koff = k < 147 ? (k / 21) * Wp * 3 + (k % 21) : 0;
  const int a_cg = tid & 15, a_pg = tid >> 4;           // A staging: channels [4 a_cg, + 4) of pixels 2 a_pg, 2 a_pg + 1
  float ig, ix;
  const unsigned ag_w = amax_issue(amax_g), ax_w = amax_issue(amax_x);
  const float sg = h3_scale_bits(ag_w, false, 0u, ig), sx = h3_scale_bits(ax_w, false, 0u, ix);
  f32x4 acc[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // rows 147 ... 159 of both pieces stay zero
  for (int i = tid; i < 2 * (KR - 147) * (X6_ROWB / 4); i += 256) {
    const int pc = i / ((KR - 147) * (X6_ROWB / 4)), rem = i % ((KR - 147) * (X6_ROWB / 4));
    *reinterpret_cast<unsigned*>(Bs + (pc * KR + 147) * X6_ROWB + rem * 4) = 0u;
  }
  const int nsteps = p1 > p0 ? (int)((p1 - p0 + 31) / 32) : 0;
  float4 ra[2];
  float rb[32];
  auto load_step = [&](int st) {
    const long ps = p0 + (long)st * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long px = ps + a_pg * 2 + i;
      ra[i] = px < p1 ? ldg4(g + px * 64 + a_cg * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (k < 147) {
      int ox = (int)(ps % Wo), oy = (int)((ps / Wo) % Ho), b = (int)(ps / ((long)Wo * Ho));
      long base = (((long)b * Hp + oy * 2) * Wp + ox * 2) * 3 + koff;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        rb[i] = (ps + i) < p1 ? xpad[base] : 0.f;
        base += 6;
        if (++ox == Wo) {
          ox = 0;
          base += (long)(2 * Wp - 2 * Wo) * 3;
          if (++oy == Ho) { oy = 0; base += (long)(Hp - 2 * Ho) * Wp * 3; }
        }
      }
    }
  };
  auto store_step = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j) {                        // channel 4 a_cg + j: the two pixels' values as one fp16 pair per piece
      unsigned pc[2];
      xs_split2<2>(f4c(ra[0], j), f4c(ra[1], j), sg, pc);
      *reinterpret_cast<unsigned*>(As + (a_cg * 4 + j) * X6_ROWB + a_pg * 4) = pc[0];
      *reinterpret_cast<unsigned*>(As + (64 + a_cg * 4 + j) * X6_ROWB + a_pg * 4) = pc[1];
    }
    if (k < 147) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint4 h0, h1;
        s1_split8(make_float4(rb[8 * q], rb[8 * q + 1], rb[8 * q + 2], rb[8 * q + 3]),
                  make_float4(rb[8 * q + 4], rb[8 * q + 5], rb[8 * q + 6], rb[8 * q + 7]), sx, h0, h1);
        *reinterpret_cast<uint4*>(Bs + k * X6_ROWB + q * 16) = h0;
        *reinterpret_cast<uint4*>(Bs + (KR + k) * X6_ROWB + q * 16) = h1;
      }
    }
  };
  if (nsteps > 0) load_step(0);
  __syncthreads();
  if (nsteps > 0) store_step();
  __syncthreads();
  for (int st = 0; st < nsteps; ++st) {
    const bool more = st + 1 < nsteps;
    if (more) load_step(st + 1);
    const uint4 a0 = *reinterpret_cast<const uint4*>(As + (wave * 16 + fr) * X6_ROWB + fq * 16);
    const uint4 a1 = *reinterpret_cast<const uint4*>(As + (64 + wave * 16 + fr) * X6_ROWB + fq * 16);
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const uint4 b0 = *reinterpret_cast<const uint4*>(Bs + (j * 16 + fr) * X6_ROWB + fq * 16);
      const uint4 b1 = *reinterpret_cast<const uint4*>(Bs + (KR + j * 16 + fr) * X6_ROWB + fq * 16);
      acc[j] = MFMA_F16(__builtin_bit_cast(f16x8, a1), __builtin_bit_cast(f16x8, b0), acc[j]);
      acc[j] = MFMA_F16(__builtin_bit_cast(f16x8, a0), __builtin_bit_cast(f16x8, b1), acc[j]);
      acc[j] = MFMA_F16(__builtin_bit_cast(f16x8, a0), __builtin_bit_cast(f16x8, b0), acc[j]);
    }
    __syncthreads();
    if (more) store_step();
    __syncthreads();
  }
  const float inv = ig * ix;
  float* out = ws + (long)blockIdx.x * (64 * 147);
#pragma unroll
  for (int j = 0; j < 10; ++j) {
    const int kk = j * 16 + fr;
    if (kk < 147) {
#pragma unroll
      for (int e = 0; e < 4; ++e) out[(wave * 16 + 4 * fq + e) * 147 + kk] = acc[j][e] * inv;
    }
  }
}
void launch_stem_wgrad_h3(const float* xpad, const float* g, float* ws, int B, int H, int W, int Ho, int Wo, int chunks,
                          const unsigned* amax_g, const unsigned* amax_x, hipStream_t s) {
  hipLaunchKernelGGL(stem_wgrad_h3_kernel, dim3(chunks), dim3(256), 0, s, xpad, g, ws, B, H, W, Ho, Wo, chunks, amax_g, amax_x);
}


// Weight gradient on the bf16 matrix cores: same split, both operands K-major (a pixel's channels are contiguous).
template <int BMO, int BNI, int NP> constexpr int wgrad_xs_smem() { return xs_max(NP * (BMO + BNI) * X6_ROWB, BMO * (BNI + 4) * 4); }
template <int BMO, int BNI, int NP = 3>
__device__ __forceinline__ void wgrad_x6_body(const WgradArgs& p, const int bid, unsigned char* smem) {
  constexpr int BKP = 32;
  constexpr int A_BYTES = NP * BMO * X6_ROWB;
  constexpr int LDC = BNI + 4;
  unsigned char* const As = smem;
  unsigned char* const Bs = smem + A_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;              // fragment row / 16-byte k slot of this lane

  const int T = p.KH * p.KW;
  const int ct = (p.Cout + BMO - 1) / BMO, it = (p.Cin + BNI - 1) / BNI;
  const int tiles = ct * it * T;
  const int z = bid / tiles;
  int tile = bid - z * tiles;
  const int tap = tile % T; tile /= T;
  const int co0 = (tile / it) * BMO, ci0 = (tile % it) * BNI;
  const int ky = tap / p.KW, kx = tap - ky * p.KW;

  const int dyk = ky * p.dil - p.pad, dxk = kx * p.dil - p.pad;
  auto cdiv = [](int a, int b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); };
  auto fdiv = [](int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
  int oy_lo = cdiv(-dyk, p.stride), oy_hi = fdiv(p.Hi - 1 - dyk, p.stride);
  int ox_lo = cdiv(-dxk, p.stride), ox_hi = fdiv(p.Wi - 1 - dxk, p.stride);
  if (oy_lo < 0) oy_lo = 0;
  if (ox_lo < 0) ox_lo = 0;
  if (oy_hi > p.Ho - 1) oy_hi = p.Ho - 1;
  if (ox_hi > p.Wo - 1) ox_hi = p.Wo - 1;
  const int hv = oy_hi - oy_lo + 1 > 0 ? oy_hi - oy_lo + 1 : 0;
  const int wv = ox_hi - ox_lo + 1 > 0 ? ox_hi - ox_lo + 1 : 0;
  const int P = p.B * hv * wv;                         // contributing pixels
  const int steps = (P + BKP - 1) / BKP;
  const int st_begin = (int)(((long)steps * z) / p.splits);
  const int st_end = (int)(((long)steps * (z + 1)) / p.splits);

  // a thread owns RPT consecutive pixels x 4 channels of each operand
  constexpr int ANQ = BMO / 4, ARPT = BMO / 32, BNQ = BNI / 4, BRPT = BNI / 32;
  const int a_c4 = ARPT == 4 ? x6_kmaj_c4_128(tid) : x6_kmaj_c4_64(tid), a_kq = ARPT == 4 ? x6_kmaj_kq_128(tid) : x6_kmaj_kq_64(tid);
  const int b_c4 = BRPT == 4 ? x6_kmaj_c4_128(tid) : x6_kmaj_c4_64(tid), b_kq = BRPT == 4 ? x6_kmaj_kq_128(tid) : x6_kmaj_kq_64(tid);
  const bool a_cok = (co0 + a_c4 * 4) < p.Cout;
  const bool b_cok = (ci0 + b_c4 * 4) < p.Cin;
  float4 ra[ARPT], rb[BRPT];
  constexpr unsigned OOB = 0x80000000u;
  const __amdgpu_buffer_rsrc_t rg = make_rsrc(p.g + tap * p.g_tap_stride, (long)p.B * p.Ho * p.Wo * p.ldg * 4);
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x + tap * p.x_tap_stride, (long)p.B * p.Hi * p.Wi * p.ldx * 4);
  float sa = 1.f, sb = 1.f, inv_ab = 1.f;
  if (NP == 2) {
    float ia, ib;
    const unsigned ag_w = amax_issue(p.amax_g), ax_w = amax_issue(p.amax_x);      // both slots' words in one round trip
    sa = h3_scale_bits(ag_w, false, 0u, ia);
    sb = h3_scale_bits(ax_w, false, 0u, ib);
    inv_ab = ia * ib;
    // standing in for the pre-split kernel: the scales for the next iteration's sibling producers (presplit_kernels.hip)
    if (bid == 0 && tid == 0) {
      if (p.scn_g) { int f = (int)((__float_as_uint(sa) >> 23) & 0xffu) - p.margin_g; f = f < 1 ? 1 : f; *p.scn_g = __uint_as_float((unsigned)f << 23); }
      if (p.scn_x) { int f = (int)((__float_as_uint(sb) >> 23) & 0xffu) - p.margin_x; f = f < 1 ? 1 : f; *p.scn_x = __uint_as_float((unsigned)f << 23); }
    }
  }
  const int hw = hv * wv > 0 ? hv * wv : 1, wv1 = wv > 0 ? wv : 1;
  const float inv_hw = 1.0f / (float)hw, inv_wv = 1.0f / (float)wv1;
  // contributing pixel q -> (image, row, column) of the rectangle; q < 2^24, so one float multiply +- 1 is exact
  auto pix = [&](int q, int& img, int& y, int& x) {
    int b = (int)((float)q * inv_hw);
    if (b * hw > q) --b; else if ((b + 1) * hw <= q) ++b;
    const int rem = q - b * hw;
    int yy = (int)((float)rem * inv_wv);
    if (yy * wv1 > rem) --yy; else if ((yy + 1) * wv1 <= rem) ++yy;
    img = b; y = yy; x = rem - yy * wv1;
  };
  // The rectangle is the whole map and source / destination pixels coincide (1x1 stride-1 convs, the Winograd planes):
  // contributing pixel q is pixel q of both tensors -- no (image, row, column) bookkeeping (wave-uniform branch)
  const bool linear = hv == p.Ho && wv == p.Wo && p.stride == 1 && dyk == 0 && dxk == 0 && p.Hi == p.Ho && p.Wi == p.Wo;
  const unsigned a_lin = (unsigned)(co0 + a_c4 * 4) * 4u, b_lin = (unsigned)(ci0 + b_c4 * 4) * 4u;
  const unsigned a_pitch = (unsigned)p.ldg * 4u, b_pitch = (unsigned)p.ldx * 4u;
  auto load_tiles = [&](int st) {
    if (linear) {
      const int qa = st * BKP + a_kq * ARPT, qb = st * BKP + b_kq * BRPT;
#pragma unroll
      for (int i = 0; i < ARPT; ++i)
        ra[i] = bufld4(rg, (a_cok && qa + i < P) ? (unsigned)(qa + i) * a_pitch + a_lin : OOB);
#pragma unroll
      for (int i = 0; i < BRPT; ++i)
        rb[i] = bufld4(rx, (b_cok && qb + i < P) ? (unsigned)(qb + i) * b_pitch + b_lin : OOB);
      return;
    }
    {
      int img, y, x;
      pix(st * BKP + a_kq * ARPT, img, y, x);
#pragma unroll
      for (int i = 0; i < ARPT; ++i) {
        const bool ok = a_cok && img < p.B;
        const unsigned off = ok ? (unsigned)(((img * p.Ho + oy_lo + y) * p.Wo + ox_lo + x) * p.ldg + co0 + a_c4 * 4) * 4u : OOB;
        ra[i] = bufld4(rg, off);
        if (++x >= wv1) { x = 0; if (++y >= hv) { y = 0; ++img; } }
      }
    }
    {
      int img, y, x;
      pix(st * BKP + b_kq * BRPT, img, y, x);
#pragma unroll
      for (int i = 0; i < BRPT; ++i) {
        const int iy = (oy_lo + y) * p.stride + dyk, ix = (ox_lo + x) * p.stride + dxk;
        const bool ok = b_cok && img < p.B;
        const unsigned off = ok ? (unsigned)(((img * p.Hi + iy) * p.Wi + ix) * p.ldx + ci0 + b_c4 * 4) * 4u : OOB;
        rb[i] = bufld4(rx, off);
        if (++x >= wv1) { x = 0; if (++y >= hv) { y = 0; ++img; } }
      }
    }
  };
  auto store_op = [&](unsigned char* S, const float4* rv, int W, int NQ_, int RPT_, int c4, int kq, float sc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {              // channel 4*c4 + j of the tile lives in LDS row j*NQ + c4
      if (RPT_ == 4) {
        uint2 pc[NP];
        xs_split4<NP>(f4c(rv[0], j), f4c(rv[1], j), f4c(rv[RPT_ == 4 ? 2 : 0], j), f4c(rv[RPT_ == 4 ? 3 : 0], j), sc, pc);
#pragma unroll
        for (int q = 0; q < NP; ++q) *reinterpret_cast<uint2*>(S + (q * W + j * NQ_ + c4) * X6_ROWB + kq * 8) = pc[q];
      } else {
        unsigned pc[NP];
        xs_split2<NP>(f4c(rv[0], j), f4c(rv[1], j), sc, pc);
#pragma unroll
        for (int q = 0; q < NP; ++q) *reinterpret_cast<unsigned*>(S + (q * W + j * NQ_ + c4) * X6_ROWB + kq * 4) = pc[q];
      }
    }
  };

  constexpr int TM = BMO / 32, TN = BNI / 32;            // 16 x 16 fragments of a wave's (BMO/2) x (BNI/2) tile
  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

  if (st_begin < st_end) {
    load_tiles(st_begin);
    store_op(As, ra, BMO, ANQ, ARPT, a_c4, a_kq, sa);
    store_op(Bs, rb, BNI, BNQ, BRPT, b_c4, b_kq, sb);
  }
  __syncthreads();
  for (int st = st_begin; st < st_end; ++st) {
    const bool more = (st + 1) < st_end;
    if (more) load_tiles(st + 1);
    __builtin_amdgcn_s_setprio(1);
    x6_mma_step<TM, TN, TM, NP>(As, Bs, BMO, BNI, wm * (BMO / 2), wn * (BNI / 2), fr, fq, acc);
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    if (more) {
      store_op(As, ra, BMO, ANQ, ARPT, a_c4, a_kq, sa);
      store_op(Bs, rb, BNI, BNQ, BRPT, b_c4, b_kq, sb);
    }
    __syncthreads();
  }

  // epilogue: accumulators -> LDS tile (channels back in order) -> full-row float4 stores of the slab
  float* Cs = reinterpret_cast<float*>(smem);
  float* out = p.ws + (size_t)z * p.Cout * T * p.Cin;
  constexpr int CF4 = BNI / 4, CROWS = 256 / CF4;
  const int c_c4 = tid % CF4, c_r = tid / CF4;
  // tile row (cout) of accumulator element e of fragment tm: Ra = wm*(BMO/2) + tm*16 + 4*fq + e,
  // channel = 4*(Ra % (BMO/4)) + Ra / (BMO/4); tile column likewise from Rb = wn*(BNI/2) + tn*16 + fr.
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int ncol = x6_row_chan(wn * (BNI / 2) + tn * 16 + fr, BNI);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ch = x6_row_chan(wm * (BMO / 2) + tm * 16 + 4 * fq + e, BMO);
        Cs[ch * LDC + ncol] = NP == 2 ? acc[tm][tn][e] * inv_ab : acc[tm][tn][e];
      }
    }
  __syncthreads();
  const int ci = ci0 + c_c4 * 4;
  if (ci < p.Cin) {
#pragma unroll 4
    for (int lr = c_r; lr < BMO; lr += CROWS) {
      const int co = co0 + lr;
      if (co < p.Cout)
        *reinterpret_cast<float4*>(out + ((size_t)co * T + tap) * p.Cin + ci) = *reinterpret_cast<const float4*>(Cs + lr * LDC + c_c4 * 4);
    }
  }
}

template <int BMO, int BNI>
__global__ __launch_bounds__(256, 2) void wgrad_x6_kernel(const WgradArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[wgrad_xs_smem<BMO, BNI, 3>()];
  wgrad_x6_body<BMO, BNI, 3>(p, xcd_remap(blockIdx.x, gridDim.x), smem);
}
template <int BMO, int BNI>
__global__ __launch_bounds__(256, 2) void wgrad_h3_kernel(const WgradArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[wgrad_xs_smem<BMO, BNI, 2>()];
  wgrad_x6_body<BMO, BNI, 2>(p, xcd_remap(blockIdx.x, gridDim.x), smem);
}
// Several weight gradients in one launch (the independent GEMMs of a ResNet stage): workgroup w works on entry
// map[w].x of the table as its workgroup map[w].y.  Grouped, the small layers fill the chip with a few K splits each
// instead of 30-240 (fewer parked slabs, no per-launch tails).
template <int BMO, int BNI>
__global__ __launch_bounds__(256, 2) void wgrad_x6_group_kernel(const WgradArgs* __restrict__ tab, const int2* __restrict__ map) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[wgrad_xs_smem<BMO, BNI, 3>()];
  const int2 m = map[xcd_remap(blockIdx.x, gridDim.x)];
  const int ent = __builtin_amdgcn_readfirstlane(m.x), bid = __builtin_amdgcn_readfirstlane(m.y);
  const WgradArgs p = tab[ent];
  wgrad_x6_body<BMO, BNI, 3>(p, bid, smem);
}
template <int BMO, int BNI>
__global__ __launch_bounds__(256, 2) void wgrad_h3_group_kernel(const WgradArgs* __restrict__ tab, const int2* __restrict__ map) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[wgrad_xs_smem<BMO, BNI, 2>()];
  const int2 m = map[xcd_remap(blockIdx.x, gridDim.x)];
  const int ent = __builtin_amdgcn_readfirstlane(m.x), bid = __builtin_amdgcn_readfirstlane(m.y);
  const WgradArgs p = tab[ent];
  wgrad_x6_body<BMO, BNI, 2>(p, bid, smem);
}

// max over the finite |x| of a [rows x C] view (row pitch ld floats) -> atomicMax of the bit pattern (|x| compares like
// an unsigned integer).  HBM-bound: one read of the view.
// dense view: n4 float4 in a row
__global__ __launch_bounds__(256) void absmax_flat_kernel(const float4* __restrict__ x, long n4, unsigned* __restrict__ slot) {
  unsigned m = 0;
  const long stride = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const float4 v0 = x[i], v1 = x[i + stride], v2 = x[i + 2 * stride], v3 = x[i + 3 * stride];
    m = amax_f4(m, v0); m = amax_f4(m, v1); m = amax_f4(m, v2); m = amax_f4(m, v3);
  }
  for (; i < n4; i += stride) m = amax_f4(m, x[i]);
  amax_block_commit(m, slot);
}
// strided view: 2^txs threads walk the C4 float4 of a row, 256 >> txs rows per workgroup pass
__global__ __launch_bounds__(256) void absmax_rows_kernel(const float* __restrict__ x, int rows, int C4, int ld, int txs,
                                                          unsigned* __restrict__ slot) {
  const int tx = 1 << txs, col = threadIdx.x & (tx - 1), rl = threadIdx.x >> txs, rp = 256 >> txs;
  unsigned m = 0;
  for (int r = blockIdx.x * rp + rl; r < rows; r += gridDim.x * rp) {
    const float* row = x + (size_t)r * ld;
    for (int c = col; c < C4; c += tx) m = amax_f4(m, ldg4(row + c * 4));
  }
  amax_block_commit(m, slot);
}
void launch_absmax(const float* x, long rows, int C, int ld, unsigned* slot, hipStream_t s) {
  const int C4 = C / 4;
  if (ld == C || rows == 1) {
    const long n4 = rows * C4;
    long g = (n4 + 256 * 8 - 1) / (256 * 8);
    g = g < 1 ? 1 : (g > 1024 ? 1024 : g);
    hipLaunchKernelGGL(absmax_flat_kernel, dim3((unsigned)g), dim3(256), 0, s, reinterpret_cast<const float4*>(x), n4, slot);
    return;
  }
  int txs = 0;
  while ((1 << txs) < C4 && txs < 8) ++txs;
  const int rp = 256 >> txs;
  long g = (rows + (long)rp * 4 - 1) / ((long)rp * 4);
  g = g < 1 ? 1 : (g > 1024 ? 1024 : g);
  hipLaunchKernelGGL(absmax_rows_kernel, dim3((unsigned)g), dim3(256), 0, s, x, (int)rows, C4, ld, txs, slot);
}
// zero the slots [first, first + count): all AMAX_SUB words of each (hipMemset2DAsync does the same in 3 launches)
__global__ __launch_bounds__(256) void amax_zero_kernel(unsigned* __restrict__ first, int count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < count * AMAX_SUB) first[(size_t)(i / count) * AMAX_ROW + (i % count)] = 0u;
}
void launch_amax_zero(unsigned* first, int count, hipStream_t s) {
  if (count < 1) return;
  hipLaunchKernelGGL(amax_zero_kernel, dim3((unsigned)((count * AMAX_SUB + 255) / 256)), dim3(256), 0, s, first, count);
}
// one launch for many dense tensors (the weights): segment blockIdx.y = floats [off[y], off[y] + n[y]) of base
__global__ __launch_bounds__(256) void absmax_segments_kernel(const float* __restrict__ base, const long* __restrict__ off,
                                                              const int* __restrict__ n, unsigned* __restrict__ slots) {
  const int y = blockIdx.y;
  const int n4 = n[y] >> 2;
  if (n4 <= 0) return;
  const float4* x = reinterpret_cast<const float4*>(base + off[y]);
  unsigned m = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) m = amax_f4(m, x[i]);
  amax_block_commit(m, slots + y);   // (blockIdx.x + blockIdx.y) spreads the words
}
void launch_absmax_segments(const float* base, const long* dev_off, const int* dev_n, int nseg, unsigned* slots, hipStream_t s) {
  hipLaunchKernelGGL(absmax_segments_kernel, dim3(64, (unsigned)nseg), dim3(256), 0, s, base, dev_off, dev_n, slots);
}

// Matrix mode: 2 = f16x3 (default), 1 = bf16x6, 0 = fp32 MFMA; EOSVOS_MFMA=f16x3|bf16x6|f32 picks the initial one
static int g_mfma_mode = -1;
static thread_local int tl_mfma_mode = -1;          // an engine with a mode of its own, for the duration of one C-ABI call
void conv_set_thread_mfma_mode(int mode) { tl_mfma_mode = mode < 0 ? -1 : (mode == 2 ? 2 : (mode ? 1 : 0)); }
int conv_thread_mfma_mode() { return tl_mfma_mode; }
int conv_mfma_mode() {
  if (tl_mfma_mode >= 0) return tl_mfma_mode;
  if (g_mfma_mode < 0) {
    const char* v = getenv("EOSVOS_MFMA");
    g_mfma_mode = (v && !strcmp(v, "f32")) ? 0 : (v && !strcmp(v, "bf16x6")) ? 1 : 2;
  }
  return g_mfma_mode;
}
void conv_set_mfma_mode(int mode) { g_mfma_mode = mode == 2 ? 2 : (mode ? 1 : 0); }


// ---------------------------------------------------------------------------------------
// Per-launch timing with HIP events on the stream each kernel is launched on (bench.py's roofline: dominant kernel
// by time, its algorithmic FLOPs / its measured duration).  Off by default; no effect on results.
// ---------------------------------------------------------------------------------------
namespace {
// Run-time tile widths (128, else 64) and flags -> the std::integral_constant a launcher instantiates its kernel with
template <class F> void with_tile(int w, F&& f) {
  if (w == 128) f(std::integral_constant<int, 128>{}); else f(std::integral_constant<int, 64>{});
}
template <class F> void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{}); else f(std::false_type{});
}
struct ProfRec { hipEvent_t a, b; int kernel; double flops; };
bool g_prof_on = false;
std::vector<ProfRec> g_prof;
std::vector<hipEvent_t> g_prof_pool;
const char* const kProfNames[] = {
#define EOSVOS_PROF_NAME(id, name) name,
    EOSVOS_PROF_KERNELS(EOSVOS_PROF_NAME)
#undef EOSVOS_PROF_NAME
};
static_assert(sizeof(kProfNames) / sizeof(kProfNames[0]) == kProfKernels, "one name per id");
// Families of four records: <128, .>, <128, .>, <64, .>, <64, .> for the convs (tile width, then K-major), <bm, bn> for the
// weight gradients (128 before 64 in both)
int prof_conv(int mode, int bn, bool kmajor) {
  return (mode == 2 ? kProfConvH3 : mode == 1 ? kProfConvX6 : kProfConvIgemm) + (bn == 128 ? 0 : 2) + (kmajor ? 1 : 0);
}
int prof_wgrad(int first, int bm, int bn) { return first + (bm == 128 ? 0 : 2) + (bn == 128 ? 0 : 1); }
#define EOSVOS_PROF_FAMILY(first) static_assert(first##_1 == first + 1 && first##_2 == first + 2 && first##_3 == first + 3, "family of four")
EOSVOS_PROF_FAMILY(kProfConvX6); EOSVOS_PROF_FAMILY(kProfConvIgemm); EOSVOS_PROF_FAMILY(kProfConvH3);
EOSVOS_PROF_FAMILY(kProfWgradX6); EOSVOS_PROF_FAMILY(kProfWgrad); EOSVOS_PROF_FAMILY(kProfWgradH3);
EOSVOS_PROF_FAMILY(kProfWgradX6Group); EOSVOS_PROF_FAMILY(kProfWgradH3Group);
#undef EOSVOS_PROF_FAMILY
hipEvent_t prof_event() {
  if (!g_prof_pool.empty()) { hipEvent_t e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}
struct ProfScope {
  hipStream_t s;
  bool on;
  ProfScope(int kernel, double flops, hipStream_t st) : s(st), on(g_prof_on) {
    if (!on) return;
    ProfRec r{prof_event(), prof_event(), kernel, flops};
    (void)hipEventRecord(r.a, s);
    g_prof.push_back(r);
  }
  ~ProfScope() { if (on) (void)hipEventRecord(g_prof.back().b, s); }
};
}  // namespace
// the same bracket for launchers in other translation units (presplit_kernels.hip): begin ... launch ... end
void conv_prof_mark_begin(int kernel, double flops, hipStream_t s) {
  if (!g_prof_on || kernel < 0 || kernel >= kProfKernels) return;
  ProfRec r{prof_event(), prof_event(), kernel, flops};
  (void)hipEventRecord(r.a, s);
  g_prof.push_back(r);
}
void conv_prof_mark_end(hipStream_t s) {
  if (g_prof_on && !g_prof.empty()) (void)hipEventRecord(g_prof.back().b, s);
}
void conv_prof_enable(int on) {
  g_prof_on = on != 0;
  if (g_prof_on) {
    for (auto& r : g_prof) { g_prof_pool.push_back(r.a); g_prof_pool.push_back(r.b); }
    g_prof.clear();
  }
}
// totals per kernel symbol since conv_prof_enable(1); the caller has synchronised the streams
int conv_prof_read(int max, const char** names, long* counts, double* ms, double* flops) {
  double t[kProfKernels] = {0}, f[kProfKernels] = {0};
  long c[kProfKernels] = {0};
  for (auto& r : g_prof) {
    float m = 0.f;
    if (hipEventElapsedTime(&m, r.a, r.b) != hipSuccess) continue;
    t[r.kernel] += m; f[r.kernel] += r.flops; ++c[r.kernel];
  }
  int n = 0;
  for (int k = 0; k < kProfKernels && n < max; ++k)
    if (c[k]) { names[n] = kProfNames[k]; counts[n] = c[k]; ms[n] = t[k]; flops[n] = f[k]; ++n; }
  return n;
}
// plan log (kernels.h ConvPlanRec): what launch_conv decided, for the tests to assert the plan they claim to cover
static bool g_plan_log_on = false;
static int g_plan_log_n = 0;
static ConvPlanRec g_plan_log[kConvPlanLogCap];
void conv_plan_log_enable(int on) {
  g_plan_log_on = on != 0;
  if (g_plan_log_on) g_plan_log_n = 0;
}
int conv_plan_log_read(ConvPlanRec* out, const char** names, int max) {
  for (int i = 0; i < g_plan_log_n && i < max && i < kConvPlanLogCap; ++i) {
    out[i] = g_plan_log[i];
    names[i] = kProfNames[g_plan_log[i].kernel];
  }
  return g_plan_log_n;
}
static void plan_log_add(const ConvPlanRec& r) {
  if (g_plan_log_n < kConvPlanLogCap) g_plan_log[g_plan_log_n] = r;
  ++g_plan_log_n;
}
// share of the nominal multiply-accumulates a launch executes (taps skipped by tap tables / pixel rectangles)
double conv_exec_frac(const ConvArgs& a) {
  if (!a.tprefix || a.total_units <= 0) return 1.0;
  const int bn = conv_bn(a);
  const long tiles = (long)((a.M + 127) / 128) * ((a.N + bn - 1) / bn);
  return (double)a.total_units / (double)(tiles * (long)a.KH * a.KW * ((a.Kc + 31) / 32));
}
double wgrad_exec_frac(const WgradArgs& a) {
  if (a.g_tap_stride) return 1.0;
  long sum = 0;
  for (int ky = 0; ky < a.KH; ++ky)
    for (int kx = 0; kx < a.KW; ++kx) {
      const int dyk = ky * a.dil - a.pad, dxk = kx * a.dil - a.pad;
      int hv = 0, wv = 0;
      for (int oy = 0; oy < a.Ho; ++oy) { const int iy = oy * a.stride + dyk; hv += (iy >= 0 && iy < a.Hi); }
      for (int ox = 0; ox < a.Wo; ++ox) { const int ix = ox * a.stride + dxk; wv += (ix >= 0 && ix < a.Wi); }
      sum += (long)hv * wv;
    }
  return (double)sum / ((double)a.KH * a.KW * a.Ho * a.Wo);
}

#define CONV_MAX_WG (256 * EOSVOS_OCC)
// Workgroups a launch plans for.  An engine that shares the GPU with others (concurrent meta tasks) is better off
// splitting K less: fewer parked partial tiles, and the other engines' launches fill the rest of the chip.
int conv_clamp_wg_budget(int n) {
  if (n <= 0) return 0;
  n = (n + 63) / 64 * 64;
  return n >= CONV_MAX_WG ? 0 : n;
}
static int conv_wg_budget(int requested) {
  const int b = conv_clamp_wg_budget(requested);
  return b > 0 ? b : CONV_MAX_WG;
}
int conv_wg_budget_of(int requested) { return conv_wg_budget(requested); }
#define CONV_MAX_WG_DEEP (256 * 3)
#define EOSVOS_MINK 3      // K steps a streamed workgroup takes at least
// ConvArgs::ws: workgroup bid < nwg of a launch parks at most two BM x BN <= 128 x 128 partial tiles, ws[2 bid] and
// ws[2 bid + 1] (conv_igemm_kernel, conv_xs_body).  conv_plan starts from CONV_MAX_WG_DEEP workgroups (deep kernels) or the
// budget (<= CONV_MAX_WG), and no branch raises nwg above that start: whole tiles per workgroup take ceil(tiles / q) with
// tiles < q x start, or one per tile when tiles < start; streamed launches only lower it; uniform split-K takes
// tiles x (budget / tiles).
static_assert(CONV_MAX_WG <= CONV_MAX_WG_DEEP, "conv_ws_floats");
int64_t conv_ws_floats() { return (int64_t)CONV_MAX_WG_DEEP * 2 * 128 * 128; }

// returns the number of workgroups; fills a.deep / a.dp_q / a.per / a.nwg / a.splitk.  With nwg0 = the workgroup budget (768 for the
// deep variants):
//   tap table with its tile order, tiles >= nwg0, K <= 1536 (f16x3 / bf16x6 modes): whole tiles dealt out longest first,
//                 dp_q = ceil(tiles / nwg0) per workgroup;
//   tiles >= nwg0, no tap table: dp_q = tiles / nwg0 whole tiles per workgroup (no workspace traffic).  A leftover of at least
//                 1 % of nwg0 tiles: one more whole tile each on fewer workgroups (the last may run past `tiles` and skips);
//                 a smaller one is streamed over all workgroups in equal K runs of `per` steps (fix-up pass), or, when that
//                 gives runs of less than 2 steps, taken as whole tiles too;
//   otherwise:    short K, or many tiles with a short K: one whole tile per workgroup (per = ksteps, nwg = tiles); else
//                 stream-K: the tiles' K steps (the tap table's compacted steps) in equal runs of `per` >= EOSVOS_MINK steps
//                 (fix-up pass wherever a run ends inside a tile);
//   f16x3 mode, few tiles with a long, even K: uniform split-K (splitk chunks per tile, nwg = tiles x splitk, fix-up pass)
//                 instead of stream-K.
int conv_plan(ConvArgs& a) {
  const int bn = conv_bn(a);
  const int T = a.KH * a.KW;
  long ksteps = (long)T * ((a.Kc + EOSVOS_BK - 1) / EOSVOS_BK);
  const long tiles = (long)((a.M + 127) / 128) * ((a.N + bn - 1) / bn);
  const bool x6 = conv_mfma_mode() >= 1;
  // 3-workgroups-per-CU kernel for long-K layers with many tiles (measured: decoder 3x3 fwd/dgrad at batch >= 2); all
  // batched GEMMs take the K-step-16 variant
  const bool batched_deep = a.plane_rows != 0;
  const bool deep_ok = ksteps >= 64 || batched_deep;
  a.deep = (!x6 && bn == 128 && tiles >= EOSVOS_DEEP_TILES && deep_ok && a.total_units <= 0)
               ? (((a.Kc & 31) || batched_deep) ? 2 : 1) : 0;
  if (a.deep == 2) ksteps = (long)T * ((a.Kc + EOSVOS_BK_DEEP - 1) / EOSVOS_BK_DEEP);
  long nwg = a.deep ? CONV_MAX_WG_DEEP : conv_wg_budget(a.wg_budget), q = 0, per = 0;
  if (x6 && a.total_units > 0 && a.torder && tiles >= nwg && ksteps * EOSVOS_BK <= 1536) {
    // uneven tiles (tap table), at least one per workgroup: whole tiles, longest first, no parked partial tiles and no
    // fix-up pass (the stride-2 3x3 data gradient at batch 3: 602 tiles of 4 / 8 / 8 / 16 K steps; streamed, nearly every
    // workgroup parked two slabs: 70 + 20 us).  Short K only: the 608-tile, K = 2304 data gradients of the dilated ASPP convs
    // lose more to the quantisation into two rounds (139 + 22 -> 192 us) than the fix-up pass costs.
    q = (tiles + nwg - 1) / nwg; per = 0;
  } else if (tiles >= nwg && a.total_units <= 0) {
    q = tiles / nwg;
    const long rem = tiles - q * nwg;
    // a leftover that nearly fills another round: whole tiles for it too (q + 1 per workgroup, fewer workgroups) -- the
    // streamed form parks two slabs per workgroup and needs the fix-up pass (batch-1 decoder: 936 tiles = 512 + 424 streamed,
    // fix-up 17 us; as 468 workgroups x 2 whole tiles none); from 1 % of the budget on
    if (rem > 0 && rem * 100 >= nwg) {
      q = q + 1; per = 0;
      nwg = (tiles + q - 1) / q;
    } else if (rem > 0) {
      per = (rem * ksteps + nwg - 1) / nwg;
      if (per < 2) {                                   // tiny K: whole tiles only, <= one resident round of workgroups
        per = 0;
        q = (tiles + nwg - 1) / nwg; nwg = (tiles + q - 1) / q;
      }
    }
  } else {
    const long U = a.total_units > 0 ? a.total_units : tiles * ksteps;
    // short K, or at least one tile per CU and a K so short that the fix-up pass (a second launch, >= 10 us)
    // costs more than the idle second slot of some CUs: one whole tile per workgroup
    // (f16x3 mode, where a K step costs less against the fix-up pass: from a quarter of the budget in tiles and up to K = 512
    // -- batch 1 5.23 -> 5.12 ms, batch 3 9.89 -> 9.79; tools/budget_sweep.py showed layer3's 208-tile K = 256 launches at 22 us
    // streamed against 16 us as whole tiles)
    const int dps_div = conv_mfma_mode() == 2 ? 4 : 2;
    const int dps_k = conv_mfma_mode() == 2 ? 512 : 256;
    const bool dp_small = tiles >= conv_wg_budget(a.wg_budget) / dps_div && ksteps * EOSVOS_BK <= dps_k;
    if ((ksteps <= EOSVOS_MINK + 1 || dp_small) && a.total_units <= 0) {
      per = ksteps; nwg = tiles;                       // no fix-up
    } else {
      if (U / nwg < EOSVOS_MINK) nwg = U / EOSVOS_MINK > 0 ? U / EOSVOS_MINK : 1;   // >= MINK K-steps per workgroup
      per = (U + nwg - 1) / nwg;
      nwg = (U + per - 1) / per;
    }
  }
  a.splitk = 0;
  {
    // Long-K launches with few tiles: uniform split-K in chunk-major workgroup order instead of stream-K (see conv_xs_body).
    // Stream-K gives every workgroup its own K range of one tile -- no two workgroups of an XCD ever want the same operand
    // bytes, everything comes from the Infinity Cache; here they share the chunk's weight slice through L2.
    // Measured per launch (tools/layer_times.py, batch 3, one stream): the 3x3 convs of layer2 / layer3 - 7...10 %, layer4's
    // K = 2048 1x1 convs - 5...10 %, the d = 6 ASPP conv 187 -> 140 us; tap-table launches whose tiles keep very different
    // numbers of taps (d = 18: 100 -> 135 us) stay with stream-K, which balances them exactly.
    constexpr long min_avg = 16, min_chunk = 12, min_fill = 60;      // (fill: 85 in round 3; re-measured in round 4: batch 1 4.50 -> 4.46 ms, batch 3 +-0)
    const bool even_taps = a.total_units <= 0 || a.total_units * 100 >= 85L * tiles * ksteps;
    const long budget = conv_wg_budget(a.wg_budget);
    const long avg = a.total_units > 0 ? a.total_units / tiles : ksteps;
    const long S = tiles > 0 ? budget / tiles : 0;
    if (conv_mfma_mode() == 2 && !a.deep && even_taps && q == 0 && per > 0 && per < avg && S >= 2 && avg >= min_avg && avg / S >= min_chunk &&
        tiles * S * 100 >= min_fill * budget) {
      a.splitk = (int)S; nwg = tiles * S; per = 0;
    }
  }
  a.dp_q = (int)q; a.per = (int)per; a.nwg = (int)nwg;
  return (int)nwg;
}

void launch_conv(ConvArgs& a, hipStream_t s) {
  if (stream3x3_ok(a)) {                              // layer1's 64 -> 64 3x3 convs: all nine taps' weights resident in LDS
    a.dp_q = 0; a.per = 0; a.nwg = 0; a.splitk = 0;
    if (g_plan_log_on) { ConvPlanRec r{}; r.kernel = kProfStream3x3; r.kmajor = a.kmajor; r.budget = conv_wg_budget(a.wg_budget); plan_log_add(r); }
    ProfScope ps(kProfStream3x3, 2.0 * a.M * a.N * a.Kc * 9, s);
    launch_stream3x3(a, s);
    return;
  }
  if (const int nc = stream1x1_nc(a)) {               // short-K 1x1 convs on the large maps: the streaming kernel
    a.dp_q = 0; a.per = 0; a.nwg = 0; a.splitk = 0;
    if (g_plan_log_on) { ConvPlanRec r{}; r.kernel = nc >= 128 ? kProfStream1x1_128 : kProfStream1x1_64; r.kmajor = a.kmajor; r.budget = conv_wg_budget(a.wg_budget); plan_log_add(r); }
    ProfScope ps(nc >= 128 ? kProfStream1x1_128 : kProfStream1x1_64, 2.0 * a.M * a.N * a.Kc, s);      // (48 columns: filed under 64)
    if (nc == 128) {
      if (a.Kc == 64) launch_stream1x1<64, 128>(a, s);
      else if (a.Kc == 128) launch_stream1x1<128, 128>(a, s);
      else if (a.Kc == 304) launch_stream1x1<304, 128>(a, s);
      else launch_stream1x1<256, 128>(a, s);
    } else if (nc == 48) {
      launch_stream1x1<256, 48>(a, s);
    } else {
      if (a.Kc == 64) launch_stream1x1<64, 64>(a, s);
      else if (a.Kc == 128) launch_stream1x1<128, 64>(a, s);
      else if (a.Kc == 256) launch_stream1x1<256, 64>(a, s);
      else if (a.Kc == 304) launch_stream1x1<304, 64>(a, s);
      else launch_stream1x1<512, 64>(a, s);
    }
    return;
  }
  const int bn = conv_bn(a);
  const int nwg = conv_plan(a);
  const long tiles = (long)((a.M + 127) / 128) * ((a.N + bn - 1) / bn);
  const dim3 grid(nwg), block(256);
  const int mode = conv_mfma_mode();
  a.y2_done = (a.y2 && mode == 2) ? 1 : 0;       // conv_xs_body<NP = 2> and conv_fixup_kernel write the pair8 sibling
  const int pk = a.nseg > 0 ? (mode == 2 ? kProfConvH3Multi : kProfConvX6Multi) : prof_conv(mode, bn, a.kmajor != 0);
  {
  ProfScope ps(pk, 2.0 * a.M * a.N * a.KH * a.KW * a.Kc * conv_exec_frac(a), s);
  if (a.nseg > 0) {
    if (mode == 2) hipLaunchKernelGGL(conv_h3_multi_kernel, grid, block, 0, s, a);
    else hipLaunchKernelGGL(conv_x6_multi_kernel, grid, block, 0, s, a);
  } else if (mode == 0 && (a.deep == 1 || a.deep == 2)) {
    with_bool(a.kmajor != 0, [&](auto km) {
      if (a.deep == 1) hipLaunchKernelGGL((conv_igemm_kernel<128, km(), 1>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((conv_igemm_kernel<128, km(), 2>), grid, block, 0, s, a);
    });
  } else {
    with_tile(bn, [&](auto BN) { with_bool(a.kmajor != 0, [&](auto km) {
      if (mode == 2) hipLaunchKernelGGL((conv_h3_kernel<BN(), km()>), grid, block, 0, s, a);
      else if (mode == 1) hipLaunchKernelGGL((conv_x6_kernel<BN(), km()>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((conv_igemm_kernel<BN(), km()>), grid, block, 0, s, a);
    }); });
  }
  }
  const int T = a.KH * a.KW;
  const int bk = a.deep == 2 ? EOSVOS_BK_DEEP : EOSVOS_BK;
  const long ksteps = (long)T * ((a.Kc + bk - 1) / bk);
  const long sk_tiles = tiles - (long)a.dp_q * nwg;
  const bool fixup = a.splitk > 1 || (a.per > 0 && sk_tiles > 0 && (a.per % ksteps != 0 || a.tprefix));   // some tile is shared between workgroups
  if (g_plan_log_on)
    plan_log_add(ConvPlanRec{pk, a.kmajor != 0, bn, (int)tiles, (int)ksteps, a.deep, a.dp_q, a.per, nwg, a.splitk, a.tprefix != nullptr,
                             a.torder != nullptr, fixup, conv_wg_budget(a.wg_budget)});
  if (fixup) {
    ProfScope ps(kProfFixup, 0.0, s);
    with_tile(bn, [&](auto BN) { hipLaunchKernelGGL((conv_fixup_kernel<BN()>), dim3((unsigned)sk_tiles, 8), block, 0, s, a); });
  }
}

// ---------------------------------------------------------------------------------------
// Weight gradient.  GEMM with M = cout, N = cin (one filter tap per workgroup column),
// K = pixels.  Both operands are "k-major" in memory (a pixel's channels are contiguous),
// so tiles are staged as [pixel][channel] rows and fragments are read with ds_read_b32
// (consecutive lanes -> consecutive channels: conflict free).
// ---------------------------------------------------------------------------------------
#define EOSVOS_WG_BKP 32
#define EOSVOS_WG_OCC 2
template <int BMO, int BNI>
__global__ __launch_bounds__(256, EOSVOS_WG_OCC) void wgrad_kernel(const WgradArgs p) {
  constexpr int BKP = EOSVOS_WG_BKP;
  constexpr int LDA = BMO + 4, LDB = BNI + 4;
  constexpr int A_EL = BKP * LDA, B_EL = BKP * LDB, STAGE = A_EL + B_EL;
  __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;

  const int T = p.KH * p.KW;
  const int ct = (p.Cout + BMO - 1) / BMO, it = (p.Cin + BNI - 1) / BNI;
  const int tiles = ct * it * T;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int z = bid / tiles;
  int tile = bid - z * tiles;
  // taps fastest: the T workgroups that share one (cout, cin) tile pair read the same G tile
  const int tap = tile % T; tile /= T;
  const int co0 = (tile / it) * BMO, ci0 = (tile % it) * BNI;
  const int ky = tap / p.KW, kx = tap - ky * p.KW;

  // Only the output pixels whose tap lands inside the input contribute: a rectangle
  // [oy_lo, oy_hi] x [ox_lo, ox_hi] per image (for the dilated 3x3 convs of layer4 / ASPP on the
  // 30x54 map the corner taps of d = 18 see 27 % of the pixels).  K runs over that rectangle only.
  const int dyk = ky * p.dil - p.pad, dxk = kx * p.dil - p.pad;
  auto cdiv = [](int a, int b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); };      // ceil, b > 0
  auto fdiv = [](int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };        // floor, b > 0
  int oy_lo = cdiv(-dyk, p.stride), oy_hi = fdiv(p.Hi - 1 - dyk, p.stride);
  int ox_lo = cdiv(-dxk, p.stride), ox_hi = fdiv(p.Wi - 1 - dxk, p.stride);
  if (oy_lo < 0) oy_lo = 0;
  if (ox_lo < 0) ox_lo = 0;
  if (oy_hi > p.Ho - 1) oy_hi = p.Ho - 1;
  if (ox_hi > p.Wo - 1) ox_hi = p.Wo - 1;
  const int hv = oy_hi - oy_lo + 1 > 0 ? oy_hi - oy_lo + 1 : 0;
  const int wv = ox_hi - ox_lo + 1 > 0 ? ox_hi - ox_lo + 1 : 0;
  const int P = p.B * hv * wv;                         // contributing pixels
  const int steps = (P + BKP - 1) / BKP;
  const int st_begin = (int)(((long)steps * z) / p.splits);
  const int st_end = (int)(((long)steps * (z + 1)) / p.splits);

  constexpr int AF4 = BMO / 4, AROWS = 256 / AF4, APASS = BKP / AROWS;
  constexpr int BF4 = BNI / 4, BROWS = 256 / BF4, BPASS = BKP / BROWS;
  const int a_c4 = tid % AF4, a_r = tid / AF4;
  const int b_c4 = tid % BF4, b_r = tid / BF4;
  const bool a_cok = (co0 + a_c4 * 4) < p.Cout;
  const bool b_cok = (ci0 + b_c4 * 4) < p.Cin;

  float4 ra[APASS], rb[BPASS];
  // Each staging row follows one pixel per K step: its (image, y, x) inside the rectangle
  // advances by BKP pixels per step with carries instead of divisions; rows past the end use
  // the out-of-range offset of a range-checked buffer load (returns 0): no divergent branches.
  constexpr unsigned OOB = 0x80000000u;
  const __amdgpu_buffer_rsrc_t rg = make_rsrc(p.g + tap * p.g_tap_stride, (long)p.B * p.Ho * p.Wo * p.ldg * 4);
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x + tap * p.x_tap_stride, (long)p.B * p.Hi * p.Wi * p.ldx * 4);
  int a_img[APASS], a_ry[APASS], a_rx[APASS];
  int b_img[BPASS], b_ry[BPASS], b_rx[BPASS];
  {
    const int hw = hv * wv > 0 ? hv * wv : 1, wv1 = wv > 0 ? wv : 1;
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
      const int q = st_begin * BKP + a_r + i * AROWS;
      const int bb = q / hw, rem = q - bb * hw;
      a_img[i] = bb; a_ry[i] = rem / wv1; a_rx[i] = rem - a_ry[i] * wv1;
    }
#pragma unroll
    for (int i = 0; i < BPASS; ++i) {
      const int q = st_begin * BKP + b_r + i * BROWS;
      const int bb = q / hw, rem = q - bb * hw;
      b_img[i] = bb; b_ry[i] = rem / wv1; b_rx[i] = rem - b_ry[i] * wv1;
    }
  }
  auto load_tiles = [&](int st) {      // must be called with consecutive st
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
      const bool ok = a_cok && a_img[i] < p.B;
      const unsigned off = ok ? (unsigned)(((a_img[i] * p.Ho + oy_lo + a_ry[i]) * p.Wo + ox_lo + a_rx[i]) * p.ldg + co0 + a_c4 * 4) * 4u : OOB;
      ra[i] = bufld4(rg, off);
      a_rx[i] += BKP;
      while (a_rx[i] >= wv && wv > 0) { a_rx[i] -= wv; ++a_ry[i]; }
      while (a_ry[i] >= hv && hv > 0) { a_ry[i] -= hv; ++a_img[i]; }
    }
#pragma unroll
    for (int i = 0; i < BPASS; ++i) {
      const int iy = (oy_lo + b_ry[i]) * p.stride + dyk, ix = (ox_lo + b_rx[i]) * p.stride + dxk;
      const bool ok = b_cok && b_img[i] < p.B;
      const unsigned off = ok ? (unsigned)(((b_img[i] * p.Hi + iy) * p.Wi + ix) * p.ldx + ci0 + b_c4 * 4) * 4u : OOB;
      rb[i] = bufld4(rx, off);
      b_rx[i] += BKP;
      while (b_rx[i] >= wv && wv > 0) { b_rx[i] -= wv; ++b_ry[i]; }
      while (b_ry[i] >= hv && hv > 0) { b_ry[i] -= hv; ++b_img[i]; }
    }
  };
  auto store_tiles = [&](int buf) {
    float* As = smem + buf * STAGE;
    float* Bs = As + A_EL;
#pragma unroll
    for (int i = 0; i < APASS; ++i)
      *reinterpret_cast<float4*>(As + (a_r + i * AROWS) * LDA + a_c4 * 4) = ra[i];
#pragma unroll
    for (int i = 0; i < BPASS; ++i)
      *reinterpret_cast<float4*>(Bs + (b_r + i * BROWS) * LDB + b_c4 * 4) = rb[i];
  };

  constexpr int TM = BMO / 64, TN = BNI / 64;
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  if (st_begin < st_end) {
    load_tiles(st_begin);
    store_tiles(0);
  }
  __syncthreads();
  for (int st = st_begin; st < st_end; ++st) {
    const int buf = (st - st_begin) & 1;
    const bool more = (st + 1) < st_end;
    if (more) load_tiles(st + 1);
    const float* As = smem + buf * STAGE;
    const float* Bs = As + A_EL;
#pragma unroll
    for (int s2 = 0; s2 < BKP / 2; ++s2) {
      float av[TM], bv[TN];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) av[tm] = As[(s2 * 2 + h) * LDA + wm * (BMO / 2) + tm * 32 + r];
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) bv[tn] = Bs[(s2 * 2 + h) * LDB + wn * (BNI / 2) + tn * 32 + r];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = MFMA32(av[tm], bv[tn], acc[tm][tn]);
    }
    if (more) store_tiles(buf ^ 1);
    __syncthreads();
  }

  float* out = p.ws + (size_t)z * p.Cout * T * p.Cin;
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int ci = ci0 + wn * (BNI / 2) + tn * 32 + r;
      if (ci >= p.Cin) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = co0 + wm * (BMO / 2) + tm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (co < p.Cout) out[((size_t)co * T + tap) * p.Cin + ci] = acc[tm][tn][e];
      }
    }
}

// 128-wide tiles unless that pads the channel count by more than 15 % (e.g. 304 -> 384)
static int wg_tile(int c) {
  if (c <= 64) return 64;
  const int padded = (c + 127) / 128 * 128;
  return (padded - c) * 100 > 15 * c ? 64 : 128;
}
#define EOSVOS_WG_SMALLP 2500        // pixel count below which 64x64 tiles are used (more tiles, fewer K splits)
// few pixels AND few tiles (stride-16 layers at batch 1): 64x64 tiles give more tiles and fewer K splits
// (f16x3 mode: never -- with the faster K loop the 64x64 tiles' extra operand staging costs more than their fewer K
// splits save: batch 1 5.31 -> 5.23 ms without them, batch 3 unchanged)
static bool wg_small(int P, int Cout, int Cin, int T, int mode = -1) {
  const int t128 = ((Cout + wg_tile(Cout) - 1) / wg_tile(Cout)) * ((Cin + wg_tile(Cin) - 1) / wg_tile(Cin)) * T;
  const int smallp = (mode < 0 ? conv_mfma_mode() : mode) == 2 ? 0 : EOSVOS_WG_SMALLP;
  return P < smallp && t128 < 256;
}
int wgrad_pick_splits(int P, int Cout, int Cin, int T, int wg_budget, int mode) {
  const bool small = wg_small(P, Cout, Cin, T, mode);
  const int bm = small ? 64 : wg_tile(Cout), bn = small ? 64 : wg_tile(Cin);
  const int tiles = ((Cout + bm - 1) / bm) * ((Cin + bn - 1) / bn) * T;
  const int steps = (P + EOSVOS_WG_BKP - 1) / EOSVOS_WG_BKP;
  // pick the K split so that tiles*S fills whole rounds of the resident workgroups
  const int RES = conv_wg_budget(wg_budget) * EOSVOS_WG_OCC / EOSVOS_OCC;
  int best = 1;
  double best_eff = 0.0;
  constexpr int minsteps = 384 / EOSVOS_WG_BKP;   // 12 steps = 384 pixels per split (round 4: batch 1 4.57 -> 4.54 ms, batch 3 +-0; 8 before; 4 / 6: batch 1 +1.3 ... 2 %)
  // the first (= smallest) split count that fills its rounds to `eff_enough`: fewer splits park fewer slabs (each one a full
  // copy of the weight gradient that the update kernel reads back)
  // (round 5: 80 instead of 93 -- e.g. layer4 conv2 with 3 splits in one round instead of 7 in two, half the slab bytes -- is 0.5 %
  // faster at batch 3 (8.79 -> 8.75 ms), but the longer fp32 accumulation chains moved the fp32-MFMA mode's 240-iteration
  // trajectory (fixture G21) from 3.6e-4 to 1.04e-3 on the logits: not adopted, parity margin before half a percent)
  constexpr double eff_enough = 93 / 100.0;
  for (int s = 1; s <= 512 && steps / s >= minsteps; ++s) {
    const long wgs = (long)tiles * s;
    const long rounds = (wgs + RES - 1) / RES;
    const double eff = (double)wgs / (double)(rounds * RES);
    if (eff > best_eff + 1e-9) { best_eff = eff; best = s; }
    if (eff >= eff_enough) { best = s; break; }
  }
  return best;
}

int wgrad_group_tile(int channels) { return wg_tile(channels); }
// One launch for several weight gradients that share the tile shape bm x bn (engine.cpp plan_wgrad_group)
void launch_wgrad_group(const WgradArgs* dev_tab, const int* dev_map, int nwg, int bm, int bn, double flops, hipStream_t s) {
  const dim3 grid(nwg), block(256);
  const int2* map = reinterpret_cast<const int2*>(dev_map);
  const bool h3 = conv_mfma_mode() == 2;
  ProfScope ps(prof_wgrad(h3 ? kProfWgradH3Group : kProfWgradX6Group, bm, bn), flops, s);
  with_tile(bm, [&](auto BM) { with_tile(bn, [&](auto BN) {
    if (h3) hipLaunchKernelGGL((wgrad_h3_group_kernel<BM(), BN()>), grid, block, 0, s, dev_tab, map);
    else hipLaunchKernelGGL((wgrad_x6_group_kernel<BM(), BN()>), grid, block, 0, s, dev_tab, map);
  }); });
}

void launch_wgrad(const WgradArgs& a, hipStream_t s) {
  const int P = a.B * a.Ho * a.Wo;
  const bool small = wg_small(P, a.Cout, a.Cin, a.KH * a.KW);
  const int bm = small ? 64 : wg_tile(a.Cout), bn = small ? 64 : wg_tile(a.Cin);
  const int T = a.KH * a.KW;
  const int tiles = ((a.Cout + bm - 1) / bm) * ((a.Cin + bn - 1) / bn) * T;
  const dim3 grid(tiles * a.splits), block(256);
  const int mode = conv_mfma_mode();
  ProfScope ps(prof_wgrad(mode == 2 ? kProfWgradH3 : mode == 1 ? kProfWgradX6 : kProfWgrad, bm, bn),
               2.0 * a.Cout * a.Cin * T * (double)P * wgrad_exec_frac(a), s);
  with_tile(bm, [&](auto BM) { with_tile(bn, [&](auto BN) {
    if (mode == 2) hipLaunchKernelGGL((wgrad_h3_kernel<BM(), BN()>), grid, block, 0, s, a);
    else if (mode == 1) hipLaunchKernelGGL((wgrad_x6_kernel<BM(), BN()>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((wgrad_kernel<BM(), BN()>), grid, block, 0, s, a);
  }); });
}

}  // namespace eosvos

// ---------------------------------------------------------------------------------------
// Calibration probe: back-to-back v_mfma_f32_32x32x2_f32 on register operands (no memory),
// 2 workgroups x 4 waves per CU like the conv kernels -- the fp32 matrix rate this chip
// actually sustains at the clock it holds under load (roofline cross-check for bench.py).
// ---------------------------------------------------------------------------------------
namespace eosvos {
__global__ __launch_bounds__(256, 2) void mfma_probe_kernel(float* out, int iters, float seed) {
  f32x16 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  float a = seed + threadIdx.x * 1e-3f, b = seed - threadIdx.x * 1e-3f;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = MFMA32(a, b, acc[i]);
    }
    a += 1e-6f;
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) s += acc[i][e];
  if (s == 12345.678f) out[0] = s;   // keep the chain live
}
double launch_mfma_probe(float* scratch, int iters, hipStream_t s) {
  const int wgs = 512;
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(wgs), dim3(256), 0, s, scratch, iters, 0.5f);
  return (double)wgs * 4 /*waves*/ * iters * 16.0 * (2.0 * 32 * 32 * 2);
}
}  // namespace eosvos
