// Pre-split operand path of the f16x3 matrix mode (round 6).
//
// "pair8" sibling of an fp32 NHWC tensor: the same 4 bytes per element, but every group of 8 consecutive channels of a pixel
// holds [8 x fp16 hi | 8 x fp16 lo] (two 16-byte chunks) with hi = rn16(x * s), lo = rn16(x * s - hi) under ONE power-of-two
// scale s per tensor -- exactly the two pieces conv_xs_body / wgrad_x6_body form on the fly while staging (h3_split_pair).
// A consumer moves such operands global -> LDS with LDS-DMA (global_load_lds_dwordx4: no VGPR round trip, no VALU work, no
// ds_write) and the K loop is LDS -> MFMA only.
//
// wgrad_p_kernel: weight gradient  ws[z][cout][tap][cin] = sum_pixels G[p][cout] * X[src(p, tap)][cin]  (WgradArgs semantics,
// `wgrad_x6_body` of conv_kernels.hip; reference: the autograd of `/root/reference/src/networks/deeplabv3plus.py:32-53` convs)
// on a 256 x 256 x 32 workgroup tile, 8 waves (2 x 4, 128 x 64 each), two 64 KB LDS stages, one workgroup per CU.
//   * 64 FLOP per operand byte instead of the 128 x 128 tile's 32: the K loop of the register-staged kernels is bound by
//     (bytes in flight per CU / memory latency) x FLOP per byte, not by the MFMA pipe.
//   * Both operands are K-major in memory (a pixel's channels are contiguous): a DMA instruction copies one pixel row of the
//     tile (256 channels x 4 B = 1 KB, lane l -> 16-byte chunk l ^ f(k)); the MFMA fragments (8 consecutive k of one channel
//     per lane) come out of that [pixel][channel] image through ds_read_b64_tr_b16, gfx950's transposing LDS read
//     (cdna_hip_programming.md T10): per 16-lane group a block of 4 pixel rows x 16 channels, column-major into the VGPRs.
//   * Bank swizzle on the SOURCE address: chunk c of pixel row k lies at slot c ^ f(k), f(k) = k0 | k1 << 2 | k3 << 3; the 8
//     pixel rows x 2 chunks a 32-lane half of one transposed read touches then cover the 16 slots of a 256-byte bank row.
#include "kernels.h"
#include "conv_tile.h"
#include <stdlib.h>

namespace eosvos {

typedef _Float16 pf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 pf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 pf16x2 __attribute__((ext_vector_type(2)));
typedef float pf32x2 __attribute__((ext_vector_type(2)));
typedef float pf32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16 ph4;
#define P_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ unsigned p_pack(float e0, float e1) {
  pf32x2 v = {e0, e1};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, pf16x2));
}
__device__ __forceinline__ pf32x2 p_unpack(unsigned w) { return __builtin_convertvector(__builtin_bit_cast(pf16x2, w), pf32x2); }
__device__ __forceinline__ void p_split_pair(float x0, float x1, float s, unsigned& hi, unsigned& lo) {
  const float a = x0 * s, b = x1 * s;
  hi = p_pack(a, b);
  const pf32x2 u = p_unpack(hi);
  lo = p_pack(a - u.x, b - u.y);
}
// 8 consecutive channels (two float4) -> the hi chunk and the lo chunk of their pair8 group
__device__ __forceinline__ void p_split8(const float4& a, const float4& b, float s, uint4& hi, uint4& lo) {
  p_split_pair(a.x, a.y, s, hi.x, lo.x);
  p_split_pair(a.z, a.w, s, hi.y, lo.y);
  p_split_pair(b.x, b.y, s, hi.z, lo.z);
  p_split_pair(b.z, b.w, s, hi.w, lo.w);
}

// ---- standalone producer: fp32 view [rows][C] (row pitch ld floats) -> pair8 sibling with the same addressing ----------------
// The scale comes from the tensor's COMPLETE absmax slot: s = 2^(141 - e - margin) (largest magnitude -> [2^(14 - margin),
// 2^(15 - margin))); workgroup 0 leaves it in *sc for the consumers.  C % 8 == 0.
__device__ __forceinline__ float pair_scale_of(unsigned amax_bits, int margin) {
  const int e = (int)((amax_bits >> 23) & 0xffu);
  int f = 268 - e - margin;
  f = f < 1 ? 1 : (f > 254 ? 254 : f);
  return __uint_as_float((unsigned)f << 23);
}
__device__ __forceinline__ bool pair_scale_fits(unsigned amax_bits, float s) {
  const float t = __uint_as_float(amax_bits) * s;
  return s > 0.f && (amax_bits == 0u || (t < 32768.f && t >= 32768.f / (float)(1 << PAIR_HEADROOM)));
}
__global__ __launch_bounds__(256) void pair_split_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, long rows, int C8,
                                                         int ld, const unsigned* __restrict__ slot, int margin, float* __restrict__ sc) {
  const float s = pair_scale_of(amax_read(slot), margin);
  if (blockIdx.x == 0 && threadIdx.x == 0) *sc = s;
  const long n = rows * C8;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / C8;
    const int c = (int)(i - r * C8);
    const float* src = x + r * ld + c * 8;
    const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
    uint4 hi, lo;
    p_split8(a, b, s, hi, lo);
    uint4* dst = reinterpret_cast<uint4*>(out + (r * ld + c * 8) * 4);
    dst[0] = hi;
    dst[1] = lo;
  }
}
void launch_pair_split(const float* x, void* out, long rows, int C, int ld, const unsigned* slot, int margin, float* sc, hipStream_t s) {
  const long n = rows * (C / 8);
  long nb = (n + 255) / 256;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(pair_split_kernel, dim3((unsigned)nb), dim3(256), 0, s, x, (unsigned char*)out, rows, C / 8, ld, slot, margin, sc);
}

// ---- LDS-DMA --------------------------------------------------------------------------------------------------------------------
// One DMA as inline assembly: the compiler must not know that it writes LDS (for the builtin it puts s_waitcnt vmcnt(0) in
// front of the next ds_read of ANY stage).  M0 = LDS byte address of the wave's 1 KB destination (lane l lands at + 16 l);
// the source is a wave-uniform 64-bit base + a per-lane byte offset.
__device__ __forceinline__ void p_glds16(const unsigned char* sbase, unsigned voff, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ unsigned p_lds_addr(const void* p) {
  return __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) const char*)p);
}
// fragment of a K-major [pixel][channel] image: 8 k of one channel per lane = two transposed reads 4 pixel rows apart
__device__ __forceinline__ pf16x8 p_tr_frag(unsigned addr, int rowb) {
  const ph4 a = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) ph4*)addr);
  const ph4 b = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) ph4*)(addr + 4 * rowb));
  const pf16x4 a4 = __builtin_bit_cast(pf16x4, a), b4 = __builtin_bit_cast(pf16x4, b);
  return __builtin_shufflevector(a4, b4, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int BM, int BN>
__device__ __forceinline__ void wgrad_p_body(const WgradPArgs& p, const int bid, unsigned char* smem) {
  constexpr int BK = 32;
  constexpr int AROW = BM * 4, BROW = BN * 4;                 // bytes per pixel row of the tile
  constexpr int A_BYTES = BK * AROW, B_BYTES = BK * BROW, STAGE = 65536;
  static_assert(A_BYTES + B_BYTES <= STAGE && BM == 256 && BN == 256, "tile");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;                    // 2 x 4 waves of 128 (cout) x 64 (cin)

  const int T = p.KH * p.KW;
  const int ct = p.Cout / BM, it = p.Cin / BN;
  const int tiles = ct * it * T;
  // workgroup b = group * tiles + tile: the group's share of the K chunks ("splits": one slab each -- the K partition and the
  // order of every sum are those of wgrad_x6_body with the same split count, however many workgroups share the chunks)
  const int gi = bid / tiles;
  int tile = bid - gi * tiles;
  const int G = p.groups > 0 ? p.groups : p.splits;
  const int z0 = (int)(((long)p.splits * gi) / G), z1 = (int)(((long)p.splits * (gi + 1)) / G);
  const int tap = tile % T; tile /= T;
  const int co0 = (tile / it) * BM, ci0 = (tile % it) * BN;
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
  const int P = p.B * hv * wv;                                // contributing pixels of this tap
  const int steps = (P + BK - 1) / BK;

  // scales: the producers' (previous iteration's absmax + margin) checked against this iteration's absmax
  const unsigned mg = amax_read(p.slot_g), mx = amax_read(p.slot_x);
  float sg = *p.scp_g, sx = *p.scp_x;
  const bool okg = pair_scale_fits(mg, sg), okx = pair_scale_fits(mx, sx);
  if (!okg) sg = pair_scale_of(mg, 0);
  if (!okx) sx = pair_scale_of(mx, 0);
  if (bid == 0 && tid == 0) {
    if (p.scn_g) *p.scn_g = pair_scale_of(mg, p.margin_g);
    if (p.scn_x) *p.scn_x = pair_scale_of(mx, p.margin_x);
  }
  const float inv = 1.0f / (sg * sx);                          // powers of two: exact

  // DMA roles: row slot j (0..3) of this wave = pixel row k = 4 * wave + j of the K step, one instruction per operand
  const unsigned char* const gbase = p.g2 + ((size_t)tap * p.g_tap_stride + co0) * 4;
  const unsigned char* const xbase = p.x2 + ((size_t)tap * p.x_tap_stride + ci0) * 4;
  unsigned voff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = 4 * wave + j;
    const int f = (k & 1) | (((k >> 1) & 1) << 2) | (((k >> 3) & 1) << 3);
    voff[j] = (unsigned)((lane ^ f) << 4);
  }
  // contributing pixel q of row slot j: (image, row, column) inside the tap's rectangle, advanced by BK per K step
  int ri[4], ry[4], rx[4];
  const int hw = hv * wv > 0 ? hv * wv : 1, wv1 = wv > 0 ? wv : 1, hv1 = hv > 0 ? hv : 1;
  const unsigned lds0 = p_lds_addr(smem);
  // Slow path of an operand whose producer's scale does not fit (or that has no usable sibling): the K step's 32 pixel rows are
  // read from the fp32 tensor, split under the fresh scale and written into the same LDS image.  1024 (row, 8-channel group)
  // items per operand and step, two per thread.
  auto fill = [&](int st, unsigned char* dstS, const float* src, int ld, int c0, float sc, bool is_x) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + 512 * i;
      const int k = idx >> 5, G = idx & 31;
      const int q = st * BK + k;
      uint4 hi = make_uint4(0u, 0u, 0u, 0u), lo = hi;
      if (q < P) {
        const int img = q / hw, rem = q - img * hw;
        const int yy = rem / wv1, xx = rem - yy * wv1;
        const long pixel = is_x ? ((long)(img * p.Hi + (oy_lo + yy) * p.stride + dyk) * p.Wi + (ox_lo + xx) * p.stride + dxk)
                                : ((long)(img * p.Ho + oy_lo + yy) * p.Wo + ox_lo + xx);
        const float* a = src + pixel * ld + c0 + 8 * G;
        p_split8(*reinterpret_cast<const float4*>(a), *reinterpret_cast<const float4*>(a + 4), sc, hi, lo);
      }
      const int f = (k & 1) | (((k >> 1) & 1) << 2) | (((k >> 3) & 1) << 3);
      unsigned char* row = dstS + k * 1024;
      *reinterpret_cast<uint4*>(row + (((2 * G) ^ f) << 4)) = hi;
      *reinterpret_cast<uint4*>(row + (((2 * G + 1) ^ f) << 4)) = lo;
    }
  };
  const float* const gsrc = p.g + (size_t)tap * p.g_tap_stride;
  const float* const xsrc = p.x + (size_t)tap * p.x_tap_stride;

  auto issue = [&](int st, int buf) {
    const unsigned sA = lds0 + buf * STAGE + 4 * wave * AROW, sB = lds0 + buf * STAGE + A_BYTES + 4 * wave * BROW;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ok = ri[j] < p.B;
      const long ga = ((long)(ri[j] * p.Ho + oy_lo + ry[j]) * p.Wo + ox_lo + rx[j]) * p.ldg * 4;
      const long xa = ((long)(ri[j] * p.Hi + (oy_lo + ry[j]) * p.stride + dyk) * p.Wi + (ox_lo + rx[j]) * p.stride + dxk) * p.ldx * 4;
      const unsigned char* ga_p = ok ? gbase + ga : p.zero;
      const unsigned char* xa_p = ok ? xbase + xa : p.zero;
      if (okg) p_glds16(ga_p, voff[j], __builtin_amdgcn_readfirstlane(sA + j * AROW));
      if (okx) p_glds16(xa_p, voff[j], __builtin_amdgcn_readfirstlane(sB + j * BROW));
      // advance to the same slot of the next K step
      rx[j] += BK;
      while (rx[j] >= wv1) { rx[j] -= wv1; ++ry[j]; }
      while (ry[j] >= hv1) { ry[j] -= hv1; ++ri[j]; }
    }
    if (!okg) fill(st, smem + buf * STAGE, gsrc, p.ldg, co0, sg, false);
    if (!okx) fill(st, smem + buf * STAGE + A_BYTES, xsrc, p.ldx, ci0, sx, true);
  };

  // fragment read addresses (stage 0; the stage toggles by XOR with STAGE)
  const int g = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, pp = i16 & 3, h = pp >> 1;
  const int fl = (q4 & 1) | (((q4 >> 1) & 1) << 2) | ((g & 1) << 3);
  const unsigned kbase = (unsigned)((8 * g + q4) * 1024 + 8 * (pp & 1));     // AROW == BROW == 1024
  unsigned aoff[4][2], boff[4][2];                          // [t & 3][piece]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      const unsigned phys = (unsigned)((((a ^ (fl >> 2)) & 3) << 2) | (h << 1) | (pc ^ (fl & 1)));
      aoff[a][pc] = lds0 + kbase + (phys << 4) + (unsigned)(2 * wm) * 256u;
      boff[a][pc] = lds0 + A_BYTES + kbase + (phys << 4) + (unsigned)wn * 256u;
    }

  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll 1
  for (int z = z0; z < z1; ++z) {
  const int st_begin = (int)(((long)steps * z) / p.splits);
  const int st_end = (int)(((long)steps * (z + 1)) / p.splits);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = st_begin * BK + 4 * wave + j;
    ri[j] = q / hw;
    const int rem = q - ri[j] * hw;
    ry[j] = rem / wv1;
    rx[j] = rem - ry[j] * wv1;
  }
  pf32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

  if (z > z0) __builtin_amdgcn_s_barrier();      // every wave has read the previous chunk's last stage
  if (st_begin < st_end) issue(st_begin, 0);
  for (int st = st_begin; st < st_end; ++st) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (st + 1 < st_end) issue(st + 1, (st - st_begin + 1) & 1);
    pf16x8 fb[4][2];
#pragma unroll
    for (int tn = 0; tn < 4; ++tn)
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) fb[tn][pc] = p_tr_frag(boff[tn][pc], 1024);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int tm = 0; tm < 8; ++tm) {
      pf16x8 fa[2];
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) fa[pc] = p_tr_frag(aoff[tm & 3][pc] + (unsigned)(tm >> 2) * 256u, 1024);
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) {
        pf32x4 c = acc[tm][tn];
        c = P_MFMA(fa[1], fb[tn][0], c);                   // smallest terms first (as wgrad_x6_body)
        c = P_MFMA(fa[0], fb[tn][1], c);
        c = P_MFMA(fa[0], fb[tn][0], c);
        acc[tm][tn] = c;
      }
    }
    __builtin_amdgcn_s_setprio(0);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) { aoff[a][pc] ^= (unsigned)STAGE; boff[a][pc] ^= (unsigned)STAGE; }
  }

  if ((st_end - st_begin) & 1) {                  // an odd number of K steps leaves the fragment addresses on stage 1
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) { aoff[a][pc] ^= (unsigned)STAGE; boff[a][pc] ^= (unsigned)STAGE; }
  }
  // slab z of the tile.  D row (cout) = 4 * (lane >> 4) + e, column (cin) = lane & 15.
  float* out = p.ws + (size_t)z * p.Cout * T * p.Cin;
#pragma unroll
  for (int tm = 0; tm < 8; ++tm)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int co = co0 + wm * 128 + tm * 16 + 4 * fq + e;
      float* row = out + ((size_t)co * T + tap) * p.Cin + ci0 + wn * 64 + fr;
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) row[tn * 16] = acc[tm][tn][e] * inv;
    }
  }
}

template <int BM, int BN>
__global__ __launch_bounds__(512, 1) void wgrad_p_kernel(const WgradPArgs p) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[131072];
  wgrad_p_body<BM, BN>(p, xcd_remap(blockIdx.x, gridDim.x), smem);
}
// several weight gradients in one launch (wgrad_h3_group_kernel's scheme): workgroup w works on entry map[w].x as its workgroup map[w].y
template <int BM, int BN>
__global__ __launch_bounds__(512, 1) void wgrad_p_group_kernel(const WgradPArgs* __restrict__ tab, const int2* __restrict__ map) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[131072];
  const int2 m = map[xcd_remap(blockIdx.x, gridDim.x)];
  const int ent = __builtin_amdgcn_readfirstlane(m.x), bid = __builtin_amdgcn_readfirstlane(m.y);
  const WgradPArgs p = tab[ent];
  wgrad_p_body<BM, BN>(p, bid, smem);
}

bool wgrad_p_supported(const WgradPArgs& a) {
  return a.Cout % 256 == 0 && a.Cin % 256 == 0 && a.ldg % 8 == 0 && a.ldx % 8 == 0;
}
int wgrad_p_tiles(const WgradPArgs& a) { return (a.Cout / 256) * (a.Cin / 256) * a.KH * a.KW; }
// K splits: one resident round of the 256 one-per-CU workgroups, at least 4 K steps of 32 pixels each.  Measured on the
// stride-16 shapes (profiles/r06_wgrad_p_probe.txt): tiles x splits at 85-100 % of 256 is the optimum; half or double is 10-40 % slower.
// workgroups a pre-split weight-gradient launch plans for: one per CU of the budget's share of the chip
int wgrad_p_resident(int wg_budget) {
  const int r = conv_wg_budget_of(wg_budget) / 2;
  return r < 8 ? 8 : r;
}
int wgrad_p_pick_splits(int P, int Cout, int Cin, int T, int wg_budget) {
  const int tiles = (Cout / 256) * (Cin / 256) * T;
  const int res = wgrad_p_resident(wg_budget);
  const int steps = (P + 31) / 32;
  int s = tiles > 0 ? res / tiles : 1;
  if (s > steps / 4) s = steps / 4;
  return s < 1 ? 1 : (s > 512 ? 512 : s);
}
static double wgrad_p_flops(const WgradPArgs& a) {
  WgradArgs w{};
  w.B = a.B; w.Ho = a.Ho; w.Wo = a.Wo; w.Hi = a.Hi; w.Wi = a.Wi; w.KH = a.KH; w.KW = a.KW; w.stride = a.stride; w.pad = a.pad; w.dil = a.dil;
  w.g_tap_stride = a.g_tap_stride;
  return 2.0 * a.Cout * a.Cin * a.KH * a.KW * (double)a.B * a.Ho * a.Wo * wgrad_exec_frac(w);
}
void launch_wgrad_p(const WgradPArgs& a, hipStream_t s) {
  const int nwg = wgrad_p_tiles(a) * (a.groups > 0 ? a.groups : a.splits);
  conv_prof_mark_begin(kProfWgradP, wgrad_p_flops(a), s);
  hipLaunchKernelGGL((wgrad_p_kernel<256, 256>), dim3(nwg), dim3(512), 0, s, a);
  conv_prof_mark_end(s);
}
void launch_wgrad_p_group(const WgradPArgs* dev_tab, const int* dev_map, int nwg, double flops, hipStream_t s) {
  conv_prof_mark_begin(kProfWgradPGroup, flops, s);
  hipLaunchKernelGGL((wgrad_p_group_kernel<256, 256>), dim3(nwg), dim3(512), 0, s, dev_tab, reinterpret_cast<const int2*>(dev_map));
  conv_prof_mark_end(s);
}

}  // namespace eosvos
