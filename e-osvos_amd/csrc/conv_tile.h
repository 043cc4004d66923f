// Device-only helpers shared by the convolution kernels (conv_kernels.hip) and the pre-split weight gradient
// (presplit_kernels.hip): the XCD remap, the 16-byte loads, the destination-pixel map and the pair8 store.
#pragma once
#include "kernels.h"

namespace eosvos {

// Blocks are dealt round-robin over the 8 XCDs; give each XCD a contiguous range of tiles
// so neighbouring tiles (which share the gathered operand) meet in one L2.  Bijective for
// every grid size.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

__device__ __forceinline__ float4 ldg4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// 16-byte buffer load; offsets past the descriptor's size return 0 (hardware range check)
__device__ __forceinline__ float4 bufld4(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
  auto v = __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0);
  return *reinterpret_cast<float4*>(&v);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const float* p, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, (int)(bytes > 0x7fffffffL ? 0x7fffffffL : bytes), 0x00020000);
}

// destination pixel of GEMM row m: dense, or (1x1 stride-2 data gradient) the even pixels of
// the finer destination grid -- the odd ones receive no contribution and are never touched
__device__ __forceinline__ size_t dst_pixel(const ConvArgs& p, int m) {
  if (p.par) return (size_t)conv_par_pixel(p.B, p.Ho, p.Wo, m);
  if (!p.dst_up) return (size_t)m;
  const int hw = p.Ho * p.Wo;
  const int b = m / hw, rem = m - b * hw;
  const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
  return ((size_t)b * p.Hf + (oy << 1)) * p.Wf + (ox << 1);
}

// pre-split operand path: 4 consecutive channels n .. n + 3 of pixel `pix` into the destination's pair8 sibling
// (presplit_kernels.hip: per 8 channels [8 x fp16 hi | 8 x fp16 lo]; same two pieces as h3_split_pair)
__device__ __forceinline__ void pair_store4(unsigned char* y2, size_t pix, int ldy, int n, const float4& v, float s) {
  typedef _Float16 ph2 __attribute__((ext_vector_type(2)));
  typedef float pf2 __attribute__((ext_vector_type(2)));
  const pf2 a = {v.x * s, v.y * s}, b = {v.z * s, v.w * s};
  const ph2 ha = __builtin_convertvector(a, ph2), hb = __builtin_convertvector(b, ph2);
  const pf2 ua = __builtin_convertvector(ha, pf2), ub = __builtin_convertvector(hb, pf2);
  const pf2 ra = {a.x - ua.x, a.y - ua.y}, rb = {b.x - ub.x, b.y - ub.y};
  const ph2 la = __builtin_convertvector(ra, ph2), lb = __builtin_convertvector(rb, ph2);
  unsigned char* q = y2 + (pix * (size_t)ldy + (size_t)(n & ~7)) * 4 + (n & 4) * 2;
  *reinterpret_cast<uint2*>(q) = make_uint2(__builtin_bit_cast(unsigned, ha), __builtin_bit_cast(unsigned, hb));
  *reinterpret_cast<uint2*>(q + 16) = make_uint2(__builtin_bit_cast(unsigned, la), __builtin_bit_cast(unsigned, lb));
}

}  // namespace eosvos
