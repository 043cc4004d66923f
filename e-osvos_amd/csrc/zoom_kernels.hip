// Object-centred zoom pass of the inference path, for gfx950: the box of a frame's first-pass foreground, the frame cut to
// that box and magnified to the frame's own size, the view's logits put back into the box, and the blend with the first
// pass.  The rules are stated in include/eosvos.h (eosvos_zoom_boxes .. eosvos_zoom_blend) and restated in numpy / torch by
// eosvos_amd/zoom.py (boxes_host, refine_host).
//
//   zoom_bounds_kernel      a wave owns one 64-pixel segment of a row at a time (four rows per wave): the ballot word of
//                           p >= threshold gives the segment's lowest and highest foreground column and its popcount the
//                           count, all wave-uniform.  The four waves combine in LDS, thread 0 issues at most five integer
//                           atomics on the frame's record {max (H - 1 - y), max y, max (W - 1 - x), max x, count}.  The
//                           record is zeroed by the caller's memset on the same stream: every bound is kept as a maximum, so
//                           zero is the neutral start.  Integer atomics only: the result does not depend on any order.
//   zoom_box_kernel         a second tiny launch, one thread per frame: steps 2-5 of the rule in 64-bit integers.
//   zoom_crop_kernel        one thread per output element: the bilinear rule of tta_src applied to the slice (clamped at the
//                           box edge); an invalid frame is copied through.
//   zoom_accumulate_kernel  one thread per frame pixel, pixels outside a valid box leave: the boxed sibling of
//                           tta_accumulate_kernel, logits H x W -> bh x bw.
//   zoom_blend_kernel       one thread per frame pixel, in place inside valid boxes.
// A box is read from device memory and clamped into the frame before it addresses anything (zoom_load_box): whatever the
// five words hold, every read and write stays inside the tensors.  No launch is cooperative, no workgroup waits for another,
// one writer per element.  Vector stores only.
#include "kernels.h"

namespace eosvos {
namespace {
struct ZoomBox { int valid, y0, x0, bh, bw; };

__device__ __forceinline__ ZoomBox zoom_load_box(const int* __restrict__ boxes, long frame, int H, int W) {
  const int* b = boxes + frame * 5;
  ZoomBox z;
  z.valid = b[0] != 0;
  z.y0 = min(max(b[1], 0), H - 1);
  z.x0 = min(max(b[2], 0), W - 1);
  z.bh = min(max(b[3], 1), H - z.y0);
  z.bw = min(max(b[4], 1), W - z.x0);
  return z;
}

// grid (ceil(W / 64), ceil(H / 16), frames), block 256.  No thread leaves before the ballots: they see whole waves.
__global__ __launch_bounds__(256) void zoom_bounds_kernel(const float* __restrict__ probs, int H, int W, float threshold,
                                                           int* __restrict__ rec) {
  __shared__ int sh[4][5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t f = blockIdx.z;
  const float* p = probs + f * (size_t)H * W;
  const int xb = (int)blockIdx.x * 64, x = xb + lane;
  int ylo = H, yhi = -1, xlo = W, xhi = -1, cnt = 0;      // wave-uniform
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = (int)blockIdx.y * 16 + wave + 4 * k;    // wave-uniform
    const bool on = y < H && x < W && p[(size_t)y * W + x] >= threshold;
    const unsigned long long m = __ballot(on);
    if (m) {
      ylo = min(ylo, y);
      yhi = max(yhi, y);
      xlo = min(xlo, xb + (__ffsll((long long)m) - 1));
      xhi = max(xhi, xb + 63 - __clzll((long long)m));
      cnt += __popcll(m);
    }
  }
  if (lane == 0) { sh[wave][0] = ylo; sh[wave][1] = yhi; sh[wave][2] = xlo; sh[wave][3] = xhi; sh[wave][4] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      ylo = min(ylo, sh[w][0]); yhi = max(yhi, sh[w][1]); xlo = min(xlo, sh[w][2]); xhi = max(xhi, sh[w][3]); cnt += sh[w][4];
    }
    if (cnt) {
      int* r = rec + f * 8;
      atomicMax(r + 0, H - 1 - ylo);
      atomicMax(r + 1, yhi);
      atomicMax(r + 2, W - 1 - xlo);
      atomicMax(r + 3, xhi);
      atomicAdd(r + 4, cnt);
    }
  }
}

__device__ __forceinline__ long long zoom_ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// one thread per frame: steps 2-5.  Every product fits 64 bits by far (sides <= 4096, Q16 factors <= 4 * 65536).
__global__ void zoom_box_kernel(const int* __restrict__ rec, int n_frames, int H, int W, int min_pixels, int margin_q16,
                                int margin_px, int min_zoom_q16, int max_zoom_q16, int* __restrict__ boxes) {
  const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (f >= n_frames) return;
  const int* r = rec + (size_t)f * 8;
  int* out = boxes + (size_t)f * 5;
  const int cnt = r[4];
  bool valid = cnt >= min_pixels;
  long long y0 = 0, x0 = 0, bh = H, bw = W;
  if (valid) {
    const long long my0 = H - 1 - r[0], my1 = r[1], mx0 = W - 1 - r[2], mx1 = r[3];
    const long long mh = my1 - my0 + 1, mw = mx1 - mx0 + 1;
    const long long pad = (((mh > mw ? mh : mw) * margin_q16) >> 16) + margin_px;
    const long long gh = mh + 2 * pad, gw = mw + 2 * pad;
    long long want = gh;
    const long long asp = zoom_ceil_div(gw * H, W), flo = zoom_ceil_div((long long)H * 65536, max_zoom_q16);
    if (asp > want) want = asp;
    if (flo > want) want = flo;
    bh = want < H ? want : H;
    bw = zoom_ceil_div(bh * W, H);
    if (bw > W) bw = W;
    if (bh * min_zoom_q16 > (long long)H * 65536) {
      valid = false;
      bh = H;
      bw = W;
    } else {
      y0 = (2 * my0 + mh - bh) >> 1;                      // arithmetic shift: floor
      x0 = (2 * mx0 + mw - bw) >> 1;
      y0 = y0 < 0 ? 0 : (y0 > H - bh ? H - bh : y0);
      x0 = x0 < 0 ? 0 : (x0 > W - bw ? W - bw : x0);
    }
  }
  out[0] = valid ? 1 : 0;
  out[1] = (int)y0;
  out[2] = (int)x0;
  out[3] = (int)bh;
  out[4] = (int)bw;
}

// out (B, C, H, W) = bilinear(frame[:, y0:y0+bh, x0:x0+bw] -> H x W), the slice's own align_corners=False rule
__global__ __launch_bounds__(256) void zoom_crop_kernel(const float* __restrict__ frames, const int* __restrict__ boxes, int B, int C,
                                                         int H, int W, float* __restrict__ out) {
  const long plane = (long)H * W, n = (long)B * C * plane;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int ox = (int)(i % W), oy = (int)((i / W) % H);
    const long pl = i / plane;
    const ZoomBox z = zoom_load_box(boxes, pl / C, H, W);
    if (!z.valid) {
      out[i] = frames[i];
      continue;
    }
    int y0, y1, x0, x1;
    float ly, lx;
    tta_src(oy, (float)z.bh / (float)H, z.bh, y0, y1, ly);
    tta_src(ox, (float)z.bw / (float)W, z.bw, x0, x1, lx);
    const float* src = frames + pl * plane + (long)z.y0 * W + z.x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float v00 = src[(long)y0 * W + x0], v01 = src[(long)y0 * W + x1];
    const float v10 = src[(long)y1 * W + x0], v11 = src[(long)y1 * W + x1];
    out[i] = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
  }
}

// pz (B, H, W) inside each valid box = (first ? 0 : pz) + weight * sigmoid(bilinear(unmirror(logits) (H x W) -> bh x bw))
__global__ __launch_bounds__(256) void zoom_accumulate_kernel(const float* __restrict__ logits, const int* __restrict__ boxes, int B,
                                                               int H, int W, int mirror, float weight, int first,
                                                               float* __restrict__ pz) {
  const long plane = (long)H * W, n = (long)B * plane;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const long f = i / plane;
    const ZoomBox z = zoom_load_box(boxes, f, H, W);
    const int by = y - z.y0, bx = x - z.x0;
    if (!z.valid || by < 0 || by >= z.bh || bx < 0 || bx >= z.bw) continue;
    const float* src = logits + f * plane;
    float xv;
    if (z.bh == H && z.bw == W) {                         // the box is the frame: the logit itself
      xv = src[(long)by * W + (mirror ? W - 1 - bx : bx)];
    } else {
      int y0, y1, x0, x1;
      float ly, lx;
      tta_src(by, (float)H / (float)z.bh, H, y0, y1, ly);
      tta_src(bx, (float)W / (float)z.bw, W, x0, x1, lx);
      if (mirror) { x0 = W - 1 - x0; x1 = W - 1 - x1; }   // column x of the un-mirrored view is column W - 1 - x of the logits
      const float hy = 1.f - ly, hx = 1.f - lx;
      const float v00 = src[(long)y0 * W + x0], v01 = src[(long)y0 * W + x1];
      const float v10 = src[(long)y1 * W + x0], v11 = src[(long)y1 * W + x1];
      xv = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
    }
    const float e = expf(-fabsf(xv));                     // the sigmoid of tta_accumulate_kernel
    const float p = weight * (xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e));
    pz[i] = first ? p : pz[i] + p;
  }
}

// probs = p0 + (weight * f) * (pz - p0) inside valid boxes, f the linear ramp at the box sides that are not frame borders
__global__ __launch_bounds__(256) void zoom_blend_kernel(const int* __restrict__ boxes, int B, int H, int W, float weight, int feather,
                                                          const float* __restrict__ pz, float* __restrict__ probs) {
  const long plane = (long)H * W, n = (long)B * plane;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const ZoomBox z = zoom_load_box(boxes, i / plane, H, W);
    const int by = y - z.y0, bx = x - z.x0;
    if (!z.valid || by < 0 || by >= z.bh || bx < 0 || bx >= z.bw) continue;
    int d = 0x7fffffff;
    if (z.y0 > 0) d = min(d, by);
    if (z.y0 + z.bh < H) d = min(d, z.bh - 1 - by);
    if (z.x0 > 0) d = min(d, bx);
    if (z.x0 + z.bw < W) d = min(d, z.bw - 1 - bx);
    float f = 1.f;
    if (feather > 0 && d < feather) f = __fdiv_rn((float)(d + 1), (float)(feather + 1));
    const float p0 = probs[i];
    probs[i] = __fadd_rn(p0, __fmul_rn(__fmul_rn(weight, f), __fsub_rn(pz[i], p0)));      // in this order, nothing contracted
  }
}

inline int zoom_grid(long n) {
  const long b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : b > 8192 ? 8192 : b);
}
}  // namespace

void launch_zoom_boxes(const float* probs, int n_frames, int H, int W, float threshold, int min_pixels, int margin_q16, int margin_px,
                       int min_zoom_q16, int max_zoom_q16, int* rec, int* boxes, hipStream_t s) {
  hipLaunchKernelGGL(zoom_bounds_kernel, dim3((W + 63) / 64, (H + 15) / 16, n_frames), dim3(256), 0, s, probs, H, W, threshold, rec);
  hipLaunchKernelGGL(zoom_box_kernel, dim3((n_frames + 63) / 64), dim3(64), 0, s, rec, n_frames, H, W, min_pixels, margin_q16,
                     margin_px, min_zoom_q16, max_zoom_q16, boxes);
}

void launch_zoom_crop(const float* frames, const int* boxes, int B, int C, int H, int W, float* out, hipStream_t s) {
  hipLaunchKernelGGL(zoom_crop_kernel, dim3(zoom_grid((long)B * C * H * W)), dim3(256), 0, s, frames, boxes, B, C, H, W, out);
}

void launch_zoom_accumulate(const float* logits, const int* boxes, int B, int H, int W, int mirror, float weight, int first, float* pz,
                            hipStream_t s) {
  hipLaunchKernelGGL(zoom_accumulate_kernel, dim3(zoom_grid((long)B * H * W)), dim3(256), 0, s, logits, boxes, B, H, W, mirror, weight,
                     first, pz);
}

void launch_zoom_blend(const int* boxes, int B, int H, int W, float weight, int feather, const float* pz, float* probs, hipStream_t s) {
  hipLaunchKernelGGL(zoom_blend_kernel, dim3(zoom_grid((long)B * H * W)), dim3(256), 0, s, boxes, B, H, W, weight, feather, pz, probs);
}
}  // namespace eosvos
