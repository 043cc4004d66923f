// Bootstrapped (hard-pixel) BCE with logits + gradient for gfx950: per set of pixels keep the k hardest, average those.
//
// For one set, V its non-void pixels, n = |V|:
//   key_p = -x_p * (2 * (t_p >= .5) - 1)        (an exact sign flip: for hard targets BCE is strictly increasing in the key)
//   u_p   = the key as an order-preserving unsigned word: -0 -> +0, NaN -> 0xffffffff, negative -> ~bits, else bits | 2^31
//   k     = max(1, (n * q + 32768) >> 16),  q = round(fraction * 65536) in [1, 65536]
//   tau   = the k-th largest u;  G = #{u > tau},  T = #{u == tau},  r = k - G  (1 <= r <= T)
//   w_p   = 1 where u_p > tau,  (float)r / (float)T where u_p == tau,  0 elsewhere and at every void pixel
//   loss  = mean over the sets of (sum_V w_p bce_p) / k;   dL/dx_p = w_p (sigmoid(x_p) - t_p) / (k * sets), exactly +0 where w_p = 0
// The ties at the threshold share the remaining r slots, so nothing depends on which of them would be taken.
//
// Pipeline (one stream; every dependency is a kernel boundary, no workgroup waits for another):
//   zero      the three 2048-bin histograms of every set
//   hist 0    digit = u >> 21 of every valid pixel
//   hist 1    [pick 0]  digit = (u >> 10) & 2047 of the pixels whose top 11 bits are the picked ones
//   hist 2    [pick 1]  digit = u & 1023 of the pixels whose top 22 bits are the picked ones
//   value     [pick 2]  w * bce into per-workgroup partials (fp64), the gradient
//   final     partials summed in a fixed order, / k, mean over the sets
// A histogram pass keeps 2048 LDS bins per workgroup; a wave first merges the lanes that share a digit (the logits of a real
// map fall into a few dozen top-digit bins) and sends one LDS atomic per merged group, then each non-zero bin goes to the
// set's global histogram with one integer atomic.  `pick` is the prologue of the following launch: every workgroup walks the
// set's 2048 bins from the top (8 bins per thread and a suffix sum over the threads) and finds the digit that holds the
// remaining rank; workgroup 0 of the set records it for the launches after.  Integer atomics only: the counts, and with
// them tau, G, T and r, do not depend on arrival order, and the float sums run in a fixed order -- the result is bit-
// reproducible.  All keys equal is the slowest case of the wave merge's fallback (one group per row), never a wrong one.
// Sets of fewer than 2^31 pixels.
#include "kernels.h"
#include "loss_expr.h"

namespace eosvos {
namespace {

constexpr int BS_THREADS = 256;
constexpr int BS_BINS = 2048;                    // per pass (the last one uses 1024 of them)
constexpr int BS_STATE = 16;                     // words per set, see BsState
constexpr int BS_MERGE_ROUNDS = 4;               // merged digit groups per wave row before plain LDS atomics take the rest

// per-set words, each written by workgroup 0 of the launch named and read by the launches after it
enum BsState {
  BS_N = 0, BS_K = 1, BS_D0 = 2, BS_R1 = 3, BS_G1 = 4,      // hist 1: valid pixels, k, top digit, rank within it, count above it
  BS_P22 = 5, BS_R2 = 6, BS_G2 = 7,                         // hist 2: top 22 bits, rank within them, count above them
  BS_TAU = 8, BS_G = 9, BS_T = 10, BS_R = 11                // value: the threshold, G, T, r
};

struct BsScratch {
  int *hist, *state;
  double* partial;
};
inline BsScratch bs_carve(float* scratch, int max_sets) {
  BsScratch S;
  S.partial = (double*)scratch;                                   // (hipMalloc alignment keeps the fp64 words aligned)
  S.hist = (int*)(S.partial + (int64_t)max_sets * BOOTSTRAP_BLOCKS);
  S.state = S.hist + (int64_t)max_sets * 3 * BS_BINS;
  return S;
}

// the order-preserving word of a pixel's key; `valid` false for a void pixel
template <bool VOID>
__device__ __forceinline__ unsigned bs_key(float xv, float tv, float ign, bool& valid) {
  valid = !VOID || tv != ign;
  const float key = tv >= 0.5f ? -xv : xv;
  unsigned b = __float_as_uint(key);
  if (key != key) return 0xffffffffu;
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// fp64 sum over the 256 threads in a fixed order, valid in every thread
__device__ __forceinline__ double bs_block_sum_d(double v, double* sh /*4*/) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// The bin of h[0 .. 2048) that holds the R-th largest element counted from the top bin down: res = {bin, count in the bins
// above it, count in it}, valid in every thread; `total` = the sum of all bins.  R <= 0 asks for the rank k of a set of `total`
// pixels at fraction q / 65536 (the first pick), returned in R.  With total == 0 (or R out of range) res is {0, 0, 0}.
__device__ __forceinline__ void bs_pick(const int* __restrict__ h, int& R, int q, int& total, int* res /*shared, 3*/,
                                        int* sh /*shared, 4*/) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int c[8], own = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) { c[j] = h[t * 8 + j]; own += c[j]; }
  int v = own;                                   // inclusive suffix sum over the lanes of the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int d = __shfl_down(v, o, 64);
    if (lane + o < 64) v += d;
  }
  __syncthreads();
  if (lane == 0) sh[w] = v;
  if (t == 0) { res[0] = 0; res[1] = 0; res[2] = 0; }
  __syncthreads();
  int above = v - own;                           // count in the bins of the threads after this one
  for (int ww = w + 1; ww < 4; ++ww) above += sh[ww];
  total = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  if (R <= 0) {
    const long long kk = ((long long)total * q + 32768) >> 16;
    R = total > 0 ? (int)(kk < 1 ? 1 : kk) : 0;
  }
  if (R > 0 && above < R && R <= above + own) {  // one thread
    int a = above;
#pragma unroll
    for (int j = 7; j >= 0; --j) {
      if (R > a && R <= a + c[j]) { res[0] = t * 8 + j; res[1] = a; res[2] = c[j]; }
      a += c[j];
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(BS_THREADS) void bootstrap_zero_kernel(int* __restrict__ hist, long n) {
  for (long i = (long)blockIdx.x * BS_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * BS_THREADS) hist[i] = 0;
}

// PASS 0 / 1 / 2: the histogram of the digit at bits 31..21 / 20..10 / 9..0 among the set's valid pixels whose higher bits
// match the digits picked so far.  blockIdx.y = set.  VOID = false never reads `ign`.
template <bool VOID, int PASS>
__global__ __launch_bounds__(BS_THREADS) void bootstrap_hist_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                    int* __restrict__ hist, int* __restrict__ state,
                                                                    long seg_len, int q, float ign) {
  __shared__ int h[BS_BINS];
  __shared__ int res[3], sh[4];
  const int set = blockIdx.y, lane = threadIdx.x & 63;
  int* st = state + set * BS_STATE;
  int* hs = hist + (long)set * 3 * BS_BINS;
  unsigned prefix = 0;
  if (PASS == 1) {
    int R = 0, total;
    bs_pick(hs, R, q, total, res, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      st[BS_N] = total; st[BS_K] = R; st[BS_D0] = res[0]; st[BS_R1] = R - res[1]; st[BS_G1] = res[1];
    }
    if (total == 0) return;
    prefix = (unsigned)res[0];
  } else if (PASS == 2) {
    if (st[BS_N] == 0) return;
    int R = st[BS_R1], total;
    bs_pick(hs + BS_BINS, R, q, total, res, sh);
    prefix = ((unsigned)st[BS_D0] << 11) | (unsigned)res[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      st[BS_P22] = (int)prefix; st[BS_R2] = R - res[1]; st[BS_G2] = st[BS_G1] + res[1];
    }
  }
  for (int i = threadIdx.x; i < BS_BINS; i += BS_THREADS) h[i] = 0;
  __syncthreads();
  const long seg0 = (long)set * seg_len;
  for (long base = (long)blockIdx.x * BS_THREADS; base < seg_len; base += (long)gridDim.x * BS_THREADS) {   // wave-uniform trips
    const long i = base + threadIdx.x;
    bool in = false;
    unsigned d = 0;
    if (i < seg_len) {
      const unsigned u = bs_key<VOID>(x[seg0 + i], t[seg0 + i], ign, in);
      if (PASS == 0) d = u >> 21;
      else if (PASS == 1) { d = (u >> 10) & 2047u; in = in && (u >> 21) == prefix; }
      else { d = u & 1023u; in = in && (u >> 10) == prefix; }
    }
    unsigned long long rem = __ballot(in);
    for (int it = 0; it < BS_MERGE_ROUNDS && rem; ++it) {           // the lanes that share the first remaining lane's digit
      const int first = __ffsll((long long)rem) - 1;
      const unsigned d0 = (unsigned)__shfl((int)d, first, 64);
      const unsigned long long m = __ballot(in && d == d0) & rem;
      if (lane == first) atomicAdd(&h[d0], __popcll(m));
      rem &= ~m;
    }
    if ((rem >> lane) & 1ull) atomicAdd(&h[d], 1);
  }
  __syncthreads();
  int* out = hs + PASS * BS_BINS;
  for (int i = threadIdx.x; i < BS_BINS; i += BS_THREADS) {
    const int c = h[i];
    if (c) atomicAdd(&out[i], c);
  }
}

// w * bce into partial[set][block], the gradient into dx.  `sets`: the divisor of the mean (the gradient's scale).
template <bool VOID>
__global__ __launch_bounds__(BS_THREADS) void bootstrap_value_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                     float* __restrict__ dx, const int* __restrict__ hist,
                                                                     int* __restrict__ state, double* __restrict__ partial,
                                                                     long seg_len, int q, int sets, float ign) {
  __shared__ int res[3], sh[4];
  __shared__ double shd[4];
  const int set = blockIdx.y;
  int* st = state + set * BS_STATE;
  const long seg0 = (long)set * seg_len;
  const int n = st[BS_N];
  if (n == 0) {                                  // an empty valid set: loss 0, gradient +0
    for (long i = (long)blockIdx.x * BS_THREADS + threadIdx.x; i < seg_len; i += (long)gridDim.x * BS_THREADS) dx[seg0 + i] = 0.f;
    if (threadIdx.x == 0) partial[(long)set * BOOTSTRAP_BLOCKS + blockIdx.x] = 0.0;
    return;
  }
  int R = st[BS_R2], total;
  bs_pick(hist + ((long)set * 3 + 2) * BS_BINS, R, q, total, res, sh);
  const unsigned tau = ((unsigned)st[BS_P22] << 10) | (unsigned)res[0];
  const int k = st[BS_K], G = st[BS_G2] + res[1], T = res[2], r = k - G;
  if (blockIdx.x == 0 && threadIdx.x == 0) { st[BS_TAU] = (int)tau; st[BS_G] = G; st[BS_T] = T; st[BS_R] = r; }
  const float wt = (float)r / (float)T;          // exactly 1 when r == T
  const float inv = 1.0f / ((float)k * (float)sets);
  float s = 0.f;
  for (long i = (long)blockIdx.x * BS_THREADS + threadIdx.x; i < seg_len; i += (long)gridDim.x * BS_THREADS) {
    const float xv = x[seg0 + i], tv = t[seg0 + i];
    bool ok;
    const unsigned u = bs_key<VOID>(xv, tv, ign, ok);
    const float w = !ok ? 0.f : u > tau ? 1.f : u == tau ? wt : 0.f;
    const float e = expf(-fabsf(xv));
    const float v = bce_value(xv, tv, e);
    const float g = bce_grad(xv, tv, e, inv);
    s = w != 0.f ? s + w * v : s;                // selected, never multiplied by 0: a dropped logit may be NaN / inf
    dx[seg0 + i] = w != 0.f ? w * g : 0.f;
  }
  const double sd = bs_block_sum_d((double)s, shd);
  if (threadIdx.x == 0) partial[(long)set * BOOTSTRAP_BLOCKS + blockIdx.x] = sd;
}

__global__ __launch_bounds__(BS_THREADS) void bootstrap_final_kernel(const double* __restrict__ partial, const int* __restrict__ state,
                                                                     float* __restrict__ loss, int sets, int nb) {
  __shared__ double shd[4];
  double tot = 0.0;
  for (int set = 0; set < sets; ++set) {
    const int k = state[set * BS_STATE + BS_K];
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += BS_THREADS) a += partial[(long)set * BOOTSTRAP_BLOCKS + b];
    a = bs_block_sum_d(a, shd);
    tot += k > 0 ? a / (double)k : 0.0;
  }
  if (threadIdx.x == 0) loss[0] = (float)(tot / (double)sets);
}

template <bool VOID>
void bootstrap_launches(const float* logits, const float* gt, float* dlogits, float* loss, float* scratch, int64_t n_per_set,
                        int sets, int q, float ign, hipStream_t s) {
  const BsScratch S = bs_carve(scratch, sets);
  const long seg_len = (long)n_per_set;
  int64_t nbl = (n_per_set + BS_THREADS - 1) / BS_THREADS;
  const int nb = (int)(nbl < 1 ? 1 : nbl > BOOTSTRAP_BLOCKS ? BOOTSTRAP_BLOCKS : nbl);
  const dim3 grid(nb, sets), block(BS_THREADS);
  const long nh = (long)sets * 3 * BS_BINS;
  hipLaunchKernelGGL(bootstrap_zero_kernel, dim3((unsigned)((nh + BS_THREADS - 1) / BS_THREADS)), block, 0, s, S.hist, nh);
  hipLaunchKernelGGL((bootstrap_hist_kernel<VOID, 0>), grid, block, 0, s, logits, gt, S.hist, S.state, seg_len, q, ign);
  hipLaunchKernelGGL((bootstrap_hist_kernel<VOID, 1>), grid, block, 0, s, logits, gt, S.hist, S.state, seg_len, q, ign);
  hipLaunchKernelGGL((bootstrap_hist_kernel<VOID, 2>), grid, block, 0, s, logits, gt, S.hist, S.state, seg_len, q, ign);
  hipLaunchKernelGGL((bootstrap_value_kernel<VOID>), grid, block, 0, s, logits, gt, dlogits, S.hist, S.state, S.partial, seg_len, q,
                     sets, ign);
  hipLaunchKernelGGL(bootstrap_final_kernel, dim3(1), block, 0, s, S.partial, S.state, loss, sets, nb);
}
}  // namespace

int64_t bootstrap_scratch_floats(int max_sets) {
  return (int64_t)max_sets * (2 * BOOTSTRAP_BLOCKS + 3 * BS_BINS + BS_STATE) + 16;
}

void launch_bootstrap_bce(const float* logits, const float* gt, float* dlogits, float* loss, float* scratch, int64_t n_per_set,
                          int sets, int q, const float* ignore, hipStream_t s) {
  if (ignore) bootstrap_launches<true>(logits, gt, dlogits, loss, scratch, n_per_set, sets, q, *ignore, s);
  else bootstrap_launches<false>(logits, gt, dlogits, loss, scratch, n_per_set, sets, q, 0.f, s);
}

}  // namespace eosvos
