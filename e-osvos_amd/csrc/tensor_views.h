// The network's activation / gradient tensors and their channel-slice views (engine.cpp), with everything the engine keeps
// ABOUT a tensor hanging off its record: ReLU mask bytes, absmax slot, fp16-pair sibling.
// Host-only C++17, no HIP: tests/host/tensor_views_main.cpp prints what the accessors compute and
// tests/test_tensor_views_host.py checks it against the formulas written out there.
#pragma once
#include <cstdint>
#include <deque>

constexpr int TSLOTS = 384;          // absmax slots of tensors, per phase

// pre-split operand path (presplit_kernels.hip): the "pair8" sibling of an fp32 tensor -- the two fp16 pieces of the f16x3
// product laid out for LDS-DMA.  One sibling per TENSOR; a view's sibling is the same offset into it.  Once a consumer has
// asked for a tensor's sibling (`want`), the conv epilogues / fix-up passes that write the tensor also write the sibling,
// under the scale the consumer side left for them at the end of the previous iteration (sc[1 + parity]); the consumer side
// validates that scale against this iteration's absmax and re-splits the view from the fp32 tensor if it does not fit
// (pair_split_multi_kernel) -- always correct, and free of split passes whenever the tensor's magnitude moves by less than
// the margin between two iterations.
struct PairBuf {
  unsigned char* p = nullptr;
  float* sc = nullptr;             // [0] the scale the sibling holds now (consumers), [1], [2]: for the producers of even / odd iterations
  int64_t floats = 0;
  bool want = false;
  bool fresh = true;               // no producer scale yet (new sibling / pair_reset): this iteration's consumers run the
                                   // register-staged kernels, which leave the scale for the next iteration's producers
  bool covered = false;            // every writer of the tensor in iteration cover_iter wrote the sibling too
  long cover_iter = -1;
};

// One activation (phase 0: written by a forward) or gradient (phase 1: written by a backward) buffer, NHWC with C the pitch
// of every pixel, for up to the engine's largest batch.
struct Tensor {
  float* p = nullptr;
  int H = 0, W = 0, C = 0;
  int phase = 0;
  // ReLU mask as bytes (ConvArgs::mask8), one per 4 floats: written by the forward pass that applies the ReLU (conv epilogue,
  // fix-up, Winograd output transform, GroupNorm apply pass, pooling broadcast); the only form of the mask the backward reads
  uint8_t* mask = nullptr;
  bool mask_frozen = false;        // only a frozen conv's data gradient would read the mask: the forward does not write it
  // absmax slot: accumulated by the kernels that WRITE the tensor.  `valid`: the last writer that covered the whole tensor,
  // and every writer since, had the fused absmax -- only then a consumer trusts it
  int slot = -1;                   // index among the phase's slots, given on first use (TensorSet::slot_of)
  bool valid = false;
  PairBuf pair;
  int64_t floats(int B) const { return (int64_t)B * H * W * C; }
};

// Channels [c0, c0 + C) of a tensor (both multiples of 4); a default View is "no operand".  The one place that derives a
// slice's pointers from its tensor's.
struct View {
  Tensor* t = nullptr;
  int c0 = 0, C = 0;
  View(Tensor* t = nullptr) : t(t), C(t ? t->C : 0) {}        // the whole tensor
  View(Tensor* t, int c0, int C) : t(t), c0(c0), C(C) {}
  float* ptr() const { return t ? t->p + c0 : nullptr; }
  int ld() const { return t ? t->C : 0; }
  bool whole() const { return C == t->C; }                     // (then c0 = 0: a view lies inside its tensor)
  uint8_t* mask() const { return t->mask ? t->mask + c0 / 4 : nullptr; }
  uint8_t* mask_to_write() const { return t->mask_frozen ? nullptr : mask(); }
  int ldmask() const { return t->C / 4; }
  unsigned char* sibling() const { return t->pair.p + (int64_t)c0 * 4; }
};

// The tensors of one engine.  A record never moves (std::deque): PairBuf pointers are kept across calls and the grouped
// launches' device tables hold sibling addresses.
struct TensorSet {
  std::deque<Tensor> all;
  int nslot[2] = {0, 0};
  Tensor* add(float* p, int H, int W, int C, int phase) {
    all.push_back(Tensor{p, H, W, C, phase});
    return &all.back();
  }
  // the tensor's absmax slot index, given in first-use order; -1 when the phase's table is full
  int slot_of(Tensor& t) {
    if (t.slot < 0 && nslot[t.phase] < TSLOTS) t.slot = nslot[t.phase]++;
    return t.slot;
  }
  // a new forward (phase 0) / backward (phase 1): no slot of the phase can be trusted until its tensor is written again
  void new_phase(int phase) {
    for (Tensor& t : all)
      if (t.phase == phase) t.valid = false;
  }
};
