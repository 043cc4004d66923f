// Prints what csrc/tensor_views.h computes, for tests/test_tensor_views_host.py: the pointers a channel-slice view derives
// from its tensor (as offsets from the tensor's own buffers) and the absmax-slot bookkeeping of a TensorSet.  Host only.
#include <cstdio>
#include <vector>

#include "../../e-osvos_amd/csrc/tensor_views.h"

// view <tensor C> <c0> <C>: data offset (floats) and pitch, mask offset (bytes) and pitch, sibling offset (bytes), whole
static void print_view(TensorSet& ts, int C, int c0, int n) {
  std::vector<float> data(C);
  std::vector<uint8_t> mask(C / 4);
  std::vector<unsigned char> pair(4 * (size_t)C);
  Tensor* t = ts.add(data.data(), 3, 5, C, 0);
  const View bare(t, c0, n);
  printf("view %d %d %d nomask %d\n", C, c0, n, (int)(bare.mask() == nullptr && bare.mask_to_write() == nullptr));
  t->mask = mask.data();
  t->pair.p = pair.data();
  const View v(t, c0, n);
  printf("view %d %d %d data %ld ld %d mask %ld ldmask %d sibling %ld whole %d\n", C, c0, n, (long)(v.ptr() - t->p), v.ld(),
         (long)(v.mask() - t->mask), v.ldmask(), (long)(v.sibling() - t->pair.p), (int)v.whole());
  printf("view %d %d %d towrite %ld", C, c0, n, (long)(v.mask_to_write() - t->mask));
  t->mask_frozen = true;
  printf(" frozen_towrite_null %d frozen_read %ld\n", (int)(v.mask_to_write() == nullptr), (long)(v.mask() - t->mask));
  if (c0 == 0 && n == C) {
    const View w(t);
    printf("whole_ctor %d %d %d %d\n", C, w.c0, w.C, (int)w.whole());
  }
}

int main() {
  TensorSet views;
  for (int c0 : {0, 256}) print_view(views, 304, c0, c0 ? 48 : 256);
  print_view(views, 304, 0, 304);
  for (int i = 0; i < 4; ++i) print_view(views, 1280, 256 * i, 256);
  print_view(views, 1280, 1024, 256);
  print_view(views, 1280, 0, 1280);
  const View none;
  printf("none %d %d\n", (int)(none.ptr() == nullptr), none.ld());

  // slots: 400 tensors per phase, created alternately; used in an order of their own
  TensorSet ts;
  const int N = 400;
  std::vector<Tensor*> t[2];
  for (int i = 0; i < N; ++i)
    for (int ph = 0; ph < 2; ++ph) t[ph].push_back(ts.add(nullptr, 1, 1, 4, ph));
  const Tensor* first = t[0][0];
  for (int k = 0; k < N; ++k) {                       // phase 0 in descending order of creation, phase 1 every 7th (mod N)
    const int a = N - 1 - k, b = (7 * k) % N;
    printf("use 0 %d %d\n", a, ts.slot_of(*t[0][a]));
    printf("use 1 %d %d\n", b, ts.slot_of(*t[1][b]));
  }
  for (int ph = 0; ph < 2; ++ph)
    for (int i = 0; i < N; ++i) printf("again %d %d %d\n", ph, i, ts.slot_of(*t[ph][i]));
  for (int ph = 0; ph < 2; ++ph)
    for (int i = 0; i < N; ++i) t[ph][i]->valid = t[ph][i]->slot >= 0;
  ts.new_phase(0);
  for (int ph = 0; ph < 2; ++ph)
    for (int i = 0; i < N; ++i) printf("newphase0 %d %d %d %d\n", ph, i, t[ph][i]->slot, (int)t[ph][i]->valid);
  ts.new_phase(1);
  for (int i = 0; i < N; ++i) printf("newphase1 1 %d %d %d\n", i, t[1][i]->slot, (int)t[1][i]->valid);
  for (int i = 0; i < 5000; ++i) ts.add(nullptr, 1, 1, 4, 0);
  printf("stable %d\n", (int)(first == &ts.all.front() && t[1][N - 1] == &ts.all[2 * N - 1]));
  return 0;
}
