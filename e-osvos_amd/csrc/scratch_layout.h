// Where every evaluation-stage entry point keeps its regions inside the engine's one scratch arena (engine.cpp: scratch_for).
// Host-only C++17, no HIP: tests/host/scratch_layout_main.cpp prints these layouts and tests/test_scratch_layout_host.py
// checks them (bounds, overlap, alignment, the cleared range, the sizes the Python modules chunk by).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

struct ScratchRegion { const char* name; size_t at, bytes, elem; };
template <class T> struct ScratchAt { size_t at; };              // the byte offset of a region of T
typedef unsigned long long scratch_u64;                          // the kernels' 64-bit counters

// A bump layout: take<T>(name, count) aligns to alignof(T) and returns the region's typed byte offset; need() is the arena
// size of the call, a multiple of four bytes.  A stage's regions are its members, taken in the order they are declared; the
// arena clears [clear_at, clear_at + clear_bytes) before the stage's first launch.
struct ScratchLayout {
  ScratchRegion region[10];
  int regions = 0;
  size_t end = 0, clear_at = 0, clear_bytes = 0;
  template <class T> ScratchAt<T> take(const char* name, size_t count) {
    const size_t at = (end + alignof(T) - 1) / alignof(T) * alignof(T);
    region[regions++] = {name, at, count * sizeof(T), sizeof(T)};
    end = at + count * sizeof(T);
    return {at};
  }
  void clear(size_t from, size_t to) { clear_at = from; clear_bytes = to - from; }
  size_t need() const { return (end + 3) / 4 * 4; }
};
inline size_t slic_clusters(int h, int w, int step) { return (size_t)((h + step - 1) / step) * ((w + step - 1) / step); }

// n = frames, np = pixels and nk = SLIC clusters of the call, nl = n_obj + 1
struct LabelComponentsLayout : ScratchLayout {
  ScratchAt<int> parent, tarea;
  explicit LabelComponentsLayout(size_t np) : parent(take<int>("parent", np)), tarea(take<int>("tarea", np)) {}
};
struct FilterComponentsLayout : ScratchLayout {
  size_t n, np;
  ScratchAt<int> parent = take<int>("parent", np), tarea = take<int>("tarea", np), ids = take<int>("ids", np), area = take<int>("area", np);
  ScratchAt<scratch_u64> best = take<scratch_u64>("best", n * 256), removed = take<scratch_u64>("removed", n);
  ScratchAt<uint8_t> cand = take<uint8_t>("cand", np), pres = take<uint8_t>("pres", (n + 1) * 256);  // a `pres` row for `prev` too
  FilterComponentsLayout(size_t n, size_t np) : n(n), np(np) { clear(area.at, end); }
};
struct FillHolesLayout : ScratchLayout {
  size_t n, np;
  ScratchAt<int> parent = take<int>("parent", np), tarea = take<int>("tarea", np), ids = take<int>("ids", np), area = take<int>("area", np);
  ScratchAt<unsigned> rec = take<unsigned>("rec", np), cnt = take<unsigned>("cnt", np), hist = take<unsigned>("hist", n * 256);
  ScratchAt<scratch_u64> filled = take<scratch_u64>("filled", n);
  ScratchAt<uint8_t> pres = take<uint8_t>("pres", (n + 1) * 256);
  FillHolesLayout(size_t n, size_t np) : n(n), np(np) { clear(area.at, end); }
};
struct SuperpixelsLayout : ScratchLayout {
  size_t nk;
  ScratchAt<int> centres = take<int>("centres", 5 * nk);
  ScratchAt<unsigned> sums = take<unsigned>("sums", 6 * nk);
  explicit SuperpixelsLayout(size_t nk) : nk(nk) { clear(sums.at, end); }
};
struct SnapLabelsLayout : ScratchLayout {
  size_t n, np, nk, nl;
  ScratchAt<int> ids = take<int>("ids", np), centres = take<int>("centres", 5 * nk);
  ScratchAt<unsigned> sums = take<unsigned>("sums", 6 * nk), votes = take<unsigned>("votes", nl * nk);
  ScratchAt<scratch_u64> changed = take<scratch_u64>("changed", n);
  SnapLabelsLayout(size_t n, size_t np, size_t nk, size_t nl) : n(n), np(np), nk(nk), nl(nl) { clear(sums.at, end); }
};
struct BlockMotionLayout : ScratchLayout {                     // n + 1 luma planes, each row padded to whole 32-bit words
  ScratchAt<unsigned> luma;
  BlockMotionLayout(size_t n, int height, int width) : luma(take<unsigned>("luma", (n + 1) * height * (((size_t)width + 3) / 4))) {}
};
struct CrfLabelsLayout : ScratchLayout {                       // plane = n * nl * pixels of a frame
  size_t plane;
  ScratchAt<float> unary = take<float>("unary", plane), q[2] = {take<float>("q0", plane), take<float>("q1", plane)};
  explicit CrfLabelsLayout(size_t plane) : plane(plane) {}
};
struct DistanceSqLayout : ScratchLayout {
  ScratchAt<uint16_t> g;
  explicit DistanceSqLayout(size_t np) : g(take<uint16_t>("g", np)) {}
};
struct AdaptTargetsLayout : ScratchLayout {                    // only the counters start out as 0
  size_t n, np;
  ScratchAt<int> count_e = take<int>("count_e", n), n_pos = take<int>("n_pos", n);
  ScratchAt<uint16_t> g = take<uint16_t>("g", np);
  ScratchAt<uint8_t> eroded;
  AdaptTargetsLayout(size_t n, size_t np, bool erode) : n(n), np(np), eroded(take<uint8_t>("eroded", erode ? np : 0)) { clear(0, g.at); }
};
// n = images, np = their pixels: the 32-bit words of the two vertical-distance planes, which the capped distances overwrite
// in place (first, so 16-byte aligned), then the partial sums, counts and per-image scales of the loss (partial_words per
// image: 2 * SURFACE_BLOCKS + 1 of kernels.h); nothing needs clearing
struct SurfaceLayout : ScratchLayout {
  ScratchAt<uint32_t> g;
  ScratchAt<float> partial;
  SurfaceLayout(size_t n, size_t np, size_t partial_words) : g(take<uint32_t>("g", np)), partial(take<float>("partial", n * partial_words)) {}
};
// words = potts_scratch_floats of kernels.h: the pairwise loss's two partials per tile and one scale per image; every word is
// written before it is read, so nothing needs clearing
struct PottsLayout : ScratchLayout {
  ScratchAt<float> partial;
  explicit PottsLayout(size_t words) : partial(take<float>("partial", words)) {}
};
// words = cldice_scratch_floats / cldice_skeleton_scratch_floats of kernels.h: the centreline loss's fp64 partials (first, so
// the region is taken as 8-byte words), planes, per-level increments and codes; every word is written before it is read
struct CldiceLayout : ScratchLayout {
  ScratchAt<double> words;
  explicit CldiceLayout(size_t floats) : words(take<double>("words", (floats + 1) / 2)) {}
};
struct LucidLayersLayout : ScratchLayout {                     // the visible-pixel counts [n][8 layers] start out as 0
  ScratchAt<int> counts;
  explicit LucidLayersLayout(size_t n) : counts(take<int>("counts", n * 8)) { clear(0, end); }
};
// the counts of all frames (they start out as 0), then the two bit-packed boundary maps (map_words per frame each) of one chunk
// of frames: as many frames as 64 MB hold, at least one
struct DavisCountsLayout : ScratchLayout {
  size_t n, n_obj, map_words, chunk = std::max<size_t>(1, std::min<size_t>({(size_t)(64 << 20) / (2 * map_words * 8), n, 65535}));
  ScratchAt<int64_t> counts = take<int64_t>("counts", n * n_obj * 6);
  ScratchAt<scratch_u64> pred_map = take<scratch_u64>("pred_map", chunk * map_words), gt_map = take<scratch_u64>("gt_map", chunk * map_words);
  DavisCountsLayout(size_t n, size_t n_obj, int height, int width)
      : n(n), n_obj(n_obj), map_words(n_obj * height * (((size_t)width + 63) / 64)) { clear(0, pred_map.at); }
};
