// Prints the scratch layouts of csrc/scratch_layout.h for tests/test_scratch_layout_host.py (built with ASan + UBSan).
// Every argument is one case, "stage,n,H,W,n_obj,step,erode"; per case one line per region
//   <case> region <name> <offset> <bytes> <element bytes>
// and one line  <case> need <bytes> clear <offset> <bytes>.
#include <cstdio>
#include <cstring>

#include "../../e-osvos_amd/csrc/scratch_layout.h"

static void dump(const char* arg, const ScratchLayout& L) {
  for (int i = 0; i < L.regions; ++i)
    printf("%s region %s %zu %zu %zu\n", arg, L.region[i].name, L.region[i].at, L.region[i].bytes, L.region[i].elem);
  printf("%s need %zu clear %zu %zu\n", arg, L.need(), L.clear_at, L.clear_bytes);
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    char stage[32];
    size_t n, n_obj;
    int H, W, step, erode;
    if (sscanf(argv[i], "%31[^,],%zu,%d,%d,%zu,%d,%d", stage, &n, &H, &W, &n_obj, &step, &erode) != 7 || n < 1 || H < 1 || W < 1 ||
        step < 1) {
      fprintf(stderr, "bad case: %s\n", argv[i]);
      return 2;
    }
    const size_t np = n * H * W, nk = n * slic_clusters(H, W, step);
    const auto is = [&](const char* s) { return strcmp(stage, s) == 0; };
    if (is("label_components")) dump(argv[i], LabelComponentsLayout(np));
    else if (is("filter_components")) dump(argv[i], FilterComponentsLayout(n, np));
    else if (is("fill_holes")) dump(argv[i], FillHolesLayout(n, np));
    else if (is("superpixels")) dump(argv[i], SuperpixelsLayout(nk));
    else if (is("snap_labels")) dump(argv[i], SnapLabelsLayout(n, np, nk, n_obj + 1));
    else if (is("block_motion")) dump(argv[i], BlockMotionLayout(n, H, W));
    else if (is("crf_labels")) dump(argv[i], CrfLabelsLayout(np * (n_obj + 1)));
    else if (is("distance_sq")) dump(argv[i], DistanceSqLayout(np));
    else if (is("adapt_targets")) dump(argv[i], AdaptTargetsLayout(n, np, erode != 0));
    else if (is("davis_counts")) dump(argv[i], DavisCountsLayout(n, n_obj, H, W));
    else {
      fprintf(stderr, "unknown stage: %s\n", stage);
      return 2;
    }
  }
  return 0;
}
