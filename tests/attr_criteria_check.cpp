// Host-side check of csrc/dmf_attr_criteria.h: the three criteria, compiled with the host compiler, printed for the
// cases given on the command line so that tests/test_attr_multi_host.py can compare them with Python's unbounded integers.
//   attr_criteria_check "area SIZE TAU" "diag XMIN XMAX YMIN YMAX TAU" "std SIZE SUM_Q SUM_Q2 TAU" ...
// One line of output per argument: 0 or 1.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../dual-modal-fusion_amd/csrc/dmf_attr_criteria.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    char kind[8] = {0};
    uint64_t v[5] = {0, 0, 0, 0, 0};
    const int got = std::sscanf(argv[i], "%7s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, kind, &v[0], &v[1], &v[2], &v[3], &v[4]);
    bool ok;
    if (!std::strcmp(kind, "area") && got == 3) {
      ok = dmf::attr_crit_area((uint32_t)v[0], (uint32_t)v[1]);
    } else if (!std::strcmp(kind, "diag") && got == 6) {
      ok = dmf::attr_crit_diagonal((int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3], (uint32_t)v[4]);
    } else if (!std::strcmp(kind, "std") && got == 5) {
      ok = dmf::attr_crit_std((uint32_t)v[0], v[1], v[2], (uint32_t)v[3]);
    } else {
      std::fprintf(stderr, "attr_criteria_check: cannot read '%s'\n", argv[i]);
      return 2;
    }
    std::printf("%d\n", ok ? 1 : 0);
  }
  return 0;
}
