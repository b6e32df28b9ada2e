// Stand-alone host program for tests/test_reduce_words_host.py: packs the reduce launch's two geometry words for the shapes
// given on the command line ("C C2 P S F G H K B" per argument) and prints what the kernel's side unpacks from them, next to
// the layouts they must reproduce.
#include <cstdio>
#include <cstdlib>

#include "../dual-modal-fusion_amd/csrc/dmf_shapes.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    int v[9];
    if (std::sscanf(argv[i], "%d %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8) != 9) return 2;
    const dmf::Layout L = dmf::make_layout(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
    const dmf::WsLayout w = dmf::make_ws(L, v[8]);
    int w3 = -1, w4 = -1;
    const bool ok = dmf::reduce_words_pack(L, v[8], &w3, &w4);
    const dmf::ReduceGeom g = dmf::reduce_words_unpack(w3, w4, v[8]);
    std::printf("%d %d %d %d %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld | %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", ok ? 1 : 0, w3, w4,
                g.H, g.F2, g.K, g.NCONV, (long long)g.oFc1w, (long long)g.oFc1b, (long long)g.oFc2w, (long long)g.oFc2b, (long long)g.z,
                (long long)g.h, (long long)g.dh, (long long)g.dl, (long long)L.off[8], (long long)L.off[9], (long long)L.off[10],
                (long long)L.off[11], (long long)w.slab, (long long)w.z, (long long)w.h, (long long)w.dh, (long long)w.dl);
  }
  return 0;
}
