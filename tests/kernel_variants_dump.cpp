// kernel_variants_dump.cpp -- what mcbrat_variants.h lists and picks, printed for tests/test_kernel_variants_host.py.  Includes
// nothing of the library but that header (plain C++17: built with the host compiler, no HIP, no GPU).
//   kernel_variants_dump list          -> one line per built variant: "<trace|block> <valid> <kernel name>"
//   kernel_variants_dump pick < codes  -> for every line "T <hex>" / "B <hex>" of the input (the input codes of
//                                         scripts/kernel_choice.hip): "<T|B> <hex> <block> <lds> <kernel name>", or "<T|B> <hex> !<refusal>";
//                                         after the name: " invalid" / " unbuilt" where the picked variant is not valid / not in the list
//   kernel_variants_dump rules         -> the rule list in its order: "<stages, hex> <message>"
//   kernel_variants_dump refuse < asks -> for every line "<stage, hex> <settings, hex>": the message refusal() gives, or "-".  Settings bits, from
//                                         bit 0: inten, orders, limitContrib, levels, direct, actinic, side, brdf, debug, emit, fitOrders, fitLevels,
//                                         fitBins, fitStride
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../mcbrat3d_amd/csrc/mcbrat_variants.h"

using namespace mcbrat;

namespace {

const char *tf(bool b) { return b ? "true" : "false"; }
std::string name(const TraceVariant &v) {  // as the demangler prints the instantiation
  char buf[256];
  snprintf(buf, sizeof(buf), "trace_kernel<%d, %s, %d, %s, %s, %s, %s, %d, %s, %s, %s, %s, %s, %s>", v.block, tf(v.tblLds), v.priv, tf(v.brick), tf(v.debug),
           tf(v.inten), tf(v.emit), v.spec, tf(v.ord), tf(v.brdf), tf(v.lvl), tf(v.direct), tf(v.act), tf(v.side));
  return buf;
}
std::string name(const BlockVariant &v) {
  char buf[256];
  snprintf(buf, sizeof(buf), "trace_block_kernel<%d, %s, %s, %s, %d, %d, %s>", v.block, tf(v.tblLds), tf(v.debug), tf(v.emit), v.simple, v.opt, tf(v.nospan));
  return buf;
}

constexpr auto kTraceList = trace_variants();
constexpr auto kBlockList = block_variants();
static_assert(kTraceList.n == kTraceVariants && kBlockList.n == kBlockVariants, "the lists are as long as they say");

bool bit(uint32_t v, int b) { return (v >> b) & 1u; }

// the bit layouts of scripts/kernel_choice.hip
void pick_trace_line(uint32_t code) {
  static const int blocks[4] = {256, 512, 768, 1024};
  static const size_t ldsValues[4] = {4096, 20000, 60000, 0};
  LaunchPlan L{};
  L.wide = bit(code, 0); L.tblLds = bit(code, 1); L.priv = bit(code, 2); L.gridLds = bit(code, 3); L.brick = bit(code, 4);
  L.block = blocks[(code >> 5) & 3];
  L.lds = ldsValues[(code >> 26) & 3];
  Settings s{};  // (the tallies' flags as the picker's inputs have them: direct and side only with levels)
  s.debug = bit(code, 7); s.emit = bit(code, 8); s.inten = bit(code, 9); s.orders = bit(code, 10);
  s.levels = bit(code, 11); s.direct = s.levels && bit(code, 12); s.actinic = bit(code, 13); s.side = s.levels && bit(code, 14);
  s.brdf = bit(code, 15);
  TraceWalk w{};
  w.rec = bit(code, 16); w.layerSkip = bit(code, 17); w.fly = bit(code, 18); w.surface = bit(code, 19);
  w.xyRegularWalk = bit(code, 20); w.zRegularWalk = bit(code, 21); w.useRR = bit(code, 22);
  w.nc = 1 + (int)((code >> 23) & 3); w.solarKind = bit(code, 25);
  const bool rayDefer = !bit(code, 28);
  s.fitOrders = s.fitLevels = s.fitBins = s.fitStride = true;
  if (const char *why = refusal(s, Launch)) { printf("T %x !%s\n", code, why); return; }
  const TraceVariant v = pick_trace(L, s, w);
  size_t lds = L.lds;
  if (s.inten) lds = ray_lds(v.block, L.lds, ray_cap(v.block, L.priv, L.lds, 160 * 1024, rayDefer, true));  // (the context's default LDS per compute unit)
  printf("T %x %d %zu %s%s%s\n", code, v.block, lds, name(v).c_str(), valid(v) ? "" : " invalid", find_variant(kTraceList, v) >= 0 ? "" : " unbuilt");
}

void pick_block_line(uint32_t code) {
  static const int sizes[4] = {0, 256, 512, 768};
  LaunchPlan L{};
  L.wide = bit(code, 0); L.tblLds = bit(code, 1);
  L.optics = (int)((code >> 2) & 3); L.blockLite = L.optics != 0;
  L.priv = true; L.gridLds = !L.blockLite;
  BlockWalk w{};
  w.blockSize = sizes[(code >> 6) & 3];
  w.xyRegular = bit(code, 8); w.zRegular = bit(code, 9); w.oneComponent = !bit(code, 10); w.surface = bit(code, 11); w.xz = bit(code, 12);
  w.xyNearUniform = bit(code, 13); w.zNearUniform = bit(code, 14); w.noSimple3 = bit(code, 15);
  w.spansX = !bit(code, 16); w.spansY = !bit(code, 17); w.spanKernel = bit(code, 18);
  const BlockVariant v = pick_block(L, bit(code, 4), bit(code, 5), w);
  printf("B %x %d 0 %s%s%s\n", code, v.block, name(v).c_str(), valid(v) ? "" : " invalid", find_variant(kBlockList, v) >= 0 ? "" : " unbuilt");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "list")) {
    for (int i = 0; i < kTraceList.n; ++i) printf("trace %d %s\n", valid(kTraceList.v[i]) ? 1 : 0, name(kTraceList.v[i]).c_str());
    for (int i = 0; i < kBlockList.n; ++i) printf("block %d %s\n", valid(kBlockList.v[i]) ? 1 : 0, name(kBlockList.v[i]).c_str());
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "pick")) {
    char kind;
    unsigned code;
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
      if (sscanf(line, "%c %x", &kind, &code) != 2) continue;
      if (kind == 'T') pick_trace_line(code);
      else if (kind == 'B') pick_block_line(code);
    }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "rules")) {
    for (const Rule &r : kRules) printf("%x %s\n", r.stages, r.message);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "refuse")) {
    unsigned stage, b;
    while (scanf("%x %x", &stage, &b) == 2) {
      const Settings s{bit(b, 0), bit(b, 1), bit(b, 2), bit(b, 3), bit(b, 4), bit(b, 5), bit(b, 6), bit(b, 7), bit(b, 8), bit(b, 9), bit(b, 10), bit(b, 11), bit(b, 12), bit(b, 13)};
      const char *m = refusal(s, (Stage)stage);
      puts(m ? m : "-");
    }
    return 0;
  }
  fprintf(stderr, "usage: kernel_variants_dump list | rules | pick < codes | refuse < asks\n");
  return 2;
}
