// kernel_choice.hip -- which kernel the host library launches, for every input its choice reads.  No GPU needed: the program
// includes mcbrat_api.hip textually, fills in a context, a parameter block and a LaunchPlan by hand, calls choose_trace /
// choose_block and names the returned host stub with dladdr (built with -rdynamic) and the demangler.  Driver: kernel_choice.py;
// output: tests/golden/kernel_choice.txt, which tests/test_kernel_variants_host.py holds the picker of mcbrat_variants.h to.
//
// The inputs are packed into one integer code per line (bit layouts: run_trace / run_block below; the dump program of the
// test, tests/kernel_variants_dump.cpp, decodes the same bits).
//
// PRUNING 1 -- combinations that plan_launch, check_ready or the refusals of launch_trace make unreachable are left out:
//   a. plan_launch: gridLds implies priv; bricks exclude priv and gridLds, intensity directions, scattering orders and the
//      face-walk tallies (levels, actinic); the wide plan has priv, 1024 lanes, no bricks, no flight, no directions, orders or
//      face-walk tallies and no blockSize option; every other plan has 256, 512 or 768 lanes (768 without gridLds: the blockSize
//      option), at most 512 with a face-walk tally; blockLite (optics 1, 2) is set in the wide plan only; flight excludes gridLds,
//      bricks, directions and the face-walk tallies and needs the layer-skipping walk, which the face-walk tallies switch off; the
//      collision records (rec) exist for dense grids of at most two components.
//   b. check_ready and launch_trace: levels with counters, a BRDF surface, directions or orders; direct without levels or with the
//      thermal source; actinic with counters, BRDF, directions, orders, the thermal source or direct; side without levels or with
//      the thermal source, direct or actinic; a BRDF surface with counters or the thermal source (and it is a surface description).
//      Counters with directions and counters with orders ARE kept: choose_trace is where they are refused (an `!` result).
//   c. set_grid: an axis the reference's test calls regular is equally spaced to 1e-6 of a cell.
// PRUNING 2 -- inputs that the ladder reads on some paths only are enumerated in full there and held at two settings elsewhere
// (all off, and the set that would pick a walk-specialised kernel), so that the file stays small:
//   a. trace: rec, layerSkip, fly, the surface description, the two regular-walk flags, useRR, nc and solarKind are read for
//      256 lanes, not instrumented, no tally flag, no directions, tallies in global memory, dense grid: full product there.
//      The plan's LDS (three values) and rayDefer are read on radiance runs: full product there, one value elsewhere.
//   b. block walk: blockSpansX/Y and blockSpanKernel are read for the 768-lane, not instrumented kernel of the shared plan: full
//      product there, the defaults elsewhere.
// solarKind takes 0 and 1 (the ladder asks whether it is 0); nc takes 1, 2, 3 (the ladder tells 1, 2 and more; rec needs <= 2).
#include <cxxabi.h>
#include <dlfcn.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "mcbrat_api.hip"  // (the driver puts mcbrat3d_amd/csrc on the include path)

namespace {

std::string kernel_name(const void *k) {
  Dl_info info;
  if (!k || !dladdr(k, &info) || !info.dli_sname) return "?";
  int st = 0;
  char *d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &st);
  std::string s = (st == 0 && d) ? d : info.dli_sname;
  free(d);
  return s;
}

// kernels ("K"), named once, without the `void mcbrat::` and `(mcbrat::DevParams)` every one of them carries, and results ("R":
// kernel, block, dynamic LDS, or a refusal), both in order of first use
std::vector<std::string> kernels, results;
std::map<std::string, int> kernelIndex, resultIndex;
std::vector<std::string> lines;
int intern(std::vector<std::string> &list, std::map<std::string, int> &index, const std::string &s) {
  auto it = index.find(s);
  if (it == index.end()) { it = index.emplace(s, (int)list.size()).first; list.push_back(s); }
  return it->second;
}
std::string strip(std::string s, const std::string &what) {
  const size_t at = s.find(what);
  return at == std::string::npos ? s : s.erase(at, what.size());
}
void record(char kind, uint32_t code, mcbrat_ctx &c, const KernelChoice &k) {
  char buf[64];
  std::string r;
  if (k.kernel) {
    snprintf(buf, sizeof(buf), "%d %d %zu", intern(kernels, kernelIndex, strip(strip(kernel_name(k.kernel), "void mcbrat::"), "(mcbrat::DevParams)")), k.block, k.lds);
    r = buf;
  } else r = "!" + c.err;
  snprintf(buf, sizeof(buf), "%c %x %d", kind, code, intern(results, resultIndex, r));
  lines.push_back(buf);
}

inline bool bit(uint32_t v, int b) { return (v >> b) & 1u; }
constexpr size_t kLdsValues[3] = {4096, 20000, 60000};
constexpr int kBlocks[4] = {256, 512, 768, 1024};

// trace code: bit 0 wide, 1 tblLds, 2 priv, 3 gridLds, 4 brick, 5-6 block (256, 512, 768, 1024), 7 debug, 8 thermal source, 9 directions,
// 10 orders, 11 levels, 12 direct, 13 actinic, 14 side, 15 BRDF, 16 rec, 17 layerSkip, 18 fly, 19 surface description, 20 xyRegularWalk,
// 21 zRegularWalk, 22 useRR, 23-24 nc - 1, 25 solarKind, 26-27 the plan's LDS (4096, 20000, 60000), 28 rayDefer off
void run_trace(uint32_t code) {
  mcbrat_ctx c;
  DevParams p;
  std::memset(&p, 0, sizeof(p));
  LaunchPlan L{};
  L.wide = bit(code, 0); L.tblLds = bit(code, 1); L.priv = bit(code, 2); L.gridLds = bit(code, 3); L.brick = bit(code, 4);
  L.block = kBlocks[(code >> 5) & 3];
  L.lds = kLdsValues[(code >> 26) & 3];
  const bool debug = bit(code, 7);
  c.srcKind = p.srcKind = bit(code, 8);
  c.nDir = p.nDir = bit(code, 9) ? 2 : 0;
  c.numRecScatOrd = p.numRecScatOrd = bit(code, 10) ? 1 : -1;
  c.levelFluxes = bit(code, 11); c.directLevelFluxes = bit(code, 12); c.actinicFlux = bit(code, 13); c.sideFluxes = bit(code, 14);
  c.surfNumX = c.surfNumY = p.surfNumX = p.surfNumY = bit(code, 19) ? 2 : 0;
  c.surfKind = p.surfKind = bit(code, 15) ? 1 : 0;
  static const uint4 someRec{};
  p.rec = bit(code, 16) ? &someRec : nullptr;
  p.layerSkip = bit(code, 17); p.fly = bit(code, 18);
  p.xyRegularWalk = bit(code, 20); p.zRegularWalk = bit(code, 21);
  c.useRR = p.useRR = bit(code, 22);
  c.nc = p.nc = 1 + (int)((code >> 23) & 3);
  c.solarKind = p.solarKind = bit(code, 25);
  c.rayDefer = bit(code, 28) ? 0 : 1;
  c.nx = c.ny = c.nz = 2;
  record('T', code, c, choose_trace(&c, p, L, debug));
}

// block-walk code: bit 0 wide, 1 tblLds, 2-3 optics (not 0: blockLite), 4 debug, 5 thermal source, 6-7 blockSize (0, 256, 512, 768),
// 8 xyRegular, 9 zRegular, 10 more than one component, 11 surface description, 12 ny == 1, 13 xyNearUniform, 14 zNearUniform, 15 noSimple3,
// 16 no block spans x, 17 no block spans y, 18 blockSpanKernel
void run_block(uint32_t code) {
  mcbrat_ctx c;
  DevParams p;
  std::memset(&p, 0, sizeof(p));
  LaunchPlan L{};
  L.wide = bit(code, 0); L.tblLds = bit(code, 1);
  L.optics = (int)((code >> 2) & 3); L.blockLite = L.optics != 0;
  L.priv = true; L.gridLds = !L.blockLite;
  const bool debug = bit(code, 4);
  c.srcKind = p.srcKind = bit(code, 5);
  static const int sizes[4] = {0, 256, 512, 768};
  c.blockSize = sizes[(code >> 6) & 3];
  c.xyRegular = p.xyRegular = bit(code, 8); c.zRegular = p.zRegular = bit(code, 9);
  c.nc = p.nc = bit(code, 10) ? 2 : 1;
  c.surfNumX = c.surfNumY = p.surfNumX = p.surfNumY = bit(code, 11) ? 2 : 0;
  c.nx = c.nz = 2; c.ny = bit(code, 12) ? 1 : 2;
  p.xyNearUniform = bit(code, 13); p.zNearUniform = bit(code, 14);
  c.noSimple3 = bit(code, 15);
  c.blockSpansX = !bit(code, 16); c.blockSpansY = !bit(code, 17); c.blockSpanKernel = bit(code, 18);
  record('B', code, c, choose_block(&c, p, L, debug));
}

void enumerate_trace() {
  for (uint32_t plan = 0; plan < 128; ++plan) {  // bits 0-6
    const bool wide = bit(plan, 0), priv = bit(plan, 2), gridLds = bit(plan, 3), brick = bit(plan, 4);
    const int block = kBlocks[(plan >> 5) & 3];
    if (gridLds && !priv) continue;
    if (brick && (priv || wide)) continue;
    if (wide != (block == 1024) || (wide && !priv)) continue;
    for (uint32_t s = 0; s < 512; ++s) {  // bits 7-15
      const uint32_t set = s << 7;
      const bool debug = bit(set, 7), emit = bit(set, 8), inten = bit(set, 9), orders = bit(set, 10), levels = bit(set, 11),
                 direct = bit(set, 12), act = bit(set, 13), side = bit(set, 14), brdf = bit(set, 15);
      const bool facewalk = levels || act;
      if (levels && (debug || brdf || inten || orders)) continue;
      if (direct && (!levels || emit)) continue;
      if (act && (debug || brdf || inten || orders || emit || direct)) continue;
      if (side && (!levels || emit || direct || act)) continue;
      if (brdf && (debug || emit)) continue;
      if (brick && (inten || orders || facewalk)) continue;
      if (wide && (inten || orders || facewalk)) continue;
      if (facewalk && block > 512) continue;
      // the walk inputs: in full where the ladder reads them, else all off and the walk-specialised set
      const bool walkRead = block == 256 && !debug && !inten && !orders && !facewalk && !brdf && !priv && !brick;
      std::vector<uint32_t> walks;
      if (walkRead) {
        for (uint32_t w = 0; w < 1024; ++w) {  // bits 16-25
          const uint32_t ws = w << 16;
          const int nc = 1 + (int)((ws >> 23) & 3);
          if (nc > 3) continue;
          if (bit(ws, 16) && nc > 2) continue;                       // rec: at most two components
          if (bit(ws, 18) && !bit(ws, 17)) continue;                 // flight needs the layer-skipping walk
          if (bit(ws, 25) && emit) continue;                         // solarKind: solar sources
          walks.push_back(ws);
        }
      } else {
        walks.push_back(brdf ? 1u << 19 : 0u);
        const bool canFly = !gridLds && !brick && !inten && !facewalk && !wide;
        walks.push_back((brick ? 0u : 1u << 16) | (facewalk ? 0u : 1u << 17) | (canFly ? 1u << 18 : 0u) | (brdf ? 1u << 19 : 0u) | 1u << 20 | 1u << 21 | 1u << 22);
      }
      for (uint32_t ws : walks) {
        if (brdf && !bit(ws, 19)) continue;
        if (inten) {
          for (uint32_t l = 0; l < 3; ++l)
            for (uint32_t d = 0; d < 2; ++d) run_trace(plan | set | ws | l << 26 | d << 28);
        } else run_trace(plan | set | ws);
      }
    }
  }
}

void enumerate_block() {
  for (uint32_t code = 0; code < (1u << 16); ++code) {
    const bool wide = bit(code, 0), debug = bit(code, 4);
    const int optics = (int)((code >> 2) & 3), size = (int)((code >> 6) & 3);
    if (optics == 3 || (!wide && optics != 0) || (wide && size != 0)) continue;
    if ((bit(code, 8) && !bit(code, 13)) || (bit(code, 9) && !bit(code, 14))) continue;  // regular implies near-uniform
    const bool spansRead = !wide && !debug && (size == 0 || size == 3);
    for (uint32_t sp = 0; sp < (spansRead ? 8u : 1u); ++sp) run_block(code | sp << 16);
  }
}

}  // namespace

int main() {
  enumerate_trace();
  enumerate_block();
  // (the driver groups these lines by kernel: kernel_choice.py)
  for (size_t i = 0; i < kernels.size(); ++i) printf("K %zu %s\n", i, kernels[i].c_str());
  for (size_t i = 0; i < results.size(); ++i) printf("R %zu %s\n", i, results[i].c_str());
  for (const std::string &l : lines) puts(l.c_str());
  return 0;
}
