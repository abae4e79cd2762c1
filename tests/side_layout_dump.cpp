// Prints the tally layout (mcbrat3d_amd/csrc/mcbrat_layout.h) of the shapes given on the command line with the side part, one
// line per shape:
//   side_layout_dump BUDGET_BYTES nx,ny,nz,nc,nDir,limitContrib,nOrd,levels,direct,actinic,side ...
// Built and read by tests/test_side_flux_host.py, once plainly and once with the sanitizers for the shapes that would overflow.
// (tests/tally_layout_dump.cpp, which knows nothing of the side part, stays as the witness of every older field.)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../mcbrat3d_amd/csrc/mcbrat_layout.h"

int main(int argc, char **argv) {
  using namespace mcbrat;
  if (argc < 3) return 2;
  const uint64_t budget = strtoull(argv[1], nullptr, 10);
  for (int a = 2; a < argc; ++a) {
    int32_t v[11];
    if (sscanf(argv[a], "%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32,
               &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9], &v[10]) != 11) return 2;
    TallyShape s{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]};
    s.side = v[10];
    const TallyLayout l = tally_layout(s);
    const TallyFit fit = tally_fit(s, budget);
#define FIELD(name) printf(#name "=%" PRId64 " ", l.name)
    FIELD(slabFluxUp); FIELD(slabFluxDown); FIELD(slabVolume); FIELD(slabIntensity); FIELD(slabByComponent); FIELD(slabExcess);
    FIELD(slabOrders); FIELD(slabLevels); FIELD(slabActinic); FIELD(slabSide); FIELD(slabStride); FIELD(slabLds);
    FIELD(momMeans); FIELD(momColumns); FIELD(momProfile); FIELD(momVolume); FIELD(momIntensity); FIELD(momOrders); FIELD(momLevels);
    FIELD(momDirect); FIELD(momActinic); FIELD(momSide); FIELD(momentsLen);
    FIELD(scalOrders); FIELD(scalLevels); FIELD(scalActinic); FIELD(scalSide); FIELD(scalPerBatch);
#undef FIELD
    printf("fluxRunStride=%" PRId64 " ", tally_layout(flux_run(s)).slabStride);
    printf("fitOrders=%d fitGlobalBins=%d fitStride=%d %s\n", (int)fit.orders, (int)fit.globalBins, (int)fit.stride, fit.stride ? "fits" : "does not fit");
  }
  return 0;
}
