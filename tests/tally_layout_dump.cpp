// Prints the tally layout (mcbrat3d_amd/csrc/mcbrat_layout.h) of the shapes given on the command line, one line per shape:
//   tally_layout_dump BUDGET_BYTES nx,ny,nz,nc,nDir,limitContrib,nOrd,levels,direct,actinic ...
// Built and read by tests/test_tally_layout_host.py, once plainly and once with the sanitizers for the shapes that would overflow.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../mcbrat3d_amd/csrc/mcbrat_layout.h"

int main(int argc, char **argv) {
  using namespace mcbrat;
  if (argc < 3) return 2;
  const uint64_t budget = strtoull(argv[1], nullptr, 10);
  for (int a = 2; a < argc; ++a) {
    int32_t v[10];
    if (sscanf(argv[a], "%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32,
               &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9]) != 10) return 2;
    const TallyShape s{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]};
    const TallyLayout l = tally_layout(s);
    const TallyFit fit = tally_fit(s, budget);
#define FIELD(name) printf(#name "=%" PRId64 " ", l.name)
    FIELD(slabFluxUp); FIELD(slabFluxDown); FIELD(slabVolume); FIELD(slabIntensity); FIELD(slabByComponent); FIELD(slabExcess);
    FIELD(slabOrders); FIELD(slabLevels); FIELD(slabActinic); FIELD(slabStride); FIELD(slabLds);
    FIELD(momMeans); FIELD(momColumns); FIELD(momProfile); FIELD(momVolume); FIELD(momIntensity); FIELD(momOrders); FIELD(momLevels);
    FIELD(momDirect); FIELD(momActinic); FIELD(momentsLen);
    FIELD(scalOrders); FIELD(scalLevels); FIELD(scalActinic); FIELD(scalPerBatch);
#undef FIELD
    printf("fluxRunStride=%" PRId64 " ", tally_layout(flux_run(s)).slabStride);
    printf("fitOrders=%d fitGlobalBins=%d fitStride=%d %s\n", (int)fit.orders, (int)fit.globalBins, (int)fit.stride, fit.stride ? "fits" : "does not fit");
  }
  return 0;
}
