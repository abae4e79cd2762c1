// Prints the tally layout (mcbrat3d_amd/csrc/mcbrat_layout.h) of the shapes given on the command line, one line per shape:
//   tally_layout_dump BUDGET_BYTES nx,ny,nz,nc,nDir,limitContrib,nOrd,levels,direct,actinic ...
// or, with the word `parts`, the workgroups of every part of the finish kernels (finish_parts) in a launch round of NB batches:
//   tally_layout_dump parts NB nx,ny,nz,nc,nDir,limitContrib,nOrd,levels,direct,actinic,side ...
// or, with the word `starts`, the slab starts as trace_kernel takes them from the slab_*_start functions: in plain 64-bit integers,
// from ncol, nz, nDir and numRecScatOrd + 1 alone, the flags LVL = levels, DIRECT = direct, ACT = actinic deciding as its template flags do:
//   tally_layout_dump starts nx,ny,nz,nc,nDir,limitContrib,nOrd,levels,direct,actinic ...
// Built and read by tests/test_tally_layout_host.py, once plainly and once with the sanitizers for the shapes that would overflow.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../mcbrat3d_amd/csrc/mcbrat_layout.h"

int main(int argc, char **argv) {
  using namespace mcbrat;
  if (argc < 3) return 2;
  const bool parts = strcmp(argv[1], "parts") == 0, starts = strcmp(argv[1], "starts") == 0;
  if (parts && argc < 4) return 2;
  const uint64_t budget = (parts || starts) ? 0 : strtoull(argv[1], nullptr, 10);
  const int nb = parts ? atoi(argv[2]) : 0;
  for (int a = parts ? 3 : 2; a < argc; ++a) {
    int32_t v[11] = {};
    if (sscanf(argv[a], "%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32 ",%" SCNd32,
               &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9], &v[10]) != (parts ? 11 : 10)) return 2;
    TallyShape s{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]};
    s.side = v[10];
    if (starts) {
      const int64_t ncol = (int64_t)s.nx * s.ny, nz = s.nz, nDir = s.nDir, nOrd = s.nOrd;
#define START(name, value) printf(#name "=%" PRId64 " ", (int64_t)(value))
      START(ordUp, slab_orders_start<int64_t>(ncol, nz, nDir, nOrd, 0)); START(ordDown, slab_orders_start<int64_t>(ncol, nz, nDir, nOrd, 1));
      START(ordI, slab_orders_start<int64_t>(ncol, nz, nDir, nOrd, 2));
      START(lvlUp, slab_levels_start<int64_t>(ncol, nz, 0, 0, 0)); START(lvlDown, slab_levels_start<int64_t>(ncol, nz, 1, 0, 0));
      START(lvlDirect, slab_levels_start<int64_t>(ncol, nz, 2, 0, 0));
      START(actBins, slab_actinic_start<int64_t>(ncol, nz, s.levels ? 2 : 0, 0, 0));
      START(sideBins, slab_side_start<int64_t>(ncol, nz, 2, 0, 0, 0));
      START(ibase, slab_intensity_start<int64_t>(ncol, nz));
#undef START
      printf("\n");
      continue;
    }
    if (parts) {
      const FinishParts p = finish_parts(s, nb);
#define GATHER(name) printf("gather" #name "=%" PRIu32 " ", p.gather(kGather##name))
#define FOLD(name) printf("fold" #name "=%" PRIu32 " ", p.fold(kFold##name))
      GATHER(Columns); GATHER(Volume); GATHER(Reduce); GATHER(Intensity); GATHER(Orders); GATHER(OrderMeans); GATHER(Levels);
      GATHER(LevelMeans); GATHER(Actinic); GATHER(ActinicMeans); GATHER(Side); GATHER(SideMeans);
      FOLD(Columns); FOLD(Scalars); FOLD(OrderMeans); FOLD(LevelMeans); FOLD(ActinicMeans); FOLD(SideMeans);
#undef GATHER
#undef FOLD
      // (in order, as the kernels walk them: the position of every part in the list)
      printf("gatherParts=%d foldParts=%d gatherGrid=%" PRIu32 " foldGrid=%" PRIu32 "\n", (int)kGatherParts, (int)kFoldParts, p.gatherGrid(), p.foldGrid());
      continue;
    }
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
