// Prints what the arithmetic of the expected-value estimator (mcbrat3d_amd/csrc/mcbrat_expected.h) gives for the questions on
// its standard input, one per line, one line of answer each:
//   seg tauIn dTau                          -> e^(-tauIn) (1 - e^(-dTau))       (both read as floats)
//   emis nc ext S cum[nc - 1] ssa[nc]       -> E[v]                             (floats; nan is read as a NaN)
//   emis2 nc ext S cum[nc - 1] ssa[nc]      -> E[v] of the middle cell of three: the arrays strided as the grids are
//   cut                                     -> the optical depth behind which a ray stops adding
//   lds nx ny nz                            -> the bytes of the second grid in LDS
// A stand-alone host program (plain C++, no HIP): tests/test_expected_host.py builds it with the address and undefined-behaviour
// sanitizers and holds the lines to closed forms written out in double.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../mcbrat3d_amd/csrc/mcbrat_expected.h"

int main() {
  char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    std::vector<std::string> w;
    for (char *t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) w.push_back(t);
    if (w.empty()) continue;
    const size_t n = w.size() - 1;
    auto f = [&](size_t i) { return strtof(w.at(i).c_str(), nullptr); };
    auto u = [&](size_t i) { return (int)strtol(w.at(i).c_str(), nullptr, 10); };
    if (w[0] == "seg" && n == 2) {
      printf("%.9g\n", (double)mcbrat::expected_segment(f(1), f(2)));
    } else if ((w[0] == "emis" || w[0] == "emis2") && n >= 4 && u(1) >= 1 && n == 3 + 2 * (size_t)u(1) - 1) {
      const int nc = u(1);
      const bool strided = w[0] == "emis2";
      const long long stride = strided ? 3 : 1;
      // (strided: the cell between two others whose values are poison -- a read beside the cell shows in the answer)
      std::vector<float> cum((size_t)(nc - 1) * stride + 1, -7.0f), ssa((size_t)nc * stride, -7.0f);
      for (int c = 0; c < nc - 1; ++c) cum[(size_t)(c * stride + (strided ? 1 : 0))] = f(4 + c);
      for (int c = 0; c < nc; ++c) ssa[(size_t)(c * stride + (strided ? 1 : 0))] = f(4 + nc - 1 + c);
      printf("%.9g\n", (double)mcbrat::expected_emission(nc, nc > 1 ? cum.data() + (strided ? 1 : 0) : nullptr, ssa.data() + (strided ? 1 : 0), stride, f(2), f(3)));
    } else if (w[0] == "cut" && n == 0) {
      printf("%.9g\n", (double)mcbrat::kExpectedTauCut);
    } else if (w[0] == "lds" && n == 3) {
      printf("%zu\n", mcbrat::expected_lds_bytes(u(1), u(2), u(3)));
    } else {
      fprintf(stderr, "expected_dump: cannot read '%s ...'\n", w[0].c_str());
      return 2;
    }
  }
  return 0;
}
