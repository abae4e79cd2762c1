// Prints what the host rules of a backward render (mcbrat3d_amd/csrc/mcbrat_backward.h) give for the questions on its standard
// input, one per line, one line of answer each:
//   sun nx ny nz H Lx Ly sx sy sz        -> maxCross invFourPiMu0          (the sun as floats)
//   leg nx ny nz H Lx Ly                 -> maxCross
//   scale samples candidate...           -> scale pathMax
//   bins n numBatches arrays             -> 0 | 1
//   paths nBins samples firstSample numBatches -> 0 | 1
//   shape total numCUs block             -> pathsPerLane blocks
//   stats m0 m1 ...                      -> mean error                     (one series of batch means)
//   sum f0 f1 ... | d0 d1 ...            -> error                          (the per-batch sum of two series, as the sensors form it)
//   reduce arrays numBatches n slots unit[n] bins[arrays][numBatches][n][slots]
//                                        -> mean[2][slots][n] error[2][slots][n] totalError[slots][n] batchMeans[numBatches][arrays][slots][n]
//                                           (reduce_batches with every output; -1: not written)
// A stand-alone host program (plain C++, no HIP): tests/test_backward_host.py builds it with the address and undefined-behaviour
// sanitizers and holds the lines to closed forms written out in numpy.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../mcbrat3d_amd/csrc/mcbrat_backward.h"

int main() {
  char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    std::vector<std::string> w;
    for (char *t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) w.push_back(t);
    if (w.empty()) continue;
    const size_t n = w.size() - 1;
    auto d = [&](size_t i) { return strtod(w.at(i).c_str(), nullptr); };
    auto u = [&](size_t i) { return strtoull(w.at(i).c_str(), nullptr, 10); };
    if (w[0] == "sun" && n == 9) {
      const float sun[3] = {(float)d(7), (float)d(8), (float)d(9)};
      const mcbrat::SunBound b = mcbrat::sun_bound((int)u(1), (int)u(2), (int)u(3), d(4), d(5), d(6), sun);
      printf("%u %.9g\n", b.maxCross, (double)b.invFourPiMu0);
    } else if (w[0] == "leg" && n == 6) {
      printf("%u\n", mcbrat::leg_bound((int)u(1), (int)u(2), (int)u(3), d(4), d(5), d(6)));
    } else if (w[0] == "scale" && n >= 2 && n <= 4) {
      const double c[3] = {d(2), n >= 3 ? d(3) : 0.0, n >= 4 ? d(4) : 0.0};
      const mcbrat::FixedPoint f = mcbrat::fixed_point((long long)u(1), {c[0], c[1], c[2]});
      printf("%.17g %.17g\n", f.scale, f.pathMax);
    } else if (w[0] == "bins" && n == 3) {
      printf("%d\n", (int)mcbrat::bins_fit(u(1), u(2), (int)u(3)));
    } else if (w[0] == "paths" && n == 4) {
      printf("%d\n", (int)mcbrat::paths_fit(u(1), (long long)u(2), u(3), (int)u(4)));
    } else if (w[0] == "shape" && n == 3) {
      const mcbrat::LaunchShape s = mcbrat::launch_shape(u(1), (int)u(2), (int)u(3));
      printf("%llu %llu\n", s.pathsPerLane, s.blocks);
    } else if (w[0] == "stats" && n >= 1) {
      mcbrat::BatchSeries s;
      for (size_t i = 1; i <= n; ++i) s.add(d(i) - d(1));
      printf("%.17g %.17g\n", d(1) + s.shift((int)n), s.error((int)n));
    } else if (w[0] == "sum" && n >= 3 && n % 2 == 1 && w[(n + 1) / 2] == "|") {
      const size_t nb = (n - 1) / 2, d0 = nb + 2;
      mcbrat::BatchSeries s;
      for (size_t b = 0; b < nb; ++b) s.add((d(1 + b) - d(1)) + (d(d0 + b) - d(d0)));
      printf("%.17g\n", s.error((int)nb));
    } else if (w[0] == "reduce" && n >= 4 && n == 4 + u(3) + u(1) * u(2) * u(3) * u(4)) {
      const int arrays = (int)u(1), numBatches = (int)u(2);
      const size_t nr = u(3), slots = u(4), values = nr * slots;
      std::vector<double> unit(nr);
      std::vector<long long> bins((size_t)arrays * numBatches * values);
      for (size_t i = 0; i < nr; ++i) unit[i] = d(5 + i);
      for (size_t i = 0; i < bins.size(); ++i) bins[i] = strtoll(w.at(5 + nr + i).c_str(), nullptr, 10);
      // every output is asked for, poisoned first: what the reduction does not write shows
      std::vector<float> mean(2 * values, -1.0f), error(2 * values, -1.0f), total(values, -1.0f), means(bins.size(), -1.0f);
      mcbrat::reduce_batches(bins.data(), arrays, numBatches, nr, slots, unit.data(),
                             {{mean.data(), arrays == 2 ? mean.data() + values : nullptr}, {error.data(), arrays == 2 ? error.data() + values : nullptr},
                              arrays == 2 ? total.data() : nullptr, means.data()});
      for (const std::vector<float> *v : {&mean, &error, &total, &means})
        for (float x : *v) printf("%.9g ", (double)x);
      printf("\n");
      // ... and none but the means: the same means, nothing else touched
      std::vector<float> alone(values, -1.0f);
      mcbrat::reduce_batches(bins.data(), arrays, numBatches, nr, slots, unit.data(), {{alone.data(), nullptr}, {nullptr, nullptr}, nullptr, nullptr});
      if (memcmp(alone.data(), mean.data(), sizeof(float) * values) != 0) return 3;
    } else {
      fprintf(stderr, "backward_dump: cannot read '%s ...'\n", w[0].c_str());
      return 2;
    }
  }
  return 0;
}
