// Prints what the rules of the path-length bins (mcbrat3d_amd/csrc/mcbrat_pathbins.h) give for the questions on its standard
// input, one per line, one line of answer each:
//   bin e0 e1 ... | L0 L1 ...            -> the bin of every L among the edges
//   edges n e0 e1 ...                    -> ok | the refusal's text        (n: the count handed over; "edges n null": no array)
// Numbers are read with strtod and rounded to float (the test writes floats).  A stand-alone host program (plain C++, no HIP):
// tests/test_pathbins_host.py builds it plain and with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../mcbrat3d_amd/csrc/mcbrat_pathbins.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::vector<std::string> w;
    for (std::string t; in >> t;) w.push_back(t);
    if (w.empty()) continue;
    auto f = [&](size_t i) { return (float)strtod(w.at(i).c_str(), nullptr); };
    size_t bar = 0;
    for (size_t i = 1; i < w.size(); ++i)
      if (w[i] == "|") bar = i;
    if (w[0] == "bin" && bar >= 2 && bar + 1 < w.size()) {
      std::vector<float> e;
      for (size_t i = 1; i < bar; ++i) e.push_back(f(i));
      for (size_t i = bar + 1; i < w.size(); ++i) printf("%s%d", i > bar + 1 ? " " : "", mcbrat::path_bin(e.data(), (int)e.size(), f(i)));
      printf("\n");
    } else if (w[0] == "edges" && w.size() >= 2) {
      const int n = atoi(w[1].c_str());
      std::vector<float> e;
      const bool null = w.size() == 3 && w[2] == "null";
      for (size_t i = 2; !null && i < w.size(); ++i) e.push_back(f(i));
      if (!null && n >= 1 && n <= mcbrat::kMaxPathBins && (size_t)n != e.size()) {
        fprintf(stderr, "pathbins_dump: %d edges announced, %zu given\n", n, e.size());
        return 2;
      }
      const char *msg = mcbrat::path_edges_refusal(null ? nullptr : e.data(), n);
      printf("%s\n", msg ? msg : "ok");
    } else {
      fprintf(stderr, "pathbins_dump: cannot read '%s ...'\n", w[0].c_str());
      return 2;
    }
  }
  return 0;
}
