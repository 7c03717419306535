// csrc/tvl1_planes.hpp on a CPU (tests/test_planes_cpu.py builds this with ASan + UBSan): reads
// case lines, runs check_planes and then check_overlaps as an entry point does, and prints the
// first fault's status and message, one line per case.  A case line is
//   n w h limit skip in_place np {name pointer pitch stride elem shared} x np nov {a b unless_in_place} x nov
// with limit 24 (kFloatXLimit) or 19 (kMap32Limit) and the pointer as an integer: nothing is
// dereferenced.
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tvl1_planes.hpp"

using namespace tvl1k;

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    int32_t n, w, h;
    int limit, skip, in_place, np, nov;
    ss >> n >> w >> h >> limit >> skip >> in_place >> np;
    if (!ss || np < 0 || np > 16 || (limit != 24 && limit != 19)) return 3;
    std::vector<std::string> names((size_t)np);
    std::vector<Plane> pl((size_t)np);
    for (int i = 0; i < np; ++i) {
      uint64_t p, pitch, stride;
      int elem, shared;
      ss >> names[(size_t)i] >> p >> pitch >> stride >> elem >> shared;
      pl[(size_t)i] = {nullptr, reinterpret_cast<const void *>((uintptr_t)p), (size_t)pitch, (size_t)stride, elem,
                       shared != 0};
    }
    for (int i = 0; i < np; ++i) pl[(size_t)i].name = names[(size_t)i].c_str();
    ss >> nov;
    if (!ss || nov < 0 || nov > 64) return 3;
    std::vector<Overlap> ov((size_t)nov);
    for (int k = 0; k < nov; ++k) {
      int flag;
      ss >> ov[(size_t)k].a >> ov[(size_t)k].b >> flag;
      ov[(size_t)k].unless_in_place = flag != 0;
      if (ov[(size_t)k].a < 0 || ov[(size_t)k].a >= np || ov[(size_t)k].b < 0 || ov[(size_t)k].b >= np) return 3;
    }
    if (!ss) return 3;
    const PlaneSet ps = {n, w, h, pl.data(), np, skip};
    std::string msg;
    tvl1_status st = check_planes(ps, limit == 24 ? kFloatXLimit : kMap32Limit, &msg);
    if (st == TVL1_OK) st = check_overlaps(ps, ov.data(), nov, in_place != 0, &msg);
    std::printf("%d\t%s\n", (int)st, st == TVL1_OK ? "" : msg.c_str());
  }
  return 0;
}
