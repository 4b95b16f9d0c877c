// TEST INFRASTRUCTURE (tests/test_pair_keep_cpu.py): the round-trip kernel's variant selection (pair_keep_variant,
// vw_plan.cpp) and the parsing of its switch VW_PAIR_KEEP, as a host program over vw_plan.cpp.
//   pair_keep rule REQUESTED N0 N1 N2   -> the variant for that request and those workgroups per CU
//   pair_keep set VALUE                 -> Tuning::pair_keep after set_tuning("VW_PAIR_KEEP", VALUE)
//   pair_keep env                       -> Tuning::pair_keep as read_tuning() takes it from the environment
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "vw_plan.h"

using namespace vw;

int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "rule")) {
    const int n[kPairMaxKeep + 1] = {atoi(argv[3]), atoi(argv[4]), atoi(argv[5])};
    printf("%d\n", pair_keep_variant(atoi(argv[2]), n));
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "set")) {
    Tuning t;
    t.pair_keep = 1;  // so that "the default" is told from "left alone"
    if (!set_tuning(t, "VW_PAIR_KEEP", atoi(argv[2]))) return 2;
    printf("%d\n", t.pair_keep);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "env")) {
    printf("%d\n", read_tuning().pair_keep);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "limits")) {
    printf("%d %d %d\n", kPairMaxKeep, kPairAutoKeep, Tuning().pair_keep);
    return 0;
  }
  return 1;
}
