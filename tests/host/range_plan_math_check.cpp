// Host check of os2d_amd/csrc_train/range_plan_math.h on its own (tests/test_range_plan_device_model.py): the first line is the layout
// of the two result buffers, then one line "floor_log2 out_exp weight_exp" per argument, each argument the bit pattern of a
// double as 16 hex digits.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "range_plan_math.h"

int main(int argc, char** argv) {
  using namespace os2d_rp;
  printf("%d %d %d %d %d %d %d %d %d %d\n", RP_WEXP1, RP_E1, RP_UNIT, RP_WEXP2, RP_E2, RP_WEXP3, RP_INTS, RP_B1, RP_B2, RP_DOUBLES);
  for (int i = 1; i < argc; ++i) {
    const unsigned long long bits = strtoull(argv[i], nullptr, 16);
    double x;
    memcpy(&x, &bits, sizeof(x));
    printf("%d %d %d\n", floor_log2(x), out_exp(x), weight_exp(x));
  }
  return 0;
}
