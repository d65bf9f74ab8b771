// Host check of os2d_amd/csrc_backbone_conv_bf16/bf16x3_split.h on its own (tests/test_backbone_conv_bf16_model.py): reads bit patterns of
// fp32 values from standard input, 8 hex digits each, and prints one line "b0 b1 b2 special x0 x1 x2" per value: the parts of bf16x3_split
// as 4 hex digits, bf16x3_special, the parts of bf16x3_split_x.
#include <stdio.h>

#include "bf16x3_split.h"

int main() {
  unsigned int u;
  while (scanf("%x", &u) == 1) {
    uint16_t b0, b1, b2;
    const float x = bf16x3_float(u);
    bf16x3_split(x, &b0, &b1, &b2);
    uint16_t x0, x1, x2;
    bf16x3_split_x(x, &x0, &x1, &x2);
    printf("%04x %04x %04x %d %04x %04x %04x\n", (unsigned)b0, (unsigned)b1, (unsigned)b2, bf16x3_special(x) ? 1 : 0, (unsigned)x0, (unsigned)x1,
           (unsigned)x2);
  }
  return 0;
}
