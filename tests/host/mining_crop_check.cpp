// Host run of os2d_amd/csrc_train/mining_crop.h - the same source the GPU runs: os2d_mine_crop_box over a table of geometries.
//   mining_crop_check <table> <out>
// <table> (text): a line "n", then per geometry "H W stride box img_w img_h crop_w crop_h nops" followed by nops triples
// "kind ax ay" with ax, ay as the hexadecimal bits of a float32.  <out> (binary): per geometry and anchor the crop window and the
// anchor box, 8 float32.  Built, run and compared with the reference's fixture and the loop model by tests/test_mining_crop_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct float4 {
  float x, y, z, w;
};
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }

#define OS2D_HOST_EMU 1
#define DET_DEV static inline
#define DET_BARRIER() ((void)0)
#define DET_BALLOT(p) ((p) ? 1ull : 0ull) /* a wave of one lane */
#define DET_READLANE(v, lane) (v)
#include "mining_crop.h"

static float bits_to_float(unsigned u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int n = 0;
  if (std::fscanf(in, "%d", &n) != 1 || n < 0) return 3;
  long boxes = 0;
  for (int i = 0; i < n; ++i) {
    int H, W, stride, box, img_w, img_h, crop_w, crop_h, nops;
    if (std::fscanf(in, "%d %d %d %d %d %d %d %d %d", &H, &W, &stride, &box, &img_w, &img_h, &crop_w, &crop_h, &nops) != 9) return 3;
    if (H < 1 || W < 1 || H * W > (1 << 20) || nops < 0 || nops > OS2D_BOX_MAX_OPS) return 3;
    int kinds[OS2D_BOX_MAX_OPS];
    float args[2 * OS2D_BOX_MAX_OPS];
    for (int k = 0; k < nops; ++k) {
      unsigned ax, ay;
      if (std::fscanf(in, "%d %x %x", &kinds[k], &ax, &ay) != 3) return 3;
      args[2 * k] = bits_to_float(ax);
      args[2 * k + 1] = bits_to_float(ay);
    }
    Os2dBoxOps ops;
    if (!os2d_box_ops_from(kinds, args, nops, &ops)) return 4;
    Os2dCropGeometry g;        // filled as mining.hip's geometry() fills it
    g.W = W;
    g.stride = (float)stride;
    g.box_size = (float)box;
    g.img_w = (float)img_w;
    g.img_h = (float)img_h;
    g.crop_w = (float)crop_w;
    g.crop_h = (float)crop_h;
    std::vector<float> rec((size_t)H * W * 8);
    for (int p = 0; p < H * W; ++p) {
      float4 c, a;
      os2d_mine_crop_box(p, g, ops, &c, &a);
      const float v[8] = {c.x, c.y, c.z, c.w, a.x, a.y, a.z, a.w};
      std::memcpy(&rec[(size_t)p * 8], v, sizeof v);
    }
    if (std::fwrite(rec.data(), 4, rec.size(), out) != rec.size()) return 5;
    boxes += (long)H * W;
  }
  std::fclose(out);
  std::fclose(in);
  std::printf("mining_crop_check: %d geometries, %ld anchors\nok\n", n, boxes);
  return 0;
}
