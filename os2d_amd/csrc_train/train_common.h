// What the host code of train.hip and bn_live.hip shares: the layer table of the TransformNet, the shape limit of the plane
// layout and the grid size of a one-thread-per-element launch.
#pragma once
#include "../csrc/os2d_common.h"

namespace os2d_train {

struct Layer {
  int cout, cin, ks;
};
inline bool layer_shape(int layer, int P, Layer* s) {
  switch (layer) {
    case 1: *s = {128, OS2D_K, 7}; return true;
    case 2: *s = {64, 128, 5}; return true;
    case 3:
      if (P != 6 && P != 4) return false;
      *s = {P, 64, 5};
      return true;
    default: return false;
  }
}
// channel count of the forward buffer that feeds a layer: rnorm keeps 226 planes per pair (OS2D_KP)
inline int input_planes(int layer) { return layer == 1 ? OS2D_KP : layer == 2 ? 128 : 64; }
// output channels of a layer with a BatchNorm (1 or 2), 0 for any other
inline int layer_channels(int layer) {
  Layer L;
  return (layer == 1 || layer == 2) && layer_shape(layer, 6, &L) ? L.cout : 0;
}

inline bool shape_ok(int NB, int H, int W) { return NB >= 1 && H >= 1 && W >= 1 && W <= OS2D_MAX_W_DIRECT7 && H <= OS2D_MAX_H; }

inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace os2d_train

// a failed check in one statement: the text becomes the thread's last error, the value is `rc`
#define OS2D_REFUSE(rc, ...) (os2d_set_error(__VA_ARGS__), (rc))
