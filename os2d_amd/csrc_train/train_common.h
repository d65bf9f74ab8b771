// What the host code of train.hip and bn_live.hip shares: the layers of the TransformNet as the forward library's table
// (csrc/os2d_common.h) has them, the shape limit of the plane layout and the grid size of a one-thread-per-element launch.
#pragma once
#include "../csrc/os2d_common.h"

namespace os2d_train {

using Layer = Os2dLayer;
inline bool layer_shape(int layer, int P, Layer* s) {
  if (layer < 1 || layer > 3 || (layer == 3 && P != 6 && P != 4)) return false;
  *s = os2d_layer(layer, P);
  return true;
}
// channel count of the forward buffer that feeds a layer: rnorm keeps 226 planes per pair (OS2D_KP)
inline int input_planes(int layer) { return os2d_layer(layer).planes(); }
// output channels of a layer with a BatchNorm (1 or 2), 0 for any other
inline int layer_channels(int layer) { return layer == 1 || layer == 2 ? os2d_layer(layer).cout : 0; }

inline bool shape_ok(int NB, int H, int W) { return NB >= 1 && H >= 1 && W >= 1 && W <= OS2D_MAX_W_DIRECT7 && H <= OS2D_MAX_H; }

inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace os2d_train
