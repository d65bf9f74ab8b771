// The crop window of one anchor for hard-patch mining: reference os2d/modeling/box_coder.py:78-166
// (BoxGridGenerator.get_box_to_cut_anchor) as a closed form of the anchor index, with the reference's float32 tensor
// expressions operation for operation (no fused multiply-adds), so that the windows - and the NMS decisions made on them - have
// the reference's bits.  Shared by os2d_train_crop_boxes and os2d_train_mine_select (mining.hip).
#pragma once
#include "../csrc/detect_common.h"

struct Os2dCropGeometry {
  int W;                        // feature map width (anchors are row-major: index = y * W + x)
  float stride, box_size;       // anchor stride and size, both isotropic
  float img_w, img_h;           // the level's image
  float crop_w, crop_h;         // the window wanted
};

// torch's floor_divide on float32 (c10::div_floor_floating) for a positive divisor
DET_DEV float os2d_floor_div(float a, float b) {
#pragma clang fp contract(off)
  const float mod = fmodf(a, b);
  float div = (a - mod) / b;
  if (mod != 0.f && mod < 0.f) div = div - 1.f;
  if (div == 0.f) return copysignf(0.f, a / b);
  float fl = floorf(div);
  if (div - fl > 0.5f) fl = fl + 1.f;
  return fl;
}

// one axis: centre c of the anchor, window length `crop`, image length `img` -> (lo, hi)
DET_DEV void os2d_crop_axis(float c, float crop, float img, float stride, float* lo_out, float* hi_out) {
#pragma clang fp contract(off)
  const float raw = c - crop / 2.f;
  // floor_to_stride where the corner is positive, else 0
  float lo = raw > 0.f ? os2d_floor_div(floorf(raw), stride) * stride : 0.f;
  float hi = lo + crop;
  if (lo < 0.f) {   // move right / down (never taken after the line above; kept as the reference has it)
    hi = hi - lo;
    lo = 0.f;
  }
  if (hi > img) {
    const float shift = floorf(ceilf(floorf(hi - img) / stride)) * stride;   // ceil_to_stride
    if (lo - shift >= 0.f) {   // shift left / up
      lo = lo - shift;
      hi = hi - shift;
    } else {                   // full width / height
      lo = 0.f;
      hi = crop;
    }
  }
  *lo_out = lo;
  *hi_out = hi;
}

// anchor p of a level -> its crop window and the anchor box, both through the level's chain
DET_DEV void os2d_mine_crop_box(int p, const Os2dCropGeometry& g, const Os2dBoxOps& ops, float4* crop, float4* anchor) {
#pragma clang fp contract(off)
  const int y = p / g.W, x = p - y * g.W;
  const float cx = ((float)x + 0.5f) * g.stride, cy = ((float)y + 0.5f) * g.stride;
  const float half = g.box_size / 2.f;
  float4 c;
  os2d_crop_axis(cx, g.crop_w, g.img_w, g.stride, &c.x, &c.z);
  os2d_crop_axis(cy, g.crop_h, g.img_h, g.stride, &c.y, &c.w);
  *crop = os2d_apply_box_ops(c, ops);
  *anchor = os2d_apply_box_ops(make_float4(cx - half, cy - half, cx + half, cy + half), ops);
}
