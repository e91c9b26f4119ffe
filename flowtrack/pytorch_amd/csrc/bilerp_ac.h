// What the NHWC element-wise kernels with a bilinear align_corners=True gather share (fpn_ops.hip, hourglass_ops.hip): the 16-byte
// channel group of a thread and the coordinate rule of ft_upsample_bilinear_ac_fwd (include/flowtrack_hip.h).
#pragma once
#include "ft_common.h"

namespace ft {

// G channels of T = 16 bytes
template <typename T> struct Group;
template <> struct Group<half_t> {
  static constexpr int G = 8;
  typedef half8_t vec;
};
template <> struct Group<float> {
  static constexpr int G = 4;
  typedef float4_t vec;
};

// source index pair and weights of output index o along one axis: torch's rule for float inputs (see the header comment of
// ft_upsample_bilinear_ac_fwd).  The min() never acts for the ratios the host passes (r * (out - 1) <= in - 1 up to one rounding,
// which (int) truncates back onto in - 1); it is there so that no ratio can index past the row.
// Contraction is off here: `src` must be the ROUNDED product before i0 is taken off it (hipcc's default would fuse the product
// into the subtraction, l1 = fma(r, o, -i0), which is not the rule's l1 and moves a result by up to a few 2^-24 of the data).
__device__ __forceinline__ void ac_source(float r, int o, int in, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
  const float src = r * (float)o;
  i0 = min((int)src, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

// the host side of the rule: the ratio of one axis
static inline float ac_ratio(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

}  // namespace ft
