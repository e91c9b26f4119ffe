// The one operator of the lateral-deconv pose head (models.pose) that is not a conv: a per-channel affine + activation on an NHWC
// view, y = act(scale[c] * x + shift[c]).  The head's first step reads relu(bn(c5)) of layer4's already activated output, an
// affine + ReLU that folds into no conv epilogue (the ReLU in front of it is in the way).  Bound by HBM: one thread per
// (pixel, 16-byte channel group), one 16-byte load and one 16-byte store; where a view is not 16-byte aligned, one element per thread.
// The arithmetic is the conv epilogue's: fma(scale, x, shift) in fp32, act_mul, one rounding to the output type.
#include "ft_common.h"

namespace ft {

template <typename T> struct SsaGroup;
template <> struct SsaGroup<half_t> {
  static constexpr int G = 8;
  typedef half8_t vec;
};
template <> struct SsaGroup<float> {
  static constexpr int G = 4;
  typedef float4_t vec;
};

__device__ __forceinline__ float ssa_one(float x, float s, float b, float k) {
  const float v = __builtin_fmaf(s, x, b);
  if (k <= 1.f) return act_mul(v, k);
  return v > 0.f ? v : v * k;      // (a slope > 1: conv_common.h's apply_act takes the same compare-and-select form)
}

// items = pixels * groups, item i = (pixel i / groups, channel group i % groups); a grid-stride loop, so any grid covers any size.
// x and y may be the same view (every element is read before it is written, by the thread that writes it).
template <typename T>
__global__ __launch_bounds__(256) void scale_shift_act_vec_kernel(const T* x, T* y, const float* __restrict__ scale, const float* __restrict__ shift,
                                                                   unsigned items, unsigned groups, int x_cstride, int x_coff, int y_cstride,
                                                                   int y_coff, float k) {
  constexpr int G = SsaGroup<T>::G;
  typedef typename SsaGroup<T>::vec vec;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < items; i += gridDim.x * 256u) {
    const unsigned pix = i / groups;
    const int c0 = (int)(i - pix * groups) * G;
    const vec v = *reinterpret_cast<const vec*>(x + (size_t)pix * x_cstride + x_coff + c0);
    vec o;
#pragma unroll
    for (int q = 0; q < G / 4; ++q) {
      const float4_t s = *reinterpret_cast<const float4_t*>(scale + c0 + 4 * q), b = *reinterpret_cast<const float4_t*>(shift + c0 + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[4 * q + e] = (T)ssa_one((float)v[4 * q + e], s[e], b[e], k);
    }
    *reinterpret_cast<vec*>(y + (size_t)pix * y_cstride + y_coff + c0) = o;
  }
}

// the element-wise form: any C, any offsets and strides, any pointer alignment of the element type
template <typename T>
__global__ __launch_bounds__(256) void scale_shift_act_elem_kernel(const T* x, T* y, const float* __restrict__ scale, const float* __restrict__ shift,
                                                                    unsigned items, unsigned C, int x_cstride, int x_coff, int y_cstride,
                                                                    int y_coff, float k) {
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < items; i += gridDim.x * 256u) {
    const unsigned pix = i / C;
    const int c = (int)(i - pix * C);
    y[(size_t)pix * y_cstride + y_coff + c] = (T)ssa_one((float)x[(size_t)pix * x_cstride + x_coff + c], scale[c], shift[c], k);
  }
}

constexpr unsigned kSsaMaxBlocks = 2048;      // 8 workgroups per CU of a 256-CU chip; the grid-stride loop takes the rest

template <typename T>
static int launch_scale_shift_act(const void* x, void* y, long long npix, int C, int x_cstride, int x_coff, int y_cstride, int y_coff,
                                  const float* scale, const float* shift, float k, hipStream_t s) {
  constexpr int G = SsaGroup<T>::G;
  const bool vec = C % G == 0 && x_coff % G == 0 && y_coff % G == 0 && x_cstride % G == 0 && y_cstride % G == 0 &&
                   ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(scale) |
                     reinterpret_cast<uintptr_t>(shift)) & 15) == 0;
  const long long items = npix * (vec ? C / G : C);
  if (items > 0x7fffffffLL) return FT_ERR_UNSUPPORTED;       // the item index is 32-bit
  const long long blocks = (items + 255) / 256;
  const dim3 grid((unsigned)(blocks < (long long)kSsaMaxBlocks ? blocks : (long long)kSsaMaxBlocks));
  if (vec)
    hipLaunchKernelGGL(scale_shift_act_vec_kernel<T>, grid, dim3(256), 0, s, static_cast<const T*>(x), static_cast<T*>(y), scale, shift,
                       (unsigned)items, (unsigned)(C / G), x_cstride, x_coff, y_cstride, y_coff, k);
  else
    hipLaunchKernelGGL(scale_shift_act_elem_kernel<T>, grid, dim3(256), 0, s, static_cast<const T*>(x), static_cast<T*>(y), scale, shift,
                       (unsigned)items, (unsigned)C, x_cstride, x_coff, y_cstride, y_coff, k);
  return FT_OK;
}

}  // namespace ft

using namespace ft;

extern "C" int ft_scale_shift_act_nhwc_fwd(const void* x, void* y, int dtype, long long npix, int C, int x_cstride, int x_coff, int y_cstride,
                                           int y_coff, const float* scale, const float* shift, int act, float slope, ft_stream_t stream) {
  if (!x || !y || !scale || !shift || npix <= 0 || C <= 0) return FT_ERR_INVALID_ARG;
  if (dtype != FT_F16 && dtype != FT_F32) return FT_ERR_INVALID_ARG;
  if (x_coff < 0 || y_coff < 0 || x_cstride < x_coff + C || y_cstride < y_coff + C) return FT_ERR_INVALID_ARG;
  if (act < FT_ACT_NONE || act > FT_ACT_LEAKY) return FT_ERR_INVALID_ARG;
  const size_t esz = dtype_size(dtype);
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & (esz - 1)) ||
      ((reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(shift)) & 3))
    return FT_ERR_INVALID_ARG;
  const float k = act == FT_ACT_RELU ? 0.f : (act == FT_ACT_LEAKY ? slope : 1.f);
  const int rc = dtype == FT_F16
                     ? launch_scale_shift_act<half_t>(x, y, npix, C, x_cstride, x_coff, y_cstride, y_coff, scale, shift, k, as_stream(stream))
                     : launch_scale_shift_act<float>(x, y, npix, C, x_cstride, x_coff, y_cstride, y_coff, scale, shift, k, as_stream(stream));
  if (rc != FT_OK) return rc;
  FT_LAUNCH_CHECK("scale_shift_act_kernel");
  return FT_OK;
}
