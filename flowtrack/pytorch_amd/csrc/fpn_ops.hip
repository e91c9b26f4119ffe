// The one operator of the FPN pose head (models.fpn) that is not a conv: NHWC bilinear resize with align_corners=True to an
// arbitrary output size, times an optional per-channel scale (the BatchNorm scale of the toplayer that follows the
// upsample-and-add, so that the add itself rides in the lateral conv's residual input).  A pure gather, bound by HBM: one thread
// per (output pixel, 16-byte channel group), four 16-byte loads and one 16-byte store, fp32 arithmetic, one rounding on store.
#include "bilerp_ac.h"      // Group<T>, ac_source: shared with hourglass_ops.hip

namespace ft {

// grid = (ho, images in flight, pieces of one output row): blockIdx.x is the output row, so its source rows and weights are
// uniform over the workgroup; a thread takes the (column, channel group) items j, j + 256 gridDim.z, .. of that row — lanes run
// along the channels, then along x, which is the order of both the output row and the two input rows — and, per item, the images
// blockIdx.y, blockIdx.y + gridDim.y, .. (one image per workgroup up to N = 65535, the y extent; the stride is what lifts the cap on
// N).  The only division is one 32-bit j / groups: no flat 64-bit index is split.
template <typename T>
__global__ __launch_bounds__(256) void upsample_bilinear_ac_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ scale,
                                                                   int N, int C, int hi, int wi, int ho, int wo, int x_cstride, int x_coff,
                                                                   int y_cstride, int y_coff, float rh, float rw, unsigned groups,
                                                                   unsigned row_items) {
  constexpr int G = Group<T>::G;
  typedef typename Group<T>::vec vec;
  const int oy = blockIdx.x;
  int y0, y1;
  float l0h, l1h;
  ac_source(rh, oy, hi, y0, y1, l0h, l1h);
  const size_t x_image = (size_t)hi * wi * x_cstride, y_image = (size_t)ho * wo * y_cstride;
  for (unsigned j = blockIdx.z * 256u + threadIdx.x; j < row_items; j += 256u * gridDim.z) {
    const unsigned ox = j / groups;
    const int c0 = (int)(j - ox * groups) * G;
    int x0, x1;
    float l0w, l1w;
    ac_source(rw, (int)ox, wi, x0, x1, l0w, l1w);
    const size_t oa = ((size_t)y0 * wi + x0) * x_cstride + x_coff + c0, ob = ((size_t)y0 * wi + x1) * x_cstride + x_coff + c0;
    const size_t oc = ((size_t)y1 * wi + x0) * x_cstride + x_coff + c0, od = ((size_t)y1 * wi + x1) * x_cstride + x_coff + c0;
    const size_t oo = ((size_t)oy * wo + ox) * y_cstride + y_coff + c0;
    if (c0 + G <= C) {
      float s[G];
#pragma unroll
      for (int e = 0; e < G; ++e) s[e] = scale ? scale[c0 + e] : 1.f;       // (v * 1 = v: the same bits as no scale)
      for (size_t n = blockIdx.y; n < (size_t)N; n += gridDim.y) {
        const T* xn = x + n * x_image;
        const vec a = *reinterpret_cast<const vec*>(xn + oa), b = *reinterpret_cast<const vec*>(xn + ob);
        const vec c = *reinterpret_cast<const vec*>(xn + oc), d = *reinterpret_cast<const vec*>(xn + od);
        vec o;
#pragma unroll
        for (int e = 0; e < G; ++e)
          o[e] = (T)(s[e] * (l0h * (l0w * (float)a[e] + l1w * (float)b[e]) + l1h * (l0w * (float)c[e] + l1w * (float)d[e])));
        *reinterpret_cast<vec*>(y + n * y_image + oo) = o;
      }
    } else {
      // the last group of a C that is no multiple of G: element by element, channels >= C are neither read nor written
      for (size_t n = blockIdx.y; n < (size_t)N; n += gridDim.y) {
        const T* xn = x + n * x_image;
        T* yn = y + n * y_image + oo;
        for (int e = 0; c0 + e < C; ++e) {
          const float v = l0h * (l0w * (float)xn[oa + e] + l1w * (float)xn[ob + e]) + l1h * (l0w * (float)xn[oc + e] + l1w * (float)xn[od + e]);
          yn[e] = (T)((scale ? scale[c0 + e] : 1.f) * v);
        }
      }
    }
  }
}

}  // namespace ft

using namespace ft;

extern "C" int ft_upsample_bilinear_ac_fwd(const void* x, void* y, int dtype, int N, int C, int hi, int wi, int ho, int wo, int x_cstride,
                                           int x_coff, int y_cstride, int y_coff, const float* scale, ft_stream_t stream) {
  if (!x || !y || N <= 0 || C <= 0 || hi <= 0 || wi <= 0 || ho <= 0 || wo <= 0) return FT_ERR_INVALID_ARG;
  if (dtype != FT_F16 && dtype != FT_F32) return FT_ERR_INVALID_ARG;
  if (x_coff < 0 || y_coff < 0 || x_cstride < x_coff + C || y_cstride < y_coff + C) return FT_ERR_INVALID_ARG;
  const int G = dtype == FT_F16 ? 8 : 4;
  // every 16-byte access must be aligned: offsets and strides in whole groups, base pointers on 16 bytes
  if (x_coff % G || y_coff % G || x_cstride % G || y_cstride % G) return FT_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) return FT_ERR_INVALID_ARG;
  // source coordinates are fp32 (torch's rule): above 2^24 rows or columns they stop being exact integers at the far end
  if (hi > (1 << 24) || wi > (1 << 24) || ho > (1 << 24) || wo > (1 << 24)) return FT_ERR_UNSUPPORTED;
  const int groups = (C + G - 1) / G;
  const long long row_items = (long long)wo * groups;       // (column, channel group) items of one output row: a 32-bit index
  if (row_items > 0x7fffffffLL) return FT_ERR_UNSUPPORTED;
  const float rh = ho > 1 ? (float)(hi - 1) / (float)(ho - 1) : 0.f;
  const float rw = wo > 1 ? (float)(wi - 1) / (float)(wo - 1) : 0.f;
  const long long pieces = (row_items + 255) / 256;
  // no cap on N: a workgroup strides over the images the grid's y extent (at most 65535) does not cover
  const dim3 grid((unsigned)ho, (unsigned)(N < 65535 ? N : 65535), (unsigned)(pieces < 64 ? pieces : 64));
  if (dtype == FT_F16)
    hipLaunchKernelGGL(upsample_bilinear_ac_kernel<half_t>, grid, dim3(256), 0, as_stream(stream), static_cast<const half_t*>(x),
                       static_cast<half_t*>(y), scale, N, C, hi, wi, ho, wo, x_cstride, x_coff, y_cstride, y_coff, rh, rw, (unsigned)groups,
                       (unsigned)row_items);
  else
    hipLaunchKernelGGL(upsample_bilinear_ac_kernel<float>, grid, dim3(256), 0, as_stream(stream), static_cast<const float*>(x),
                       static_cast<float*>(y), scale, N, C, hi, wi, ho, wo, x_cstride, x_coff, y_cstride, y_coff, rh, rw, (unsigned)groups,
                       (unsigned)row_items);
  FT_LAUNCH_CHECK("upsample_bilinear_ac_kernel");
  return FT_OK;
}
