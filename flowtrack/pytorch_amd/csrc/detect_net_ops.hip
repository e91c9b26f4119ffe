// Glue kernels of the Faster R-CNN detector network (reference lib/detection: model/test.py, nets/network.py, nets/resnet_v1.py):
// the steps the reference runs on the host or as torch ops between its convolutions.
//   ft_detect_blob_fwd        model/test.py:37-58 (_get_image_blob: mean subtraction + cv2.resize INTER_LINEAR) and
//                             nets/network.py:378 (the HWC -> CHW transpose): u8 BGR frame -> the trunk's NCHW fp32 input
//   ft_rpn_softmax_fwd        nets/network.py:234-238: the two-way softmax over the channel pairs (a, a + A)
//   ft_rcnn_mean_pool_fwd     nets/resnet_v1.py:113: `.mean(3).mean(2)` behind layer4, on the NHWC map
//   ft_rcnn_detections_fwd    nets/network.py:270 (softmax over classes), :386-389 (bbox_pred * stds + means) and
//                             model/test.py:97-104 (rois / im_scale, bbox_transform_inv per class, _clip_boxes)
// All four are memory-bound and run in fp32 with every operation rounded separately (no FMA contraction, IEEE division, expf),
// like detect_ops.hip.  Device safety: every address is formed from kernel arguments and clamped indices only; no kernel reads
// an index from device data, loops on device data or waits on another workgroup.
#include "ft_common.h"

#pragma clang fp contract(off)

namespace ft {

constexpr int DN_THREADS = 256;
constexpr long long DN_MAX_ELEMS = 1ll << 31;        // element counts stay below this: every flat index fits an int

// ---- blob -------------------------------------------------------------------------------------------------------------------
// One axis of OpenCV's INTER_LINEAR table for float images (imgproc resize.cpp: the xofs / alpha tables): the source coordinate
// (d + 0.5) * scale - 0.5 is formed in double and rounded to float, floor, the fraction; left of the image the weight is zeroed
// and the index clamped to 0, at or past the last pixel the weight is zeroed and the index clamped to size - 1.
__device__ __forceinline__ void blob_axis(int d, double scale, int size, int& i0, int& i1, float& w0, float& w1) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  f = fminf(fmaxf(f, -2.f), (float)size + 1.f);      // keeps the cast below in range (a NaN takes the lower limit); no in-range value moves
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= size - 1) { f = 0.f; s = size - 1; }
  i0 = s;
  i1 = s + 1 < size ? s + 1 : size - 1;
  w0 = 1.f - f;
  w1 = f;
}

// One thread per output pixel, x fastest: the three channel planes are written with coalesced 4-byte stores (a row of an
// arbitrary-width plane has no 16-byte alignment to offer); the four source pixels are 3-byte reads that neighbours share.
__global__ __launch_bounds__(DN_THREADS) void detect_blob_kernel(const uint8_t* __restrict__ frame, int H, int W, double m0, double m1,
                                                                 double m2, int Hb, int Wb, double scale_y, double scale_x,
                                                                 float* __restrict__ blob) {
  const int idx = blockIdx.x * DN_THREADS + threadIdx.x;
  if (idx >= Hb * Wb) return;
  const int dx = idx % Wb, dy = idx / Wb;
  int x0, x1, y0, y1;
  float a0, a1, b0, b1;
  blob_axis(dx, scale_x, W, x0, x1, a0, a1);
  blob_axis(dy, scale_y, H, y0, y1, b0, b1);
  const uint8_t* p00 = frame + ((size_t)y0 * W + x0) * 3;
  const uint8_t* p01 = frame + ((size_t)y0 * W + x1) * 3;
  const uint8_t* p10 = frame + ((size_t)y1 * W + x0) * 3;
  const uint8_t* p11 = frame + ((size_t)y1 * W + x1) * 3;
  const double mean[3] = {m0, m1, m2};     // (float)((double)u8 - mean): the reference subtracts its float64 means into a float32 image
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float s00 = (float)((double)p00[c] - mean[c]), s01 = (float)((double)p01[c] - mean[c]);
    const float s10 = (float)((double)p10[c] - mean[c]), s11 = (float)((double)p11[c] - mean[c]);
    const float top = s00 * a0 + s01 * a1, bottom = s10 * a0 + s11 * a1;       // the horizontal pass of the two rows
    blob[(size_t)c * Hb * Wb + idx] = top * b0 + bottom * b1;                   // the vertical pass
  }
}

// ---- RPN softmax ------------------------------------------------------------------------------------------------------------
// One thread per (pixel, anchor): the pair (a, a + A) of the pixel's 2A scores.  Neighbouring threads read neighbouring
// channels; a row of 2A values has no 16-byte structure (A = 9).
template <typename T>
__global__ __launch_bounds__(DN_THREADS) void rpn_softmax_kernel(const T* __restrict__ x, long long rows, int A, int x_stride,
                                                                 int x_off, float* __restrict__ prob) {
  const long long idx = (long long)blockIdx.x * DN_THREADS + threadIdx.x;
  if (idx >= rows * A) return;
  const long long row = idx / A;
  const int a = (int)(idx - row * A);
  const T* p = x + (size_t)row * x_stride + x_off;
  const float v0 = (float)p[a], v1 = (float)p[a + A];
  const float m = fmaxf(v0, v1);
  const float e0 = expf(v0 - m), e1 = expf(v1 - m);
  const float s = e0 + e1;
  float* o = prob + (size_t)row * 2 * A;
  o[a] = e0 / s;
  o[a + A] = e1 / s;
}

// ---- mean pool --------------------------------------------------------------------------------------------------------------
// One thread per (RoI, 16-byte piece of C): P * P independent 16-byte loads C elements apart (neighbouring threads read
// neighbouring pieces), the row sums in x order, their means summed in y order, one 16-byte store.
template <typename T> struct dn_piece;
template <> struct dn_piece<half_t> { typedef half8_t type; static constexpr int N = 8; };
template <> struct dn_piece<float> { typedef float4_t type; static constexpr int N = 4; };

template <typename T>
__global__ __launch_bounds__(DN_THREADS) void rcnn_mean_pool_kernel(const T* __restrict__ x, int R, int P, int C, T* __restrict__ out) {
  typedef typename dn_piece<T>::type piece_t;
  constexpr int N = dn_piece<T>::N;
  const int pieces = C / N;
  const long long idx = (long long)blockIdx.x * DN_THREADS + threadIdx.x;
  if (idx >= (long long)R * pieces) return;
  const int r = (int)(idx / pieces), v = (int)(idx - (long long)r * pieces);
  const T* src = x + (size_t)r * P * P * C + (size_t)v * N;
  const float fp = (float)P;
  float acc[N];
#pragma unroll
  for (int e = 0; e < N; ++e) acc[e] = 0.f;
  for (int y = 0; y < P; ++y) {
    float row[N];
#pragma unroll
    for (int e = 0; e < N; ++e) row[e] = 0.f;
    for (int xx = 0; xx < P; ++xx) {
      const piece_t q = *reinterpret_cast<const piece_t*>(src + (size_t)(y * P + xx) * C);
#pragma unroll
      for (int e = 0; e < N; ++e) row[e] = row[e] + (float)q[e];
    }
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = acc[e] + row[e] / fp;
  }
  piece_t o;
#pragma unroll
  for (int e = 0; e < N; ++e) o[e] = (T)(acc[e] / fp);
  *reinterpret_cast<piece_t*>(out + (size_t)r * C + (size_t)v * N) = o;
}

// ---- detections -------------------------------------------------------------------------------------------------------------
// One wave per RoI.  The class softmax reduces over the wave with shuffles (a fixed tree: the result does not depend on the
// launch); then every lane owns the classes lane, lane + 64, ...: one 16-byte load of the class's four deltas, the
// un-normalisation, the decode against the RoI's box in frame pixels and the one-sided clip, two 16-byte stores.
// BOXES = false is the instantiation for calls without pred_boxes: it holds no read of `rois` at all (the entry passes NULL on), so
// that a caller who skips the boxes may leave the RoIs out, as the header says.
struct det_consts { float std[4], mean[4]; };

template <bool BOXES>
__global__ __launch_bounds__(64) void rcnn_detections_kernel(const float* __restrict__ cls_score, const float* __restrict__ bbox_pred,
                                                             const float* __restrict__ rois, int K, det_consts k, float im_scale,
                                                             float im_h, float im_w, float* __restrict__ cls_prob,
                                                             float* __restrict__ deltas, float* __restrict__ pred_boxes) {
  const int r = blockIdx.x, lane = threadIdx.x;
  if (cls_prob) {
    const float* s = cls_score + (size_t)r * K;
    float m = -__builtin_inff();
    for (int c = lane; c < K; c += 64) m = fmaxf(m, s[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float sum = 0.f;
    for (int c = lane; c < K; c += 64) sum = sum + expf(s[c] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum = sum + __shfl_xor(sum, o, 64);
    for (int c = lane; c < K; c += 64) cls_prob[(size_t)r * K + c] = expf(s[c] - m) / sum;
  }
  if (!deltas && !(BOXES && pred_boxes)) return;
  float w = 0.f, h = 0.f, cx = 0.f, cy = 0.f;
  if constexpr (BOXES) {
    const float* roi = rois + (size_t)r * 5;
    const float x1 = roi[1] / im_scale, y1 = roi[2] / im_scale, x2 = roi[3] / im_scale, y2 = roi[4] / im_scale;
    w = x2 - x1 + 1.0f;
    h = y2 - y1 + 1.0f;
    cx = x1 + 0.5f * w;
    cy = y1 + 0.5f * h;
  }
  const float xl = im_w - 1.f, yl = im_h - 1.f;
  for (int c = lane; c < K; c += 64) {
    const size_t at = ((size_t)r * K + c) * 4;
    const float4_t p = *reinterpret_cast<const float4_t*>(bbox_pred + at);
    float4_t d;
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = p[e] * k.std[e] + k.mean[e];
    if (deltas) *reinterpret_cast<float4_t*>(deltas + at) = d;
    if constexpr (BOXES) {
      const float pcx = d[0] * w + cx, pcy = d[1] * h + cy;
      const float pw = expf(d[2]) * w, ph = expf(d[3]) * h;
      float4_t o;
      o[0] = fmaxf(pcx - 0.5f * pw, 0.f);            // _clip_boxes: x1, y1 are only raised, x2, y2 only lowered
      o[1] = fmaxf(pcy - 0.5f * ph, 0.f);
      o[2] = fminf(pcx + 0.5f * pw, xl);
      o[3] = fminf(pcy + 0.5f * ph, yl);
      *reinterpret_cast<float4_t*>(pred_boxes + at) = o;
    }
  }
}

static inline bool dn_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline unsigned dn_blocks(long long total) { return (unsigned)((total + DN_THREADS - 1) / DN_THREADS); }

}  // namespace ft

using namespace ft;

extern "C" int ft_detect_blob_fwd(const uint8_t* frame, int H, int W, const double* means, int Hb, int Wb, double scale_y,
                                  double scale_x, float* blob, ft_stream_t stream) {
  if (H < 0 || W < 0 || Hb < 0 || Wb < 0) return FT_ERR_INVALID_ARG;
  if (Hb == 0 || Wb == 0) return FT_OK;
  if (H == 0 || W == 0 || !frame || !means || !blob || !(scale_y > 0.0) || !(scale_x > 0.0) || scale_y > 1e6 || scale_x > 1e6)
    return FT_ERR_INVALID_ARG;
  if (3ll * H * W >= DN_MAX_ELEMS || 3ll * Hb * Wb >= DN_MAX_ELEMS) return FT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(detect_blob_kernel, dim3(dn_blocks((long long)Hb * Wb)), dim3(DN_THREADS), 0, as_stream(stream), frame, H, W,
                     means[0], means[1], means[2], Hb, Wb, scale_y, scale_x, blob);
  FT_LAUNCH_CHECK("detect_blob_kernel");
  return FT_OK;
}

extern "C" int ft_rpn_softmax_fwd(int dtype, const void* scores, long long rows, int A, int x_cstride, int x_coff, float* prob,
                                  ft_stream_t stream) {
  if ((dtype != FT_F16 && dtype != FT_F32) || rows < 0 || A <= 0 || x_coff < 0 || x_cstride < 0 ||
      (long long)x_cstride < (long long)x_coff + 2ll * A)       // (in 64 bits: 2 * A may not fit an int)
    return FT_ERR_INVALID_ARG;
  if (rows == 0) return FT_OK;
  if (!scores || !prob) return FT_ERR_INVALID_ARG;
  if (rows >= DN_MAX_ELEMS || rows * x_cstride >= DN_MAX_ELEMS || rows * 2 * A >= DN_MAX_ELEMS) return FT_ERR_UNSUPPORTED;
  if (dtype == FT_F16)
    hipLaunchKernelGGL(rpn_softmax_kernel<half_t>, dim3(dn_blocks(rows * A)), dim3(DN_THREADS), 0, as_stream(stream),
                       static_cast<const half_t*>(scores), rows, A, x_cstride, x_coff, prob);
  else
    hipLaunchKernelGGL(rpn_softmax_kernel<float>, dim3(dn_blocks(rows * A)), dim3(DN_THREADS), 0, as_stream(stream),
                       static_cast<const float*>(scores), rows, A, x_cstride, x_coff, prob);
  FT_LAUNCH_CHECK("rpn_softmax_kernel");
  return FT_OK;
}

extern "C" int ft_rcnn_mean_pool_fwd(int dtype, const void* x, int R, int P, int C, void* out, ft_stream_t stream) {
  if ((dtype != FT_F16 && dtype != FT_F32) || R < 0 || P <= 0 || C <= 0 || C % 8 != 0) return FT_ERR_INVALID_ARG;
  if (R == 0) return FT_OK;
  if (!x || !out || !dn_aligned16(x) || !dn_aligned16(out)) return FT_ERR_INVALID_ARG;
  if ((long long)R * P * P * C >= DN_MAX_ELEMS) return FT_ERR_UNSUPPORTED;
  const long long total = (long long)R * (C / (dtype == FT_F16 ? 8 : 4));
  if (dtype == FT_F16)
    hipLaunchKernelGGL(rcnn_mean_pool_kernel<half_t>, dim3(dn_blocks(total)), dim3(DN_THREADS), 0, as_stream(stream),
                       static_cast<const half_t*>(x), R, P, C, static_cast<half_t*>(out));
  else
    hipLaunchKernelGGL(rcnn_mean_pool_kernel<float>, dim3(dn_blocks(total)), dim3(DN_THREADS), 0, as_stream(stream),
                       static_cast<const float*>(x), R, P, C, static_cast<float*>(out));
  FT_LAUNCH_CHECK("rcnn_mean_pool_kernel");
  return FT_OK;
}

extern "C" int ft_rcnn_detections_fwd(const float* cls_score, const float* bbox_pred, const float* rois, int R, int K,
                                      const float* stds, const float* means, float im_scale, float im_h, float im_w,
                                      float* cls_prob, float* deltas, float* pred_boxes, ft_stream_t stream) {
  if (R < 0 || K < 1 || !(im_scale > 0.f) || !(im_h >= 1.f) || !(im_w >= 1.f)) return FT_ERR_INVALID_ARG;
  if (R == 0) return FT_OK;
  if (!stds || !means) return FT_ERR_INVALID_ARG;
  if (cls_prob && !cls_score) return FT_ERR_INVALID_ARG;
  if ((deltas || pred_boxes) && (!bbox_pred || !dn_aligned16(bbox_pred) || (deltas && !dn_aligned16(deltas)) ||
                                 (pred_boxes && !dn_aligned16(pred_boxes))))
    return FT_ERR_INVALID_ARG;
  if (pred_boxes && !rois) return FT_ERR_INVALID_ARG;
  if (4ll * R * K >= DN_MAX_ELEMS) return FT_ERR_UNSUPPORTED;
  if (!cls_prob && !deltas && !pred_boxes) return FT_OK;
  det_consts k;
  for (int e = 0; e < 4; ++e) {
    k.std[e] = stds[e];
    k.mean[e] = means[e];
  }
  if (pred_boxes)
    hipLaunchKernelGGL(rcnn_detections_kernel<true>, dim3((unsigned)R), dim3(64), 0, as_stream(stream), cls_score, bbox_pred, rois, K, k,
                       im_scale, im_h, im_w, cls_prob, deltas, pred_boxes);
  else
    hipLaunchKernelGGL(rcnn_detections_kernel<false>, dim3((unsigned)R), dim3(64), 0, as_stream(stream), cls_score, bbox_pred, rois, K, k,
                       im_scale, im_h, im_w, cls_prob, deltas, pred_boxes);
  FT_LAUNCH_CHECK("rcnn_detections_kernel");
  return FT_OK;
}
