// The detector's region stage (reference lib/detection: nms/, layer_utils/roi_pooling, layer_utils/roi_align, model/bbox_transform.py,
// nets/network.py:_crop_pool_layer): everything between the RPN's two output maps and the tensor layer4 consumes.
//   ft_box_nms                 IoU bit mask in 64 x 64 tiles + the greedy sweep as ONE single-workgroup launch (the reference copies the
//                              whole mask to the host and sweeps it there)
//   ft_roi_pool_fwd / _bwd     max pooling over RoI bins, NCHW fp32, arg-max in-image; backward scatters with float atomics
//   ft_crop_and_resize_fwd/bwd TensorFlow's crop_and_resize, NCHW fp32; backward (image gradient) with float atomics
//   ft_roi_crop_nhwc_fwd       _crop_pool_layer fused for dense NHWC fp16 / fp32 features: writes the [R,7,7,C] input of ft_conv2d_fwd
//   ft_rpn_decode_boxes        bbox_transform_inv + clip_boxes in one pass
// The bar is BIT-EXACT against fp32 restatements that round every operation separately, so nothing below may be contracted into an
// FMA (the pragma; the build passes no fast-math flag, so `/` is the correctly rounded division).
// Device safety: every index that comes from device data (a RoI's batch index, a box's image index, a stored arg-max, a sample's
// neighbours) is range-checked before it becomes an address; every loop bound is a kernel argument or a value clipped against
// one; no kernel waits on another workgroup.
#include "ft_common.h"

#pragma clang fp contract(off)

namespace ft {

constexpr int DET_THREADS = 256;
constexpr int NMS_TILE = 64;                         // boxes per mask word
constexpr int NMS_MAX_BOXES = 16384;                 // 256 words per row: one word per thread of the sweep's workgroup
constexpr long long DET_MAX_ELEMS = 1ll << 31;       // element counts stay below this: every flat index fits an int

// ---- NMS --------------------------------------------------------------------------------------------------------------------
// Tile (row block, column block) of the mask: bit j of word [i][col] is set when box i suppresses box col * 64 + j > i.  Tiles
// below the diagonal are neither computed nor read.
__global__ __launch_bounds__(NMS_TILE) void nms_mask_kernel(const float* __restrict__ dets, int n, float thresh, int inclusive,
                                                            unsigned long long* __restrict__ mask) {
  const int row_blk = blockIdx.y, col_blk = blockIdx.x;
  if (row_blk > col_blk) return;
  const int words = (n + NMS_TILE - 1) / NMS_TILE;
  const int col0 = col_blk * NMS_TILE, row0 = row_blk * NMS_TILE;
  const int col_size = n - col0 < NMS_TILE ? n - col0 : NMS_TILE;
  __shared__ float s_box[NMS_TILE][4];
  __shared__ float s_area[NMS_TILE];
  const int t = threadIdx.x;
  if (t < col_size) {
    const float* b = dets + (size_t)(col0 + t) * 5;
    s_box[t][0] = b[0]; s_box[t][1] = b[1]; s_box[t][2] = b[2]; s_box[t][3] = b[3];
    s_area[t] = (b[2] - b[0] + 1.f) * (b[3] - b[1] + 1.f);
  }
  __syncthreads();
  const int i = row0 + t;
  if (i >= n) return;
  const float* a = dets + (size_t)i * 5;
  const float ax1 = a[0], ay1 = a[1], ax2 = a[2], ay2 = a[3];
  const float sa = (ax2 - ax1 + 1.f) * (ay2 - ay1 + 1.f);
  unsigned long long bits = 0;
  const int start = row_blk == col_blk ? t + 1 : 0;
  for (int j = start; j < col_size; ++j) {
    const float left = fmaxf(ax1, s_box[j][0]), right = fminf(ax2, s_box[j][2]);
    const float top = fmaxf(ay1, s_box[j][1]), bottom = fminf(ay2, s_box[j][3]);
    const float w = fmaxf(right - left + 1.f, 0.f), h = fmaxf(bottom - top + 1.f, 0.f);
    const float inter = w * h;
    const float iou = inter / (sa + s_area[j] - inter);
    if (inclusive ? iou >= thresh : iou > thresh) bits |= 1ull << j;
  }
  mask[(size_t)i * words + col_blk] = bits;
}

// The sweep: box i is kept iff no earlier kept box marked it.  One workgroup; thread t owns word t of the removed set in a
// register.  Per 64-box word w: wave 0 resolves the word from the diagonal tile alone (lane l holds row w * 64 + l of it, the
// walk jumps from kept box to kept box with one shuffle each), then all threads OR the rows of the boxes kept in this word into
// their own later words (independent loads) and thread w + 1 publishes its word for the next step.
__global__ __launch_bounds__(DET_THREADS) void nms_sweep_kernel(const unsigned long long* __restrict__ mask, int n, int cap,
                                                                int32_t* __restrict__ keep, int32_t* __restrict__ count) {
  const int words = (n + NMS_TILE - 1) / NMS_TILE;
  const int tid = threadIdx.x;
  __shared__ unsigned long long s_removed;           // the removed word of the current step
  __shared__ unsigned long long s_kept;              // the boxes kept in the current word
  __shared__ int s_cnt;
  unsigned long long removed = 0;                    // word `tid`
  if (tid == 0) {
    s_removed = 0;
    s_cnt = 0;
  }
  __syncthreads();
  for (int w = 0; w < words; ++w) {
    if (tid < 64) {
      const int row = w * NMS_TILE + tid;
      const unsigned long long diag = row < n ? mask[(size_t)row * words + w] : 0ull;
      const int left = n - w * NMS_TILE;
      unsigned long long open = left >= 64 ? ~0ull : ((1ull << left) - 1ull);   // positions of this word still to visit
      unsigned long long rem = s_removed, kept = 0;
      const int base = s_cnt;
      int cnt = base;
      while (cnt < cap) {
        const unsigned long long avail = open & ~rem;
        if (!avail) break;
        const int b = __ffsll((long long)avail) - 1;
        kept |= 1ull << b;
        ++cnt;
        rem |= __shfl(diag, b, 64);
        open &= b == 63 ? 0ull : ~((2ull << b) - 1ull);
      }
      if ((kept >> tid) & 1ull) keep[base + __popcll(kept & ((1ull << tid) - 1ull))] = row;
      if (tid == 0) {                                // nobody reads either word before the barrier below
        s_kept = kept;
        s_cnt = cnt;
      }
    }
    __syncthreads();
    unsigned long long kept = s_kept;
    const bool full = s_cnt >= cap;                  // uniform; both words are next written after the barrier that ends the step
    if (tid > w && tid < words) {
      while (kept) {
        const int b = __ffsll((long long)kept) - 1;
        kept &= kept - 1ull;
        removed |= mask[(size_t)(w * NMS_TILE + b) * words + tid];
      }
      if (tid == w + 1) s_removed = removed;
    }
    __syncthreads();
    if (full) break;
  }
  const int cnt = s_cnt;
  for (int i = cnt + tid; i < n; i += DET_THREADS) keep[i] = -1;
  if (tid == 0) *count = cnt;
}

// ---- RoI pooling ------------------------------------------------------------------------------------------------------------
// round(v) half away from zero as an int; the clamp keeps every later sum of these far from the int range (a map is many
// orders smaller, so no RoI that touches it is changed; a NaN takes the lower limit and its bins come out empty).
__device__ __forceinline__ int roi_round(float v) {
  const float r = roundf(v);
  return (int)fminf(fmaxf(r, -16777216.f), 16777216.f);
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(DET_THREADS) void roi_pool_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ rois, int B,
                                                                   int C, int H, int W, int R, float scale, int PH, int PW,
                                                                   float* __restrict__ out, int32_t* __restrict__ argmax) {
  const long long idx = (long long)blockIdx.x * DET_THREADS + threadIdx.x;
  if (idx >= (long long)R * C * PH * PW) return;
  int n = (int)idx;
  const int pw = n % PW; n /= PW;
  const int ph = n % PH; n /= PH;
  const int c = n % C; n /= C;
  const float* roi = rois + (size_t)n * 5;
  const int b = (int)fminf(fmaxf(roi[0], -1.f), (float)B);       // the reference's truncating cast; outside [0, B) (or NaN) stays outside
  float maxval = 0.f;
  int maxidx = -1;
  if (b >= 0 && b < B) {
    const int sw = roi_round(roi[1] * scale), sh = roi_round(roi[2] * scale);
    const int ew = roi_round(roi[3] * scale), eh = roi_round(roi[4] * scale);
    const int rw = ew - sw + 1 > 1 ? ew - sw + 1 : 1, rh = eh - sh + 1 > 1 ? eh - sh + 1 : 1;   // malformed RoIs are 1 x 1
    const float bin_h = (float)rh / (float)PH, bin_w = (float)rw / (float)PW;
    const int hstart = clampi((int)floorf((float)ph * bin_h) + sh, 0, H), hend = clampi((int)ceilf((float)(ph + 1) * bin_h) + sh, 0, H);
    const int wstart = clampi((int)floorf((float)pw * bin_w) + sw, 0, W), wend = clampi((int)ceilf((float)(pw + 1) * bin_w) + sw, 0, W);
    const bool empty = hend <= hstart || wend <= wstart;
    maxval = empty ? 0.f : -__FLT_MAX__;
    const float* img = feat + (size_t)b * C * H * W;
    for (int h = hstart; h < hend; ++h)
      for (int w = wstart; w < wend; ++w) {
        const int at = (c * H + h) * W + w;
        const float v = img[at];
        if (v > maxval) {
          maxval = v;
          maxidx = at;
        }
      }
  }
  out[idx] = maxval;
  if (argmax) argmax[idx] = maxidx;
}

__global__ __launch_bounds__(DET_THREADS) void roi_pool_bwd_kernel(const float* __restrict__ grad_out, const float* __restrict__ rois,
                                                                   const int32_t* __restrict__ argmax, int B, int C, int H, int W, int R,
                                                                   int PH, int PW, float* __restrict__ grad_in) {
  const long long idx = (long long)blockIdx.x * DET_THREADS + threadIdx.x;
  if (idx >= (long long)R * C * PH * PW) return;
  const int n = (int)(idx / ((long long)C * PH * PW));
  const float fb = rois[(size_t)n * 5];
  const int b = (int)fminf(fmaxf(fb, -1.f), (float)B);
  const int at = argmax[idx];
  if (b < 0 || b >= B || at < 0 || at >= C * H * W) return;
  unsafeAtomicAdd(grad_in + (size_t)b * C * H * W + at, grad_out[idx]);
}

// ---- crop_and_resize --------------------------------------------------------------------------------------------------------
// One axis of a crop sample: the source coordinate of output position `o` of `crop` along an axis of `size` pixels for the
// normalised box edge pair (lo, hi).  Returns false where the sample leaves [0, size - 1] (a NaN leaves it too).
__device__ __forceinline__ bool crop_axis(float lo, float hi, int o, int crop, int size, int& i0, int& i1, float& lerp) {
  const float last = (float)(size - 1);
  float in;
  if (crop > 1) {
    const float step = (hi - lo) * last / (float)(crop - 1);
    in = lo * last + (float)o * step;
  } else {
    in = 0.5f * (lo + hi) * last;
  }
  if (!(in >= 0.f && in <= last)) return false;
  i0 = (int)floorf(in);
  i1 = (int)ceilf(in);
  lerp = in - (float)i0;
  return true;
}

__global__ __launch_bounds__(DET_THREADS) void crop_resize_fwd_kernel(const float* __restrict__ image, const float* __restrict__ boxes,
                                                                      const int32_t* __restrict__ box_ind, int B, int C, int H, int W,
                                                                      int R, int CH, int CW, float extrapolation,
                                                                      float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * DET_THREADS + threadIdx.x;
  if (idx >= (long long)R * C * CH * CW) return;
  int n = (int)idx;
  const int x = n % CW; n /= CW;
  const int y = n % CH; n /= CH;
  const int d = n % C; n /= C;
  const int b = box_ind[n];
  if (b < 0 || b >= B) {
    out[idx] = 0.f;
    return;
  }
  const float* box = boxes + (size_t)n * 4;
  int y0, y1, x0, x1;
  float ly, lx;
  if (!crop_axis(box[0], box[2], y, CH, H, y0, y1, ly) || !crop_axis(box[1], box[3], x, CW, W, x0, x1, lx)) {
    out[idx] = extrapolation;
    return;
  }
  const float* p = image + ((size_t)b * C + d) * H * W;
  const float tl = p[y0 * W + x0], tr = p[y0 * W + x1], bl = p[y1 * W + x0], br = p[y1 * W + x1];
  const float top = tl + (tr - tl) * lx, bottom = bl + (br - bl) * lx;
  out[idx] = top + (bottom - top) * ly;
}

__global__ __launch_bounds__(DET_THREADS) void crop_resize_bwd_kernel(const float* __restrict__ grad_out, const float* __restrict__ boxes,
                                                                      const int32_t* __restrict__ box_ind, int B, int C, int H, int W,
                                                                      int R, int CH, int CW, float* __restrict__ grad_image) {
  const long long idx = (long long)blockIdx.x * DET_THREADS + threadIdx.x;
  if (idx >= (long long)R * C * CH * CW) return;
  int n = (int)idx;
  const int x = n % CW; n /= CW;
  const int y = n % CH; n /= CH;
  const int d = n % C; n /= C;
  const int b = box_ind[n];
  if (b < 0 || b >= B) return;
  const float* box = boxes + (size_t)n * 4;
  int y0, y1, x0, x1;
  float ly, lx;
  if (!crop_axis(box[0], box[2], y, CH, H, y0, y1, ly) || !crop_axis(box[1], box[3], x, CW, W, x0, x1, lx)) return;
  float* p = grad_image + ((size_t)b * C + d) * H * W;
  const float g = grad_out[idx];
  const float dtop = (1.f - ly) * g, dbottom = ly * g;
  unsafeAtomicAdd(p + y0 * W + x0, (1.f - lx) * dtop);
  unsafeAtomicAdd(p + y0 * W + x1, lx * dtop);
  unsafeAtomicAdd(p + y1 * W + x0, (1.f - lx) * dbottom);
  unsafeAtomicAdd(p + y1 * W + x1, lx * dbottom);
}

// ---- the fused NHWC inference form ------------------------------------------------------------------------------------------
// One workgroup per (RoI, output cell): the box geometry is uniform over the workgroup (it depends on blockIdx alone), the
// threads (one per 16-byte piece of C, in whole waves, at most 256) run along C; the four neighbours of a sample are four
// contiguous C-runs.  T = half_t (8 per piece) or float (4 per piece).  max_pool: the cell is the 2 x 2 max of the crop at
// 2 * pooled (torch's max_pool2d rule: a later value replaces the running one only when it is greater, or a NaN).
template <typename T> struct nhwc_piece;
template <> struct nhwc_piece<half_t> { typedef half8_t type; static constexpr int N = 8; };
template <> struct nhwc_piece<float> { typedef float4_t type; static constexpr int N = 4; };

struct crop_tap {
  int ok;                                            // 0: the sample is the extrapolation value (0)
  int o00, o01, o10, o11;                            // pixel offsets (y * W + x) of the four neighbours
  float lx, ly;
};

template <typename T, int TAPS>
__global__ __launch_bounds__(DET_THREADS) void roi_crop_nhwc_kernel(const T* __restrict__ feat, const float* __restrict__ rois, int B,
                                                                    int H, int W, int C, int R, float feat_stride, int pooled,
                                                                    T* __restrict__ out) {
  typedef typename nhwc_piece<T>::type piece_t;
  constexpr int N = nhwc_piece<T>::N;
  const int cell = blockIdx.x;
  const int px = cell % pooled, py = (cell / pooled) % pooled, r = cell / (pooled * pooled);
  const float* roi = rois + (size_t)r * 5;
  const float fb = roi[0];
  const int b = (int)fminf(fmaxf(fb, -1.f), (float)B);           // `.int()`: truncation; outside [0, B) (or NaN) stays outside
  piece_t* dst = reinterpret_cast<piece_t*>(out + (size_t)cell * C);
  const int pieces = C / N;
  if (b < 0 || b >= B) {
    for (int v = threadIdx.x; v < pieces; v += blockDim.x) {
      piece_t z;
      for (int e = 0; e < N; ++e) z[e] = (T)0.f;
      dst[v] = z;
    }
    return;
  }
  const float wl = (float)(W - 1), hl = (float)(H - 1);
  const float bx1 = roi[1] / feat_stride / wl, by1 = roi[2] / feat_stride / hl;
  const float bx2 = roi[3] / feat_stride / wl, by2 = roi[4] / feat_stride / hl;
  constexpr bool max_pool = TAPS == 4;
  const int crop = max_pool ? 2 * pooled : pooled;
  crop_tap tap[TAPS];
#pragma unroll
  for (int k = 0; k < TAPS; ++k) {
    tap[k].ok = 0;
    const int oy = max_pool ? 2 * py + (k >> 1) : py, ox = max_pool ? 2 * px + (k & 1) : px;
    int y0, y1, x0, x1;
    if (crop_axis(by1, by2, oy, crop, H, y0, y1, tap[k].ly) && crop_axis(bx1, bx2, ox, crop, W, x0, x1, tap[k].lx)) {
      tap[k].ok = 1;
      tap[k].o00 = y0 * W + x0; tap[k].o01 = y0 * W + x1; tap[k].o10 = y1 * W + x0; tap[k].o11 = y1 * W + x1;
    }
  }
  const T* img = feat + (size_t)b * H * W * C;
  for (int v = threadIdx.x; v < pieces; v += blockDim.x) {
    float acc[N];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) {
      float val[N];
      if (tap[k].ok) {
        const piece_t tl = *reinterpret_cast<const piece_t*>(img + (size_t)tap[k].o00 * C + v * N);
        const piece_t tr = *reinterpret_cast<const piece_t*>(img + (size_t)tap[k].o01 * C + v * N);
        const piece_t bl = *reinterpret_cast<const piece_t*>(img + (size_t)tap[k].o10 * C + v * N);
        const piece_t br = *reinterpret_cast<const piece_t*>(img + (size_t)tap[k].o11 * C + v * N);
#pragma unroll
        for (int e = 0; e < N; ++e) {
          const float ftl = (float)tl[e], ftr = (float)tr[e], fbl = (float)bl[e], fbr = (float)br[e];
          const float top = ftl + (ftr - ftl) * tap[k].lx, bottom = fbl + (fbr - fbl) * tap[k].lx;
          val[e] = top + (bottom - top) * tap[k].ly;
        }
      } else {
#pragma unroll
        for (int e = 0; e < N; ++e) val[e] = 0.f;
      }
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] = (k == 0 || val[e] > acc[e] || val[e] != val[e]) ? val[e] : acc[e];
    }
    piece_t o;
#pragma unroll
    for (int e = 0; e < N; ++e) o[e] = (T)acc[e];
    dst[v] = o;
  }
}

// ---- RPN box decode ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DET_THREADS) void rpn_decode_kernel(const float* __restrict__ anchors, const float* __restrict__ deltas,
                                                                 int A, float im_h, float im_w, float* __restrict__ boxes) {
  const int i = blockIdx.x * DET_THREADS + threadIdx.x;
  if (i >= A) return;
  const float4_t a = *reinterpret_cast<const float4_t*>(anchors + (size_t)i * 4);
  const float4_t d = *reinterpret_cast<const float4_t*>(deltas + (size_t)i * 4);
  const float w = a[2] - a[0] + 1.0f, h = a[3] - a[1] + 1.0f;
  const float cx = a[0] + 0.5f * w, cy = a[1] + 0.5f * h;
  const float pcx = d[0] * w + cx, pcy = d[1] * h + cy;
  const float pw = expf(d[2]) * w, ph = expf(d[3]) * h;
  const float xl = im_w - 1.f, yl = im_h - 1.f;
  float4_t o;
  o[0] = fminf(fmaxf(pcx - 0.5f * pw, 0.f), xl);
  o[1] = fminf(fmaxf(pcy - 0.5f * ph, 0.f), yl);
  o[2] = fminf(fmaxf(pcx + 0.5f * pw, 0.f), xl);
  o[3] = fminf(fmaxf(pcy + 0.5f * ph, 0.f), yl);
  *reinterpret_cast<float4_t*>(boxes + (size_t)i * 4) = o;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline unsigned blocks_for(long long total) { return (unsigned)((total + DET_THREADS - 1) / DET_THREADS); }

}  // namespace ft

using namespace ft;

extern "C" long long ft_box_nms_workspace_bytes(int n) {
  if (n <= 0 || n > NMS_MAX_BOXES) return 0;
  return (long long)n * ((n + NMS_TILE - 1) / NMS_TILE) * (long long)sizeof(unsigned long long);
}

extern "C" int ft_box_nms(const float* dets, int n, float thresh, int inclusive, int max_keep, void* workspace, int32_t* keep,
                          int32_t* count, ft_stream_t stream) {
  if (n < 0 || (inclusive != 0 && inclusive != 1) || !(thresh == thresh)) return FT_ERR_INVALID_ARG;
  if (n == 0) return FT_OK;
  if (!dets || !workspace || !keep || !count) return FT_ERR_INVALID_ARG;
  if (n > NMS_MAX_BOXES) return FT_ERR_UNSUPPORTED;
  const int words = (n + NMS_TILE - 1) / NMS_TILE;
  const int cap = max_keep <= 0 || max_keep > n ? n : max_keep;
  hipLaunchKernelGGL(nms_mask_kernel, dim3(words, words), dim3(NMS_TILE), 0, as_stream(stream), dets, n, thresh, inclusive,
                     static_cast<unsigned long long*>(workspace));
  FT_LAUNCH_CHECK("nms_mask_kernel");
  hipLaunchKernelGGL(nms_sweep_kernel, dim3(1), dim3(DET_THREADS), 0, as_stream(stream),
                     static_cast<const unsigned long long*>(workspace), n, cap, keep, count);
  FT_LAUNCH_CHECK("nms_sweep_kernel");
  return FT_OK;
}

extern "C" int ft_roi_pool_fwd(const float* features, const float* rois, int B, int C, int H, int W, int R, float spatial_scale,
                               int pooled_h, int pooled_w, float* out, int32_t* argmax, ft_stream_t stream) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || R < 0 || pooled_h <= 0 || pooled_w <= 0 || !(spatial_scale == spatial_scale))
    return FT_ERR_INVALID_ARG;
  if (R == 0) return FT_OK;
  if (!features || !rois || !out) return FT_ERR_INVALID_ARG;
  const long long total = (long long)R * C * pooled_h * pooled_w;
  if ((long long)B * C * H * W >= DET_MAX_ELEMS || total >= DET_MAX_ELEMS || (long long)C * pooled_h * pooled_w >= DET_MAX_ELEMS)
    return FT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(roi_pool_fwd_kernel, dim3(blocks_for(total)), dim3(DET_THREADS), 0, as_stream(stream), features, rois, B, C, H, W, R,
                     spatial_scale, pooled_h, pooled_w, out, argmax);
  FT_LAUNCH_CHECK("roi_pool_fwd_kernel");
  return FT_OK;
}

extern "C" int ft_roi_pool_bwd(const float* grad_out, const float* rois, const int32_t* argmax, int B, int C, int H, int W, int R,
                               int pooled_h, int pooled_w, float* grad_in, ft_stream_t stream) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || R < 0 || pooled_h <= 0 || pooled_w <= 0 || !grad_in) return FT_ERR_INVALID_ARG;
  if (R > 0 && (!grad_out || !rois || !argmax)) return FT_ERR_INVALID_ARG;
  const long long total = (long long)R * C * pooled_h * pooled_w, in_elems = (long long)B * C * H * W;
  if (in_elems >= DET_MAX_ELEMS || total >= DET_MAX_ELEMS || (long long)C * pooled_h * pooled_w >= DET_MAX_ELEMS) return FT_ERR_UNSUPPORTED;
  FT_HIP_CHECK(hipMemsetAsync(grad_in, 0, (size_t)in_elems * sizeof(float), as_stream(stream)));
  if (R == 0) return FT_OK;
  hipLaunchKernelGGL(roi_pool_bwd_kernel, dim3(blocks_for(total)), dim3(DET_THREADS), 0, as_stream(stream), grad_out, rois, argmax, B, C, H,
                     W, R, pooled_h, pooled_w, grad_in);
  FT_LAUNCH_CHECK("roi_pool_bwd_kernel");
  return FT_OK;
}

extern "C" int ft_crop_and_resize_fwd(const float* image, const float* boxes, const int32_t* box_ind, int B, int C, int H, int W, int R,
                                      int crop_h, int crop_w, float extrapolation_value, float* out, ft_stream_t stream) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || R < 0 || crop_h <= 0 || crop_w <= 0) return FT_ERR_INVALID_ARG;
  if (R == 0) return FT_OK;
  if (!image || !boxes || !box_ind || !out) return FT_ERR_INVALID_ARG;
  const long long total = (long long)R * C * crop_h * crop_w;
  if ((long long)B * C * H * W >= DET_MAX_ELEMS || total >= DET_MAX_ELEMS || (long long)C * crop_h * crop_w >= DET_MAX_ELEMS)
    return FT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(crop_resize_fwd_kernel, dim3(blocks_for(total)), dim3(DET_THREADS), 0, as_stream(stream), image, boxes, box_ind, B, C,
                     H, W, R, crop_h, crop_w, extrapolation_value, out);
  FT_LAUNCH_CHECK("crop_resize_fwd_kernel");
  return FT_OK;
}

extern "C" int ft_crop_and_resize_bwd(const float* grad_out, const float* boxes, const int32_t* box_ind, int B, int C, int H, int W, int R,
                                      int crop_h, int crop_w, float* grad_image, ft_stream_t stream) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || R < 0 || crop_h <= 0 || crop_w <= 0 || !grad_image) return FT_ERR_INVALID_ARG;
  if (R > 0 && (!grad_out || !boxes || !box_ind)) return FT_ERR_INVALID_ARG;
  const long long total = (long long)R * C * crop_h * crop_w, in_elems = (long long)B * C * H * W;
  if (in_elems >= DET_MAX_ELEMS || total >= DET_MAX_ELEMS || (long long)C * crop_h * crop_w >= DET_MAX_ELEMS) return FT_ERR_UNSUPPORTED;
  FT_HIP_CHECK(hipMemsetAsync(grad_image, 0, (size_t)in_elems * sizeof(float), as_stream(stream)));
  if (R == 0) return FT_OK;
  hipLaunchKernelGGL(crop_resize_bwd_kernel, dim3(blocks_for(total)), dim3(DET_THREADS), 0, as_stream(stream), grad_out, boxes, box_ind, B,
                     C, H, W, R, crop_h, crop_w, grad_image);
  FT_LAUNCH_CHECK("crop_resize_bwd_kernel");
  return FT_OK;
}

extern "C" int ft_roi_crop_nhwc_fwd(int dtype, const void* features, const float* rois, int B, int H, int W, int C, int R,
                                    float feat_stride, int pooled, int max_pool, void* out, ft_stream_t stream) {
  if ((dtype != FT_F16 && dtype != FT_F32) || B <= 0 || H < 2 || W < 2 || C <= 0 || C % 8 != 0 || R < 0 || pooled <= 0 ||
      !(feat_stride > 0.f) || (max_pool != 0 && max_pool != 1))
    return FT_ERR_INVALID_ARG;
  if (R == 0) return FT_OK;
  if (!features || !rois || !out || !aligned16(features) || !aligned16(out)) return FT_ERR_INVALID_ARG;
  const long long cells = (long long)R * pooled * pooled;
  if ((long long)B * H * W * C >= DET_MAX_ELEMS || cells * C >= DET_MAX_ELEMS) return FT_ERR_UNSUPPORTED;
  const int pieces = C / (dtype == FT_F16 ? 8 : 4);
  const int threads = pieces >= DET_THREADS ? DET_THREADS : round_up(pieces, 64);
#define FT_ROI_CROP_LAUNCH(T, TAPS)                                                                                                  \
  hipLaunchKernelGGL((roi_crop_nhwc_kernel<T, TAPS>), dim3((unsigned)cells), dim3(threads), 0, as_stream(stream),                     \
                     static_cast<const T*>(features), rois, B, H, W, C, R, feat_stride, pooled, static_cast<T*>(out))
  if (dtype == FT_F16) {
    if (max_pool) FT_ROI_CROP_LAUNCH(half_t, 4); else FT_ROI_CROP_LAUNCH(half_t, 1);
  } else {
    if (max_pool) FT_ROI_CROP_LAUNCH(float, 4); else FT_ROI_CROP_LAUNCH(float, 1);
  }
#undef FT_ROI_CROP_LAUNCH
  FT_LAUNCH_CHECK("roi_crop_nhwc_kernel");
  return FT_OK;
}

extern "C" int ft_rpn_decode_boxes(const float* anchors, const float* deltas, int A, float im_h, float im_w, float* boxes,
                                   ft_stream_t stream) {
  if (A < 0 || !(im_h >= 1.f) || !(im_w >= 1.f)) return FT_ERR_INVALID_ARG;
  if (A == 0) return FT_OK;
  if (!anchors || !deltas || !boxes || !aligned16(anchors) || !aligned16(deltas) || !aligned16(boxes)) return FT_ERR_INVALID_ARG;
  if (4ll * A >= DET_MAX_ELEMS) return FT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(rpn_decode_kernel, dim3(blocks_for(A)), dim3(DET_THREADS), 0, as_stream(stream), anchors, deltas, A, im_h, im_w, boxes);
  FT_LAUNCH_CHECK("rpn_decode_kernel");
  return FT_OK;
}
