// The clip's sequential tracking pass on the device (tools/tracking/demo.py: tracking_pass_steps): what the host did per frame
// in numpy between two pose replays — move the previous frame's poses by the flow, build the propagated boxes, union them with
// the detector boxes, box NMS, cap, crop parameters, rows back into image pixels — as three single-workgroup kernels whose
// counts live in device words, so a whole clip is enqueued without a host wait (tracking/device_pass.py).
// The bar is BIT-EXACT against the host functions they restate (tracking/tracker.py: propagate_keypoints,
// tracking/flow_utils.py: box_propagation / nms, tracking/net_utils.py: boxes_to_center_scale / heatmap_rows_to_image):
// numpy rounds every operation separately, float64 for the geometry and float32 for the NMS, so nothing below may be
// contracted into an FMA (the pragma; the build passes no fast-math flag, so `/` is the correctly rounded division).
#include "ft_common.h"

#pragma clang fp contract(off)

namespace ft {

constexpr int TRK_THREADS = 256;
constexpr int TRK_MAX_BOXES = 512;                 // union size of ft_track_select: the pairwise hit mask is 512 x 512 bits of LDS
constexpr int TRK_WORDS = TRK_MAX_BOXES / 64;
constexpr int TRK_MAX_K = 32;

// `np.clip(v.astype(int), 0, hi)`: truncate towards zero, then clip.  fmax / fmin drop a NaN, so the index is in range for
// every input (the contract covers finite coordinates only; the bound has to hold regardless).
__device__ __forceinline__ int trk_pixel(double v, int hi) {
  return (int)fmin(fmax(trunc(v), 0.0), (double)hi);
}

// One joint moved by the flow at its (truncated, clipped) pixel: propagate_keypoints / box_propagation's `shifted`.
__device__ __forceinline__ void trk_move(const float* __restrict__ flow, int H, int W, double x, double y, double& mx, double& my) {
  const size_t at = (size_t)trk_pixel(y, H - 1) * W + trk_pixel(x, W - 1);
  mx = x + (double)flow[at];
  my = y + (double)flow[(size_t)H * W + at];
}

__global__ __launch_bounds__(TRK_THREADS) void track_propagate_kernel(const float* __restrict__ kps_prev, const float* __restrict__ flow,
                                                                      int H, int W, const double* __restrict__ older_in, int n_old,
                                                                      int P, int K, double* __restrict__ moved_out,
                                                                      float* __restrict__ boxes_out) {
  const int PK = P * K;
  for (int e = threadIdx.x; e < (1 + n_old) * PK; e += TRK_THREADS) {
    const int a = e / PK, pk = e - a * PK;
    double x, y;
    if (a == 0) {
      x = (double)kps_prev[(size_t)pk * 3];
      y = (double)kps_prev[(size_t)pk * 3 + 1];
    } else {
      x = older_in[((size_t)(a - 1) * PK + pk) * 2];
      y = older_in[((size_t)(a - 1) * PK + pk) * 2 + 1];
    }
    double mx, my;
    trk_move(flow, H, W, x, y, mx, my);
    moved_out[(size_t)e * 2] = mx;
    moved_out[(size_t)e * 2 + 1] = my;
  }
  // box_propagation: min / max over the joints with score > 0 (fill max(H, W) / 0.0), grown by 15 %, clipped to the image
  const double big = (double)(H > W ? H : W);
  for (int p = threadIdx.x; p < P; p += TRK_THREADS) {
    double mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    for (int k = 0; k < K; ++k) {
      const float* kp = kps_prev + ((size_t)p * K + k) * 3;
      if (!(kp[2] > 0.f)) {                          // a masked joint contributes the fill values to both reductions
        mnx = big < mnx ? big : mnx;
        mny = big < mny ? big : mny;
        mxx = 0.0 > mxx ? 0.0 : mxx;
        mxy = 0.0 > mxy ? 0.0 : mxy;
        continue;
      }
      double sx, sy;
      trk_move(flow, H, W, (double)kp[0], (double)kp[1], sx, sy);
      mnx = sx < mnx ? sx : mnx;
      mny = sy < mny ? sy : mny;
      mxx = sx > mxx ? sx : mxx;
      mxy = sy > mxy ? sy : mxy;
    }
    const double ex = (mxx - mnx) * 0.15 / 2, ey = (mxy - mny) * 0.15 / 2;
    boxes_out[(size_t)p * 4 + 0] = (float)fmax(mnx - ex, 0.0);
    boxes_out[(size_t)p * 4 + 1] = (float)fmax(mny - ey, 0.0);
    boxes_out[(size_t)p * 4 + 2] = (float)fmin(mxx + ex, (double)(W - 1));
    boxes_out[(size_t)p * 4 + 3] = (float)fmin(mxy + ey, (double)(H - 1));
  }
}

// boxes_to_center_scale of one float32 box, in float64: centre = mean of the corners, scale = aspect-corrected height.
__device__ __forceinline__ void trk_center_scale(float x1, float y1, float x2, float y2, int rh, int rw, double& cx, double& cy, double& sc) {
  cx = ((double)x1 + (double)x2) / 2.0;
  cy = ((double)y1 + (double)y2) / 2.0;
  const double hgt = (double)y2 - (double)y1, wid = ((double)x2 - (double)x1) / (double)rw * (double)rh;
  sc = hgt > wid ? hgt : wid;
}

__global__ __launch_bounds__(TRK_THREADS) void track_select_kernel(const float* __restrict__ dets, const float* __restrict__ kp_det, int n,
                                                                   const float* __restrict__ prop_boxes, const float* __restrict__ prev_boxes,
                                                                   int P, const int32_t* __restrict__ count_prev, int K, float thresh,
                                                                   int max_keep, int cap, int rh, int rw, int bucket,
                                                                   float* __restrict__ boxes, int32_t* __restrict__ src,
                                                                   int32_t* __restrict__ count, float* __restrict__ kps,
                                                                   int32_t* __restrict__ nprop, int32_t* __restrict__ prop_slot,
                                                                   float* __restrict__ params) {
  __shared__ float s_sc[TRK_MAX_BOXES];                                  // scores by union index
  __shared__ float s_x1[TRK_MAX_BOXES], s_y1[TRK_MAX_BOXES], s_x2[TRK_MAX_BOXES], s_y2[TRK_MAX_BOXES], s_ar[TRK_MAX_BOXES];  // by rank
  __shared__ int s_order[TRK_MAX_BOXES];                                 // rank -> union index (argsort(-scores, stable))
  __shared__ int s_keep[TRK_MAX_BOXES];                                  // kept list: ranks, in kept order
  __shared__ int s_slot[TRK_MAX_BOXES];                                  // the kept slots that hold propagated boxes
  __shared__ unsigned long long s_hit[TRK_MAX_BOXES * TRK_WORDS];        // row i: bit j set when box i suppresses box j > i
  __shared__ int s_cnt[2];                                               // kept, propagated among them
  const int tid = threadIdx.x;
  const int KK = K * 3;
  int M = count_prev ? *count_prev : 0;
  M = M < 0 ? 0 : (M > P ? P : M);

  if (M == 0) {                                      // no previous poses: the detector boxes as they are (no NMS, no cap)
    for (int s = tid; s < cap; s += TRK_THREADS) {
      for (int c = 0; c < 5; ++c) boxes[(size_t)s * 5 + c] = s < n ? dets[(size_t)s * 5 + c] : 0.f;
      src[s] = s < n ? s : -1;
    }
    for (int e = tid; e < cap * KK; e += TRK_THREADS) kps[e] = e < n * KK ? kp_det[e] : 0.f;
    for (int j = tid; j < bucket; j += TRK_THREADS) {
      prop_slot[j] = -1;
      params[(size_t)j * 3 + 0] = 0.f;
      params[(size_t)j * 3 + 1] = 0.f;
      params[(size_t)j * 3 + 2] = 1.f;
    }
    if (tid == 0) {
      *count = n;
      *nprop = 0;
    }
    return;
  }

  const int N = n + M, NW = (N + 63) >> 6;
  auto union_ptr = [&](int u) { return u < n ? dets + (size_t)u * 5 : prop_boxes + (size_t)(u - n) * 4; };
  for (int u = tid; u < N; u += TRK_THREADS) s_sc[u] = u < n ? dets[(size_t)u * 5 + 4] : prev_boxes[(size_t)(u - n) * 5 + 4];
  __syncthreads();
  // rank by counting = the stable descending argsort: boxes with a higher score, plus equal ones that come earlier
  for (int u = tid; u < N; u += TRK_THREADS) {
    const float s = s_sc[u];
    int r = 0;
    for (int v = 0; v < N; ++v) {
      const float sv = s_sc[v];
      r += (sv > s || (sv == s && v < u)) ? 1 : 0;
    }
    const float* b = union_ptr(u);
    const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
    s_x1[r] = x1; s_y1[r] = y1; s_x2[r] = x2; s_y2[r] = y2;
    s_ar[r] = (x2 - x1 + 1.f) * (y2 - y1 + 1.f);
    s_order[r] = u;
  }
  __syncthreads();
  // the pairwise hit mask in rank order, 64 columns per task; a wave's lanes share the word and take neighbouring rows
  for (int task = tid; task < NW * N; task += TRK_THREADS) {
    const int w = task / N, i = task - w * N;
    const int j0 = (w << 6) > i + 1 ? (w << 6) : i + 1, j1 = ((w + 1) << 6) < N ? ((w + 1) << 6) : N;
    const float x1 = s_x1[i], y1 = s_y1[i], x2 = s_x2[i], y2 = s_y2[i], ar = s_ar[i];
    unsigned long long bits = 0;
    for (int j = j0; j < j1; ++j) {
      const float iw = fmaxf(0.f, fminf(x2, s_x2[j]) - fmaxf(x1, s_x1[j]) + 1.f);
      const float ih = fmaxf(0.f, fminf(y2, s_y2[j]) - fmaxf(y1, s_y1[j]) + 1.f);
      const float inter = iw * ih;
      const float iou = inter / (ar + s_ar[j] - inter);
      if (iou >= thresh) bits |= 1ull << (j & 63);
    }
    s_hit[i * TRK_WORDS + w] = bits;
  }
  __syncthreads();
  // greedy walk by one wave: lane l < NW owns word l of the suppressed set, so a kept box ORs its whole row in one step and
  // the walk jumps from kept box to kept box (no workgroup barrier, no step for a suppressed box)
  if (tid < 64) {
    unsigned long long removed = 0;
    int cnt = 0;
    for (int w = 0; w < NW && cnt < max_keep; ++w) {
      const int left = N - (w << 6);
      unsigned long long open = left >= 64 ? ~0ull : ((1ull << left) - 1ull);   // positions of this word still to visit
      while (cnt < max_keep) {
        const unsigned long long avail = open & ~__shfl(removed, w, 64);
        if (!avail) break;
        const int b = __ffsll((long long)avail) - 1;
        const int i = (w << 6) + b;
        if (tid == 0) s_keep[cnt] = i;
        ++cnt;
        if (tid < NW) removed |= s_hit[i * TRK_WORDS + tid];
        open &= b == 63 ? 0ull : ~((2ull << b) - 1ull);
      }
    }
    if (tid == 0) {
      int np = 0;
      for (int s = 0; s < cnt; ++s)
        if (s_order[s_keep[s]] >= n) s_slot[np++] = s;
      s_cnt[0] = cnt;
      s_cnt[1] = np;
    }
  }
  __syncthreads();
  const int cnt = s_cnt[0], np = s_cnt[1];
  for (int s = tid; s < cap; s += TRK_THREADS) {
    float* o = boxes + (size_t)s * 5;
    if (s < cnt) {
      const int r = s_keep[s], u = s_order[r];
      o[0] = s_x1[r]; o[1] = s_y1[r]; o[2] = s_x2[r]; o[3] = s_y2[r]; o[4] = s_sc[u];
      src[s] = u;
    } else {
      o[0] = o[1] = o[2] = o[3] = o[4] = 0.f;
      src[s] = -1;
    }
  }
  for (int e = tid; e < cap * KK; e += TRK_THREADS) {
    const int s = e / KK;
    const int u = s < cnt ? s_order[s_keep[s]] : n;
    kps[e] = u < n ? kp_det[(size_t)u * KK + (e - s * KK)] : 0.f;
  }
  for (int j = tid; j < bucket; j += TRK_THREADS) {
    prop_slot[j] = j < np ? s_slot[j] : -1;
    float* o = params + (size_t)j * 3;
    if (np == 0) {
      o[0] = 0.f; o[1] = 0.f; o[2] = 1.f;
    } else {                                         // padding crops repeat row 0 (PoseRunner._fill_params)
      const int r = s_keep[s_slot[j < np ? j : 0]];
      double cx, cy, sc;
      trk_center_scale(s_x1[r], s_y1[r], s_x2[r], s_y2[r], rh, rw, cx, cy, sc);
      o[0] = (float)cx; o[1] = (float)cy; o[2] = (float)sc;
    }
  }
  if (tid == 0) {
    *count = cnt;
    *nprop = np;
  }
}

__global__ __launch_bounds__(TRK_THREADS) void track_place_rows_kernel(const float* __restrict__ rows, const float* __restrict__ boxes,
                                                                       const int32_t* __restrict__ prop_slot, const int32_t* __restrict__ nprop,
                                                                       int bucket, int cap, int K, int h, int w, int rh, int rw,
                                                                       float* __restrict__ kps) {
  int np = *nprop;
  np = np < 0 ? 0 : (np > bucket ? bucket : np);
  const double hx = 0.5 * (double)w, hy = 0.5 * (double)h;
  for (int e = threadIdx.x; e < np * K; e += TRK_THREADS) {
    const int j = e / K, k = e - j * K;
    const int slot = prop_slot[j];
    if (slot < 0 || slot >= cap) continue;
    const float* b = boxes + (size_t)slot * 5;
    double cx, cy, sc;
    trk_center_scale(b[0], b[1], b[2], b[3], rh, rw, cx, cy, sc);
    const double g = sc / (double)h;                 // heatmap_rows_to_image: (x - w / 2) * scale / h + cx
    const float* r = rows + ((size_t)j * K + k) * 3;
    float* o = kps + ((size_t)slot * K + k) * 3;
    o[0] = (float)(((double)r[0] - hx) * g + cx);
    o[1] = (float)(((double)r[1] - hy) * g + cy);
    o[2] = r[2];
  }
}

}  // namespace ft

using namespace ft;

extern "C" int ft_track_propagate(const float* kps_prev, const float* flow, int H, int W, const double* older_in, int n_old, int P,
                                  int K, double* moved_out, float* boxes_out, ft_stream_t stream) {
  if (!kps_prev || !flow || !moved_out || !boxes_out || H <= 0 || W <= 0 || P <= 0 || K <= 0 || n_old < 0 || (n_old > 0 && !older_in))
    return FT_ERR_INVALID_ARG;
  if ((long long)(1 + n_old) * P * K > (1 << 24)) return FT_ERR_UNSUPPORTED;     // one workgroup: tens of poses, not a batch op
  hipLaunchKernelGGL(track_propagate_kernel, dim3(1), dim3(TRK_THREADS), 0, as_stream(stream), kps_prev, flow, H, W, older_in, n_old,
                     P, K, moved_out, boxes_out);
  FT_LAUNCH_CHECK("track_propagate_kernel");
  return FT_OK;
}

extern "C" int ft_track_select(const float* dets, const float* kp_det, int n, const float* prop_boxes, const float* prev_boxes, int P,
                               const int32_t* count_prev, int K, float thresh, int max_keep, int cap, int rh, int rw, int bucket,
                               float* boxes, int32_t* src, int32_t* count, float* kps, int32_t* nprop, int32_t* prop_slot,
                               float* params, ft_stream_t stream) {
  if (n < 0 || P < 0 || K <= 0 || cap <= 0 || max_keep <= 0 || max_keep > cap || n > cap || rh <= 0 || rw <= 0 || bucket <= 0 ||
      !boxes || !src || !count || !kps || !nprop || !prop_slot || !params || (n > 0 && (!dets || !kp_det)) ||
      (count_prev && P > 0 && (!prop_boxes || !prev_boxes)))
    return FT_ERR_INVALID_ARG;
  if (n + P > TRK_MAX_BOXES || K > TRK_MAX_K || bucket < (cap < P ? cap : P)) return FT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(track_select_kernel, dim3(1), dim3(TRK_THREADS), 0, as_stream(stream), dets, kp_det, n, prop_boxes, prev_boxes, P,
                     count_prev, K, thresh, max_keep, cap, rh, rw, bucket, boxes, src, count, kps, nprop, prop_slot, params);
  FT_LAUNCH_CHECK("track_select_kernel");
  return FT_OK;
}

extern "C" int ft_track_place_rows(const float* rows, const float* boxes, const int32_t* prop_slot, const int32_t* nprop, int bucket,
                                   int cap, int K, int h, int w, int rh, int rw, float* kps, ft_stream_t stream) {
  if (!rows || !boxes || !prop_slot || !nprop || !kps || bucket <= 0 || cap <= 0 || K <= 0 || h <= 0 || w <= 0 || rh <= 0 || rw <= 0)
    return FT_ERR_INVALID_ARG;
  if (K > TRK_MAX_K) return FT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(track_place_rows_kernel, dim3(1), dim3(TRK_THREADS), 0, as_stream(stream), rows, boxes, prop_slot, nprop, bucket,
                     cap, K, h, w, rh, rw, kps);
  FT_LAUNCH_CHECK("track_place_rows_kernel");
  return FT_OK;
}
