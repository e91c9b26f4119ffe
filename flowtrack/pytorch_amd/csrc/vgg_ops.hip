// The two kernels the VGG16 trunk of the Faster R-CNN detector adds (reference lib/detection: nets/vgg16.py, torchvision's VGG
// config D behind it):
//   ft_maxpool2x2s2_fwd   nn.MaxPool2d(2, 2) of `vgg.features` on dense NHWC maps (floor mode: the last row / column of an odd map
//                         is never read)
//   ft_fc_fwd             `vgg.classifier.0` / `.3` (nets/vgg16.py:46-50): y[R, N] = act(x[R, K] . W[N, K]^T + bias[N]) on a few hundred
//                         RoI rows, as a weight-streaming split-K GEMM (ft_fc_pack, ft_fc_supported, ft_fc_workspace_bytes with it)
//                         Measured at 300 rows it is slower than ft_conv2d_fwd on the [rows,1,1,K] view (138 against 115 us at
//                         K = 25088, 38 against 33 us at K = 4096: profiles/README.md), so it is declared under FT_EXPERIMENTAL
//                         and detection.nets.vgg16 records it as the second option.
// Device safety, as detect_net_ops.hip: every address is formed from kernel arguments and clamped indices only; no kernel reads an
// index from device data, loops on device data or waits on another workgroup.  A refused call launches nothing; zero rows return
// FT_OK without a launch.
#include "ft_common.h"

namespace ft {

constexpr int VG_THREADS = 256;
constexpr long long VG_MAX_ELEMS = 1ll << 31;        // element counts stay below this: every flat index fits an int

static inline bool vg_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline unsigned vg_blocks(long long total) { return (unsigned)((total + VG_THREADS - 1) / VG_THREADS); }

// ---- MaxPool2d(2, 2), NHWC --------------------------------------------------------------------------------------------------
// One thread per (output pixel, 16-byte piece of C): four independent 16-byte loads (neighbouring threads read neighbouring
// pieces), the max of the four values themselves (no initial value: an all-negative window gives its negative max; a NaN in the
// window stays, as nn.MaxPool2d keeps it), one 16-byte store.  The output is one of the inputs: bit-exact.
template <typename T> struct vg_piece;
template <> struct vg_piece<half_t> { typedef half8_t type; static constexpr int N = 8; };
template <> struct vg_piece<float> { typedef float4_t type; static constexpr int N = 4; };

template <typename T>
__global__ __launch_bounds__(VG_THREADS) void maxpool2x2s2_kernel(const T* __restrict__ x, T* __restrict__ y, int Hi, int Wi, int Ho,
                                                                  int Wo, int C, int total) {
  typedef typename vg_piece<T>::type piece_t;
  constexpr int E = vg_piece<T>::N;
  const int idx = blockIdx.x * VG_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int pieces = C / E;
  const int v = idx % pieces;
  int t = idx / pieces;
  const int ox = t % Wo;
  t /= Wo;
  const int oy = t % Ho;
  const int n = t / Ho;
  const T* src = x + (((size_t)n * Hi + 2 * oy) * Wi + 2 * ox) * C + (size_t)v * E;
  const piece_t a = *reinterpret_cast<const piece_t*>(src);
  const piece_t b = *reinterpret_cast<const piece_t*>(src + C);
  const piece_t c = *reinterpret_cast<const piece_t*>(src + (size_t)Wi * C);
  const piece_t d = *reinterpret_cast<const piece_t*>(src + (size_t)Wi * C + C);
  piece_t m = a;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    m[e] = (b[e] > m[e] || b[e] != b[e]) ? b[e] : m[e];
    m[e] = (c[e] > m[e] || c[e] != c[e]) ? c[e] : m[e];
    m[e] = (d[e] > m[e] || d[e] != d[e]) ? d[e] : m[e];
  }
  *reinterpret_cast<piece_t*>(y + (size_t)idx * E) = m;
}

// ---- fully connected layer --------------------------------------------------------------------------------------------------
// Shape of the work: R <= ~300 rows, N = 4096 outputs, K = 25088 or 4096: the weights (205 MB / 34 MB of fp16) are read once and
// are most of the bytes.  A workgroup (four waves, 2 x 2) owns 128 outputs x all rows of a chunk x one slice of K:
//   * the weights come packed in the order a wave reads them (ft_fc_pack): per 32 outputs and 64-wide K-step one 4 KB block,
//     lane (r, h) = (lane & 31, lane >> 5) holding W[g * 32 + r][t * 64 + 32 h + 0..31] as 64 contiguous bytes.  They go straight
//     to registers, four 16-byte loads per lane and block; the two waves that share 64 outputs read the same lines (L1 / L2).
//   * the rows' K-step [rows, 64] is staged through LDS (global -> registers while the previous step computes, then LDS);
//     lane (r, h) reads row r at 32 h + 8 s for MFMA step s, so both operands of mfma_f32_32x32x16_f16 see K in the same order.
//   * fp32 accumulators, written as the slice's slab [slice][R][N] into the caller's workspace with plain stores.
// fc_reduce_kernel (the second launch) sums the slabs in slice order, adds the bias, applies the activation and rounds once to
// fp16: the same bits on every call.  Block b = tile * ksplit + slice: with ksplit = 8 all tiles of a slice sit on one XCD,
// whose L2 then holds the slice of x they share.
constexpr int FC_BK = 64;                 // halves per K-step
constexpr int FC_BN = 128;                // outputs per workgroup (64 per wave)
constexpr int FC_LDS_ROW = FC_BK + 8;     // halves per staged row: 144 bytes, 16-byte aligned, rows spread over the banks
constexpr int FC_MT_BIG = 5;              // 32-row accumulator tiles per wave: 2 x 5 x 32 = 320 rows per workgroup
constexpr int FC_MAX_KSPLIT = 64;
constexpr int FC_TARGET_WGS = 256;        // one workgroup per CU

struct fc_plan {
  int mt, row_chunks, ntiles, steps, sps, ksplit;
};

static inline fc_plan fc_plan_for(int R, int K, int N) {
  fc_plan p;
  p.mt = R <= 64 ? 1 : FC_MT_BIG;
  const int rb = 64 * p.mt;
  p.row_chunks = (R + rb - 1) / rb;
  p.ntiles = (N + FC_BN - 1) / FC_BN;
  p.steps = K / FC_BK;
  int want = FC_TARGET_WGS / (p.ntiles * p.row_chunks);
  want = want < 1 ? 1 : (want > FC_MAX_KSPLIT ? FC_MAX_KSPLIT : want);
  want = want > p.steps ? p.steps : want;
  p.sps = (p.steps + want - 1) / want;              // K-steps per slice; the last slice may be shorter, none is empty
  p.ksplit = (p.steps + p.sps - 1) / p.sps;
  return p;
}

__global__ __launch_bounds__(VG_THREADS) void fc_pack_kernel(const half_t* __restrict__ w, half_t* __restrict__ wp, int K, long long pieces) {
  // one thread per 16-byte piece of the packed buffer: [group g][step t][lane][4 pieces]
  const long long idx = (long long)blockIdx.x * VG_THREADS + threadIdx.x;
  if (idx >= pieces) return;
  const int q = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
  const long long blk = idx >> 8;
  const int steps = K / FC_BK;
  const int t = (int)(blk % steps);
  const long long g = blk / steps;
  const int r = lane & 31, h = lane >> 5;
  const half_t* src = w + (size_t)(g * 32 + r) * K + (size_t)t * FC_BK + 32 * h + 8 * q;
  *reinterpret_cast<half8_t*>(wp + (size_t)idx * 8) = *reinterpret_cast<const half8_t*>(src);
}

template <int MT>
__global__ __launch_bounds__(VG_THREADS) void fc_slab_kernel(const half_t* __restrict__ x, int x_stride, const half_t* __restrict__ wp,
                                                             float* __restrict__ slab, int R, int K, int N, int ksplit, int sps) {
  constexpr int RB = 64 * MT;             // rows per workgroup
  constexpr int XP = RB / 32;             // 16-byte pieces of the staged step per thread
  __shared__ __attribute__((aligned(16))) half_t xs[RB * FC_LDS_ROW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int tile = blockIdx.x / ksplit, ks = blockIdx.x - tile * ksplit;
  const int row0 = blockIdx.y * RB;
  const int steps = K / FC_BK;
  const int t0 = ks * sps, t1 = (t0 + sps < steps) ? t0 + sps : steps;
  const int n0 = tile * FC_BN + wn * 64;
  const bool active = n0 < N;             // (wave-uniform; N % 64 == 0: an active wave owns 64 whole outputs)

  float16_t acc[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // staging addresses: piece p = tid + q * 256 of the step is row p >> 3, halves 8 (p & 7) ..; rows past R read row R - 1 (their
  // results are never stored)
  const half_t* xsrc[XP];
  int xdst[XP];
#pragma unroll
  for (int q = 0; q < XP; ++q) {
    const int p = tid + q * VG_THREADS;
    const int row = p >> 3, c = p & 7;
    int grow = row0 + row;
    grow = grow < R ? grow : R - 1;
    xsrc[q] = x + (size_t)grow * x_stride + c * 8;
    xdst[q] = row * FC_LDS_ROW + c * 8;
  }
  const size_t wblock = (size_t)64 * 32;                                  // halves per packed block
  const half_t* wsrc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int g = active ? n0 / 32 + j : 0;
    wsrc[j] = wp + ((size_t)g * steps) * wblock + (size_t)lane * 32;
  }

  half8_t xr[XP], wr[2][4];
#pragma unroll
  for (int q = 0; q < XP; ++q) xr[q] = *reinterpret_cast<const half8_t*>(xsrc[q] + (size_t)t0 * FC_BK);
  if (active) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int s = 0; s < 4; ++s) wr[j][s] = *reinterpret_cast<const half8_t*>(wsrc[j] + (size_t)t0 * wblock + s * 8);
  }
  for (int t = t0; t < t1; ++t) {
    __syncthreads();                      // the previous step's LDS reads are done
#pragma unroll
    for (int q = 0; q < XP; ++q) *reinterpret_cast<half8_t*>(xs + xdst[q]) = xr[q];
    half8_t wc[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int s = 0; s < 4; ++s) wc[j][s] = wr[j][s];
    __syncthreads();
    if (t + 1 < t1) {                     // the next step's operands travel while this one computes
#pragma unroll
      for (int q = 0; q < XP; ++q) xr[q] = *reinterpret_cast<const half8_t*>(xsrc[q] + (size_t)(t + 1) * FC_BK);
      if (active) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int s = 0; s < 4; ++s) wr[j][s] = *reinterpret_cast<const half8_t*>(wsrc[j] + (size_t)(t + 1) * wblock + s * 8);
      }
    }
    if (active) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const half8_t a = *reinterpret_cast<const half8_t*>(xs + ((wm * MT + i) * 32 + r) * FC_LDS_ROW + 32 * h + 8 * s);
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, wc[j][s], acc[i][j], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
  // accumulator register e of lane (r, h): row (e & 3) + 8 (e >> 2) + 4 h, column r of the 32 x 32 tile
  float* out = slab + (size_t)ks * R * N;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = row0 + (wm * MT + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (row < R) {
#pragma unroll
        for (int j = 0; j < 2; ++j) out[(size_t)row * N + n0 + j * 32 + r] = acc[i][j][e];
      }
    }
  }
}

// One thread per four neighbouring outputs of a row: the slabs' 16-byte pieces in slice order, + bias, activation, one 8-byte store.
__global__ __launch_bounds__(VG_THREADS) void fc_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bias,
                                                               half_t* __restrict__ y, int y_stride, int R, int N, int ksplit, int relu) {
  const int idx = blockIdx.x * VG_THREADS + threadIdx.x;
  const int quads = N / 4;
  if (idx >= R * quads) return;
  const int row = idx / quads, n = (idx - row * quads) * 4;
  const size_t at = (size_t)row * N + n, slice = (size_t)R * N;
  float4_t s = *reinterpret_cast<const float4_t*>(slab + at);
  for (int k = 1; k < ksplit; ++k) s = s + *reinterpret_cast<const float4_t*>(slab + (size_t)k * slice + at);
  if (bias) s = s + *reinterpret_cast<const float4_t*>(bias + n);
  half4_t o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (half_t)(relu ? act_mul(s[e], 0.f) : s[e]);
  *reinterpret_cast<half4_t*>(y + (size_t)row * y_stride + n) = o;
}

static int fc_check(int dtype, int R, int K, int N, int x_stride, int y_stride) {
  if (dtype != FT_F16 && dtype != FT_F32) return FT_ERR_INVALID_ARG;
  if (R < 0 || K <= 0 || N <= 0 || x_stride < K || y_stride < N || x_stride % 8 || y_stride % 8) return FT_ERR_INVALID_ARG;
  if (dtype == FT_F32 || K % FC_BK || N % 64) return FT_ERR_UNSUPPORTED;
  if ((long long)N * K >= VG_MAX_ELEMS || (long long)R * x_stride >= VG_MAX_ELEMS || (long long)R * y_stride >= VG_MAX_ELEMS ||
      (long long)FC_MAX_KSPLIT * R * N >= VG_MAX_ELEMS)
    return FT_ERR_UNSUPPORTED;
  return FT_OK;
}

}  // namespace ft

using namespace ft;

extern "C" int ft_maxpool2x2s2_fwd(const void* x, void* y, int N, int Hi, int Wi, int C, int dtype, ft_stream_t stream) {
  if (!x || !y || N <= 0 || Hi < 2 || Wi < 2 || C <= 0 || C % 8 || (dtype != FT_F16 && dtype != FT_F32) || !vg_aligned16(x) ||
      !vg_aligned16(y))
    return FT_ERR_INVALID_ARG;
  if ((long long)N * Hi * Wi * C >= VG_MAX_ELEMS) return FT_ERR_UNSUPPORTED;
  const int Ho = Hi / 2, Wo = Wi / 2;
  const long long total = (long long)N * Ho * Wo * (C / (dtype == FT_F16 ? 8 : 4));
  if (dtype == FT_F16)
    hipLaunchKernelGGL(maxpool2x2s2_kernel<half_t>, dim3(vg_blocks(total)), dim3(VG_THREADS), 0, as_stream(stream),
                       static_cast<const half_t*>(x), static_cast<half_t*>(y), Hi, Wi, Ho, Wo, C, (int)total);
  else
    hipLaunchKernelGGL(maxpool2x2s2_kernel<float>, dim3(vg_blocks(total)), dim3(VG_THREADS), 0, as_stream(stream),
                       static_cast<const float*>(x), static_cast<float*>(y), Hi, Wi, Ho, Wo, C, (int)total);
  FT_LAUNCH_CHECK("maxpool2x2s2_kernel");
  return FT_OK;
}

extern "C" int ft_fc_supported(int dtype, int R, int K, int N, int x_stride, int y_stride) {
  return fc_check(dtype, R, K, N, x_stride, y_stride);
}

extern "C" long long ft_fc_workspace_bytes(int R, int K, int N) {
  if (R <= 0 || fc_check(FT_F16, R, K, N, K, N) != FT_OK) return 0;
  return 4ll * fc_plan_for(R, K, N).ksplit * R * N;
}

extern "C" int ft_fc_pack(const void* w, int N, int K, void* wpack, ft_stream_t stream) {
  if (!w || !wpack || !vg_aligned16(w) || !vg_aligned16(wpack) || N <= 0 || K <= 0) return FT_ERR_INVALID_ARG;
  if (K % FC_BK || N % 64 || (long long)N * K >= VG_MAX_ELEMS) return FT_ERR_UNSUPPORTED;
  const long long pieces = (long long)N * K / 8;
  hipLaunchKernelGGL(fc_pack_kernel, dim3(vg_blocks(pieces)), dim3(VG_THREADS), 0, as_stream(stream), static_cast<const half_t*>(w),
                     static_cast<half_t*>(wpack), K, pieces);
  FT_LAUNCH_CHECK("fc_pack_kernel");
  return FT_OK;
}

extern "C" int ft_fc_fwd(int dtype, const void* x, int x_stride, const void* wpack, const float* bias, void* y, int y_stride, int R,
                         int K, int N, int act, void* workspace, size_t workspace_bytes, ft_stream_t stream) {
  const int st = fc_check(dtype, R, K, N, x_stride, y_stride);
  if (st != FT_OK) return st;
  if (act != FT_ACT_NONE && act != FT_ACT_RELU) return FT_ERR_INVALID_ARG;
  if (R == 0) return FT_OK;
  if (!x || !wpack || !y || !workspace || !vg_aligned16(x) || !vg_aligned16(wpack) || !vg_aligned16(y) || !vg_aligned16(workspace) ||
      (bias && !vg_aligned16(bias)))
    return FT_ERR_INVALID_ARG;
  const fc_plan p = fc_plan_for(R, K, N);
  if (workspace_bytes < (size_t)4 * p.ksplit * R * N) return FT_ERR_INVALID_ARG;
  const dim3 grid((unsigned)(p.ntiles * p.ksplit), (unsigned)p.row_chunks);
  if (p.mt == 1)
    hipLaunchKernelGGL(fc_slab_kernel<1>, grid, dim3(VG_THREADS), 0, as_stream(stream), static_cast<const half_t*>(x), x_stride,
                       static_cast<const half_t*>(wpack), static_cast<float*>(workspace), R, K, N, p.ksplit, p.sps);
  else
    hipLaunchKernelGGL(fc_slab_kernel<FC_MT_BIG>, grid, dim3(VG_THREADS), 0, as_stream(stream), static_cast<const half_t*>(x), x_stride,
                       static_cast<const half_t*>(wpack), static_cast<float*>(workspace), R, K, N, p.ksplit, p.sps);
  FT_LAUNCH_CHECK("fc_slab_kernel");
  hipLaunchKernelGGL(fc_reduce_kernel, dim3(vg_blocks((long long)R * (N / 4))), dim3(VG_THREADS), 0, as_stream(stream),
                     static_cast<const float*>(workspace), bias, static_cast<half_t*>(y), y_stride, R, N, p.ksplit,
                     act == FT_ACT_RELU ? 1 : 0);
  FT_LAUNCH_CHECK("fc_reduce_kernel");
  return FT_OK;
}
