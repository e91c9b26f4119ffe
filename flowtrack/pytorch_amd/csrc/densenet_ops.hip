// The one kernel the DenseNet trunks of the FPN pose model add (reference lib/pose/models/densenet.py:19-36, 47-54):
//   ft_preact_conv1x1_fwd   y = act(post_scale * (W . relu(pre_scale * x + pre_shift)) + post_shift), a 1x1 conv whose INPUT goes
//                           through a per-channel affine + ReLU on its way into the GEMM (and, pool = 1, through the 2x2 average of
//                           the transition layers, which commutes with the 1x1 conv), with the ordinary scale / shift / activation
//                           epilogue behind it.  hip_ops.pack_preact_weights builds its weight operand.
// A dense layer's first BatchNorm belongs to the CONSUMER and runs over the whole concatenated input, so no producer's epilogue can
// carry it; unfused, the activated copy of the block's buffer is written and read again by every layer.
//
// fp16 (preact_f16_kernel).  The work is bound by the bytes of x: K = 64..1000 against N = 128 outputs.  A wave owns 32 output pixels
// and 32 TN outputs; it reads its pixels' channels straight from global memory into the B operand of mfma_f32_32x32x16_f16 (lane
// (r, h) = (lane & 31, lane >> 5) holds pixel r, channels 64 c + 32 h + 8 s .. + 7 for step s of chunk c: 64 contiguous bytes per
// lane and chunk, four 16-byte loads), applies the affine + ReLU (+ the average of the four source pixels) in fp32 registers and
// rounds once.  No wave reads another wave's pixels, so x never passes through LDS.  The weights do: they come packed in operand
// order ([group g of 32 outputs][chunk c][step s][lane][8], one 4 KB block per (g, c): lane (r, h) holds W[32 g + r][64 c + 32 h + 8 s ..], zeros past Cin),
// the workgroup copies its TN blocks of a chunk to LDS with one linear 16-byte copy per thread and piece, and every wave reads them
// back lane-contiguous (no bank conflicts).  The next chunk's x pieces and weight pieces travel while this chunk multiplies.
// The accumulator of lane (r, h) holds pixel r, outputs 32 g + 8 q + 4 h + {0..3} in registers 4 q .. 4 q + 3: four 8-byte stores.
// Shapes of workgroup: 4 waves x (32 pixels, 128 outputs) where there are pixels enough to fill the chip that
// way — x is then read exactly once; 1 wave x (32 pixels, 32 outputs) for the late dense blocks, whose few pixel tiles would leave
// most CUs idle (x is read Cout / 32 times there, from L2: at 3072 pixels the whole map is 6 MB).  A pooled launch off the first
// shape shares its operand (four loads and four affines per element) among 128 outputs: 1 wave x (32 pixels, 128 outputs).
//
// fp32 (preact_f32_kernel): the parity mode.  32 pixels x 32 outputs per workgroup, both operands through LDS, one fmaf per
// product in ascending channel order.
//
// Channels at or above Cin of a pixel are never loaded into an operand: a piece past Cin is replaced by zeros after its (clamped,
// in-bounds) load, so whatever later layers of the block wrote there — a NaN included — contributes nothing.
// Device safety, as vgg_ops.hip: every address is formed from kernel arguments and clamped indices only; no kernel reads an index
// from device data, loops on device data or waits on another workgroup.  A refused call launches nothing.
#include "ft_common.h"

namespace ft {

constexpr int PA_BK = 64;                     // fp16: channels per chunk
constexpr int PA_BLOCK = 32 * PA_BK;          // halves per packed (32 outputs, chunk) block
constexpr long long PA_MAX_PIX = 1ll << 31;
constexpr int PA_BIG_MIN_WGS = 256;           // the 4-wave shape needs at least one workgroup per CU

static inline bool pa_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

struct pa_args {
  const void* x;
  const void* w;
  const float* pre_scale;
  const float* pre_shift;
  const float* post_scale;
  const float* post_shift;
  void* y;
  int H, W, Ho, Wo;          // source and output map (Ho = H, Wo = W without the pool)
  int npix;                  // N * Ho * Wo output pixels
  int Cin, x_cstride, x_coff, Cout, y_cstride, y_coff, pool, relu;
};

// element offset of output pixel `pix`'s (first) source pixel
__device__ __forceinline__ size_t pa_src_pixel(const pa_args& a, int pix) {
  if (!a.pool) return (size_t)pix;
  const int ox = pix % a.Wo;
  const int t = pix / a.Wo;
  const int oy = t % a.Ho, n = t / a.Ho;
  return ((size_t)n * a.H + 2 * oy) * a.W + 2 * ox;
}

__device__ __forceinline__ float pa_relu_fma(float x, float s, float b) { return act_mul(__builtin_fmaf(s, x, b), 0.f); }

template <int TN, int WAVES, bool POOL>
__global__ __launch_bounds__(64 * WAVES) void preact_f16_kernel(const pa_args a) {
  constexpr int THREADS = 64 * WAVES;
  constexpr int WPIECES = TN * (PA_BLOCK / 8);      // 16-byte pieces of the workgroup's weights per chunk
  constexpr int WPT = WPIECES / THREADS;
  static_assert(WPIECES % THREADS == 0, "weight pieces must divide over the threads");
  __shared__ __attribute__((aligned(16))) half8_t wl[WPIECES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int pix = (blockIdx.x * WAVES + wave) * 32 + r;
  const bool live = pix < a.npix;
  const int chunks = (a.Cin + PA_BK - 1) / PA_BK;
  const int g0 = blockIdx.y * TN;

  const half_t* x = static_cast<const half_t*>(a.x);
  const half_t* src = x + pa_src_pixel(a, live ? pix : a.npix - 1) * (size_t)a.x_cstride + a.x_coff;
  const size_t dx = (size_t)a.x_cstride, dy = (size_t)a.W * a.x_cstride;
  const half_t* wp = static_cast<const half_t*>(a.w);

  float16_t acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

  constexpr int NSRC = POOL ? 4 : 1;
  half8_t xr[NSRC][4], wr[WPT];
  auto fetch = [&](int c) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      int k0 = c * PA_BK + 32 * h + 8 * s;
      k0 = k0 < a.Cin ? k0 : 0;           // a piece past Cin: a clamped load, replaced by zeros below
      xr[0][s] = *reinterpret_cast<const half8_t*>(src + k0);
      if constexpr (POOL) {
        xr[1][s] = *reinterpret_cast<const half8_t*>(src + dx + k0);
        xr[2][s] = *reinterpret_cast<const half8_t*>(src + dy + k0);
        xr[3][s] = *reinterpret_cast<const half8_t*>(src + dy + dx + k0);
      }
    }
#pragma unroll
    for (int q = 0; q < WPT; ++q) {
      const int p = tid + q * THREADS;
      const int j = p / (PA_BLOCK / 8), within = p % (PA_BLOCK / 8);
      wr[q] = *reinterpret_cast<const half8_t*>(wp + ((size_t)(g0 + j) * chunks + c) * PA_BLOCK + (size_t)within * 8);
    }
  };

  fetch(0);
  for (int c = 0; c < chunks; ++c) {
    __syncthreads();                      // the previous chunk's LDS reads are done
#pragma unroll
    for (int q = 0; q < WPT; ++q) wl[tid + q * THREADS] = wr[q];
    // the B operand: affine + ReLU (+ the 2x2 average) in fp32, one rounding
    half8_t op[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int kk = c * PA_BK + 32 * h + 8 * s;
      const bool ok = kk < a.Cin;
      const int k0 = ok ? kk : 0;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float4_t sc = *reinterpret_cast<const float4_t*>(a.pre_scale + k0 + 4 * q);
        const float4_t sh = *reinterpret_cast<const float4_t*>(a.pre_shift + k0 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * q + e;
          float v = pa_relu_fma((float)xr[0][s][i], sc[e], sh[e]);
          if constexpr (POOL) {
            const float r01 = pa_relu_fma((float)xr[1][s][i], sc[e], sh[e]);
            const float r10 = pa_relu_fma((float)xr[2][s][i], sc[e], sh[e]);
            const float r11 = pa_relu_fma((float)xr[3][s][i], sc[e], sh[e]);
            v = 0.25f * ((v + r01) + (r10 + r11));
          }
          op[s][i] = ok ? (half_t)v : (half_t)0.f;
        }
      }
    }
    __syncthreads();
    if (c + 1 < chunks) fetch(c + 1);     // the next chunk travels while this one multiplies
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[j * (PA_BLOCK / 8) + s * 64 + lane], op[s], acc[j], 0, 0, 0);
  }
  if (!live) return;
  // register e of lane (r, h): output (e & 3) + 8 (e >> 2) + 4 h of the group, pixel r
  half_t* y = static_cast<half_t*>(a.y) + (size_t)pix * a.y_cstride + a.y_coff;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = (g0 + j) * 32 + 8 * q + 4 * h;
      float4_t v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = acc[j][4 * q + e];
      if (a.post_scale) {
        const float4_t sc = *reinterpret_cast<const float4_t*>(a.post_scale + n);
        const float4_t sh = *reinterpret_cast<const float4_t*>(a.post_shift + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(sc[e], v[e], sh[e]);
      }
      half4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (half_t)(a.relu ? act_mul(v[e], 0.f) : v[e]);
      *reinterpret_cast<half4_t*>(y + n) = o;
    }
  }
}

// fp32: 256 threads, 32 pixels x 32 outputs, chunks of 32 channels.  Thread t stages one 16-byte piece of each operand (pixel or
// output t >> 3, channels 4 (t & 7) ..) and accumulates pixel t & 31, outputs 4 (t >> 5) .. + 3.
constexpr int PF_BK = 32;
constexpr int PF_ROW = PF_BK + 1;         // floats per staged row: the 32 pixels of a wave hit 32 different banks

__global__ __launch_bounds__(256) void preact_f32_kernel(const pa_args a) {
  __shared__ float as[32 * PF_ROW], ws[32 * PF_ROW];
  const int tid = threadIdx.x;
  const int lrow = tid >> 3, lk = 4 * (tid & 7);
  const int p = tid & 31, ng = tid >> 5;
  const int pix0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  const int lpix = pix0 + lrow < a.npix ? pix0 + lrow : a.npix - 1;
  const float* x = static_cast<const float*>(a.x);
  const float* src = x + pa_src_pixel(a, lpix) * (size_t)a.x_cstride + a.x_coff;
  const size_t dx = (size_t)a.x_cstride, dy = (size_t)a.W * a.x_cstride;
  const float* wrow = static_cast<const float*>(a.w) + (size_t)(n0 + lrow) * a.Cin;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int kc = 0; kc < a.Cin; kc += PF_BK) {
    const bool ok = kc + lk < a.Cin;      // (Cin % 4 == 0: a piece is inside or outside as a whole)
    const int k0 = ok ? kc + lk : 0;
    const float4_t sc = *reinterpret_cast<const float4_t*>(a.pre_scale + k0), sh = *reinterpret_cast<const float4_t*>(a.pre_shift + k0);
    const float4_t x00 = *reinterpret_cast<const float4_t*>(src + k0);
    float4_t v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = pa_relu_fma(x00[e], sc[e], sh[e]);
    if (a.pool) {
      const float4_t x01 = *reinterpret_cast<const float4_t*>(src + dx + k0);
      const float4_t x10 = *reinterpret_cast<const float4_t*>(src + dy + k0);
      const float4_t x11 = *reinterpret_cast<const float4_t*>(src + dy + dx + k0);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        v[e] = 0.25f * ((v[e] + pa_relu_fma(x01[e], sc[e], sh[e])) + (pa_relu_fma(x10[e], sc[e], sh[e]) + pa_relu_fma(x11[e], sc[e], sh[e])));
    }
    const float4_t wv = *reinterpret_cast<const float4_t*>(wrow + k0);
    __syncthreads();                      // the previous chunk's reads are done
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      as[lrow * PF_ROW + lk + e] = ok ? v[e] : 0.f;
      ws[lrow * PF_ROW + lk + e] = ok ? wv[e] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < PF_BK; ++k) {
      const float av = as[p * PF_ROW + k];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(av, ws[(ng * 4 + j) * PF_ROW + k], acc[j]);
    }
  }
  const int pix = pix0 + p;
  if (pix >= a.npix) return;
  const int n = n0 + ng * 4;
  float4_t o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float v = acc[j];
    if (a.post_scale) v = __builtin_fmaf(a.post_scale[n + j], v, a.post_shift[n + j]);
    o[j] = a.relu ? act_mul(v, 0.f) : v;
  }
  *reinterpret_cast<float4_t*>(static_cast<float*>(a.y) + (size_t)pix * a.y_cstride + a.y_coff + n) = o;
}

static int pa_check(int dtype, int N, int H, int W, int Cin, int x_cstride, int x_coff, int Cout, int y_cstride, int y_coff, int pool, int act) {
  if (dtype != FT_F16 && dtype != FT_F32) return FT_ERR_INVALID_ARG;
  if (act != FT_ACT_NONE && act != FT_ACT_RELU) return FT_ERR_INVALID_ARG;
  if (pool != 0 && pool != 1) return FT_ERR_INVALID_ARG;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || x_coff < 0 || y_coff < 0) return FT_ERR_INVALID_ARG;
  if (x_cstride < x_coff + Cin || y_cstride < y_coff + Cout) return FT_ERR_INVALID_ARG;
  const int G = dtype == FT_F16 ? 8 : 4;
  if (Cout % 32 || Cin % G || x_coff % G || y_coff % G || x_cstride % G || y_cstride % G) return FT_ERR_UNSUPPORTED;
  if (pool && (H < 2 || W < 2)) return FT_ERR_UNSUPPORTED;
  if ((long long)N * H * W >= PA_MAX_PIX) return FT_ERR_UNSUPPORTED;
  return FT_OK;
}

}  // namespace ft

using namespace ft;

extern "C" int ft_preact_conv1x1_fwd(const void* x, const void* w, const float* pre_scale, const float* pre_shift, const float* post_scale,
                                     const float* post_shift, void* y, int dtype, int N, int H, int W, int Cin, int x_cstride, int x_coff,
                                     int Cout, int y_cstride, int y_coff, int pool, int act, ft_stream_t stream) {
  if (!x || !w || !pre_scale || !pre_shift || !y || (post_scale == nullptr) != (post_shift == nullptr)) return FT_ERR_INVALID_ARG;
  const int st = pa_check(dtype, N, H, W, Cin, x_cstride, x_coff, Cout, y_cstride, y_coff, pool, act);
  if (st != FT_OK) return st;
  if (!pa_aligned16(x) || !pa_aligned16(w) || !pa_aligned16(y) || !pa_aligned16(pre_scale) || !pa_aligned16(pre_shift) ||
      (post_scale && (!pa_aligned16(post_scale) || !pa_aligned16(post_shift))))
    return FT_ERR_INVALID_ARG;
  pa_args a;
  a.x = x; a.w = w; a.pre_scale = pre_scale; a.pre_shift = pre_shift; a.post_scale = post_scale; a.post_shift = post_shift; a.y = y;
  a.H = H; a.W = W; a.Ho = pool ? H / 2 : H; a.Wo = pool ? W / 2 : W;
  a.npix = N * a.Ho * a.Wo;
  a.Cin = Cin; a.x_cstride = x_cstride; a.x_coff = x_coff; a.Cout = Cout; a.y_cstride = y_cstride; a.y_coff = y_coff;
  a.pool = pool; a.relu = act == FT_ACT_RELU ? 1 : 0;
  const unsigned tiles32 = (unsigned)((a.npix + 31) / 32);
  if (dtype == FT_F32) {
    hipLaunchKernelGGL(preact_f32_kernel, dim3(tiles32, (unsigned)(Cout / 32)), dim3(256), 0, as_stream(stream), a);
  } else if (Cout % 128 == 0 && (a.npix + 127) / 128 * (Cout / 128) >= PA_BIG_MIN_WGS) {
    const dim3 grid((unsigned)((a.npix + 127) / 128), (unsigned)(Cout / 128));
    if (pool)
      hipLaunchKernelGGL((preact_f16_kernel<4, 4, true>), grid, dim3(256), 0, as_stream(stream), a);
    else
      hipLaunchKernelGGL((preact_f16_kernel<4, 4, false>), grid, dim3(256), 0, as_stream(stream), a);
  } else {
    const dim3 grid(tiles32, (unsigned)(Cout / 32));
    if (pool && Cout % 128 == 0)      // a pooled operand costs four loads and four affines per element: share it among 128 outputs
      hipLaunchKernelGGL((preact_f16_kernel<4, 1, true>), dim3(tiles32, (unsigned)(Cout / 128)), dim3(64), 0, as_stream(stream), a);
    else if (pool)
      hipLaunchKernelGGL((preact_f16_kernel<1, 1, true>), grid, dim3(64), 0, as_stream(stream), a);
    else
      hipLaunchKernelGGL((preact_f16_kernel<1, 1, false>), grid, dim3(64), 0, as_stream(stream), a);
  }
  FT_LAUNCH_CHECK("preact_conv1x1_kernel");
  return FT_OK;
}
