// FlowNet2's three custom operators, forward and backward (the reference ships them as CUDA-only cffi
// extensions; its CPU entry points are empty stubs, correlation_package/src/correlation.c:3-33):
//   Correlation   correlation_package/src/correlation_cuda_kernel.cu:10-106
//   Resample2d    resample2d_package/src/Resample2d_kernel.cu:20-66
//   ChannelNorm   channelnorm_package/src/ChannelNorm_kernel.cu:19-51
// plus the fused warp/diff/norm/concat stage that sits between stacked FlowNets (models.py:396-403).
// The reference's NCHW->padded-NHWC copy kernels (`channels_first`) do not exist here: padding is a
// bounds test, and the in-network form reads the NHWC activations the conv stack already produces.
#include <stdlib.h>

#include <type_traits>

#include "ft_common.h"

namespace ft {

// ---- Correlation, reference-compatible API: NCHW fp32, any parameters ---------------------------
// One thread per output element, lanes along x so both feature reads are coalesced; the sum runs over
// (j, i, c) of the kernel window exactly as correlation_cuda_kernel.cu:75-88 (fp32 accumulation,
// different association order: within fp32 round-off, tolerance stated in the tests).
__global__ __launch_bounds__(256) void correlation_nchw_kernel(const float* __restrict__ in1, const float* __restrict__ in2,
                                                               float* __restrict__ out, int C, int H, int W, int oc, int oh,
                                                               int ow, int pad, int ksize, int max_disp, int s1, int s2,
                                                               size_t total) {
  const int krad = (ksize - 1) / 2;
  const int drad = max_disp / s2;
  const int D = 2 * drad + 1;
  const float nelems = (float)(ksize * ksize * C);
  const size_t HW = (size_t)H * W;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(idx % ow);
    size_t t = idx / ow;
    const int y = (int)(t % oh);
    t /= oh;
    const int tc = (int)(t % oc);
    const size_t n = t / oc;
    const int tj = tc / D - drad, ti = tc % D - drad;
    // coordinates in the zero-padded frame of the reference, shifted back by pad
    const int y1 = y * s1 + max_disp + krad - pad, x1 = x * s1 + max_disp + krad - pad;
    const int y2 = y1 + tj * s2, x2 = x1 + ti * s2;
    const float* p1 = in1 + n * C * HW;
    const float* p2 = in2 + n * C * HW;
    float acc = 0.f;
    for (int j = -krad; j <= krad; ++j) {
      const int ya = y1 + j, yb = y2 + j;
      if ((unsigned)ya >= (unsigned)H || (unsigned)yb >= (unsigned)H) continue;  // zero padding
      for (int i = -krad; i <= krad; ++i) {
        const int xa = x1 + i, xb = x2 + i;
        if ((unsigned)xa >= (unsigned)W || (unsigned)xb >= (unsigned)W) continue;
        const float* a = p1 + (size_t)ya * W + xa;
        const float* b = p2 + (size_t)yb * W + xb;
        for (int c = 0; c < C; ++c) acc += a[c * HW] * b[c * HW];
      }
    }
    out[idx] = acc / nelems;
  }
}

// ---- Correlation, in-network form: NHWC features, kernel_size 1, stride1 1, pad = max_disp --------
// out[pix, coff + (dy+r)*D + (dx+r)] = act( 1/C * sum_c f1[pix, c] * f2[pix + s2*(dy,dx), c] )
// Workgroup = TX consecutive pixels of one image row.  The f1 row tile stays in LDS for the whole
// workgroup; for each of the D displaced rows the (TX + 2*max_disp)-pixel f2 window is staged once in
// LDS and reused by all D horizontal displacements (the reference re-reads both operands from global
// for every displacement with one 32-thread block per pixel, correlation_cuda_kernel.cu:69-101).
// Thread = (pixel x, group of GX horizontal displacements): the f1 chunk is loaded once per GX dots.
// Results collect in an LDS tile and leave as contiguous D*D-channel runs per pixel.
// act(v) = v > 0 ? v : k * v with torch's value for EVERY input and every slope: the negated ordered compare keeps a NaN and +inf,
// ReLU takes a literal 0 (ReLU(-inf) = 0), leaky the IEEE product (slope 0 and -inf give NaN, as torch's x * negative_slope does;
// act_mul's legacy multiply would return 0 there).  k = slope for FT_ACT_LEAKY, 1 for FT_ACT_NONE.
__device__ __forceinline__ float corr_act(float v, int act, float k) {
  return !(v <= 0.f) ? v : (act == FT_ACT_RELU ? 0.f : v * k);
}

template <typename T, int TX, int GX, int NT>
__global__ __launch_bounds__(NT) void correlation_nhwc_kernel(const T* __restrict__ f1, const T* __restrict__ f2,
                                                               T* __restrict__ y, int C, int H, int W, int max_disp,
                                                               int s2, int f_cstride, int y_cstride, int y_coff, int act,
                                                               float slope) {
  constexpr int VEC = 16 / sizeof(T);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int drad = max_disp / s2;
  const int D = 2 * drad + 1;
  const int DD = D * D;
  const int win = TX + 2 * max_disp;           // f2 pixels per displaced row
  const int pstride = C * (int)sizeof(T) + 16;  // LDS bytes per pixel (+16: bank spread)
  char* s_f1 = smem;
  char* s_f2 = s_f1 + TX * pstride;
  float* s_out = reinterpret_cast<float*>(s_f2 + win * pstride);  // [TX][DD]

  const int tilesx = (W + TX - 1) / TX;
  const int bx = blockIdx.x % tilesx;
  const int yrow = blockIdx.x / tilesx;
  const int n = blockIdx.y;
  const int x0 = bx * TX;
  const int cvecs = C / VEC;
  const T* f1row = f1 + ((size_t)n * H + yrow) * W * f_cstride;

  for (int i = threadIdx.x; i < TX * cvecs; i += NT) {
    const int px = i / cvecs, cv = i - px * cvecs;
    uint4_t v = {0u, 0u, 0u, 0u};
    if (x0 + px < W) v = *reinterpret_cast<const uint4_t*>(f1row + (size_t)(x0 + px) * f_cstride + cv * VEC);
    *reinterpret_cast<uint4_t*>(s_f1 + px * pstride + cv * 16) = v;
  }

  const int ngx = (D + GX - 1) / GX;  // displacement groups per pixel
  const int nwork = TX * ngx;
  const float inv_c = 1.0f / (float)C;
  const float act_k = act == FT_ACT_LEAKY ? slope : 1.f;   // corr_act

  for (int dyi = 0; dyi < D; ++dyi) {
    const int y2 = yrow + (dyi - drad) * s2;
    const bool row_ok = (unsigned)y2 < (unsigned)H;
    __syncthreads();  // previous row's readers are done with s_f2 (and s_f1 is written, first time)
    if (row_ok) {
      const T* f2row = f2 + ((size_t)n * H + y2) * W * f_cstride;
      for (int i = threadIdx.x; i < win * cvecs; i += NT) {
        const int px = i / cvecs, cv = i - px * cvecs;
        const int x2 = x0 - max_disp + px;
        uint4_t v = {0u, 0u, 0u, 0u};
        if ((unsigned)x2 < (unsigned)W) v = *reinterpret_cast<const uint4_t*>(f2row + (size_t)x2 * f_cstride + cv * VEC);
        *reinterpret_cast<uint4_t*>(s_f2 + px * pstride + cv * 16) = v;
      }
    }
    __syncthreads();
    for (int wk = threadIdx.x; wk < nwork; wk += NT) {
      const int px = wk % TX, g = wk / TX;
      float acc[GX];
#pragma unroll
      for (int e = 0; e < GX; ++e) acc[e] = 0.f;
      if (row_ok) {
        const char* a = s_f1 + px * pstride;
        for (int cv = 0; cv < cvecs; ++cv) {
          const uint4_t av = *reinterpret_cast<const uint4_t*>(a + cv * 16);
#pragma unroll
          for (int e = 0; e < GX; ++e) {
            const int dxi = g * GX + e;
            if (dxi < D) {
              const int p2 = px + max_disp + (dxi - drad) * s2;  // index inside the staged window
              const uint4_t bv = *reinterpret_cast<const uint4_t*>(s_f2 + p2 * pstride + cv * 16);
              if constexpr (sizeof(T) == 2) {
                const half8_t ah = __builtin_bit_cast(half8_t, av), bh = __builtin_bit_cast(half8_t, bv);
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[e] += (float)ah[q] * (float)bh[q];
              } else {
                const float4_t af = __builtin_bit_cast(float4_t, av), bf = __builtin_bit_cast(float4_t, bv);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[e] += af[q] * bf[q];
              }
            }
          }
        }
      }
#pragma unroll
      for (int e = 0; e < GX; ++e) {
        const int dxi = g * GX + e;
        if (dxi < D) {
          s_out[px * DD + dyi * D + dxi] = corr_act(acc[e] * inv_c, act, act_k);
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TX * DD; i += NT) {
    const int px = i / DD, ch = i - px * DD;
    if (x0 + px < W)
      y[(((size_t)n * H + yrow) * W + x0 + px) * y_cstride + y_coff + ch] = (T)s_out[i];
  }
}

// ---- Correlation on the matrix cores (fp16 features, kernel 1, stride1 1, stride2 2) ------------------
// stride2 = 2 means an output pixel only ever meets f2 pixels of ITS OWN column parity, so per image row y,
// displaced row y2 = y + 2*dy and parity p the whole cost-volume slice is one small GEMM
//     G[x', x2'] = sum_c f1[y, 2x'+p, c] * f2[y2, 2x2'+p, c],      out[y, 2x'+p, (dy, dx)] = G[x', x'+dx] / C
// of which the band |dx| <= drad is kept.  Workgroup = (image, row, 64-pixel column chunk); wave = (parity,
// 32-column tile of the f2 window).  The f1 fragments (32 pixels x C channels) live in REGISTERS for all D
// displaced rows; each f2 row window (64 + 4*drad pixels) is DMA'd into a 2-slot LDS ring
// (buffer_load ... lds, out-of-image pixels / rows are out-of-range offsets -> zeros) and consumed by
// KS = C/16 back-to-back v_mfma_f32_32x32x16_f16.  MFMA does 64/(2*drad+1) ~ 3x the useful MACs but at
// ~16x the fp32 VALU rate; the band leaves as runs of up to D contiguous channels per pixel.
template <int KS>
__global__ __launch_bounds__(256) void correlation_mfma_kernel(const half_t* __restrict__ f1, const half_t* __restrict__ f2,
                                                               half_t* __restrict__ y, int H, int W, int drad,
                                                               unsigned f2_bytes, int f_cstride, int y_cstride,
                                                               int y_coff, int act, float slope) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int C = KS * 16;
  constexpr int ROWB = C * 2;               // bytes per window pixel in LDS
  constexpr int RPI = 1024 / ROWB;          // window pixels per 1-KiB wave load
  constexpr int CHUNKS = ROWB / 16;
  static_assert(ROWB <= 1024 && CHUNKS >= 16, "C in {128, 256, 512}");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) void* lds_ptr;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int par = wave & 1, jt = wave >> 1;
  const int c = lane & 31, h = lane >> 5;
  const int x0 = blockIdx.x * 64, yrow = blockIdx.y, n = blockIdx.z;
  const int D = 2 * drad + 1;
  const int wrows = 64 + 4 * drad;          // f2 window: pixels x0 - 2*drad ... x0 + 63 + 2*drad
  const int stage = ((wrows * ROWB + 1023) / 1024) * 1024;
  const float inv_c = 1.0f / (float)C;
  const float act_k = act == FT_ACT_LEAKY ? slope : 1.f;   // corr_act

  // f1 fragments (operand A: row = f1 pixel of this parity, k = channel)
  uint4_t a[KS];
  {
    const int x = x0 + 2 * c + par;
    const half_t* src = f1 + ((size_t)(n * H + yrow) * W + x) * f_cstride + h * 8;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      uint4_t v = {0u, 0u, 0u, 0u};
      if (x < W) v = *reinterpret_cast<const uint4_t*>(src + s * 16);
      a[s] = v;
    }
  }
  // operand B: column = window pixel 64*jt + 2*c + par (clamped: columns past the window are never in the band)
  int wr = 64 * jt + 2 * c + par;
  wr = wr < wrows ? wr : wrows - 1;
  const int b_base = wr * ROWB;
  const int b_key = (wr >> 1) & 15;

  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(f2), 0, f2_bytes, 0x00020000);
  constexpr unsigned kOOB = 0x80000000u;
  const int ninstr = stage / 1024;
  auto issue = [&](int dyi, int slot) {
    const int y2 = yrow + 2 * (dyi - drad);
    const bool row_ok = dyi < D && (unsigned)y2 < (unsigned)H;
    for (int i = wave; i < ninstr; i += 4) {
      const int row = i * RPI + lane / CHUNKS, pos = lane % CHUNKS;
      const int lc = pos ^ ((row >> 1) & 15);
      const int x2 = x0 - 2 * drad + row;
      const bool ok = row_ok && row < wrows && (unsigned)x2 < (unsigned)W;
      const unsigned voff = ok ? (unsigned)((((n * H + y2) * W + x2) * f_cstride) * 2 + lc * 16) : kOOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr)(smem + slot * stage + i * 1024), 16, voff, 0, 0, 0);
    }
  };

  issue(0, 0);
  for (int dyi = 0; dyi < D; ++dyi) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's part of row dyi has landed (and its last stores left)
    __builtin_amdgcn_s_barrier();                       // everyone's has; everyone is done reading the other slot
    issue(dyi + 1, (dyi + 1) & 1);
    const int y2 = yrow + 2 * (dyi - drad);
    float16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if ((unsigned)y2 < (unsigned)H) {
      const char* st = smem + (dyi & 1) * stage + b_base;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const uint4_t b = *reinterpret_cast<const uint4_t*>(st + (((2 * s + h) ^ b_key) << 4));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, a[s]), __builtin_bit_cast(half8_t, b), acc, 0, 0, 0);
      }
    }
    // band extraction: accumulator row r = f1 pixel x' (this parity), column c = window column -> dx index c + 32*jt - r
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int r = (g & 3) + 8 * (g >> 2) + 4 * h;
      const int x = x0 + 2 * r + par;
      const int dxi = c + 32 * jt - r;
      if (x < W && (unsigned)dxi < (unsigned)D) {
        const float v = corr_act(acc[g] * inv_c, act, act_k);
        y[((size_t)(n * H + yrow) * W + x) * y_cstride + y_coff + dyi * D + dxi] = (half_t)v;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the (all out-of-range) look-ahead load of the last iteration
#endif
}

// ---- the same band GEMM with R output rows per workgroup -------------------------------------------------------
// stride2 = 2 also ties the ROWS together: output row y only meets f2 rows of its own parity, and an f2 row is
// shared by the D output rows around it.  A workgroup therefore owns R consecutive output rows of one row-parity class
// (y = 2i + q, i = i0 .. i0+R-1) of a 64-pixel column chunk, keeps their f1 fragments in REGISTERS (R x C/16 x 4
// VGPRs) and streams the R + 2*drad f2 rows of that class through a 3-slot LDS ring ONCE: every f2 row feeds up to R
// band products.  At R = 3 that is 23 row loads for 63 products instead of 63 (3.6 x fewer L2 -> LDS bytes, and 2-3
// products of matrix work per barrier instead of one).  The ring runs two rows ahead on a counted vmcnt: the band
// leaves as unconditional 2-byte buffer stores (lanes outside the band / the image store to an out-of-range offset), so
// the number of vector-memory operations between a row load and its wait is a compile-time constant.
template <int KS, int R, int DRAD>
__global__ __launch_bounds__(256, 1) void correlation_mfma_rows_kernel(const half_t* __restrict__ f1, const half_t* __restrict__ f2,
                                                                        half_t* __restrict__ y, int H, int W, unsigned f2_bytes,
                                                                        unsigned y_bytes, int f_cstride, int y_cstride, int y_coff,
                                                                        int act, float slope, int ngx, int ngy) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int C = KS * 16, ROWB = C * 2, RPI = 1024 / ROWB, CHUNKS = ROWB / 16;
  constexpr int D = 2 * DRAD + 1, WROWS = 64 + 4 * DRAD;
  constexpr int STAGE = (WROWS * ROWB + 1023) / 1024 * 1024, NINSTR = STAGE / 1024, NL = NINSTR / 4;
  constexpr int NJ = R + 2 * DRAD;          // f2 rows of the class this workgroup walks
  static_assert(ROWB <= 1024 && CHUNKS >= 16 && NINSTR % 4 == 0 && 3 * STAGE <= 160 * 1024, "shape");
  static_assert(NL + 16 * R <= 63, "vmcnt immediate");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) void* lds_ptr;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int par = wave & 1, jt = wave >> 1;
  const int c = lane & 31, h = lane >> 5;
  // workgroup b runs on XCD b % 8 (each with its own L2): hand every XCD a contiguous range of (image, row group) pairs,
  // so the f2 rows its workgroups share are fetched into ONE L2 instead of all eight (measured: 139 -> ~30 MB of f2 reads)
  int x0, n, q, i0;
  {
    const int total = gridDim.x, b = blockIdx.x;
    const int qq = total >> 3, rr = total & 7, xcd = b & 7, loc = b >> 3;
    int logical = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + loc;
    const int gy = logical % ngy;
    logical /= ngy;
    x0 = (logical % ngx) * 64;
    n = logical / ngx;
    q = gy & 1;
    i0 = (gy >> 1) * R;
  }
  const int Hq = (H - q + 1) >> 1;          // rows of this parity class
  const float inv_c = 1.0f / (float)C;

  // f1 fragments of the R rows (operand A: row = f1 pixel of this column parity, k = channel)
  constexpr unsigned kOOB = 0x80000000u;
  uint4_t a[R][KS];
  {
    // buffer loads: pixels / rows outside the image are out-of-range offsets (zeros), no branches, all in flight at once
    const __amdgpu_buffer_rsrc_t rsrc1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(f1), 0, f2_bytes, 0x00020000);
    const int x = x0 + 2 * c + par;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int yy = 2 * (i0 + r) + q;
      const unsigned voff = (x < W && yy < H) ? (unsigned)((((n * H + yy) * W + x) * f_cstride + h * 8) * 2) : kOOB;
#pragma unroll
      for (int s = 0; s < KS; ++s) a[r][s] = __builtin_amdgcn_raw_buffer_load_b128(rsrc1, voff, s * 32, 0);
    }
  }
  // operand B: column = window pixel 64*jt + 2*c + par (clamped: columns past the window are never in the band)
  int wr = 64 * jt + 2 * c + par;
  wr = wr < WROWS ? wr : WROWS - 1;
  const int b_base = wr * ROWB;
  const int b_key = (wr >> 1) & 15;

  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(f2), 0, f2_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_y = __builtin_amdgcn_make_buffer_rsrc(y, 0, y_bytes, 0x00020000);
  // loader lanes: wave-load i covers window rows i*RPI .. ; XOR swizzle on the source chunk as in correlation_mfma_kernel
  unsigned l_voff[NL];
#pragma unroll
  for (int t = 0; t < NL; ++t) {
    const int i = t * 4 + wave;
    const int row = i * RPI + lane / CHUNKS, pos = lane % CHUNKS;
    const int lc = pos ^ ((row >> 1) & 15);
    const int x2 = x0 - 2 * DRAD + row;
    l_voff[t] = (row < WROWS && (unsigned)x2 < (unsigned)W) ? (unsigned)(((n * H) * W + x2) * f_cstride * 2 + lc * 16) : kOOB;
  }
  const int row_bytes = W * f_cstride * 2;
  auto issue = [&](int jj, int slot) {       // always NL loads per wave: rows outside the image / past the walk are out of range
    const int j = i0 - DRAD + jj;
    const bool row_ok = jj < NJ && (unsigned)j < (unsigned)Hq;
    const int soff = row_ok ? (2 * j + q) * row_bytes : 0;
#pragma unroll
    for (int t = 0; t < NL; ++t)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr)(smem + slot * STAGE + (t * 4 + wave) * 1024), 16,
                                               row_ok ? l_voff[t] : kOOB, soff, 0, 0);
  };
  // band extraction: accumulator register g of lane (c, h) = f1 pixel rr(g) x window column c -> displacement c + 32*jt - rr
  unsigned s_voff[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int rr = (g & 3) + 8 * (g >> 2) + 4 * h;
    const int x = x0 + 2 * rr + par;
    const int dxi = c + 32 * jt - rr;
    s_voff[g] = (x < W && (unsigned)dxi < (unsigned)D) ? (unsigned)(((n * H) * W + x) * y_cstride + y_coff + dxi) * 2u : kOOB;
  }
  const int yrow_bytes = W * y_cstride * 2;
  // act(v) = max(v, s*v) for s in [0, 1] (relu: 0, leaky: slope, none: 1); the 1/C of the correlation rides along
  const float k_pos = inv_c, k_neg = inv_c * (act == FT_ACT_RELU ? 0.f : (act == FT_ACT_LEAKY ? slope : 1.f));

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the f1 fragments sit in registers before the ring starts counting ..
  // .. and the compiler has to know it: it cannot see the wait above, and with the products behind branches it kept "a[] may still be
  // in flight" alive at every join, i.e. s_waitcnt vmcnt(15) .. vmcnt(0) in front of the sixteen MFMAs of EVERY step — the last one
  // drains the whole queue (look-ahead ring rows and the band stores of the previous steps).  An empty asm that redefines the
  // registers ends that (round 6; found in the ISA of correlation_mfma_rows64_kernel: 23 x sixteen descending waits).
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(a[r][s]));
  issue(0, 0);
  issue(1, 1);
  int slot = 0;
  for (int jj = 0; jj < NJ; ++jj) {
    // row jj has landed (this wave's share): behind it only row jj+1 and the 16*R stores of the previous step may fly
    if (jj == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NL) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NL + 16 * R) : "memory");
    asm volatile("s_barrier" ::: "memory");             // everyone's share has; everyone is done reading the slot refilled now
    issue(jj + 2, slot == 0 ? 2 : slot - 1);
    const int j = i0 - DRAD + jj;
    const bool row_ok = (unsigned)j < (unsigned)Hq;
    const char* st = smem + slot * STAGE + b_base;
    uint4_t b[KS];
    if (row_ok) {
#pragma unroll
      for (int s = 0; s < KS; ++s) b[s] = *reinterpret_cast<const uint4_t*>(st + (((2 * s + h) ^ b_key) << 4));
    }
    // all R band products first (independent accumulators keep the matrix pipe busy), then their stores
    float16_t acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[r][e] = 0.f;
      const int dyi = jj - r;                           // f2 row j is displacement dyi - DRAD of output row i0 + r
      if ((unsigned)dyi < (unsigned)D && i0 + r < Hq && row_ok) {
#pragma unroll
        for (int s = 0; s < KS; ++s)
          acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, a[r][s]), __builtin_bit_cast(half8_t, b[s]), acc[r], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int dyi = jj - r;
      const bool live = (unsigned)dyi < (unsigned)D && i0 + r < Hq;
      if (live) {                                        // wave-uniform
        const int soff = (2 * (i0 + r) + q) * yrow_bytes + dyi * D * 2;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const float v = __builtin_fmaxf(acc[r][g] * k_pos, acc[r][g] * k_neg);   // act(v / C), slopes in [0, 1]
          const half_t hv = (half_t)v;
          __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, hv), rsrc_y, s_voff[g], soff, 0);
        }
      } else {                                           // same count of vector-memory operations, nothing stored
#pragma unroll
        for (int g = 0; g < 16; ++g) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)0, rsrc_y, kOOB, 0, 0);
      }
    }
    slot = slot == 2 ? 0 : slot + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the two (all out-of-range) look-ahead rows of the last steps
#endif
}

// ---- the rows kernel for maps up to 64 pixels wide ---------------------------------------------------------------------
// At W <= 64 (FlowNetC at 512x384: 48 x 64) only 64 of the 104 window columns of an f2 row exist, so a ring slot shrinks from 52
// to 32 KiB and four of them fit.  The MFMA tile's columns are the IMAGE columns of one parity (32 of them) instead of two
// 32-column halves of the 104-column window: half the MFMAs and half the band store instructions per (f2 row, output row).
// The band of f1 pixel i then is f2 pixel i2 = i + dxi - DRAD in [0, 32); the displacements that fall off the image (i2 < 0 or
// >= 32: structural zeros) are written by the lanes of the columns i2 mod 32, which are out of band for that row: every lane slot
// with (c - i + DRAD) mod 32 < D stores, a real product where the difference did not wrap, zero where it did.  Six waves =
// R = 3 output rows x 2 column parities, one row per wave (256 workgroups at 16 x 48 rows): 50.2-51.2 us at [16,256,48,64]
// against 65.6-67.3 for the 104-column, four-wave rows kernel (same box).  Window-column tiles with four or eight waves, an
// eight-wave R = 4 form of this one, a transposed band and bands staged through LDS were all tried and were slower, as were three
// rewrites of the band's way out: profiles/HISTORY.md ("Retired A/B switches").  Ablations of this kernel (FT_CORR_DBG, same box):
// full 54.2 us; no band store instructions 37.5 (stores kept but all out of range: 40.8 of 50.2); also no MFMAs 27.2; also no
// fragment reads 26.9; also no ring loads 20.4; also no barriers 17.7 (launch + the f1 fragments + 23 empty steps).
template <int N, int I = 0, typename F>
__device__ __forceinline__ void corr_unroll(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    corr_unroll<N, I + 1>(f);
  }
}

constexpr int kCorr64Waves = 6;
template <int KS, int R, int DRAD>
__global__ __launch_bounds__(64 * kCorr64Waves, 1) void correlation_mfma_rows64_kernel(const half_t* __restrict__ f1, const half_t* __restrict__ f2,
                                                                                   half_t* __restrict__ y, int H, int W, unsigned f2_bytes,
                                                                                   unsigned y_bytes, int f_cstride, int y_cstride, int y_coff,
                                                                                   int act, float slope, int ngy) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NWV = kCorr64Waves;
  constexpr int C = KS * 16, ROWB = C * 2;
  constexpr int D = 2 * DRAD + 1;
  constexpr int NJ = R + 2 * DRAD;          // f2 rows of the class this workgroup walks
  constexpr int NSETS = NWV / 2;            // row sets among the waves: each a pair of waves, one per column parity
  constexpr int RW = R / NSETS;             // output rows per wave
  constexpr int SLOT = 64 * ROWB, NL = (SLOT / 1024 + NWV - 1) / NWV;   // wave-loads per wave and ring row (the last ones may fall behind the slot: scratch)
  static_assert(R % NSETS == 0 && D <= 32 && NWV % 2 == 0, "row sets");
  // Four ring slots, rows issued THREE steps ahead.  vmcnt counts loads and stores in one queue, in order, so "row jj has
  // landed" can only be asked as "everything older than the ops issued after it is done"; at distance three the stores of three
  // steps may still be in flight (vmcnt(2 NL + 48) <= 63).  Measured: no gain over distance two (52.0 vs 51.6 us) — the store
  // round trip is not what a step waits for; kept because it costs nothing.
  constexpr int DEPTH = 3, NSLOT = DEPTH + 1;
  constexpr int ZROW = NSLOT * SLOT;        // one zero row behind the ring: operand B of the columns outside the image
  constexpr int SPILL = ZROW + ROWB + 128;  // 1 KiB behind it: where the wave-loads past the end of a slot land
  static_assert(ROWB == 512, "shape");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) void* lds_ptr;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int par = wave & 1, rs = wave >> 1;  // column parity and row set of this wave
  const int c = lane & 31, h = lane >> 5;
  int n, q, i0;
  {
    const int total = gridDim.x, b = blockIdx.x;
    const int qq = total >> 3, rr = total & 7, xcd = b & 7, loc = b >> 3;
    const int logical = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + loc;
    const int gy = logical % ngy;
    n = logical / ngy;
    q = gy & 1;
    i0 = (gy >> 1) * R;
  }
  const int Hq = (H - q + 1) >> 1;          // rows of this parity class
  const float inv_c = 1.0f / (float)C;
  constexpr unsigned kOOB = 0x80000000u;
  // developer ablation (FT_CORR_DBG, timing only): 1 = every band store out of range, 2 = no MFMAs, 4 = no fragment
  // reads, 8 = no ring loads, 16 = no barriers, 32 = no band store instructions at all; 0 in production
  const int cdbg = act >> 8;
  act &= 0xff;

  // f1 fragments of the R rows (operand A: row = f1 pixel of this column parity, k = channel)
  uint4_t a[RW][KS];
  {
    const __amdgpu_buffer_rsrc_t rsrc1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(f1), 0, f2_bytes, 0x00020000);
    const int x = 2 * c + par;
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int yy = 2 * (i0 + rs * RW + r) + q;
      const unsigned voff = (x < W && yy < H) ? (unsigned)((((n * H + yy) * W + x) * f_cstride + h * 8) * 2) : kOOB;
#pragma unroll
      for (int s = 0; s < KS; ++s) a[r][s] = __builtin_amdgcn_raw_buffer_load_b128(rsrc1, voff, s * 32, 0);
    }
  }
  // operand B: column = image column x2 = 2*c + par (ring row x2), the zero row outside the image
  const int x2 = 2 * c + par;
  const bool in_img = (unsigned)x2 < (unsigned)W;
  const int b_base = in_img ? x2 * ROWB : ZROW;          // slot-relative for image columns; ZROW is absolute
  const int b_key = in_img ? (x2 >> 1) & 15 : 0;

  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(f2), 0, f2_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_y = __builtin_amdgcn_make_buffer_rsrc(y, 0, y_bytes, 0x00020000);
  // loader lanes: wave-load i = t*NWV + wave covers ring rows 2i, 2i+1; XOR swizzle on the source chunk
  unsigned l_voff[NL];
#pragma unroll
  for (int t = 0; t < NL; ++t) {
    const int i = t * NWV + wave;
    const int row = i * 2 + (lane >> 5), pos = lane & 31;
    const int lc = pos ^ ((row >> 1) & 15);
    l_voff[t] = (row < W && i < SLOT / 1024) ? (unsigned)(((n * H) * W + row) * f_cstride * 2 + lc * 16) : kOOB;
  }
  const int row_bytes = W * f_cstride * 2;
  auto issue = [&](int jj, int slot) {       // always NL loads per wave: rows outside the image / past the walk are out of range
    const int j = i0 - DRAD + jj;
    const bool row_ok = jj < NJ && (unsigned)j < (unsigned)Hq;
    const int soff = row_ok ? (2 * j + q) * row_bytes : 0;
    if (cdbg & 8) return;
#pragma unroll
    for (int t = 0; t < NL; ++t)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr)(t * NWV + wave < SLOT / 1024 ? smem + slot * SLOT + (t * NWV + wave) * 1024
                                                                                           : smem + SPILL), 16,
                                               row_ok ? l_voff[t] : kOOB, soff, 0, 0);
  };
  // band lanes: accumulator register g of lane (c, h) = f1 pixel rr = G(g) + 4h (of this column parity) x image column c
  // -> displacement index dxi = (c - rr + DRAD) mod 32, stored when < D and the pixel lies inside the image
  const int dxi0 = c - 4 * h + DRAD;
  int vmask = 0, realmask = 0;       // stores / stores that carry a product (the others are the off-image zeros)
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int G = (g & 3) + 8 * (g >> 2);
    const int dr = dxi0 - G, dd = dr & 31;
    if ((unsigned)dd < (unsigned)D && 2 * (G + 4 * h) + par < W) vmask |= 1 << g;
    if (dd == dr) realmask |= 1 << g;
  }
  // act(v) = max(v, s*v) for s in [0, 1] (relu: 0, leaky: slope, none: 1); the 1/C of the correlation rides along
  const float k_pos = inv_c, k_neg = inv_c * (act == FT_ACT_RELU ? 0.f : (act == FT_ACT_LEAKY ? slope : 1.f));
  const int yrow_bytes = W * y_cstride * 2;
  unsigned s_voff[16];                       // the band leaves as 2-byte stores in the accumulator layout
  // (px0 as a sum of its own on purpose: hipcc's schedule of the WHOLE kernel changes with the way this address is associated,
  // profiles/HISTORY.md "Checks of this change"; run tools/dev/isa_diff.py after touching it)
  const int px0 = (n * H) * W + par;         // pixel (row 0, column par) of image n
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int G = (g & 3) + 8 * (g >> 2);
    const int dd = (dxi0 - G) & 31;
    s_voff[g] = (((vmask >> g) & 1) && !(cdbg & 1)) ? (unsigned)((px0 + 2 * (G + 4 * h)) * y_cstride + y_coff + dd) * 2u : kOOB;
  }

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the f1 fragments sit in registers before the ring starts counting ..
  // .. and the compiler has to know it: it cannot see the wait above, and with the products behind branches it kept "a[] may still be
  // in flight" alive at every join, i.e. s_waitcnt vmcnt(15) .. vmcnt(0) in front of the sixteen MFMAs of EVERY step — the last one
  // drains the whole queue (look-ahead ring rows and the band stores of the previous steps).  An empty asm that redefines the
  // registers ends that (round 6; found in the ISA: 23 x sixteen descending waits).
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(a[r][s]));
  if (tid < ROWB / 16) *reinterpret_cast<uint4_t*>(smem + ZROW + tid * 16) = uint4_t{0u, 0u, 0u, 0u};
  corr_unroll<DEPTH>([&](auto pc) { issue(decltype(pc)::value, decltype(pc)::value); });
  corr_unroll<NJ>([&](auto jc) {
    constexpr int jj = decltype(jc)::value;
    constexpr int slot = jj % NSLOT;
    // row jj has landed (this wave's share): behind it rows jj+1, jj+2 and the 16 band stores per row of up to three steps may fly
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((DEPTH - 1) * NL + 16 * RW * (jj < DEPTH ? jj : DEPTH)) : "memory");
    if (!(cdbg & 16)) asm volatile("s_barrier" ::: "memory");   // everyone's has; everyone is done reading the slot refilled now
    issue(jj + DEPTH, (jj + DEPTH) % NSLOT);
    const int j = i0 - DRAD + jj;
    const bool row_ok = (unsigned)j < (unsigned)Hq;
    uint4_t b[KS];
    if (cdbg & 4) {
#pragma unroll
      for (int s = 0; s < KS; ++s) b[s] = uint4_t{(unsigned)jj, 0u, 0u, 0u};
    } else if (row_ok) {
      const char* st = smem + (in_img ? slot * SLOT : 0) + b_base;
#pragma unroll
      for (int s = 0; s < KS; ++s) b[s] = *reinterpret_cast<const uint4_t*>(st + (((2 * s + h) ^ b_key) << 4));
    }
    corr_unroll<RW>([&](auto rc) {
      constexpr int rw = decltype(rc)::value;
      // always 16 stores per (step, row) so that the waits can count them
      const int r = rs * RW + rw;                        // wave-uniform
      const int dyi = jj - r;                            // f2 row j is displacement dyi - DRAD of output row i0 + r
      const bool live = dyi >= 0 && dyi < D && i0 + r < Hq;
      if (live) {
        float16_t acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        if (row_ok && !(cdbg & 2)) {
#pragma unroll
          for (int s = 0; s < KS; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, a[rw][s]), __builtin_bit_cast(half8_t, b[s]), acc, 0, 0, 0);
        }
        const int soff = (2 * (i0 + r) + q) * yrow_bytes + dyi * D * 2;
        if (cdbg & 32) {
          float keep = 0.f;
#pragma unroll
          for (int g = 0; g < 16; ++g) keep += acc[g];
          if (keep == 12345.678f) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)1, rsrc_y, s_voff[0], soff, 0);
        } else {
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            half_t hv = (half_t)__builtin_fmaxf(acc[g] * k_pos, acc[g] * k_neg);
            hv = ((realmask >> g) & 1) ? hv : (half_t)0.f;   // the off-image displacements: zeros
            __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, hv), rsrc_y, s_voff[g], soff, 0);
          }
        }
      } else if (!(cdbg & 32)) {
#pragma unroll
        for (int g = 0; g < 16; ++g) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)0, rsrc_y, kOOB, 0, 0);
      }
    });
  });
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the (all out-of-range) look-ahead rows of the last steps
#endif
}

// Workgroup b of a 1-D grid runs on XCD b % 8 and every XCD has its own L2.  The gather kernels below read a 2 x 2
// neighbourhood around a displaced position: with the plain blockIdx order the rows one workgroup touches are also touched
// by its neighbours on seven other XCDs and every L2 fetches them again (PMC: 2.7-2.9 x the algorithmic read bytes).  This
// bijective remap hands each XCD one contiguous eighth of the blocks, i.e. whole images.
__device__ __forceinline__ size_t xcd_contiguous_block() {
  const unsigned total = gridDim.x, b = blockIdx.x;
  const unsigned q = total >> 3, r = total & 7, xcd = b & 7, loc = b >> 3;
  return (size_t)((xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc);
}

// ---- Resample2d: backward bilinear warp with border clamp -----------------------------------------
// Weights from the UNclamped floor, neighbour indices clamped, no renormalisation
// (Resample2d_kernel.cu:42-59).  Thread = output pixel, all channels (flow read once).
__global__ __launch_bounds__(256) void resample2d_kernel(const float* __restrict__ in1, const float* __restrict__ flow,
                                                         float* __restrict__ out, int C, int H, int W, size_t total) {
  const size_t HW = (size_t)H * W;
  for (size_t i = xcd_contiguous_block() * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / HW, pix = i - b * HW;
    const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
    const float dx = flow[(b * 2 + 0) * HW + pix], dy = flow[(b * 2 + 1) * HW + pix];
    const float xf = (float)x + dx, yf = (float)y + dy;
    const float fx = floorf(xf), fy = floorf(yf);
    const float alpha = xf - fx, beta = yf - fy;
    // clamp in float first so huge/inf flows cannot overflow the int conversion
    const int xL = (int)fminf(fmaxf(fx, 0.f), (float)(W - 1));
    const int xR = (int)fminf(fmaxf(fx + 1.f, 0.f), (float)(W - 1));
    const int yT = (int)fminf(fmaxf(fy, 0.f), (float)(H - 1));
    const int yB = (int)fminf(fmaxf(fy + 1.f, 0.f), (float)(H - 1));
    const float w00 = (1.f - alpha) * (1.f - beta), w01 = alpha * (1.f - beta);
    const float w10 = (1.f - alpha) * beta, w11 = alpha * beta;
    for (int c = 0; c < C; ++c) {
      const float* p = in1 + (b * C + c) * HW;
      float v = w00 * p[(size_t)yT * W + xL];
      v += w01 * p[(size_t)yT * W + xR];
      v += w10 * p[(size_t)yB * W + xL];
      v += w11 * p[(size_t)yB * W + xR];
      out[(b * C + c) * HW + pix] = v;
    }
  }
}

// The same with the two x-neighbours of a row fetched as ONE 8-byte load: the kernel is bound by cache-line requests (every
// lane gathers from its own line: 4 taps x C channels = 12 requests per pixel, 38 M per launch at BASELINE configs[3] shapes
// = the measured 58 us at ~1 request per clock per CU), not by bytes and not by the per-thread dependency chain (four pixels
// per thread with all 48 gathers independent measured 70 us).  xL and xR are adjacent except where the clamp folds them onto
// one column, so a pair starting at column min(xL, W - 2) always holds both: 2 requests per row pair instead of 4.
template <int C>
__global__ __launch_bounds__(256) void resample2d_pair_kernel(const float* __restrict__ in1, const float* __restrict__ flow,
                                                              float* __restrict__ out, int H, int W, size_t total) {
  typedef float float2_t __attribute__((ext_vector_type(2), aligned(4)));
  const size_t HW = (size_t)H * W;
  for (size_t i = xcd_contiguous_block() * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / HW, pix = i - b * HW;
    const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
    const float dx = flow[(b * 2 + 0) * HW + pix], dy = flow[(b * 2 + 1) * HW + pix];
    const float xf = (float)x + dx, yf = (float)y + dy;
    const float fx = floorf(xf), fy = floorf(yf);
    const float alpha = xf - fx, beta = yf - fy;
    const int xL = (int)fminf(fmaxf(fx, 0.f), (float)(W - 1));
    const int xR = (int)fminf(fmaxf(fx + 1.f, 0.f), (float)(W - 1));
    const int yT = (int)fminf(fmaxf(fy, 0.f), (float)(H - 1));
    const int yB = (int)fminf(fmaxf(fy + 1.f, 0.f), (float)(H - 1));
    const float w00 = (1.f - alpha) * (1.f - beta), w01 = alpha * (1.f - beta);
    const float w10 = (1.f - alpha) * beta, w11 = alpha * beta;
    const int xb = xL < W - 2 ? xL : W - 2;       // pair [xb, xb + 1] holds columns xL and xR
    const bool l1 = xL != xb, r1 = xR != xb;
    float2_t t[C], u[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float* p = in1 + (b * C + c) * HW;
      t[c] = *reinterpret_cast<const float2_t*>(p + (size_t)yT * W + xb);
      u[c] = *reinterpret_cast<const float2_t*>(p + (size_t)yB * W + xb);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float v = w00 * (l1 ? t[c][1] : t[c][0]);
      v += w01 * (r1 ? t[c][1] : t[c][0]);
      v += w10 * (l1 ? u[c][1] : u[c][0]);
      v += w11 * (r1 ? u[c][1] : u[c][0]);
      out[(b * C + c) * HW + pix] = v;
    }
  }
}

// ---- Resample2d through an LDS window (round 4) ---------------------------------------------------------------------------
// The gather kernels above are bound by cache-line REQUESTS, not bytes: with incoherent per-pixel flows every lane's taps sit
// in their own lines (12 requests per pixel at C = 3), 38 M requests per launch at configs[3] shapes.  Here a workgroup owns a
// 16 x 64 tile of output pixels (4 per thread): it reads the tile's flow once, reduces the bounding box of every tap the tile
// touches (clamped indices, so the box is inside the image), loads that window of in1 — all C planes — into LDS with
// row-contiguous, fully coalesced loads (LDS-DMA), and serves the four taps of every pixel from LDS.  A tile whose box does not
// fit the LDS budget keeps a window CLIPPED around its own pixels: per pixel, taps that lie inside the window come from LDS and
// the pixels with a tap outside it gather theirs from memory as 8-byte pairs (see `window` / `inw` below); only a field that
// spreads over more than four such windows skips the window altogether.  Same weights, same order of the four products as
// Resample2d_kernel.cu:42-59 restated above: results are bit-identical to the gather kernels.
constexpr int kRsTH = 16, kRsTW = 64, kRsPPT = 4;          // tile rows / columns, pixels per thread
#ifndef FT_RS_CLIP_PITCH
#define FT_RS_CLIP_PITCH 96
#endif
constexpr int kRsClipPitch = FT_RS_CLIP_PITCH;                           // row pitch (floats) of a window clipped around its tile: 16 + 2 x 8 rows x 64 + 2 x 15 columns at the default budget

template <int C>
__global__ __launch_bounds__(256) void resample2d_window_kernel(const float* __restrict__ in1, const float* __restrict__ flow,
                                                                float* __restrict__ out, int H, int W, int tiles_x, int tiles_y,
                                                                unsigned in_bytes, int wbudget) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) float rs_smem[];
  typedef __attribute__((address_space(3))) void* lds_ptr;
  __shared__ int s_box[4][4];                              // per wave: min x, max x, min y, max y
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles = tiles_x * tiles_y;
  const int b = blockIdx.x / tiles, trem = blockIdx.x - b * tiles;
  const int ty0 = (trem / tiles_x) * kRsTH, tx0 = (trem % tiles_x) * kRsTW;
  const size_t HW = (size_t)H * W;
  const int x = tx0 + lane;
  float w00[kRsPPT], w01[kRsPPT], w10[kRsPPT], w11[kRsPPT];
  int xL[kRsPPT], xR[kRsPPT], yT[kRsPPT], yB[kRsPPT];
  int bx0 = 0x7fffffff, bx1 = -1, by0 = 0x7fffffff, by1 = -1;
#pragma unroll
  for (int k = 0; k < kRsPPT; ++k) {
    const int y = ty0 + k * 4 + wave;
    const bool live = x < W && y < H;
    float dx = 0.f, dy = 0.f;
    if (live) {
      const size_t pix = (size_t)y * W + x;
      dx = flow[(b * 2 + 0) * HW + pix];
      dy = flow[(b * 2 + 1) * HW + pix];
    }
    const float xf = (float)x + dx, yf = (float)y + dy;
    const float fx = floorf(xf), fy = floorf(yf);
    const float alpha = xf - fx, beta = yf - fy;
    xL[k] = (int)fminf(fmaxf(fx, 0.f), (float)(W - 1));
    xR[k] = (int)fminf(fmaxf(fx + 1.f, 0.f), (float)(W - 1));
    yT[k] = (int)fminf(fmaxf(fy, 0.f), (float)(H - 1));
    yB[k] = (int)fminf(fmaxf(fy + 1.f, 0.f), (float)(H - 1));
    w00[k] = (1.f - alpha) * (1.f - beta); w01[k] = alpha * (1.f - beta);
    w10[k] = (1.f - alpha) * beta;         w11[k] = alpha * beta;
    if (live) {
      bx0 = min(bx0, xL[k]); bx1 = max(bx1, xR[k]);
      by0 = min(by0, yT[k]); by1 = max(by1, yB[k]);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    bx0 = min(bx0, __shfl_xor(bx0, off)); bx1 = max(bx1, __shfl_xor(bx1, off));
    by0 = min(by0, __shfl_xor(by0, off)); by1 = max(by1, __shfl_xor(by1, off));
  }
  if (lane == 0) { s_box[wave][0] = bx0; s_box[wave][1] = bx1; s_box[wave][2] = by0; s_box[wave][3] = by1; }
  __syncthreads();
  bx0 = min(min(s_box[0][0], s_box[1][0]), min(s_box[2][0], s_box[3][0]));
  bx1 = max(max(s_box[0][1], s_box[1][1]), max(s_box[2][1], s_box[3][1]));
  by0 = min(min(s_box[0][2], s_box[1][2]), min(s_box[2][2], s_box[3][2]));
  by1 = max(max(s_box[0][3], s_box[1][3]), max(s_box[2][3], s_box[3][3]));
  if (bx1 < 0) return;                                     // (a tile without a live pixel: cannot happen for ceil-divided grids)
  bx0 = __builtin_amdgcn_readfirstlane(bx0); bx1 = __builtin_amdgcn_readfirstlane(bx1);
  by0 = __builtin_amdgcn_readfirstlane(by0); by1 = __builtin_amdgcn_readfirstlane(by1);
  // 16-byte DMA pieces need 16-byte-aligned sources: the window starts at a multiple of four columns (W % 4 == 0: every row base
  // is aligned); otherwise 4-byte pieces, four times as many instructions
  const bool vec4 = (W & 3) == 0;
  const int pgran = vec4 ? 32 : 64;                        // floats per LDS row: a multiple of 32 (16-byte pieces) / 64 (4-byte pieces)
  int wx0 = vec4 ? bx0 & ~3 : bx0, wx1 = bx1, wy0 = by0, wy1 = by1;
  int ww = wx1 - wx0 + 1, wh = wy1 - wy0 + 1;
  int pitch = (ww + pgran - 1) / pgran * pgran;
  pitch = pitch < 64 ? 64 : pitch;
  bool window = (((long long)pitch * wh + 255) & ~255LL) <= wbudget;     // the whole box fits: every tap comes from LDS
  // Round 6: a box that does not fit no longer sends the whole tile to the gathers.  The window is CLIPPED around the tile (rows of
  // kRsClipPitch floats, as many as the budget holds, centred on the tile's own pixels), pixels whose four taps lie inside it take
  // them from LDS and only the others gather from memory (8-byte x-neighbour pairs, issued before the window's wait): with
  // per-pixel N(0, 4 px) flows about one pixel in eight gathers instead of all of them.  A field that spreads over more than four
  // such windows (the "wide" image of the tests) skips the window.
  const int clip_pitch = vec4 ? kRsClipPitch : 128;        // (4-byte pieces fill 64-float row segments)
  if (!window && ww <= 4 * clip_pitch && wh <= 4 * (wbudget / clip_pitch)) {
    const int cp = pitch < clip_pitch ? pitch : clip_pitch;
    const int rows = wbudget / cp;
    if (rows >= kRsTH + 2 && cp >= kRsTW + 2) {
      int cx0 = tx0 - ((cp - (kRsTW + 1)) >> 1);
      cx0 = cx0 > wx0 ? cx0 : wx0;
      if (vec4) cx0 &= ~3;                                  // wx0 is a multiple of four already: cx0 >= wx0 still
      int cy0 = ty0 - ((rows - (kRsTH + 1)) >> 1);
      cy0 = cy0 > wy0 ? cy0 : wy0;
      wx0 = cx0;
      wx1 = wx1 < cx0 + cp - 1 ? wx1 : cx0 + cp - 1;
      wy0 = cy0;
      wy1 = wy1 < cy0 + rows - 1 ? wy1 : cy0 + rows - 1;
      ww = wx1 - wx0 + 1;
      wh = wy1 - wy0 + 1;
      pitch = cp;
      window = ww > 0 && wh > 0;
    }
  }
  // pixels outside the window: their taps as 8-byte pairs straight from memory, in flight while the window loads
  typedef float float2_t __attribute__((ext_vector_type(2), aligned(4)));
  float2_t gt[kRsPPT][C], gu[kRsPPT][C];
  bool inw[kRsPPT];
#pragma unroll
  for (int k = 0; k < kRsPPT; ++k) {
    const int y = ty0 + k * 4 + wave;
    const bool live = x < W && y < H;
    inw[k] = window && xL[k] >= wx0 && xR[k] <= wx1 && yT[k] >= wy0 && yB[k] <= wy1;
#pragma unroll
    for (int c = 0; c < C; ++c) gt[k][c] = gu[k][c] = float2_t{0.f, 0.f};
    if (live && !inw[k]) {
      const int xb = xL[k] < W - 2 ? xL[k] : W - 2;         // pair [xb, xb + 1] holds columns xL and xR (W >= 2: the host's condition)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float* p = in1 + ((size_t)b * C + c) * HW;
        gt[k][c] = *reinterpret_cast<const float2_t*>(p + (size_t)yT[k] * W + xb);
        gu[k][c] = *reinterpret_cast<const float2_t*>(p + (size_t)yB[k] * W + xb);
      }
    }
  }
  const int plane = (pitch * wh + 255) & ~255;             // whole 1-KiB pieces per plane: a piece's tail never reaches the next plane
  if (window) {
    // the window of every plane through LDS-DMA, straight into LDS (no VGPR round trip, every piece in flight at once: the tile's
    // latency is ONE memory round trip, not one per row).  A wave instruction moves 1 KiB = 256 consecutive LDS floats; lanes past
    // the window read out of range = 0
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in1), 0, in_bytes, 0x00020000);
    constexpr unsigned kOOB = 0x80000000u;
    if (vec4) {
      // lane -> (row, column) of its four floats in piece `wave`, then + 1024 floats per round (no division in the loop)
      const int f0 = wave * 256 + lane * 4;
      const int r0 = f0 / pitch, q0 = f0 - r0 * pitch;
      const int dr = 1024 / pitch, dq = 1024 - dr * pitch;
      const int npieces = plane >> 8;
#pragma unroll 1
      for (int c = 0; c < C; ++c) {
        const unsigned cbase = (unsigned)((((size_t)b * C + c) * HW + (size_t)wy0 * W + wx0) * 4);
        int r = r0, q = q0;
#pragma unroll 4
        for (int pc = wave; pc < npieces; pc += 4) {
          const unsigned voff = (r < wh && q < ww) ? cbase + (unsigned)((r * W + q) * 4) : kOOB;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr)(rs_smem + c * plane + pc * 256), 16, voff, 0, 0, 0);
          q += dq;
          r += dr;
          if (q >= pitch) { q -= pitch; ++r; }
        }
      }
    } else {
      const int nch = pitch >> 6;
      const int npieces = wh * nch;
#pragma unroll 1
      for (int c = 0; c < C; ++c) {
        const unsigned cbase = (unsigned)((((size_t)b * C + c) * HW + (size_t)wy0 * W + wx0) * 4);
#pragma unroll 4
        for (int pc = wave; pc < npieces; pc += 4) {
          const int r = pc / nch, j = pc - r * nch;
          const int q = 64 * j + lane;
          const unsigned voff = q < ww ? cbase + (unsigned)((r * W + q) * 4) : kOOB;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr)(rs_smem + c * plane + r * pitch + 64 * j), 4, voff, 0, 0, 0);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kRsPPT; ++k) {
    const int y = ty0 + k * 4 + wave;
    if (x < W && y < H) {
      float tL[C], tR[C], uL[C], uR[C];
      if (inw[k]) {
        const int oT = (yT[k] - wy0) * pitch, oB = (yB[k] - wy0) * pitch, oL = xL[k] - wx0, oR = xR[k] - wx0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float* p = rs_smem + c * plane;
          tL[c] = p[oT + oL]; tR[c] = p[oT + oR]; uL[c] = p[oB + oL]; uR[c] = p[oB + oR];
        }
      } else {
        const int xb = xL[k] < W - 2 ? xL[k] : W - 2;
        const bool l1 = xL[k] != xb, r1 = xR[k] != xb;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          tL[c] = l1 ? gt[k][c][1] : gt[k][c][0]; tR[c] = r1 ? gt[k][c][1] : gt[k][c][0];
          uL[c] = l1 ? gu[k][c][1] : gu[k][c][0]; uR[c] = r1 ? gu[k][c][1] : gu[k][c][0];
        }
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float v = w00[k] * tL[c];
        v += w01[k] * tR[c];
        v += w10[k] * uL[c];
        v += w11[k] * uR[c];
        out[((size_t)b * C + c) * HW + (size_t)y * W + x] = v;
      }
    }
  }
#endif
}

// ---- ChannelNorm: sqrt(sum_c x^2) ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void channelnorm_kernel(const float* __restrict__ in, float* __restrict__ out, int C,
                                                          size_t HW, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / HW, pix = i - b * HW;
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      const float v = in[(b * C + c) * HW + pix];
      s += v * v;
    }
    out[i] = sqrtf(s);
  }
}

// Four pixels per thread, 16-byte loads and stores (round 5): HW % 4 == 0 and 16-byte aligned planes.  Same per-pixel
// arithmetic and channel order as channelnorm_kernel (bit-identical); the grid covers the tensor once (no grid-stride tail).
__global__ __launch_bounds__(256) void channelnorm_vec4_kernel(const float4_t* __restrict__ in, float4_t* __restrict__ out, int C,
                                                               size_t HW4, size_t total4) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const size_t b = i / HW4, pix = i - b * HW4;
  float4_t s = {0.f, 0.f, 0.f, 0.f};
  if (C == 3) {          // (the FlowNet2 shape: all three loads in flight before the first use)
    const float4_t v0 = in[(b * 3 + 0) * HW4 + pix], v1 = in[(b * 3 + 1) * HW4 + pix], v2 = in[(b * 3 + 2) * HW4 + pix];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s[e] += v0[e] * v0[e];
      s[e] += v1[e] * v1[e];
      s[e] += v2[e] * v2[e];
    }
  } else {
    for (int c = 0; c < C; ++c) {
      const float4_t v = in[(b * C + c) * HW4 + pix];
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += v[e] * v[e];
    }
  }
  float4_t o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = sqrtf(s[e]);
  out[i] = o;     // (plain: non-temporal loads / stores measured 34.7 us against 11.7; two / four 16-byte pieces per thread: 11.4 / 12.4 against 11.2)
}

// ---- fused inter-network stage: warp img1 by flow, brightness error, 12-channel concat ------------------
template <typename T> __device__ __forceinline__ void ld8(const T* p, float (&v)[8]);
template <> __device__ __forceinline__ void ld8<half_t>(const half_t* p, float (&v)[8]) {
  const half8_t h = *reinterpret_cast<const half8_t*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (float)h[i];
}
template <> __device__ __forceinline__ void ld8<float>(const float* p, float (&v)[8]) {
  const float4_t a = reinterpret_cast<const float4_t*>(p)[0], b = reinterpret_cast<const float4_t*>(p)[1];
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}
template <typename T> __device__ __forceinline__ void st8(T* p, const float (&v)[8]);
template <> __device__ __forceinline__ void st8<half_t>(half_t* p, const float (&v)[8]) {
  half8_t h;
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = (half_t)v[i];
  *reinterpret_cast<half8_t*>(p) = h;
}
template <> __device__ __forceinline__ void st8<float>(float* p, const float (&v)[8]) {
  const float4_t a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
  reinterpret_cast<float4_t*>(p)[0] = a;
  reinterpret_cast<float4_t*>(p)[1] = b;
}

template <typename T>
__global__ __launch_bounds__(256) void flow_warp_concat_kernel(const T* __restrict__ x6, const float* __restrict__ flow,
                                                               float div_flow, T* __restrict__ y, int H, int W, int xl,
                                                               int xp, int yl, int yp, size_t total) {
  // one thread per PHYSICAL output pixel (b, yy, col): col in [yl, yl + W) carries data, the rest is zero
  const size_t HW = (size_t)H * W;
  for (size_t i = xcd_contiguous_block() * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int col = (int)(i % yp);
    const size_t row = i / yp;
    const size_t b = row / H;
    const int yy = (int)(row - b * H);
    const int xx = col - yl;
    float lo[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, hi[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if ((unsigned)xx < (unsigned)W) {
      const size_t pix = (size_t)yy * W + xx;
      const float dx = flow[(b * 2 + 0) * HW + pix], dy = flow[(b * 2 + 1) * HW + pix];
      const float xf = (float)xx + dx, yf = (float)yy + dy;
      const float fx = floorf(xf), fy = floorf(yf);
      const float alpha = xf - fx, beta = yf - fy;
      const int xL = (int)fminf(fmaxf(fx, 0.f), (float)(W - 1));
      const int xR = (int)fminf(fmaxf(fx + 1.f, 0.f), (float)(W - 1));
      const int yT = (int)fminf(fmaxf(fy, 0.f), (float)(H - 1));
      const int yB = (int)fminf(fmaxf(fy + 1.f, 0.f), (float)(H - 1));
      const float w00 = (1.f - alpha) * (1.f - beta), w01 = alpha * (1.f - beta);
      const float w10 = (1.f - alpha) * beta, w11 = alpha * beta;
      const T* img = x6 + b * (size_t)H * xp * 8;
      float c[8], tl[8], tr[8], bl[8], br[8];
      ld8<T>(img + ((size_t)yy * xp + xl + xx) * 8, c);
      ld8<T>(img + ((size_t)yT * xp + xl + xL) * 8, tl);
      ld8<T>(img + ((size_t)yT * xp + xl + xR) * 8, tr);
      ld8<T>(img + ((size_t)yB * xp + xl + xL) * 8, bl);
      ld8<T>(img + ((size_t)yB * xp + xl + xR) * 8, br);
      float warp[3], nrm = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float v = w00 * tl[3 + k];
        v += w01 * tr[3 + k];
        v += w10 * bl[3 + k];
        v += w11 * br[3 + k];
        warp[k] = v;
        const float d = c[k] - v;
        nrm += d * d;
      }
      lo[0] = c[0]; lo[1] = c[1]; lo[2] = c[2]; lo[3] = c[3]; lo[4] = c[4]; lo[5] = c[5]; lo[6] = warp[0]; lo[7] = warp[1];
      hi[0] = warp[2]; hi[1] = dx / div_flow; hi[2] = dy / div_flow; hi[3] = sqrtf(nrm);
    }
    if constexpr (std::is_same<T, half_t>::value) {
      // A pixel's 32 output bytes leave as two 16-byte pieces; written straight from the pixel's lane a wave's store touches
      // every other 16 bytes of 2 KB (half of 16 lines, twice).  Round 5: the lanes trade pieces first (ds_bpermute), so that
      // store s writes ONE contiguous KiB = pixels 32 s .. 32 s + 31 whole (lane l: pixel 32 s + l / 2, piece l % 2).  Needs
      // the wave's 64 pixels consecutive in memory: true here (thread = physical pixel, whole wave inside `total`, else fallback).
      half8_t hl, hh;
#pragma unroll
      for (int e = 0; e < 8; ++e) { hl[e] = (half_t)lo[e]; hh[e] = (half_t)hi[e]; }
      const uint4_t vl = __builtin_bit_cast(uint4_t, hl), vh = __builtin_bit_cast(uint4_t, hh);
      const int lane = threadIdx.x & 63;
      const size_t wave_first = i - lane;
      if (wave_first + 64 <= total) {                      // wave-uniform
#pragma unroll
        for (int sidx = 0; sidx < 2; ++sidx) {
          const int src = (lane >> 1) + 32 * sidx;
          uint4_t a, b;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a[e] = (unsigned)__shfl((int)vl[e], src);
            b[e] = (unsigned)__shfl((int)vh[e], src);
          }
          const uint4_t v = (lane & 1) ? b : a;
          *reinterpret_cast<uint4_t*>(y + (wave_first + 32 * sidx) * 16 + lane * 8) = v;
        }
      } else {
        *reinterpret_cast<uint4_t*>(y + i * 16) = vl;
        *reinterpret_cast<uint4_t*>(y + i * 16 + 8) = vh;
      }
    } else {
      st8<T>(y + i * 16, lo);
      st8<T>(y + i * 16 + 8, hi);
    }
  }
}

// ---- FlowNet2 fusion input (models.py:140-168): 11 channels per pixel from img0/img1 and two flow fields -----
// (img0, sd_flow, s2_flow, |sd_flow|, |s2_flow|, |img0 - warp(img1, sd_flow)|, |img0 - warp(img1, s2_flow)|):
// two Resample2d, four ChannelNorm and the concat of the reference in one pass; NHWC [B,H,W,16] out.
template <typename T>
__device__ __forceinline__ float warp_err(const T* __restrict__ img, int H, int W, int xl, int xp, int yy, int xx,
                                          float dx, float dy, const float (&c)[8]) {
  const float xf = (float)xx + dx, yf = (float)yy + dy;
  const float fx = floorf(xf), fy = floorf(yf);
  const float alpha = xf - fx, beta = yf - fy;
  const int xL = (int)fminf(fmaxf(fx, 0.f), (float)(W - 1));
  const int xR = (int)fminf(fmaxf(fx + 1.f, 0.f), (float)(W - 1));
  const int yT = (int)fminf(fmaxf(fy, 0.f), (float)(H - 1));
  const int yB = (int)fminf(fmaxf(fy + 1.f, 0.f), (float)(H - 1));
  const float w00 = (1.f - alpha) * (1.f - beta), w01 = alpha * (1.f - beta), w10 = (1.f - alpha) * beta, w11 = alpha * beta;
  float tl[8], tr[8], bl[8], br[8];
  ld8<T>(img + ((size_t)yT * xp + xl + xL) * 8, tl);
  ld8<T>(img + ((size_t)yT * xp + xl + xR) * 8, tr);
  ld8<T>(img + ((size_t)yB * xp + xl + xL) * 8, bl);
  ld8<T>(img + ((size_t)yB * xp + xl + xR) * 8, br);
  float nrm = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float v = w00 * tl[3 + k];
    v += w01 * tr[3 + k];
    v += w10 * bl[3 + k];
    v += w11 * br[3 + k];
    const float d = c[k] - v;
    nrm += d * d;
  }
  return sqrtf(nrm);
}

template <typename T>
__global__ __launch_bounds__(256) void flow_fusion_concat_kernel(const T* __restrict__ x6, const float* __restrict__ fsd,
                                                                 const float* __restrict__ fs2, T* __restrict__ y, int H, int W,
                                                                 int xl, int xp, int yl, int yp, size_t total) {
  const size_t HW = (size_t)H * W;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / HW, pix = i - b * HW;
    const int yy = (int)(pix / W), xx = (int)(pix - (size_t)yy * W);
    const T* img = x6 + b * (size_t)H * xp * 8;
    T* dst = y + (((size_t)b * H + yy) * yp + yl + xx) * 16;
    float c[8];
    ld8<T>(img + ((size_t)yy * xp + xl + xx) * 8, c);
    const float sdx = fsd[(b * 2 + 0) * HW + pix], sdy = fsd[(b * 2 + 1) * HW + pix];
    const float s2x = fs2[(b * 2 + 0) * HW + pix], s2y = fs2[(b * 2 + 1) * HW + pix];
    const float lo[8] = {c[0], c[1], c[2], sdx, sdy, s2x, s2y, sqrtf(sdx * sdx + sdy * sdy)};
    const float hi[8] = {sqrtf(s2x * s2x + s2y * s2y), warp_err<T>(img, H, W, xl, xp, yy, xx, sdx, sdy, c),
                         warp_err<T>(img, H, W, xl, xp, yy, xx, s2x, s2y, c), 0.f, 0.f, 0.f, 0.f, 0.f};
    st8<T>(dst, lo);
    st8<T>(dst + 8, hi);
  }
}

// nn.Upsample(scale_factor=4, mode='nearest') of (x * mul)  (models.py:59-60,448)
__global__ __launch_bounds__(256) void upsample_nearest4x_kernel(const float* __restrict__ x, float* __restrict__ y, int h, int w,
                                                                 size_t total, float mul) {
  const int H = 4 * h, W = 4 * w;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ox = (int)(i % W);
    const size_t t = i / W;
    const int oy = (int)(t % H);
    const size_t nc = t / H;
    y[i] = x[nc * (size_t)h * w + (size_t)(oy >> 2) * w + (ox >> 2)] * mul;
  }
}

// ==== backward (training) ===========================================================================================
// ---- Correlation backward, any parameters: one thread per input element gathers every output element it fed ----------
// The exact adjoint of correlation_nchw_kernel: in the forward, in1[ya, xa] meets in2[ya + tj*s2, xa + ti*s2] in output
// (tc, y, x) for every kernel offset (j, i) with ya = y*s1 + max_disp + krad - pad + j (same for x).  Correctness path only.
template <bool GRAD2>
__global__ __launch_bounds__(256) void correlation_bwd_gather_kernel(const float* __restrict__ feat, const float* __restrict__ g,
                                                                     float* __restrict__ grad, int C, int H, int W, int oh, int ow,
                                                                     int pad, int ksize, int max_disp, int s1, int s2, size_t total) {
  const int krad = (ksize - 1) / 2;
  const int drad = max_disp / s2;
  const int D = 2 * drad + 1;
  const float nelems = (float)(ksize * ksize * C);
  const size_t HW = (size_t)H * W, OHW = (size_t)oh * ow;
  const int base = max_disp + krad - pad;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int xq = (int)(idx % W);
    size_t t = idx / W;
    const int yq = (int)(t % H);
    t /= H;
    const int c = (int)(t % C);
    const size_t n = t / C;
    const float* pf = feat + (n * C + c) * HW;          // grad_in1: in2, grad_in2: in1
    const float* pg = g + n * (size_t)D * D * OHW;
    float acc = 0.f;
    for (int tc = 0; tc < D * D; ++tc) {
      const int ddy = (tc / D - drad) * s2, ddx = (tc % D - drad) * s2;
      const int ya = GRAD2 ? yq - ddy : yq, xa = GRAD2 ? xq - ddx : xq;   // in1 position
      const int yo = GRAD2 ? ya : yq + ddy, xo = GRAD2 ? xa : xq + ddx;   // the other operand
      if ((unsigned)yo >= (unsigned)H || (unsigned)xo >= (unsigned)W) continue;   // zero padding
      if (GRAD2 && ((unsigned)ya >= (unsigned)H || (unsigned)xa >= (unsigned)W)) continue;
      const float v = pf[(size_t)yo * W + xo];
      for (int j = -krad; j <= krad; ++j) {
        const int yy = ya - j - base;
        if (yy < 0 || yy % s1) continue;
        const int y = yy / s1;
        if (y >= oh) continue;
        for (int i = -krad; i <= krad; ++i) {
          const int xx = xa - i - base;
          if (xx < 0 || xx % s1) continue;
          const int x = xx / s1;
          if (x >= ow) continue;
          acc += pg[(size_t)tc * OHW + (size_t)y * ow + x] * v;
        }
      }
    }
    grad[idx] = acc / nelems;
  }
}

// ---- Correlation backward, kernel_size 1 / stride1 1 (every FlowNet in the reference) ----------------------------------
// With off = max_disp - pad and displacements d_t = s2 * (dy - drad, dx - drad):
//   grad_in1[c, p] = 1/C sum_t g[t, p - off] * in2[c, p + d_t]        grad_in2[c, q] = 1/C sum_t g[t, q - d_t - off] * in1[c, q - d_t]
// Workgroup = (image, row, 32*s2 pixels, 128/s2 channels), 128 threads.  Pixels are split by their residue mod s2: a thread owns
// four consecutive pixels of one residue class (stride s2 in x) and 8 channels, so for one displaced row dy the D horizontal
// displacements slide ONE class position at a time over the feature window: the D + 3 window values of a channel are read once
// from LDS and each feeds up to four FMAs with g values held in registers (D x 4 per thread and dy, reused by all 8 channels).
// Per dy the feature row window (TX + 2*drad*s2 pixels of every channel of the chunk) and the g slab of the D displacements of
// that dy are staged in LDS.  Fixed summation order (dy, channel chunk, class position): bit-reproducible.
constexpr int kCbwCh = 8;                                   // channels per thread: LDS <= 45 KiB per block for every stride2 (4 blocks per CU at stride2 2)
template <int DRAD, bool GRAD2>
__global__ __launch_bounds__(128, 2) void correlation_bwd_k1_kernel(const float* __restrict__ feat, const float* __restrict__ g,
                                                                 float* __restrict__ grad, int C, int H, int W, int oh, int ow,
                                                                 int off, int s2, int tiles_x, int cchunks, float inv_c) {
  constexpr int D = 2 * DRAD + 1;
  extern __shared__ float cb_smem[];
  const int TX = 32 * s2, R = DRAD * s2;
  const int PR = 32 + 2 * DRAD + 1;                         // class row pitch (odd: lanes of other residues / channels hit other banks)
  const int WWp = s2 * PR;                                  // channel pitch of the window
  const int WW = TX + 2 * R;                                // window pixels
  const int npg = 8 * s2, ncg = 128 / npg;
  const int CB = kCbwCh * ncg;
  float* win = cb_smem;                                     // [CB][s2][PR]
  float* gs = cb_smem + CB * WWp;                           // [D][s2][PR]
  int bid = blockIdx.x;
  const int tx = bid % tiles_x; bid /= tiles_x;
  const int cc = bid % cchunks; bid /= cchunks;
  const int row = bid % H;
  const size_t n = (size_t)(bid / H);
  const int x0 = tx * TX, c0 = cc * CB;
  const int tid = threadIdx.x;
  const int pg = tid % npg, cg = tid / npg;
  const int rr = pg % s2, u0 = (pg / s2) * 4;
  const size_t HW = (size_t)H * W, OHW = (size_t)oh * ow;
  const float* fb = feat + n * C * HW;
  const float* gb = g + n * (size_t)D * D * OHW;
  float acc[kCbwCh][4];
#pragma unroll
  for (int cl = 0; cl < kCbwCh; ++cl)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[cl][k] = 0.f;
  const int gw = GRAD2 ? WW : TX, gx0 = (GRAD2 ? x0 - R : x0) - off;
#pragma unroll 1
  for (int dy = 0; dy < D; ++dy) {
    const int ddy = (dy - DRAD) * s2;
    const int frow = GRAD2 ? row - ddy : row + ddy;
    const int grow = (GRAD2 ? row - ddy : row) - off;
    __syncthreads();                                        // the previous step's readers are done
    // staging: a thread keeps its window column(s) i = tid + 128 * r for every row (no per-element division)
    const bool frow_ok = (unsigned)frow < (unsigned)H;
    const bool grow_ok = (unsigned)grow < (unsigned)oh;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int i = tid + 128 * r;
      const int lo = (i % s2) * PR + i / s2;
      const int x = x0 - R + i, gx = gx0 + i;
      // all loads of a 32-row chunk are issued before the first LDS store (one memory round trip per chunk, not per row)
      if (i < WW) {
        const bool xok = frow_ok && (unsigned)x < (unsigned)W;
        const float* src = fb + (size_t)c0 * HW + (size_t)frow * W + x;
        for (int cl0 = 0; cl0 < CB; cl0 += 32) {
          float t[32];
#pragma unroll
          for (int j = 0; j < 32; ++j) t[j] = (xok && c0 + cl0 + j < C) ? src[(size_t)(cl0 + j) * HW] : 0.f;
#pragma unroll
          for (int j = 0; j < 32; ++j) win[(cl0 + j) * WWp + lo] = t[j];
        }
      }
      if (i < gw) {
        const bool gok = grow_ok && (unsigned)gx < (unsigned)ow;
        const float* src = gb + (size_t)dy * D * OHW + (size_t)grow * ow + gx;
        float t[D];
#pragma unroll
        for (int dxi = 0; dxi < D; ++dxi) t[dxi] = gok ? src[(size_t)dxi * OHW] : 0.f;
#pragma unroll
        for (int dxi = 0; dxi < D; ++dxi) gs[dxi * WWp + lo] = t[dxi];
      }
    }
    __syncthreads();
    // gr[e][k]: the g value that meets window class position u0 + k + e (grad_in1: e = dx; grad_in2: e = D - 1 - dx)
    float gr[D][4];
#pragma unroll
    for (int e = 0; e < D; ++e)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        gr[e][k] = GRAD2 ? gs[(D - 1 - e) * WWp + rr * PR + u0 + k + e] : gs[e * WWp + rr * PR + u0 + k];
#pragma unroll
    for (int cl = 0; cl < kCbwCh; ++cl) {
      const float* wp = win + (cl * ncg + cg) * WWp + rr * PR + u0;
#pragma unroll
      for (int j = 0; j < D + 3; ++j) {
        const float v = wp[j];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int e = j - k;
          if (e >= 0 && e < D) acc[cl][k] = fmaf(gr[e][k], v, acc[cl][k]);
        }
      }
    }
  }
#pragma unroll
  for (int cl = 0; cl < kCbwCh; ++cl) {
    const int c = c0 + cl * ncg + cg;
    if (c >= C) continue;
    float* o = grad + (n * C + c) * HW + (size_t)row * W;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = x0 + rr + s2 * (u0 + k);
      if (x < W) o[x] = acc[cl][k] * inv_c;
    }
  }
}

// ---- Resample2d backward: grad_flow (a gather, Resample2d_kernel.cu:118-186, same operation order) ------------------------
__global__ __launch_bounds__(256) void resample2d_bwd_flow_kernel(const float* __restrict__ in1, const float* __restrict__ flow,
                                                                  const float* __restrict__ gout, float* __restrict__ gflow,
                                                                  int C, int H, int W, size_t total) {
  const size_t HW = (size_t)H * W;
  for (size_t i = xcd_contiguous_block() * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / HW, pix = i - b * HW;
    const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
    const float xf = (float)x + flow[(b * 2 + 0) * HW + pix], yf = (float)y + flow[(b * 2 + 1) * HW + pix];
    const float fx = floorf(xf), fy = floorf(yf);
    const int xL = (int)fminf(fmaxf(fx, 0.f), (float)(W - 1));
    const int xR = (int)fminf(fmaxf(fx + 1.f, 0.f), (float)(W - 1));
    const int yT = (int)fminf(fmaxf(fy, 0.f), (float)(H - 1));
    const int yB = (int)fminf(fmaxf(fy + 1.f, 0.f), (float)(H - 1));
    const float gx = 1.f - (yf - fy), gy = 1.f - (xf - fx);   // the reference's gamma of channel 0 (x) / 1 (y)
    float ox = 0.f, oy = 0.f;
    for (int c = 0; c < C; ++c) {
      const float* p = in1 + (b * C + c) * HW;
      const float go = gout[(b * C + c) * HW + pix];
      const float tL = p[(size_t)yT * W + xL], tR = p[(size_t)yT * W + xR];
      const float bL = p[(size_t)yB * W + xL], bR = p[(size_t)yB * W + xR];
      ox += gx * go * tR;
      ox -= gx * go * tL;
      ox += (1.f - gx) * go * bR;
      ox -= (1.f - gx) * go * bL;
      oy += gy * go * bL;
      oy -= gy * go * tL;
      oy += (1.f - gy) * go * bR;
      oy -= (1.f - gy) * go * tR;
    }
    gflow[(b * 2 + 0) * HW + pix] = ox;
    gflow[(b * 2 + 1) * HW + pix] = oy;
  }
}

// ---- Resample2d backward: grad_in1 (a scatter) through an LDS window -------------------------------------------------------
// The forward's tiling (16 x 64 output pixels, 4 per thread) and bounding box of the taps.  The window is the box, or, when the
// box exceeds the budget, a kRsbClipPitch-wide region centred on the tile (as resample2d_window_kernel).  Per channel: zero the
// window, every pixel whose four taps lie inside adds them with ds_add_f32, the others with global float atomics; then the
// window's nonzero entries leave as global atomics, 64 lanes along a row (256 contiguous bytes per wave instruction).  Windows
// of neighbouring tiles overlap: the flush must add, and the sum's order (hence its last bits) is not fixed.  grad_in1 is
// zero-filled by the host entry point before this kernel.
constexpr int kRsbBudget = 3072, kRsbClipPitch = 96;        // window floats (one plane at a time: 12 KiB of LDS)
__global__ __launch_bounds__(256) void resample2d_bwd_in1_kernel(const float* __restrict__ flow, const float* __restrict__ gout,
                                                                 float* __restrict__ gin, int C, int H, int W, int tiles_x,
                                                                 int tiles_y) {
  __shared__ float win[kRsbBudget];
  __shared__ int s_box[4][4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles = tiles_x * tiles_y;
  const int b = blockIdx.x / tiles, trem = blockIdx.x - b * tiles;
  const int ty0 = (trem / tiles_x) * kRsTH, tx0 = (trem % tiles_x) * kRsTW;
  const size_t HW = (size_t)H * W;
  const int x = tx0 + lane;
  float w00[kRsPPT], w01[kRsPPT], w10[kRsPPT], w11[kRsPPT];
  int xL[kRsPPT], xR[kRsPPT], yT[kRsPPT], yB[kRsPPT];
  int bx0 = 0x7fffffff, bx1 = -1, by0 = 0x7fffffff, by1 = -1;
#pragma unroll
  for (int k = 0; k < kRsPPT; ++k) {
    const int y = ty0 + k * 4 + wave;
    const bool live = x < W && y < H;
    float dx = 0.f, dy = 0.f;
    if (live) {
      const size_t pix = (size_t)y * W + x;
      dx = flow[((size_t)b * 2 + 0) * HW + pix];
      dy = flow[((size_t)b * 2 + 1) * HW + pix];
    }
    const float xf = (float)x + dx, yf = (float)y + dy;
    const float fx = floorf(xf), fy = floorf(yf);
    const float alpha = xf - fx, beta = yf - fy;
    xL[k] = (int)fminf(fmaxf(fx, 0.f), (float)(W - 1));
    xR[k] = (int)fminf(fmaxf(fx + 1.f, 0.f), (float)(W - 1));
    yT[k] = (int)fminf(fmaxf(fy, 0.f), (float)(H - 1));
    yB[k] = (int)fminf(fmaxf(fy + 1.f, 0.f), (float)(H - 1));
    w00[k] = (1.f - alpha) * (1.f - beta); w01[k] = alpha * (1.f - beta);
    w10[k] = (1.f - alpha) * beta;         w11[k] = alpha * beta;
    if (live) {
      bx0 = min(bx0, xL[k]); bx1 = max(bx1, xR[k]);
      by0 = min(by0, yT[k]); by1 = max(by1, yB[k]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    bx0 = min(bx0, __shfl_xor(bx0, o)); bx1 = max(bx1, __shfl_xor(bx1, o));
    by0 = min(by0, __shfl_xor(by0, o)); by1 = max(by1, __shfl_xor(by1, o));
  }
  if (lane == 0) { s_box[wave][0] = bx0; s_box[wave][1] = bx1; s_box[wave][2] = by0; s_box[wave][3] = by1; }
  __syncthreads();
  bx0 = min(min(s_box[0][0], s_box[1][0]), min(s_box[2][0], s_box[3][0]));
  bx1 = max(max(s_box[0][1], s_box[1][1]), max(s_box[2][1], s_box[3][1]));
  by0 = min(min(s_box[0][2], s_box[1][2]), min(s_box[2][2], s_box[3][2]));
  by1 = max(max(s_box[0][3], s_box[1][3]), max(s_box[2][3], s_box[3][3]));
  if (bx1 < 0) return;                                     // (no live pixel: cannot happen for ceil-divided grids)
  int wx0 = bx0, wx1 = bx1, wy0 = by0, wy1 = by1;
  int ww = wx1 - wx0 + 1, wh = wy1 - wy0 + 1;
  if (ww * wh > kRsbBudget) {                              // clip around the tile
    const int cp = ww < kRsbClipPitch ? ww : kRsbClipPitch;
    const int rows = kRsbBudget / cp;
    int cx0 = tx0 - ((cp - (kRsTW + 1)) >> 1), cy0 = ty0 - ((rows - (kRsTH + 1)) >> 1);
    cx0 = max(min(cx0, wx1 - cp + 1), wx0);
    cy0 = max(min(cy0, wy1 - rows + 1), wy0);
    wx0 = cx0; wx1 = min(wx1, cx0 + cp - 1);
    wy0 = cy0; wy1 = min(wy1, cy0 + rows - 1);
    ww = wx1 - wx0 + 1; wh = wy1 - wy0 + 1;
  }
  bool inw[kRsPPT];
#pragma unroll
  for (int k = 0; k < kRsPPT; ++k) inw[k] = xL[k] >= wx0 && xR[k] <= wx1 && yT[k] >= wy0 && yB[k] <= wy1;
  const int wn = ww * wh;
#pragma unroll 1
  for (int c = 0; c < C; ++c) {
    for (int i = tid; i < wn; i += 256) win[i] = 0.f;
    __syncthreads();
    const size_t plane = ((size_t)b * C + c) * HW;
#pragma unroll
    for (int k = 0; k < kRsPPT; ++k) {
      const int y = ty0 + k * 4 + wave;
      if (x < W && y < H) {
        const float go = gout[plane + (size_t)y * W + x];
        if (inw[k]) {
          const int oT = (yT[k] - wy0) * ww, oB = (yB[k] - wy0) * ww, oL = xL[k] - wx0, oR = xR[k] - wx0;
          atomicAdd(&win[oT + oL], w00[k] * go);
          atomicAdd(&win[oT + oR], w01[k] * go);
          atomicAdd(&win[oB + oL], w10[k] * go);
          atomicAdd(&win[oB + oR], w11[k] * go);
        } else {
          float* p = gin + plane;
          unsafeAtomicAdd(p + (size_t)yT[k] * W + xL[k], w00[k] * go);
          unsafeAtomicAdd(p + (size_t)yT[k] * W + xR[k], w01[k] * go);
          unsafeAtomicAdd(p + (size_t)yB[k] * W + xL[k], w10[k] * go);
          unsafeAtomicAdd(p + (size_t)yB[k] * W + xR[k], w11[k] * go);
        }
      }
    }
    __syncthreads();
    for (int r = wave; r < wh; r += 4) {
      float* dst = gin + plane + (size_t)(wy0 + r) * W + wx0;
      for (int q = lane; q < ww; q += 64) {
        const float v = win[r * ww + q];
        if (v != 0.f) unsafeAtomicAdd(dst + q, v);
      }
    }
    __syncthreads();                                       // the flush has read the window before the next channel zeroes it
  }
}

// ---- ChannelNorm backward: grad_in1 = grad_out * in1 / (out + 1e-9), ChannelNorm_kernel.cu:54-81 ----------------------------
// The reference's 1e-9 is a double literal: the quotient is taken in double and rounded once, as there.
__device__ __forceinline__ float cn_bwd(float go, float x, float o) { return (float)((double)(go * x) / ((double)o + 1e-9)); }
__global__ __launch_bounds__(256) void channelnorm_bwd_kernel(const float* __restrict__ in, const float* __restrict__ out,
                                                              const float* __restrict__ gout, float* __restrict__ gin, int C,
                                                              size_t HW, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / HW, pix = i - b * HW;
    const float go = gout[i], o = out[i];
    for (int c = 0; c < C; ++c) {
      const size_t e = (b * C + c) * HW + pix;
      gin[e] = cn_bwd(go, in[e], o);
    }
  }
}
// four pixels per thread, 16-byte loads and stores: HW % 4 == 0 and 16-byte aligned planes
__global__ __launch_bounds__(256) void channelnorm_bwd_vec4_kernel(const float4_t* __restrict__ in, const float4_t* __restrict__ out,
                                                                   const float4_t* __restrict__ gout, float4_t* __restrict__ gin,
                                                                   int C, size_t HW4, size_t total4) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const size_t b = i / HW4, pix = i - b * HW4;
  const float4_t go = gout[i], o = out[i];
  for (int c = 0; c < C; ++c) {
    const size_t e = (b * C + c) * HW4 + pix;
    const float4_t x = in[e];
    float4_t r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = cn_bwd(go[k], x[k], o[k]);
    gin[e] = r;
  }
}

static inline int grid_for(size_t total) {
  size_t g = (total + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

constexpr int kCorrGX = 3;  // horizontal displacements per thread

}  // namespace ft

using namespace ft;

extern "C" int ft_correlation_out_shape(int C, int H, int W, int pad_size, int kernel_size, int max_displacement,
                                        int stride1, int stride2, int* out_c, int* out_h, int* out_w) {
  if (C <= 0 || H <= 0 || W <= 0 || pad_size < 0 || kernel_size <= 0 || max_displacement < 0 || stride1 <= 0 ||
      stride2 <= 0)
    return FT_ERR_INVALID_ARG;
  // correlation_cuda.c:25-35
  const int krad = (kernel_size - 1) / 2;
  const int border = krad + max_displacement;
  const int ph = H + 2 * pad_size, pw = W + 2 * pad_size;
  const int D = (max_displacement / stride2) * 2 + 1;
  const int oh = (ph - 2 * border + stride1 - 1) / stride1;  // ceil
  const int ow = (pw - 2 * border + stride1 - 1) / stride1;
  if (oh <= 0 || ow <= 0) return FT_ERR_INVALID_ARG;
  if (out_c) *out_c = D * D;
  if (out_h) *out_h = oh;
  if (out_w) *out_w = ow;
  return FT_OK;
}

extern "C" int ft_correlation_fwd(const float* in1, const float* in2, float* out, int B, int C, int H, int W,
                                  int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                                  int corr_type_multiply, ft_stream_t stream) {
  if (!in1 || !in2 || !out || B <= 0) return FT_ERR_INVALID_ARG;
  if (corr_type_multiply != 1) return FT_ERR_UNSUPPORTED;
  int oc, oh, ow;
  int st = ft_correlation_out_shape(C, H, W, pad_size, kernel_size, max_displacement, stride1, stride2, &oc, &oh, &ow);
  if (st != FT_OK) return st;
  const size_t total = (size_t)B * oc * oh * ow;
  hipLaunchKernelGGL(correlation_nchw_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), in1, in2, out, C, H,
                     W, oc, oh, ow, pad_size, kernel_size, max_displacement, stride1, stride2, total);
  FT_LAUNCH_CHECK("correlation_nchw_kernel");
  return FT_OK;
}

// The one place that decides which kernel a call of ft_correlation_nhwc_fwd runs, and with which sizes (pure host code:
// ft_correlation_nhwc_form reports the form, the launch path takes everything from here).
// The two rows kernels fold the activation into max(v * k_pos, v * k_neg), which is act(v) only for a slope in [0, 1] and is
// not torch's value for a -inf sum when the slope is 0 (max(-inf, -inf * 0 = NaN) = -inf; torch: ReLU 0, leaky NaN): ReLU
// and leaky slopes outside (0, 1] take the one-row kernel, whose corr_act is right for every slope and every input.
struct CorrPlan {
  int form;                          // FT_CORR_FORM_*
  int D;                             // displacements per axis
  unsigned long long f_bytes, y_bytes;
  size_t lds;                        // dynamic LDS of the VALU form
};

static int correlation_nhwc_plan(int B, int C, int H, int W, int max_displacement, int stride2, int f_cstride, int y_cstride,
                                 int y_coff, int act, float slope, int dtype, CorrPlan* p) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || max_displacement < 0 || stride2 <= 0) return FT_ERR_INVALID_ARG;
  if (dtype != FT_F16 && dtype != FT_F32) return FT_ERR_INVALID_ARG;
  if (C % 8 || f_cstride % 8 || f_cstride < C) return FT_ERR_INVALID_ARG;
  p->D = (max_displacement / stride2) * 2 + 1;
  if (y_coff < 0 || y_cstride < y_coff + p->D * p->D) return FT_ERR_INVALID_ARG;
  const size_t esz = dtype_size(dtype);
  p->f_bytes = (unsigned long long)B * H * W * f_cstride * esz;
  p->y_bytes = (unsigned long long)B * H * W * y_cstride * esz;
  p->lds = 0;
  if (dtype == FT_F16 && stride2 == 2 && max_displacement % 2 == 0 && max_displacement <= 32 && C == 256 &&
      p->f_bytes < (1ull << 31)) {
    const bool rows_act_ok = act != FT_ACT_RELU && !(act == FT_ACT_LEAKY && !(slope > 0.f && slope <= 1.f));
    if (max_displacement == 20 && p->y_bytes < (1ull << 31) && rows_act_ok)
      p->form = W <= 64 && y_coff % 8 == 0 && y_cstride % 8 == 0 ? FT_CORR_FORM_ROWS64 : FT_CORR_FORM_ROWS;
    else
      p->form = FT_CORR_FORM_MFMA;
    return FT_OK;
  }
  // fp16: 32-pixel tiles / 256 threads; fp32 (parity mode): 16-pixel tiles / 128 threads (LDS budget)
  const size_t pstride = C * esz + 16;
  const int tx = dtype == FT_F16 ? 32 : 16;
  p->lds = (size_t)(tx + tx + 2 * max_displacement) * pstride + (size_t)tx * p->D * p->D * 4;
  if (p->lds > 160 * 1024) return FT_ERR_UNSUPPORTED;
  p->form = FT_CORR_FORM_VALU;
  return FT_OK;
}

extern "C" int ft_correlation_nhwc_form(int B, int C, int H, int W, int max_displacement, int stride2, int f_cstride,
                                        int y_cstride, int y_coff, int act, float slope, int dtype) {
  CorrPlan p;
  return correlation_nhwc_plan(B, C, H, W, max_displacement, stride2, f_cstride, y_cstride, y_coff, act, slope, dtype, &p) ==
                 FT_OK ? p.form : -1;
}

extern "C" int ft_correlation_nhwc_fwd(const void* f1, const void* f2, void* y, int B, int C, int H, int W,
                                       int max_displacement, int stride2, int f_cstride, int y_cstride, int y_coff,
                                       int act, float slope, int dtype, ft_stream_t stream) {
  if (!f1 || !f2 || !y) return FT_ERR_INVALID_ARG;
  CorrPlan plan;
  const int st = correlation_nhwc_plan(B, C, H, W, max_displacement, stride2, f_cstride, y_cstride, y_coff, act, slope, dtype,
                                       &plan);
  if (st != FT_OK) return st;
  const int form = plan.form;
  const unsigned long long f_bytes = plan.f_bytes, y_bytes = plan.y_bytes;
  if (form != FT_CORR_FORM_VALU) {
    const int drad = max_displacement / 2;
    if (form == FT_CORR_FORM_ROWS64) {
      // FlowNetC's shape on maps up to 64 wide: 64-column ring slots, six waves, 3 output rows per workgroup
      static const int cdbg = ft::dev_env_int("FT_CORR_DBG", 0);   // dev ablation, timing only: see the kernel
      constexpr int R = 3;
      auto k = correlation_mfma_rows64_kernel<16, R, 10>;
      constexpr size_t ldst = 4 * 64 * 512 + 512 + 128 + 1024;     // ring, zero row, pad, scratch KiB
      static bool raised[64] = {};
      int dev = 0;
      FT_HIP_CHECK(hipGetDevice(&dev));
      if (dev < 0 || dev >= 64 || !raised[dev]) {
        FT_HIP_CHECK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldst));
        if (dev >= 0 && dev < 64) raised[dev] = true;
      }
      const int ngy = 2 * ceil_div((H + 1) / 2, R);
      hipLaunchKernelGGL(k, dim3(ngy * B), dim3(64 * kCorr64Waves), ldst, as_stream(stream), static_cast<const half_t*>(f1),
                         static_cast<const half_t*>(f2), static_cast<half_t*>(y), H, W, (unsigned)f_bytes, (unsigned)y_bytes,
                         f_cstride, y_cstride, y_coff, act | (cdbg << 8), slope, ngy);
      FT_LAUNCH_CHECK("correlation_mfma_rows64_kernel");
      return FT_OK;
    }
    if (form == FT_CORR_FORM_ROWS) {     // FlowNetC's shape: 3 output rows per workgroup
      constexpr int R = 3;
      auto k = correlation_mfma_rows_kernel<16, R, 10>;
      constexpr size_t lds3 = 3 * (((size_t)(64 + 40) * 512 + 1023) / 1024 * 1024);
      static bool raised[64] = {};
      int dev = 0;
      FT_HIP_CHECK(hipGetDevice(&dev));
      if (dev < 0 || dev >= 64 || !raised[dev]) {
        FT_HIP_CHECK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3));
        if (dev >= 0 && dev < 64) raised[dev] = true;
      }
      const int groups = ceil_div((H + 1) / 2, R);
      const int ngx = ceil_div(W, 64), ngy = 2 * groups;
      hipLaunchKernelGGL(k, dim3(ngx * ngy * B), dim3(256), lds3, as_stream(stream), static_cast<const half_t*>(f1),
                         static_cast<const half_t*>(f2), static_cast<half_t*>(y), H, W, (unsigned)f_bytes, (unsigned)y_bytes,
                         f_cstride, y_cstride, y_coff, act, slope, ngx, ngy);
      FT_LAUNCH_CHECK("correlation_mfma_rows_kernel");
      return FT_OK;
    }
    const size_t stage = ((size_t)(64 + 4 * drad) * C * 2 + 1023) / 1024 * 1024;
    const size_t lds2 = 2 * stage;
    auto k = correlation_mfma_kernel<16>;
    FT_RAISE_LDS(k, 160 * 1024);
    hipLaunchKernelGGL(k, dim3(ceil_div(W, 64), H, B), dim3(256), lds2, as_stream(stream), static_cast<const half_t*>(f1),
                       static_cast<const half_t*>(f2), static_cast<half_t*>(y), H, W, drad, (unsigned)f_bytes, f_cstride,
                       y_cstride, y_coff, act, slope);
    FT_LAUNCH_CHECK("correlation_mfma_kernel");
    return FT_OK;
  }
  const size_t lds = plan.lds;
  dim3 grid(ceil_div(W, dtype == FT_F16 ? 32 : 16) * H, B);
  if (dtype == FT_F16) {
    auto k = correlation_nhwc_kernel<half_t, 32, kCorrGX, 256>;
    if (lds > 64 * 1024) FT_HIP_CHECK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, grid, dim3(256), lds, as_stream(stream), static_cast<const half_t*>(f1),
                       static_cast<const half_t*>(f2), static_cast<half_t*>(y), C, H, W, max_displacement, stride2,
                       f_cstride, y_cstride, y_coff, act, slope);
  } else {
    auto k = correlation_nhwc_kernel<float, 16, kCorrGX, 128>;
    if (lds > 64 * 1024) FT_HIP_CHECK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, grid, dim3(128), lds, as_stream(stream), static_cast<const float*>(f1),
                       static_cast<const float*>(f2), static_cast<float*>(y), C, H, W, max_displacement, stride2,
                       f_cstride, y_cstride, y_coff, act, slope);
  }
  FT_LAUNCH_CHECK("correlation_nhwc_kernel");
  return FT_OK;
}

extern "C" int ft_resample2d_fwd(const float* in1, const float* flow, float* out, int B, int C, int H, int W,
                                 ft_stream_t stream) {
  if (!in1 || !flow || !out || B <= 0 || C <= 0 || H <= 0 || W <= 0) return FT_ERR_INVALID_ARG;
  const size_t total = (size_t)B * H * W;
  const unsigned long long in_bytes = (unsigned long long)B * C * H * W * 4ull;
  if (C >= 1 && C <= 4 && W >= 2 && in_bytes < (1ull << 31)) {
    const int tiles_x = ceil_div(W, kRsTW), tiles_y = ceil_div(H, kRsTH);
    const long long nblk = (long long)B * tiles_x * tiles_y;
    if (nblk <= 0x7fffffffLL) {
      const dim3 grid((unsigned)nblk);
      // window budget per plane (floats): the LDS a workgroup reserves = C x budget x 4 bytes decides how many workgroups share a CU
      // (26 KiB per plane: two; 10 KiB: five); tiles whose window exceeds it keep a clipped window and gather the rest.  Budgets
      // from 1536 to 6656 floats were timed on noise and smooth flows: profiles/HISTORY.md ("Retired A/B switches").
      constexpr int wbudget = 2560;
      const size_t lds = (size_t)C * wbudget * sizeof(float);
#define FT_RS_LAUNCH(CC)                                                                                                   \
  {                                                                                                                        \
    auto kw = resample2d_window_kernel<CC>;                                                                                \
    hipLaunchKernelGGL(kw, grid, dim3(256), lds, as_stream(stream), in1, flow, out, H, W, tiles_x, tiles_y, (unsigned)in_bytes, wbudget); \
  }
      switch (C) {
        case 1: FT_RS_LAUNCH(1) break;
        case 2: FT_RS_LAUNCH(2) break;
        case 3: FT_RS_LAUNCH(3) break;
        default: FT_RS_LAUNCH(4) break;
      }
#undef FT_RS_LAUNCH
      FT_LAUNCH_CHECK("resample2d_window_kernel");
      return FT_OK;
    }
  }
  if (W >= 2 && C >= 1 && C <= 4 && (long long)H * W < (1LL << 31)) {
    const dim3 grid(grid_for(total));
    switch (C) {
      case 1: hipLaunchKernelGGL(resample2d_pair_kernel<1>, grid, dim3(256), 0, as_stream(stream), in1, flow, out, H, W, total); break;
      case 2: hipLaunchKernelGGL(resample2d_pair_kernel<2>, grid, dim3(256), 0, as_stream(stream), in1, flow, out, H, W, total); break;
      case 3: hipLaunchKernelGGL(resample2d_pair_kernel<3>, grid, dim3(256), 0, as_stream(stream), in1, flow, out, H, W, total); break;
      default: hipLaunchKernelGGL(resample2d_pair_kernel<4>, grid, dim3(256), 0, as_stream(stream), in1, flow, out, H, W, total); break;
    }
    FT_LAUNCH_CHECK("resample2d_pair_kernel");
    return FT_OK;
  }
  hipLaunchKernelGGL(resample2d_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), in1, flow, out, C, H, W,
                     total);
  FT_LAUNCH_CHECK("resample2d_kernel");
  return FT_OK;
}

extern "C" int ft_channelnorm_fwd(const float* in1, float* out, int B, int C, int H, int W, ft_stream_t stream) {
  if (!in1 || !out || B <= 0 || C <= 0 || H <= 0 || W <= 0) return FT_ERR_INVALID_ARG;
  const size_t HW = (size_t)H * W, total = (size_t)B * HW;
  if (HW % 4 == 0 && (reinterpret_cast<uintptr_t>(in1) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && total / 4 / 256 < (1u << 30)) {
    const size_t total4 = total / 4;
    hipLaunchKernelGGL(channelnorm_vec4_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float4_t*>(in1), reinterpret_cast<float4_t*>(out), C, HW / 4, total4);
    FT_LAUNCH_CHECK("channelnorm_vec4_kernel");
    return FT_OK;
  }
  hipLaunchKernelGGL(channelnorm_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), in1, out, C, HW, total);
  FT_LAUNCH_CHECK("channelnorm_kernel");
  return FT_OK;
}

extern "C" int ft_flow_warp_concat(const void* x6, const float* flow, float div_flow, void* y, int B, int H, int W,
                                   int x_lpad, int x_wpitch, int y_lpad, int y_wpitch, int dtype, ft_stream_t stream) {
  if (!x6 || !flow || !y || B <= 0 || H <= 0 || W <= 0 || div_flow == 0.f) return FT_ERR_INVALID_ARG;
  if (x_lpad < 0 || y_lpad < 0 || x_wpitch < x_lpad + W || y_wpitch < y_lpad + W) return FT_ERR_INVALID_ARG;
  if (dtype != FT_F16 && dtype != FT_F32) return FT_ERR_INVALID_ARG;
  const size_t total = (size_t)B * H * y_wpitch;
  if (dtype == FT_F16)
    hipLaunchKernelGGL(flow_warp_concat_kernel<half_t>, dim3(grid_for(total)), dim3(256), 0, as_stream(stream),
                       static_cast<const half_t*>(x6), flow, div_flow, static_cast<half_t*>(y), H, W, x_lpad, x_wpitch,
                       y_lpad, y_wpitch, total);
  else
    hipLaunchKernelGGL(flow_warp_concat_kernel<float>, dim3(grid_for(total)), dim3(256), 0, as_stream(stream),
                       static_cast<const float*>(x6), flow, div_flow, static_cast<float*>(y), H, W, x_lpad, x_wpitch,
                       y_lpad, y_wpitch, total);
  FT_LAUNCH_CHECK("flow_warp_concat_kernel");
  return FT_OK;
}

extern "C" int ft_flow_fusion_concat(const void* x6, const float* flow_sd, const float* flow_s2, void* y, int B, int H, int W,
                                     int x_lpad, int x_wpitch, int y_lpad, int y_wpitch, int dtype, ft_stream_t stream) {
  if (!x6 || !flow_sd || !flow_s2 || !y || B <= 0 || H <= 0 || W <= 0) return FT_ERR_INVALID_ARG;
  if (x_lpad < 0 || x_wpitch < x_lpad + W || y_lpad < 0 || y_wpitch < y_lpad + W) return FT_ERR_INVALID_ARG;
  if (dtype != FT_F16 && dtype != FT_F32) return FT_ERR_INVALID_ARG;
  const size_t total = (size_t)B * H * W;
  if (dtype == FT_F16)
    hipLaunchKernelGGL(flow_fusion_concat_kernel<half_t>, dim3(grid_for(total)), dim3(256), 0, as_stream(stream),
                       static_cast<const half_t*>(x6), flow_sd, flow_s2, static_cast<half_t*>(y), H, W, x_lpad, x_wpitch,
                       y_lpad, y_wpitch, total);
  else
    hipLaunchKernelGGL(flow_fusion_concat_kernel<float>, dim3(grid_for(total)), dim3(256), 0, as_stream(stream),
                       static_cast<const float*>(x6), flow_sd, flow_s2, static_cast<float*>(y), H, W, x_lpad, x_wpitch,
                       y_lpad, y_wpitch, total);
  FT_LAUNCH_CHECK("flow_fusion_concat_kernel");
  return FT_OK;
}

extern "C" int ft_upsample_nearest4x(const float* x, float* y, int N, int C, int h, int w, float mul, ft_stream_t stream) {
  if (!x || !y || N <= 0 || C <= 0 || h <= 0 || w <= 0) return FT_ERR_INVALID_ARG;
  const size_t total = (size_t)N * C * 16 * h * w;
  hipLaunchKernelGGL(upsample_nearest4x_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), x, y, h, w, total, mul);
  FT_LAUNCH_CHECK("upsample_nearest4x_kernel");
  return FT_OK;
}

// ==== backward entry points ===========================================================================================
template <int DRAD>
static int launch_correlation_bwd_k1(const float* feat, const float* g, float* grad, bool grad2, int B, int C, int H, int W, int oh,
                                     int ow, int off, int s2, hipStream_t stream) {
  const int TX = 32 * s2, ncg = 128 / (8 * s2), CB = kCbwCh * ncg;
  const int tiles_x = ceil_div(W, TX), cchunks = ceil_div(C, CB);
  const size_t lds = (size_t)(CB + 2 * DRAD + 1) * s2 * (32 + 2 * DRAD + 1) * sizeof(float);
  const long long nblk = (long long)B * H * cchunks * tiles_x;
  if (nblk > 0x7fffffffLL) return FT_ERR_UNSUPPORTED;
  auto k = grad2 ? correlation_bwd_k1_kernel<DRAD, true> : correlation_bwd_k1_kernel<DRAD, false>;
  if (lds > 64 * 1024) return FT_ERR_UNSUPPORTED;                 // (cannot happen: <= 45 KiB for stride2 <= 4, drad <= 10)
  hipLaunchKernelGGL(k, dim3((unsigned)nblk), dim3(128), lds, stream, feat, g, grad, C, H, W, oh, ow, off, s2, tiles_x, cchunks,
                     1.f / (float)C);
  FT_LAUNCH_CHECK("correlation_bwd_k1_kernel");
  return FT_OK;
}

extern "C" int ft_correlation_bwd(const float* in1, const float* in2, const float* grad_out, float* grad_in1, float* grad_in2,
                                  int B, int C, int H, int W, int pad_size, int kernel_size, int max_displacement, int stride1,
                                  int stride2, int corr_type_multiply, ft_stream_t stream) {
  if (!in1 || !in2 || !grad_out || (!grad_in1 && !grad_in2) || B <= 0) return FT_ERR_INVALID_ARG;
  if (corr_type_multiply != 1) return FT_ERR_UNSUPPORTED;
  int oc, oh, ow;
  int st = ft_correlation_out_shape(C, H, W, pad_size, kernel_size, max_displacement, stride1, stride2, &oc, &oh, &ow);
  if (st != FT_OK) return st;
  const hipStream_t s = as_stream(stream);
  const int drad = max_displacement / stride2;
  // fast path: kernel 1, stride1 1, 1 <= drad <= 10, stride2 in {1, 2, 4} (the tile = 32 pixels of each residue mod stride2)
  if (kernel_size == 1 && stride1 == 1 && drad >= 1 && drad <= 10 && (stride2 == 1 || stride2 == 2 || stride2 == 4)) {
    const int off = max_displacement - pad_size;
    for (int which = 0; which < 2; ++which) {
      float* grad = which ? grad_in2 : grad_in1;
      if (!grad) continue;
      const float* feat = which ? in1 : in2;
#define FT_CB_CASE(R) \
  case R: st = launch_correlation_bwd_k1<R>(feat, grad_out, grad, which == 1, B, C, H, W, oh, ow, off, stride2, s); break;
      switch (drad) {
        FT_CB_CASE(1) FT_CB_CASE(2) FT_CB_CASE(3) FT_CB_CASE(4) FT_CB_CASE(5)
        FT_CB_CASE(6) FT_CB_CASE(7) FT_CB_CASE(8) FT_CB_CASE(9) FT_CB_CASE(10)
      }
#undef FT_CB_CASE
      if (st != FT_OK) return st;
    }
    return FT_OK;
  }
  const size_t total = (size_t)B * C * H * W;
  if (grad_in1) {
    hipLaunchKernelGGL(correlation_bwd_gather_kernel<false>, dim3(grid_for(total)), dim3(256), 0, s, in2, grad_out, grad_in1, C, H,
                       W, oh, ow, pad_size, kernel_size, max_displacement, stride1, stride2, total);
    FT_LAUNCH_CHECK("correlation_bwd_gather_kernel");
  }
  if (grad_in2) {
    hipLaunchKernelGGL(correlation_bwd_gather_kernel<true>, dim3(grid_for(total)), dim3(256), 0, s, in1, grad_out, grad_in2, C, H,
                       W, oh, ow, pad_size, kernel_size, max_displacement, stride1, stride2, total);
    FT_LAUNCH_CHECK("correlation_bwd_gather_kernel");
  }
  return FT_OK;
}

extern "C" int ft_resample2d_bwd(const float* in1, const float* flow, const float* grad_out, float* grad_in1, float* grad_flow,
                                 int B, int C, int H, int W, ft_stream_t stream) {
  if (!in1 || !flow || !grad_out || (!grad_in1 && !grad_flow) || B <= 0 || C <= 0 || H <= 0 || W <= 0) return FT_ERR_INVALID_ARG;
  const hipStream_t s = as_stream(stream);
  const size_t total = (size_t)B * H * W;
  if (grad_flow) {
    hipLaunchKernelGGL(resample2d_bwd_flow_kernel, dim3(grid_for(total)), dim3(256), 0, s, in1, flow, grad_out, grad_flow, C, H, W,
                       total);
    FT_LAUNCH_CHECK("resample2d_bwd_flow_kernel");
  }
  if (grad_in1) {
    const int tiles_x = ceil_div(W, kRsTW), tiles_y = ceil_div(H, kRsTH);
    const long long nblk = (long long)B * tiles_x * tiles_y;
    if (nblk > 0x7fffffffLL) return FT_ERR_UNSUPPORTED;
    FT_HIP_CHECK(hipMemsetAsync(grad_in1, 0, (size_t)B * C * H * W * sizeof(float), s));
    hipLaunchKernelGGL(resample2d_bwd_in1_kernel, dim3((unsigned)nblk), dim3(256), 0, s, flow, grad_out, grad_in1, C, H, W, tiles_x,
                       tiles_y);
    FT_LAUNCH_CHECK("resample2d_bwd_in1_kernel");
  }
  return FT_OK;
}

extern "C" int ft_channelnorm_bwd(const float* in1, const float* out, const float* grad_out, float* grad_in1, int B, int C, int H,
                                  int W, ft_stream_t stream) {
  if (!in1 || !out || !grad_out || !grad_in1 || B <= 0 || C <= 0 || H <= 0 || W <= 0) return FT_ERR_INVALID_ARG;
  const size_t HW = (size_t)H * W, total = (size_t)B * HW;
  const bool aligned = ((reinterpret_cast<uintptr_t>(in1) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(grad_out) |
                         reinterpret_cast<uintptr_t>(grad_in1)) & 15) == 0;
  if (HW % 4 == 0 && aligned && total / 4 / 256 < (1u << 30)) {
    const size_t total4 = total / 4;
    hipLaunchKernelGGL(channelnorm_bwd_vec4_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float4_t*>(in1), reinterpret_cast<const float4_t*>(out),
                       reinterpret_cast<const float4_t*>(grad_out), reinterpret_cast<float4_t*>(grad_in1), C, HW / 4, total4);
    FT_LAUNCH_CHECK("channelnorm_bwd_vec4_kernel");
    return FT_OK;
  }
  hipLaunchKernelGGL(channelnorm_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), in1, out, grad_out, grad_in1, C,
                     HW, total);
  FT_LAUNCH_CHECK("channelnorm_bwd_kernel");
  return FT_OK;
}
