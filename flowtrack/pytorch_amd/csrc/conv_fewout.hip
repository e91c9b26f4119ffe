// The conv kernels for layers with <= 4 output channels (FlowNet predict_flow), where a GEMM tile would idle: the dot-product
// kernel conv_fewout_kernel (fp16, fp32) and the two LDS-patch forms conv_pflow_kernel / conv_pflow_mfma_kernel (fp16).
// Split from conv_igemm.hip; the host side meets the dispatcher in conv_dispatch.h.
#include "conv_dispatch.h"

namespace ft {

// ---- few-output-channel conv (FlowNet predict_flow: Cout = 2, K up to 9 * 1026) -----------------------
// A GEMM tile would leave 30/32 MFMA columns idle and serialise a 9k-long K loop in a handful of
// workgroups.  Instead: one wave per group of PIX consecutive output pixels, the 64 lanes split the
// (tap, channel-group) axis with 16-byte coalesced loads, fp32 dot products (v_dot2_f32_f16 for fp16: no
// explicit converts), a transpose-reduce butterfly (PIX*NCO values -> one per lane group), the (tiny) weight
// set in LDS once per workgroup, each weight vector reused for PIX pixels from registers.
// Uses the generic packed layout [Cout_pad][Kpad].
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float dot8(const uint4_t& a, const uint4_t& b, float c, half_t*) {
  // whole-vector bit casts only (bit_cast of one vector element reads element 0, see mma_slice)
  const half8_t ah = __builtin_bit_cast(half8_t, a), bh = __builtin_bit_cast(half8_t, b);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const half2_t a2 = {ah[2 * q], ah[2 * q + 1]}, b2 = {bh[2 * q], bh[2 * q + 1]};
    c = __builtin_amdgcn_fdot2(a2, b2, c, false);
  }
  return c;
}
__device__ __forceinline__ float dot8(const uint4_t& a, const uint4_t& b, float c, float*) {
  const float4_t af = __builtin_bit_cast(float4_t, a), bf = __builtin_bit_cast(float4_t, b);
#pragma unroll
  for (int q = 0; q < 4; ++q) c += af[q] * bf[q];
  return c;
}

template <typename T, int NCO, int PIX>
__global__ __launch_bounds__(256) void conv_fewout_kernel(const ConvParams p, int ppb) {
  constexpr int VEC = Elem<T>::VEC;
  constexpr int NV = PIX * NCO;  // partial sums per lane
  static_assert(NV == 8, "the reduction below folds exactly 8 values over the 64 lanes");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nvec = p.kh * p.kw * p.cin_groups;   // 16-byte vectors along K per output pixel
  // Round 5: no weight staging and no branches around the loads.  A wave makes ONE pass over its PIX pixels (ppb = 16 for every
  // layer below 32 k pixels), so copying the weight set into LDS first bought nothing but a barrier; and the input loads sat
  // each in its own divergent region behind a full wait (18 K steps x 4 dependent L2 round trips: 20 us for 28 MFLOP at
  // FlowNet's predict_flow6).  Now: weights straight from L2 (every wave reads the same lines), inputs as buffer loads whose
  // offset is out of range where the tap leaves the image, two K vectors per lane in flight = 12 independent loads per wait.
  const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.x), 0, p.x_bytes, 0x00020000);
  constexpr unsigned kOOB = 0x80000000u;
  const int m_begin = blockIdx.x * ppb;
  const int m_end = m_begin + ppb < p.M ? m_begin + ppb : p.M;
  const int tap0 = lane / p.cin_groups;
  const int cg0 = lane - tap0 * p.cin_groups;
  for (int m = m_begin + wave * PIX; m < m_end; m += 4 * PIX) {
    // decode PIX consecutive output pixels (one division pair, then carries)
    int pn[PIX], py_[PIX], px_[PIX];
    {
      int n = m / p.HqWq;
      const int rem = m - n * p.HqWq;
      int oy = rem / p.Wq;
      int ox = rem - oy * p.Wq;
#pragma unroll
      for (int i = 0; i < PIX; ++i) {
        pn[i] = n; py_[i] = oy; px_[i] = ox;
        if (++ox == p.Wq) { ox = 0; if (++oy * p.Wq == p.HqWq) { oy = 0; ++n; } }
      }
    }
    float acc[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) acc[c] = 0.f;
    int tap = tap0, cg = cg0;
    constexpr int U = 2;
    for (int v = lane; v < nvec; v += 64 * U) {
      uint4_t wv[U][NCO], xv[U][PIX];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int vv = v + 64 * u;
        const bool live = vv < nvec;
        const int vc = live ? vv : 0;
        const int ky = tap / p.kw, kx = tap - ky * p.kw;
#pragma unroll
        for (int c = 0; c < NCO; ++c) wv[u][c] = reinterpret_cast<const uint4_t*>(p.w + (size_t)c * p.Kpad * sizeof(T))[vc];
#pragma unroll
        for (int i = 0; i < PIX; ++i) {
          const int iy = py_[i] * p.sy - p.pad + ky, ix = px_[i] * p.sy - p.pad_x + kx;
          const bool ok = live && m + i < m_end && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
          const unsigned off = (unsigned)((((pn[i] * p.Hi + iy) * p.Wi + ix) * p.x_cstride + p.x_coff + cg * VEC) * (int)sizeof(T));
          xv[u][i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, ok ? off : kOOB, 0, 0);
        }
        cg += 64;
        while (cg >= p.cin_groups) { cg -= p.cin_groups; ++tap; }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < PIX; ++i)
#pragma unroll
          for (int c = 0; c < NCO; ++c) acc[i * NCO + c] = dot8(xv[u][i], wv[u][c], acc[i * NCO + c], (T*)nullptr);
    }
    // transpose-reduce: 8 values x 64 lanes -> value j summed over all lanes, held by lanes with (lane>>3)==j
    float r4[4], r2[2], r1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {   // offset 32: lower half keeps values 0..3, upper half 4..7
      const float keep = lane & 32 ? acc[4 + j] : acc[j];
      const float send = lane & 32 ? acc[j] : acc[4 + j];
      r4[j] = keep + __shfl_xor(send, 32);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {   // offset 16
      const float keep = lane & 16 ? r4[2 + j] : r4[j];
      const float send = lane & 16 ? r4[j] : r4[2 + j];
      r2[j] = keep + __shfl_xor(send, 16);
    }
    {
      const float keep = lane & 8 ? r2[1] : r2[0];
      const float send = lane & 8 ? r2[0] : r2[1];
      r1 = keep + __shfl_xor(send, 8);
    }
    r1 += __shfl_xor(r1, 4);
    r1 += __shfl_xor(r1, 2);
    r1 += __shfl_xor(r1, 1);
    if ((lane & 7) == 0) {
      const int vi = lane >> 3;            // which of the 8 values this lane group holds
      const int i = vi / NCO, c = vi - i * NCO;
      if (m + i < m_end && c < p.Cout) {
        const size_t opix = ((size_t)pn[i] * p.Ho + py_[i]) * p.Wo + px_[i];
        float v = r1;
        if (p.scale) v *= p.scale[c];
        if (p.shift) v += p.shift[c];
        if (p.res) v += (float)reinterpret_cast<const T*>(p.res)[opix * p.res_cstride + p.res_coff + c];
        v = apply_act(v, p.act, p.slope);
        if (p.out_layout == FT_LAYOUT_NHWC)
          reinterpret_cast<T*>(p.y)[opix * p.y_cstride + p.y_coff + c] = (T)v;
        else
          reinterpret_cast<float*>(p.y)[((size_t)pn[i] * p.Cout + c) * p.Ho * p.Wo + (size_t)py_[i] * p.Wo + px_[i]] = v;
      }
    }
  }
}

// ---- predict_flow path (fp16): 3x3/s1/p1 conv to <= 2 output channels from an LDS-resident input patch ------
// The few-output kernel above re-reads each input pixel for its 9 taps from L2; at 96x128 x 224 channels that is
// ~0.8 GB of L2 traffic for 88 MB of input.  Here a workgroup owns an 8x16 (or 16x8) output patch: the 10x18 input
// patch of a 64-channel chunk is DMA'd once into LDS (double-buffered over chunks, XOR-swizzled like the halo
// kernel), thread (pixel, channel half) accumulates both outputs with v_dot2_f32_f16 against weights read as LDS
// broadcasts, and the two channel halves are summed through LDS.  Uses the generic packed layout [Cout_pad][Kpad].
template <int TW>
__global__ __launch_bounds__(256, 3) void conv_pflow_kernel(const ConvParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BP = 128, TH = BP / TW, NW = 4;
  constexpr int PW = TW + 2, NPIX = (TH + 2) * PW;
  constexpr int NPWW = (NPIX + 31) / 32;                 // patch wave-loads per wave per chunk (8 pixels per load, 4 waves)
  constexpr int PB = NPWW * NW * 1024;
  constexpr int WB = 9 * 2 * 128;                        // weights of one chunk: [tap][co][64 ch] fp16
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) void* lds_ptr;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* const patch0 = smem;
  char* const wts0 = smem + 2 * PB;
  float* const red = reinterpret_cast<float*>(wts0 + 2 * WB);

  int ptile;
  {
    const int total = p.npt;
    const int b = blockIdx.x;
    const int q = total >> 3, r = total & 7, xcd = b & 7, loc = b >> 3;
    ptile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  }
  const int tiles_per_img = p.h_ty * p.h_tx;
  const int n = ptile / tiles_per_img;
  const int trem = ptile - n * tiles_per_img;
  const int tyi = trem / p.h_tx, txi = trem - tyi * p.h_tx;
  const int qy0 = tyi * TH, qx0 = txi * TW;
  const int iy_org = qy0 - 1, ix_org = qx0 - 1;

  const __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.x), 0, p.x_bytes, 0x00020000);
  constexpr unsigned kOOB = 0x80000000u;
  unsigned p_voff[NPWW];
  {
    const int ppl = lane >> 3, pos = lane & 7;
#pragma unroll
    for (int t = 0; t < NPWW; ++t) {
      const int pp = (t * NW + wave) * 8 + ppl;
      unsigned v = kOOB;
      if (pp < NPIX) {
        const int pr = pp / PW, pc = pp - pr * PW;
        const int iy = iy_org + pr, ix = ix_org + pc;
        if ((unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi)
          v = (unsigned)((((n * p.Hi + iy) * p.Wi + ix) * p.x_cstride + p.x_coff) * 2 + ((pos ^ (pp & 7)) << 4));
      }
      p_voff[t] = v;
    }
  }
  const int nchunks = (p.cin_groups + 7) >> 3;           // 64-channel chunks (cin_groups = 8-channel groups)
  const int cin8 = p.cin_groups * 8;
  auto load_patch = [&](int c) {
#pragma unroll
    for (int t = 0; t < NPWW; ++t)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_b, (lds_ptr)(patch0 + (c & 1) * PB + (t * NW + wave) * 1024), 16, p_voff[t],
                                               c * 128, 0, 0);
  };
  // weights of a chunk: 18 (tap, co) rows of 8 x 16 bytes; threads 0..143 carry one piece each
  const int w_tapco = tid >> 3, w_piece = tid & 7;
  const bool w_thread = tid < 144;
  auto fetch_w = [&](int c) {
    uint4_t v = {0u, 0u, 0u, 0u};
    const int cg = c * 8 + w_piece, tap = w_tapco >> 1, co = w_tapco & 1;
    if (w_thread && cg < p.cin_groups && co < p.Cout)
      v = *reinterpret_cast<const uint4_t*>(p.w + ((size_t)co * p.Kpad + (size_t)tap * cin8 + cg * 8) * 2);
    return v;
  };
  auto store_w = [&](int c, const uint4_t& v) {
    if (w_thread) *reinterpret_cast<uint4_t*>(wts0 + (c & 1) * WB + w_tapco * 128 + w_piece * 16) = v;
  };

  const int m = tid & (BP - 1), half = tid >> 7;        // pixel of the patch, channel half of the chunk (wave-uniform)
  const int r0 = (m / TW) * PW + (m % TW);
  float acc0 = 0.f, acc1 = 0.f;

  load_patch(0);
  store_w(0, fetch_w(0));
  for (int c = 0; c < nchunks; ++c) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    uint4_t wnext = {0u, 0u, 0u, 0u};
    const bool more = c + 1 < nchunks;
    if (more) {
      load_patch(c + 1);
      wnext = fetch_w(c + 1);
    }
    const char* pb = patch0 + (c & 1) * PB;
    const char* wb = wts0 + (c & 1) * WB + half * 64;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {     // not unrolled: the scheduler would hoist all 108 fragment reads and spill
      const int r = r0 + (tap / 3) * PW + (tap % 3);
      const char* rowp = pb + r * 128;
      const int sw = r & 7;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint4_t xv = *reinterpret_cast<const uint4_t*>(rowp + (((half * 4 + k) ^ sw) << 4));
        const uint4_t w0 = *reinterpret_cast<const uint4_t*>(wb + (tap * 2 + 0) * 128 + k * 16);
        const uint4_t w1 = *reinterpret_cast<const uint4_t*>(wb + (tap * 2 + 1) * 128 + k * 16);
        acc0 = dot8(xv, w0, acc0, (half_t*)nullptr);
        acc1 = dot8(xv, w1, acc1, (half_t*)nullptr);
      }
    }
    if (more) store_w(c + 1, wnext);
  }
  // sum the two channel halves, then bias / activation and the store
  if (half == 1) {
    red[m * 2] = acc0;
    red[m * 2 + 1] = acc1;
  }
  __syncthreads();
  if (half == 0) {
    const int oy = qy0 + m / TW, ox = qx0 + m % TW;
    if (oy < p.Ho && ox < p.Wo) {
      float v[2] = {acc0 + red[m * 2], acc1 + red[m * 2 + 1]};
#pragma unroll
      for (int co = 0; co < 2; ++co) {
        if (co < p.Cout) {
          if (p.scale) v[co] *= p.scale[co];
          if (p.shift) v[co] += p.shift[co];
          v[co] = apply_act(v[co], p.act, p.slope);
        }
      }
      if (p.out_layout == FT_LAYOUT_NHWC) {
        half_t* yp = reinterpret_cast<half_t*>(p.y) + (((size_t)n * p.Ho + oy) * p.Wo + ox) * p.y_cstride + p.y_coff;
        yp[0] = (half_t)v[0];
        if (p.Cout > 1) yp[1] = (half_t)v[1];
      } else {
        float* yp = reinterpret_cast<float*>(p.y);
        const size_t hw = (size_t)p.Ho * p.Wo, pix = (size_t)oy * p.Wo + ox;
        yp[((size_t)n * p.Cout) * hw + pix] = v[0];
        if (p.Cout > 1) yp[((size_t)n * p.Cout + 1) * hw + pix] = v[1];
      }
    }
  }
#endif
}

// ---- predict_flow on the matrix pipe (fp16): the 3x3 conv to <= 2 channels as ONE 1x1 GEMM to 18 (tap, co) rows per INPUT
// pixel + a 9-term shift-and-add.  conv_pflow_kernel above still reads every input fragment nine times from LDS and runs the
// dot products on the vector ALU (45 us at 96x128x16 x 194 channels against an 11-us byte floor); here a workgroup takes the
// 14 x 18 input patch of a 12 x 16 output tile (252 pixels = 8 MFMA pixel tiles, two per wave), streams it ONCE through a
// 4-deep ring of 32-channel chunks (LDS-DMA, 64-byte pixel rows, chunk key (pixel / 4) & 3: conflict-free fragment reads),
// multiplies each chunk by the [32 x 16] weight fragments (rows tap * 2 + co, 18 live; all chunks resident in LDS in fragment
// order), parks the fp32 [pixel][18] partials in LDS and lets 192 threads add the nine neighbours of their output pixel.
// MFMA work: 16 instructions per 32 channels per workgroup — the kernel is a stream over its input (1.31x with the halo).
// fp32 summation order differs from the other two kernels (channels inside a tap first), well inside the fp16 tolerance.
__global__ __launch_bounds__(256, 2) void conv_pflow_mfma_kernel(const ConvParams p, int nchunks) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int TW = 16, TH = 12, PW = TW + 2, NPIX = (TH + 2) * PW;   // 252
  constexpr int NW = 4, RING = 4, CHB = 16384;                       // 256 pixel slots x 64 bytes per chunk
  constexpr int SP = 20;                                             // floats per pixel of the partial tile (18 + pad: 16-byte rows)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) void* lds_ptr;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;
  char* const ring = smem;
  char* const wts = smem + RING * CHB;                               // nchunks x 2 slices x 1 KiB
  float* const part = reinterpret_cast<float*>(smem);                // aliases the ring once the last chunk has been read

  int ptile;
  {
    const int total = p.npt;
    const int b = blockIdx.x;
    const int q = total >> 3, r = total & 7, xcd = b & 7, loc = b >> 3;
    ptile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  }
  const int tiles_per_img = p.h_ty * p.h_tx;
  const int n = ptile / tiles_per_img;
  const int trem = ptile - n * tiles_per_img;
  const int tyi = trem / p.h_tx, txi = trem - tyi * p.h_tx;
  const int qy0 = tyi * TH, qx0 = txi * TW;

  // ---- weights: piece (slice s, k half, row co') = 8 consecutive channels of one (tap, co); ordinary loads, before any DMA --
  {
    const int cin8 = p.cin_groups * 8;
    const int npieces = nchunks * 2 * 64;
    for (int i = tid; i < npieces; i += 256) {
      const int sl = i >> 6, l = i & 63, row = l & 31, cg = sl * 2 + (l >> 5);
      const int tap = row >> 1, co = row & 1;
      uint4_t v = {0u, 0u, 0u, 0u};
      if (row < 18 && cg < p.cin_groups && co < p.Cout)
        v = *reinterpret_cast<const uint4_t*>(p.w + ((size_t)co * p.Kpad + (size_t)tap * cin8 + cg * 8) * 2);
      *reinterpret_cast<uint4_t*>(wts + i * 16) = v;
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

  const __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.x), 0, p.x_bytes, 0x00020000);
  constexpr unsigned kOOB = 0x80000000u;
  unsigned p_voff[4];            // 16 pixels per wave-load (4 lanes x 16 bytes each), 4 wave-loads per wave per chunk
  {
    const int ppl = lane >> 2, pos = lane & 3;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int pp = (t * NW + wave) * 16 + ppl;
      unsigned v = kOOB;
      if (pp < NPIX) {
        const int pr = pp / PW, pc = pp - pr * PW;
        const int iy = qy0 - 1 + pr, ix = qx0 - 1 + pc;
        if ((unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi)
          v = (unsigned)((((n * p.Hi + iy) * p.Wi + ix) * p.x_cstride + p.x_coff) * 2 + ((pos ^ ((pp >> 2) & 3)) << 4));
      }
      p_voff[t] = v;
    }
  }
  auto load_chunk = [&](int c) {       // past the last chunk: out-of-range loads (zeros into a slot nobody reads) keep vmcnt uniform
    const bool live = c < nchunks;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_b, (lds_ptr)(ring + (c & (RING - 1)) * CHB + (t * NW + wave) * 1024), 16,
                                               live ? p_voff[t] : kOOB, live ? c * 64 : 0, 0, 0);
  };
  load_chunk(0);
  load_chunk(1);
  load_chunk(2);

  float16_t acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  int b_off[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int pp = (wave * 2 + t) * 32 + l31;
    b_off[t] = pp * 64 + ((lhi ^ ((pp >> 2) & 3)) << 4);
  }
  const int a_off = lane * 16;

  for (int c = 0; c < nchunks; ++c) {
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");       // chunk c has landed (this wave's pieces); chunks c+1, c+2 may fly
    FT_LDS_BARRIER();                                       // ... everyone's pieces; and every read of chunk c-1 is done
    load_chunk(c + 3);
    const char* cb = ring + (c & (RING - 1)) * CHB;
    const char* wb = wts + c * 2048 + a_off;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint4_t fa = *reinterpret_cast<const uint4_t*>(wb + k * 1024);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const uint4_t fb = *reinterpret_cast<const uint4_t*>(cb + (b_off[t] ^ (k << 5)));
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, fa), __builtin_bit_cast(half8_t, fb), acc[t], 0, 0, 0);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // the dummy tail loads too: the ring becomes the partial tile
  FT_LDS_BARRIER();
  // ---- partials [pixel][18]: accumulator register r of lane (pixel, half) is row 8 * (r / 4) + 4 * half + r % 4 -------------
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int pp = (wave * 2 + t) * 32 + l31;
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int row0 = g * 8 + lhi * 4;
      if (row0 < 18)
        *reinterpret_cast<float4_t*>(part + pp * SP + row0) = float4_t{acc[t][g * 4], acc[t][g * 4 + 1], acc[t][g * 4 + 2], acc[t][g * 4 + 3]};
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  FT_LDS_BARRIER();
  if (tid < TW * TH) {
    const int oy_l = tid / TW, ox_l = tid - oy_l * TW;
    const int oy = qy0 + oy_l, ox = qx0 + ox_l;
    float v[2] = {0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const float2 s2 = *reinterpret_cast<const float2*>(part + ((oy_l + tap / 3) * PW + ox_l + tap % 3) * SP + tap * 2);
      v[0] += s2.x;
      v[1] += s2.y;
    }
    if (oy < p.Ho && ox < p.Wo) {
#pragma unroll
      for (int co = 0; co < 2; ++co) {
        if (co < p.Cout) {
          if (p.scale) v[co] *= p.scale[co];
          if (p.shift) v[co] += p.shift[co];
          v[co] = apply_act(v[co], p.act, p.slope);
        }
      }
      if (p.out_layout == FT_LAYOUT_NHWC) {
        half_t* yp = reinterpret_cast<half_t*>(p.y) + (((size_t)n * p.Ho + oy) * p.Wo + ox) * p.y_cstride + p.y_coff;
        yp[0] = (half_t)v[0];
        if (p.Cout > 1) yp[1] = (half_t)v[1];
      } else {
        float* yp = reinterpret_cast<float*>(p.y);
        const size_t hw = (size_t)p.Ho * p.Wo, pix = (size_t)oy * p.Wo + ox;
        yp[((size_t)n * p.Cout) * hw + pix] = v[0];
        if (p.Cout > 1) yp[((size_t)n * p.Cout + 1) * hw + pix] = v[1];
      }
    }
  }
#endif
}

// ---- host side ---------------------------------------------------------------------------------
int launch_fewout_forms(ConvParams p, const ft_conv_desc* d, const Geometry& g, unsigned long long x_bytes, hipStream_t s,
                        bool* taken) {
  *taken = true;
  if (!d->transposed && d->Cout <= 2 && d->dtype == FT_F16 && d->kh == 3 && d->kw == 3 && d->stride == 1 &&
      d->pad == 1 && !d->has_residual && d->x_wpitch == 0 && d->x_cstride % 8 == 0 && d->x_coff % 8 == 0 && x_bytes < (1ull << 31)) {
    p.x_bytes = (unsigned)x_bytes;
    {
      // the matrix-pipe form (12 x 16 output tiles, input streamed once) where it applies; else the dot-product kernel
      const int nchunks = ceil_div(g.cin_groups, 4);                 // 32-channel chunks
      const int ty = ceil_div(d->Ho, 12), tx = ceil_div(d->Wo, 16);
      const size_t lds = (size_t)4 * 16384 + (size_t)nchunks * 2048;
      if ((long long)d->N * ty * tx >= 256 && lds <= 160 * 1024 &&
          (long long)ty * 12 * tx * 16 * 100 <= (long long)d->Ho * d->Wo * 125) {     // ragged edges waste < 25 % of the tiles
        p.h_ty = ty;
        p.h_tx = tx;
        p.npt = d->N * ty * tx;
        auto k = conv_pflow_mfma_kernel;
        if (lds > 64 * 1024) FT_RAISE_LDS(k, 160 * 1024);
        hipLaunchKernelGGL(k, dim3(p.npt), dim3(256), lds, s, p, nchunks);
        FT_LAUNCH_CHECK("conv_pflow_mfma_kernel");
        return FT_OK;
      }
    }
    const long long t16 = (long long)ceil_div(d->Ho, 8) * ceil_div(d->Wo, 16), t8 = (long long)ceil_div(d->Ho, 16) * ceil_div(d->Wo, 8);
    const int tw = t16 <= t8 ? 16 : 8, th = 128 / tw;
    p.h_ty = ceil_div(d->Ho, th);
    p.h_tx = ceil_div(d->Wo, tw);
    p.npt = d->N * p.h_ty * p.h_tx;
    // one patch per workgroup walks ALL channels serially: only worth it with at least one patch per CU (measured on
    // FlowNet2S: predict_flow2/3 75 -> 49 us, 37 -> 28 us; the deep low-resolution predict_flow4..6 stay on the
    // few-output kernel below, which splits K over the lanes)
    if (p.npt >= 256) {
      const size_t lds = 2 * (size_t)6 * 4 * 1024 + 2 * 9 * 2 * 128 + 128 * 2 * 4;
      dim3 grid(p.npt);
      if (tw == 16) hipLaunchKernelGGL(conv_pflow_kernel<16>, grid, dim3(256), lds, s, p);
      else hipLaunchKernelGGL(conv_pflow_kernel<8>, grid, dim3(256), lds, s, p);
      FT_LAUNCH_CHECK("conv_pflow_kernel");
      return FT_OK;
    }
  }
  if (!d->transposed && d->Cout <= 4) {
    const int nco = d->Cout <= 2 ? 2 : 4;
    if (x_bytes < (1ull << 31) && g.cout_pad >= nco) {
      p.x_bytes = (unsigned)x_bytes;
      // pixels per workgroup: enough workgroups to fill the chip; a wave takes PIX = 8 / nco pixels per pass
      int ppb = ceil_div(p.M, 2048);
      ppb = ppb < 16 ? 16 : (ppb > 128 ? 128 : ppb);
      ppb = round_up(ppb, 16);
      dim3 grid(ceil_div(p.M, ppb));
#define FT_FEWOUT(T, N, P)                                          \
  do {                                                              \
    auto k = conv_fewout_kernel<T, N, P>;                           \
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, p, ppb);           \
  } while (0)
      if (d->dtype == FT_F16) { if (nco == 2) FT_FEWOUT(half_t, 2, 4); else FT_FEWOUT(half_t, 4, 2); }
      else { if (nco == 2) FT_FEWOUT(float, 2, 4); else FT_FEWOUT(float, 4, 2); }
#undef FT_FEWOUT
      FT_LAUNCH_CHECK("conv_fewout_kernel");
      return FT_OK;
    }
  }
  *taken = false;
  return FT_OK;
}

}  // namespace ft
