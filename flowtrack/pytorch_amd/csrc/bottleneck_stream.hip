// Whole-bottleneck fusion for the 128- and 256-plane ResNet stages (fp16): conv1 1x1 + bn1 + relu -> conv2 3x3 + bn2 +
// relu -> conv3 1x1 + bn3 + identity residual + relu in ONE launch, with every weight byte STREAMED through LDS
// (reference: Bottleneck.forward, lib/pose/models/blocks.py:105-120, the blocks without a projection shortcut:
// layer2.1-3 / layer3.1-5 of ResNet-50, layer3.1-22 of ResNet-101, resnet.py:29-36,51-55).
//
// Why a second fused kernel (bottleneck.hip covers the 64-plane stage): at 512 / 1024 channels the three launches of a
// block are no longer HBM-bound, they are bound by operand delivery L2 -> LDS: with 12 k .. 49 k pixels per layer the
// GEMM tiles that fill 256 CUs are small (64x64 .. 128x128), every operand byte is re-delivered M/BP or N/BC times
// (200 + 226 + 200 MB per layer3 block at batch 64) and the three launches take 82 (layer3) / 94 us (layer2) for 27.4
// GFLOP.  Here a workgroup owns a full-width strip of output rows of one image, keeps t1 and t2 in LDS and streams the
// block's weights ONCE through a ring (2.2 MB per workgroup at 256 planes, 0.55 MB at 128): the pixel operand never
// leaves the CU, the weight operand arrives as 1-KiB-contiguous DMA pieces (pre-packed in MFMA fragment order, so the
// LDS image needs no swizzle and ds_read_b128 is lane-linear).  tools/dev/ubench/stream_ring.hip is the micro-model of
// the inner loop: 1.24 PFLOP/s chip-wide at 256 workgroups (21 B/clk/CU of weights beside the matrix pipe).
//
// Geometry (P planes, C = 4P channels; 4 waves = WCOLS x WPG, wave = 2 output-channel tiles x MT pixel tiles of 32):
//   P = 256: WCOLS 4, WPG 1: strip <= 96 output pixels (MT2 = 3) on <= 120 halo pixels (MT1 = 4)   [or 64 on 96]
//   P = 128: WCOLS 2, WPG 2: strip <= 192 output pixels on <= 256 halo pixels
//   phase 1  t1 = relu(bn1(W1 . x)) on the strip + one halo row above and below: x streams in 64-channel chunks (whole
//            128-byte lines per pixel, XOR-swizzled on the source side), W1 in matching K-slices; the residual (the
//            strip's own pixels) is picked out of the chunks in phase 3's accumulator layout as they pass through LDS.
//   phase 2  t2 = relu(bn2(W2 * t1)): the pixel operand of tap (ky, kx) is T1 at row offset ky*W + kx - 1 (full-width
//            strips make the 3x3 neighbourhood a linear shift; the two x-border taps are lane-masked); only W2 streams.
//   phase 3  y = relu(bn3(W3 . t2) + x) in four quarters of P output channels; each lane owns 16 consecutive channels of
//            a pixel (the A-fragment rows are permuted at pack time), so y leaves as 32-byte runs per lane.
// LDS: T1 / T2 (aliased) <= 60 / 64 KiB, three x-chunk buffers (inside the T1 region during phase 1), three weight-step
// buffers, two folded-BN table buffers = 160 KiB, one workgroup per CU.
#include <stdlib.h>

#include <type_traits>

#include "ft_common.h"

namespace ft {
namespace {

struct BnsParams {
  const char* x;
  char* y;
  const char* ws;    // packed weight stream (ft_bottleneck_stream_pack)
  const char* tab;   // float [6][2P]: {s1 b1} {s2 b2} {s3 b3 of quarter 0} .. {quarter 3}
  int H, W, TH;      // image size, output rows per strip
  int ppi, total;    // strips per image (x column parts), workgroups
  int TWc, csplit;   // column-split form of the direct kernel: output columns per workgroup, parts per row of strips
  int Ho, Wo;        // stride-2 head form (conv1 + conv2 of a stage's entry block): output map; H, W are the INPUT map
  int x_cstride, x_coff, y_cstride, y_coff;
  unsigned x_bytes, y_bytes, ws_bytes;
  int dbg;
};

template <int N, int I = 0, typename F>
__device__ __forceinline__ void bns_unroll(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    bns_unroll<N, I + 1>(f);
  }
}

#define BNS_BARRIER() asm volatile("s_barrier" ::: "memory")
// XOR key of the x-chunk buffers' 128-byte rows: two rows share a 256-byte bank row (see bottleneck.hip: BNK_KEY)
#define BNS_XKEY(hp) (((hp) >> 1) & 7)
#ifndef FT_BNSD_ABL
#define FT_BNSD_ABL 0   // dev ablations of the direct kernel (TIMING ONLY, results are wrong): 1 = no chunk barriers in phase 1, 2 = no residual
                        // pick-up, 16 / 32 = the weight loads of phase 1 / phases 2 + 3 are not issued at all (FT_BNS_DBG=64 still issues them)
#endif

// MFMA row r of an A fragment holds output channel sigma(r) of its 32-channel tile, so that accumulator register k of
// lane (pixel, half) is channel 16 * half + k: 16 consecutive channels per lane.
__host__ __device__ constexpr int bns_sigma(int r) { return 16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3); }

template <int P>
struct BnsGeom {
  static constexpr int C = 4 * P;
  static constexpr int NCT = P / 32;          // output-channel tiles of a P-wide GEMM
  static constexpr int WCOLS = P / 64;        // wave columns (2 channel tiles each)
  static constexpr int WPG = 4 / WCOLS;       // pixel groups
  static constexpr int NC1 = C / 64;          // x chunks = weight steps of phase 1
  static constexpr int KC = P / 64;           // 64-wide K chunks of a P-deep GEMM
  static constexpr int WSTEP = NCT * 4096;    // bytes of a weight step: 4 K16 slices x NCT fragments x 1 KiB
  static constexpr int LW = NCT;              // 1-KiB weight loads per wave per step
  static constexpr int G2 = NC1, G3 = NC1 + 9 * KC, GEND = G3 + 4 * KC;
  static constexpr int ROWB = 2 * P;          // bytes of a T1 / T2 / staging row
  static constexpr int TABB = 8 * P;          // bytes of one table {scale[P], shift[P]}
  static constexpr int LT = P / 128;          // 256-byte table loads per wave
  // LDS map: [0, ..) three x-chunk buffers in phase 1, then T1, then T2 (+ the output staging tile behind it at 128
  // planes); one folded-BN table, one all-zero row (the x-border taps read it), three weight-step buffers
  static constexpr int XSTRIDE = P == 256 ? 16384 : 32768;
  static constexpr int T1_ROWS = P == 256 ? 120 : 256;
  static constexpr int TAB = P == 256 ? 61440 : 98304;
  static constexpr int ZROW = TAB + TABB;
  static constexpr int WBASE = P == 256 ? 65536 : 114688;
  static constexpr int STG = 49152;           // P = 128: staging tile [48 K, 96 K)
  static constexpr int LDS_BYTES = 163840;
  static_assert(ZROW % ROWB == 0 && ZROW + ROWB <= WBASE && WBASE + 3 * WSTEP == LDS_BYTES, "LDS map");
};

// ---- device code shared by the four kernels --------------------------------------------------------------------------------------
// hipcc's output for these kernels (422-512 VGPRs, hand-counted waits) depends on how the source is phrased: every helper below was
// checked to leave all kernels of the unit instruction-identical (tools/dev/isa_diff.py; profiles/HISTORY.md lists what was tried and
// withdrawn).  What came through: scalars by value, results by value where there is one, arrays by reference, the call where the
// block stood.  Still one copy per kernel, because a function (or even a namespace-scope constant) changed the code: kOOB, x_voff[],
// issue_touch, permA, the residual pick-up, the swizzled T1 / T2 row stores, zero_acc, row_bases.
typedef __attribute__((address_space(3))) void* lds_ptr;
constexpr unsigned kBnsOOB = 0x80000000u;   // = the kernels' own kOOB: a buffer offset out of range for every descriptor (zeros, no traffic)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t bns_rsrc(const char* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), 0, bytes, 0x00020000);
}

// x chunk c (64 channels = 128 bytes per halo pixel) into the chunk buffer `dst`: LX 1-KiB loads (8 rows each) per wave of NW
template <int NW, int LX>
__device__ __forceinline__ void bns_issue_x(__amdgpu_buffer_rsrc_t rsrc_x, char* dst, int wave, const unsigned (&x_voff)[LX], int c) {
#pragma unroll
  for (int t = 0; t < LX; ++t)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (lds_ptr)(dst + (t * NW + wave) * 1024), 16, x_voff[t], c * 128, 0, 0);
}

// T1: a halo pixel outside the image is conv2's zero padding
__device__ __forceinline__ half8_t bns_keep_if(half8_t v, bool inside) {
  uint4_t u = __builtin_bit_cast(uint4_t, v);
  u.x = inside ? u.x : 0u; u.y = inside ? u.y : 0u; u.z = inside ? u.z : 0u; u.w = inside ? u.w : 0u;
  return __builtin_bit_cast(half8_t, u);
}

// x-border flags of output column ox: bit 0 = first column (tap kx = 0 is padding), bit 1 = last column
__device__ __forceinline__ int bns_edge(int ox, int W) { return (ox == 0 ? 1 : 0) | (ox == W - 1 ? 2 : 0); }

// Folded operands (see bottleneck_stream_direct_kernel).  The shift pairs of MFMA row l31 of epilogues e0 .. e1-1 for the wave's CT
// 32-channel tiles from `tile0` on (lanes 32..63 hold k = 8..15 of the shift slice: zeros, fetched out of range) ...
template <int P, int CT>
__device__ __forceinline__ void bns_load_shp(unsigned (&shp)[6][CT], __amdgpu_buffer_rsrc_t rsrc_t, int l31, int lhi, int tile0, int e0, int e1) {
  const unsigned so = lhi == 0 ? 4u * (unsigned)bns_sigma(l31) : kBnsOOB;
#pragma unroll
  for (int e = e0; e < e1; ++e)
#pragma unroll
    for (int i = 0; i < CT; ++i)
      shp[e][i] = __builtin_amdgcn_raw_buffer_load_b32(rsrc_t, so, 4 * (e * P + (tile0 + i) * 32), 0);
}
// ... A[i][j] += the shift of one epilogue: ONE extra MFMA per tile (A row = {hi, lo, 0 ..}, B = ones at k = 0, 1), on 32-pixel tiles ...
template <int CT, int MT>
__device__ __forceinline__ void bns_add_shift(float16_t (&A)[CT][MT], const unsigned (&sh)[CT]) {
  const uint4_t onesB = uint4_t{0x3C003C00u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < CT; ++i) {
    const uint4_t sa = uint4_t{sh[i], 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < MT; ++j)
      A[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, sa), __builtin_bit_cast(half8_t, onesB), A[i][j], 0, 0, 0);
  }
}
// ... and on 16-pixel tiles ...
template <int CT, int MT>
__device__ __forceinline__ void bns_add_shift(float4_t (&A)[CT][MT], const unsigned (&sh)[CT]) {
  const uint4_t onesB = uint4_t{0x3C003C00u, 0u, 0u, 0u};
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    const uint4_t sa = uint4_t{sh[t], 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < MT; ++j)
      A[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, sa), __builtin_bit_cast(half8_t, onesB), A[t][j], 0, 0, 0);
  }
}
// ... and the last epilogue of a 32-pixel tile: shift3 of the quarter and the identity residual (its two slices through the 0/1 matrix
// permA) join the accumulator as three MFMAs.  (onesB comes from the kernel: built in here, three kernels change registers.)
__device__ __forceinline__ void bns_fold_tail(float16_t& a, unsigned sh, const uint4_t& onesB, const uint4_t (&permA)[2], const uint4_t (&res)[2]) {
  const uint4_t sa = uint4_t{sh, 0u, 0u, 0u};
  a = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, sa), __builtin_bit_cast(half8_t, onesB), a, 0, 0, 0);
#pragma unroll
  for (int h = 0; h < 2; ++h)
    a = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, permA[h]), __builtin_bit_cast(half8_t, res[h]), a, 0, 0, 0);
}

// dev (FT_BNS_DBG=32): phase timestamps of wave 0 over the strip's first output pixel (the output is garbage then).  Macros over the
// kernel's own p, ts, tid, n, y0 and W: the tail as a function changed fifteen kernels.
#define BNS_TS(i) do { if (p.dbg & 32) ts[i] = __builtin_amdgcn_s_memtime(); } while (0)
#define BNS_TS_TAIL()                                                                                                                \
  do {                                                                                                                               \
    if (p.dbg & 32) {                                                                                                                \
      ts[5] = __builtin_amdgcn_s_memtime();                                                                                          \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                               \
      ts[6] = __builtin_amdgcn_s_memtime();                                                                                          \
      if (tid == 0) {                                                                                                                \
        unsigned long long* o = reinterpret_cast<unsigned long long*>(p.y + ((size_t)((n * p.H + y0) * W) * p.y_cstride + p.y_coff) * 2); \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) o[i] = ts[i];                                                                  \
      }                                                                                                                              \
    }                                                                                                                                \
  } while (0)

// FOLD: the folded operands (see bottleneck_stream_direct_kernel): scales in the weights, shifts as (hi, lo) pairs in p.tab, shift and
// residual added by MFMA, every epilogue = fp16(relu(acc)); no table ever travels through LDS.
template <int P, int MT1, int MT2, bool FOLD = false>
__global__ __launch_bounds__(256, 1) void bottleneck_stream_kernel(const BnsParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  using G = BnsGeom<P>;
  constexpr int NCT = G::NCT, WCOLS = G::WCOLS, WPG = G::WPG, NC1 = G::NC1, KC = G::KC, WSTEP = G::WSTEP, LW = G::LW;
  constexpr int ROWB = G::ROWB;
  constexpr int XROWS = WPG * MT1 * 32, LX = WPG * MT1;     // rows of an x chunk buffer; 1-KiB x loads per wave per chunk
  constexpr int NOUT = WPG * MT2 * 32;                       // output pixels of the strip (padded)
  // the output tile of a quarter goes through LDS for whole-line stores: behind T2 at 128 planes, in the weight buffer the
  // quarter's last step has just released at 256 planes (32 KiB: the 64-pixel strips only)
  constexpr bool STAGED = P == 128 || NOUT * ROWB <= WSTEP;
  static_assert(XROWS * 128 <= G::XSTRIDE, "x chunk buffer");
  static_assert(NOUT * ROWB <= 49152, "T2 fits below the staging tile / inside the T1 region");
  static_assert(2 * (LX + LW) + 6 + 12 <= 63, "vmcnt immediate");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using c0 = std::integral_constant<int, 0>;
  using c1 = std::integral_constant<int, 1>;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wcol = wave % WCOLS, pg = wave / WCOLS;
  const int l31 = lane & 31, lhi = lane >> 5;

  const int logical = xcd_logical_wg(p.total);
  const int n = logical / p.ppi;
  const int y0 = (logical - n * p.ppi) * p.TH;
  const int W = p.W;
  const int rows_out = p.H - y0 < p.TH ? p.H - y0 : p.TH;
  const int npix_out = rows_out * W;
  const int npix_halo = (p.TH + 2) * W;

  const __amdgpu_buffer_rsrc_t rsrc_x = bns_rsrc(p.x, p.x_bytes), rsrc_y = bns_rsrc(p.y, p.y_bytes), rsrc_w = bns_rsrc(p.ws, p.ws_bytes);
  const __amdgpu_buffer_rsrc_t rsrc_t = bns_rsrc(p.tab, FOLD ? (2 * P + G::C) * 4 : 6 * G::TABB);
  constexpr unsigned kOOB = 0x80000000u;

  // folded form: shift pairs of this wave's MFMA rows per (epilogue, tile) and the residual's 0/1 matrix (see the direct kernel)
  [[maybe_unused]] unsigned shp[6][2];
  [[maybe_unused]] uint4_t permA[2];
  [[maybe_unused]] const uint4_t onesB = uint4_t{0x3C003C00u, 0u, 0u, 0u};
  auto load_shp = [&]() { bns_load_shp<P>(shp, rsrc_t, l31, lhi, 2 * wcol, 0, 6); };
  if constexpr (FOLD) {
    const int sg = bns_sigma(l31);
    const bool on = lhi == (sg >> 4);
    const int ph = (sg >> 3) & 1, pe = sg & 7;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      unsigned w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = (on && ph == hh && (pe >> 1) == k) ? (0x3C00u << (16 * (pe & 1))) : 0u;
      permA[hh] = uint4_t{w[0], w[1], w[2], w[3]};
    }
  }

  // the first round of workgroups on an XCD pulls the block's weight stream into that XCD's L2, each its own 1/n-th, one
  // dword per 128-byte line (see the direct kernel); the scratch corner sits between the zero row and the weight ring.
  // EXACTLY kTouch loads per thread (lines past the share: out of range, no traffic): the touch is issued BEHIND the first x
  // chunk (round 6: it used to sit in front of it in every wave's in-order load queue) and the first hand-counted wait counts it
  constexpr int kTouch = 6;
  auto issue_touch = [&]() {
    constexpr int SCR = P == 256 ? 64000 : 102400;
    static_assert(SCR >= G::ZROW + ROWB && SCR + 1024 <= G::WBASE, "scratch of the L2 touch loads");
    const bool on = blockIdx.x < 256 && !(p.dbg & (512 | 1024));
    const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    const int first = p.total < 256 ? p.total : 256;
    const int nloc = (first - xcd + 7) >> 3;
    const unsigned lines = (p.ws_bytes + 127u) >> 7;
    const unsigned per = (lines + nloc - 1) / nloc;
    const unsigned lo = loc * per, hi = lo + per < lines ? lo + per : lines;
#pragma unroll
    for (int k = 0; k < kTouch; ++k) {
      const unsigned l = lo + tid + 256u * k;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (lds_ptr)(smem + SCR + wave * 256), 4, (on && l < hi) ? l << 7 : kOOB, 0, 0, 0);
    }
  };
  // ---- loaders -------------------------------------------------------------------------------------------------------
  // x chunk: row = halo pixel, 128 bytes (64 channels); a 1-KiB wave load covers 8 rows, lane -> (row = lane / 8,
  // 16-byte position lane % 8), the XOR swizzle (position ^= row & 7) is applied to the SOURCE position
  unsigned x_voff[LX];
#pragma unroll
  for (int t = 0; t < LX; ++t) {
    const int hp = (t * 4 + wave) * 8 + (lane >> 3);
    const int hr = hp / W, hc = hp - hr * W;
    const int iy = y0 - 1 + hr;
    unsigned v = kOOB;
    if (hp < npix_halo && (unsigned)iy < (unsigned)p.H)
      v = (unsigned)((((n * p.H + iy) * W + hc) * p.x_cstride + p.x_coff) * 2 + (((lane & 7) ^ BNS_XKEY(hp)) << 4));
    x_voff[t] = v;
  }
  const unsigned lane16 = (unsigned)lane * 16u;
  auto issue_x = [&](int c, int buf) { bns_issue_x<4>(rsrc_x, smem + buf * G::XSTRIDE, wave, x_voff, c); };
  auto issue_w = [&](int g, int buf) {
    char* dst = smem + G::WBASE + buf * WSTEP;
#pragma unroll
    for (int t = 0; t < LW; ++t)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (lds_ptr)(dst + (t * 4 + wave) * 1024), 16, lane16,
                                               g * WSTEP + (t * 4 + wave) * 1024, 0, 0);
  };
  auto issue_tab = [&](int e) {       // {scale[P], shift[P]} of epilogue e; one buffer: issued once epilogue e-1 is behind a barrier
    if constexpr (FOLD) return;
#pragma unroll
    for (int t = 0; t < G::LT; ++t)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_t, (lds_ptr)(smem + G::TAB + (t * 4 + wave) * 256), 4, (unsigned)lane * 4u,
                                               e * G::TABB + (t * 4 + wave) * 256, 0, 0);
  };
  // per-lane A-fragment base inside a weight step: fragment (kk, channel tile 2*wcol + i) at (kk * NCT + 2*wcol + i) KiB
  const unsigned a_base = (unsigned)(G::WBASE + (2 * wcol) * 1024) + lane16;
  uint4_t fa[2][2];                   // A fragments, two register sets: slice k+1 is read while slice k multiplies

  unsigned long long ts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  BNS_TS(0);
  // prologue: chunk 0 (x + W1 slice) leads every wave's load queue, then the L2 touch and table 0 / the shift pairs, chunks 1 and 2,
  // the zero row
  issue_x(0, 0); issue_w(0, 0);
  issue_touch();
  if constexpr (FOLD) load_shp();
  else issue_tab(0);
  asm volatile("" ::: "memory");
  issue_x(1, 1); issue_w(1, 1);
  issue_x(2, 2); issue_w(2, 2);
  if (tid < ROWB / 16) *reinterpret_cast<uint4_t*>(smem + G::ZROW + tid * 16) = uint4_t{0u, 0u, 0u, 0u};

  // residual = the block input at the strip's own pixels, in phase 3's accumulator layout: [quarter][tile i][pixel tile j][half]
  uint4_t res[4][2][MT2][2];
  int m_out[MT2];       // output pixel (strip-relative, row-major at width W) of this lane per pixel tile
#pragma unroll
  for (int j = 0; j < MT2; ++j) m_out[j] = (pg * MT2 + j) * 32 + l31;

  // ================= phase 1: t1 = relu(bn1(W1 . x)) on the halo strip =============================================
  float16_t acc1[2][MT1];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < MT1; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[i][j][r] = 0.f;
  int b1_off[MT1];      // x-chunk fragment offsets (buffer-relative): row hp, 16-byte position (kk*2 + lhi) ^ BNS_XKEY(hp)
#pragma unroll
  for (int j = 0; j < MT1; ++j) {
    const int hp = (pg * MT1 + j) * 32 + l31;
    b1_off[j] = hp * 128 + ((lhi ^ BNS_XKEY(hp)) << 4);
  }
  {
    uint4_t fx[2][MT1];
    auto ld1 = [&](auto setc, int buf, int kk) {
      constexpr int S = decltype(setc)::value;
      const unsigned ab = a_base + buf * WSTEP;
      const char* xb = smem + buf * G::XSTRIDE;
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[S][i] = *reinterpret_cast<const uint4_t*>(smem + ab + (kk * NCT + i) * 1024);
#pragma unroll
      for (int j = 0; j < MT1; ++j) fx[S][j] = *reinterpret_cast<const uint4_t*>(xb + (b1_off[j] ^ (kk << 5)));
    };
    auto mma1 = [&](auto setc) {
      constexpr int S = decltype(setc)::value;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < MT1; ++j)
          acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, fa[S][i]), __builtin_bit_cast(half8_t, fx[S][j]),
                                                              acc1[i][j], 0, 0, 0);
    };
    // chunk 0 has landed (this wave's share) while the touch, the table / shift loads and chunks 1 and 2 fly; after the barrier everyone's share has
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * (LX + LW) + kTouch + (FOLD ? 12 : G::LT)) : "memory");
    BNS_BARRIER();
    ld1(c0{}, 0, 0);
    bns_unroll<NC1>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      constexpr int buf = c % 3;
      __builtin_amdgcn_sched_barrier(0);
      ld1(c1{}, buf, 1);
      __builtin_amdgcn_sched_barrier(0);
      mma1(c0{});
      __builtin_amdgcn_sched_barrier(0);
      ld1(c0{}, buf, 2);
      if (c % WCOLS == wcol) {       // this chunk holds the channels of this wave column for quarter c / WCOLS
        constexpr int q = c / WCOLS;
        const char* xb = smem + buf * G::XSTRIDE;
#pragma unroll
        for (int j = 0; j < MT2; ++j) {
          const int hp = m_out[j] + W;
          const char* rowp = xb + hp * 128;
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h)
              res[q][i][j][h] = *reinterpret_cast<const uint4_t*>(rowp + (((4 * i + 2 * lhi + h) ^ BNS_XKEY(hp)) << 4));
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      mma1(c1{});
      __builtin_amdgcn_sched_barrier(0);
      ld1(c1{}, buf, 3);
      __builtin_amdgcn_sched_barrier(0);
      mma1(c0{});
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (c + 1 < NC1) {
        // chunk c+1 has landed (chunk c+2 may fly), every read of chunk c's buffers is complete: refill them with chunk c+3
        if constexpr (c + 2 < NC1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LX + LW) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LW) : "memory");
        BNS_BARRIER();
        if constexpr (c + 3 < NC1) issue_x(c + 3, buf);
        issue_w(c + 3, buf);
        ld1(c0{}, (c + 1) % 3, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      mma1(c1{});
    });
  }
  // every wave is past its last x-chunk read once it reaches this barrier: the x buffers become T1
  BNS_TS(1);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();
  {
    if constexpr (FOLD) bns_add_shift(acc1, shp[0]);
    [[maybe_unused]] const float* tb = reinterpret_cast<const float*>(smem + G::TAB);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      [[maybe_unused]] const int ch = (2 * wcol + i) * 32 + 16 * lhi;
      [[maybe_unused]] float4_t sc[4], sh[4];
      if constexpr (!FOLD) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          sc[g4] = *reinterpret_cast<const float4_t*>(tb + ch + g4 * 4);
          sh[g4] = *reinterpret_cast<const float4_t*>(tb + P + ch + g4 * 4);
        }
      }
#pragma unroll
      for (int j = 0; j < MT1; ++j) {
        const int hp = (pg * MT1 + j) * 32 + l31;
        const int hr = hp / W;
        const int iy = y0 - 1 + hr;
        const bool inside = (unsigned)iy < (unsigned)p.H;     // out-of-image halo rows are conv2's zero padding
        half8_t h8[2];
        if constexpr (FOLD) relu_acc16(acc1[i][j], h8);
        else bn_relu_acc16(acc1[i][j], sc, sh, h8);
#pragma unroll
        for (int h = 0; h < 2; ++h) h8[h] = bns_keep_if(h8[h], inside);
        if (hp < npix_halo) {
          char* rowp = smem + hp * ROWB;
          const int cb = (2 * wcol + i) * 4 + 2 * lhi;           // 16-byte chunk of channel `ch`
#pragma unroll
          for (int h = 0; h < 2; ++h)
            *reinterpret_cast<half8_t*>(rowp + (((cb + h) ^ (hp & 15)) << 4)) = h8[h];
        }
      }
    }
  }
  BNS_TS(2);

  // ================= phases 2 + 3: weight steps G2 .. GEND-1, pixel operand from T1 / T2 ===========================
  float16_t acc[2][MT2];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < MT2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  };
  zero_acc();
  uint4_t fb[2][MT2];
  auto ld2 = [&](auto setc, int buf, int kk, const int (&rb)[MT2]) {
    constexpr int S = decltype(setc)::value;
    const unsigned ab = a_base + buf * WSTEP;
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[S][i] = *reinterpret_cast<const uint4_t*>(smem + ab + (kk * NCT + i) * 1024);
#pragma unroll
    for (int j = 0; j < MT2; ++j) fb[S][j] = *reinterpret_cast<const uint4_t*>(smem + (rb[j] ^ (kk << 5)));
  };
  auto mma2 = [&](auto setc) {
    constexpr int S = decltype(setc)::value;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < MT2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, fa[S][i]), __builtin_bit_cast(half8_t, fb[S][j]),
                                                           acc[i][j], 0, 0, 0);
  };
  // x-border flags of this lane's output pixels: bit 0 = first column (tap kx = 0 is padding), bit 1 = last column
  int edge[MT2];
#pragma unroll
  for (int j = 0; j < MT2; ++j) edge[j] = bns_edge(m_out[j] % W, W);
  // byte base of pixel row `m + off` of the T region for K chunk kc (slice kk is one more XOR); lanes whose tap is
  // x-padding read the zero row instead
  auto row_bases = [&](int off, int kc, int bad, int (&rb)[MT2]) {
#pragma unroll
    for (int j = 0; j < MT2; ++j) {
      const int row = m_out[j] + off;
      const int v = row * ROWB + (((row & 15) ^ lhi) << 4);
      rb[j] = ((edge[j] & bad) ? G::ZROW + (lhi << 4) : v) ^ (kc << 7);
    }
  };
  // one weight step (slices 1..3 of it, slice 0 already sits in register set 0) with the hand-over to the next one in front
  // of its last slice: the next step's weights have landed (this wave's share, then everyone's), every read of THIS step's
  // buffer is complete, so the buffer is refilled with step g+3 (unless `defer`: phase 3 stages its output tile there first)
  auto pstep = [&](int g, int buf, const int (&rb)[MT2], bool has_next, const int (&rb_next)[MT2], int tab_e, bool defer) {
    __builtin_amdgcn_sched_barrier(0);
    ld2(c1{}, buf, 1, rb);
    __builtin_amdgcn_sched_barrier(0);
    mma2(c0{});
    __builtin_amdgcn_sched_barrier(0);
    ld2(c0{}, buf, 2, rb);
    __builtin_amdgcn_sched_barrier(0);
    mma2(c1{});
    __builtin_amdgcn_sched_barrier(0);
    ld2(c1{}, buf, 3, rb);
    __builtin_amdgcn_sched_barrier(0);
    mma2(c0{});
    __builtin_amdgcn_sched_barrier(0);
    if (has_next) {
      if (g + 2 < G::GEND) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LW) : "memory");
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      BNS_BARRIER();
      if (tab_e >= 0) issue_tab(tab_e);
      if (g + 3 < G::GEND && !defer) issue_w(g + 3, buf);
      ld2(c0{}, buf == 2 ? 0 : buf + 1, 0, rb_next);
      __builtin_amdgcn_sched_barrier(0);
    }
    mma2(c1{});
  };
  // start of a phase: the T region has just been written, weight step g has landed: slice 0 into register set 0
  auto pstart = [&](int g, int buf, const int (&rb)[MT2], int tab_e) {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LW) : "memory");
    BNS_BARRIER();
    issue_tab(tab_e);
    issue_w(g + 2, buf == 0 ? 2 : buf - 1);          // (g + 2) % 3: the buffer of step g-1
    ld2(c0{}, buf, 0, rb);
  };

  // ---- phase 2: nine taps x KC chunks ---------------------------------------------------------------------------------
  {
    int rb[MT2], rbn[MT2];
    row_bases(-1, 0, 1, rb);                         // tap (0, 0), chunk 0
    pstart(G::G2, G::G2 % 3, rb, 1);
    int g = G::G2, buf = G::G2 % 3;
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        const bool has_next = !(tap == 8 && kc == KC - 1);
        int nky = ky, nkx = kx, nkc = kc + 1;
        if (nkc == KC) { nkc = 0; if (++nkx == 3) { nkx = 0; ++nky; } }
        row_bases(nky * W + nkx - 1, nkc, nkx == 0 ? 1 : (nkx == 2 ? 2 : 0), rbn);
        pstep(g, buf, rb, has_next, rbn, -1, false);
#pragma unroll
        for (int j = 0; j < MT2; ++j) rb[j] = rbn[j];
        ++g;
        buf = buf == 2 ? 0 : buf + 1;
      }
    }
  }
  // every wave is past its last T1 read once it reaches this barrier: T2 overwrites T1
  BNS_TS(3);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();
  {
    if constexpr (FOLD) bns_add_shift(acc, shp[1]);
    [[maybe_unused]] const float* tb = reinterpret_cast<const float*>(smem + G::TAB);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      [[maybe_unused]] const int ch = (2 * wcol + i) * 32 + 16 * lhi;
      [[maybe_unused]] float4_t sc[4], sh[4];
      if constexpr (!FOLD) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          sc[g4] = *reinterpret_cast<const float4_t*>(tb + ch + g4 * 4);
          sh[g4] = *reinterpret_cast<const float4_t*>(tb + P + ch + g4 * 4);
        }
      }
#pragma unroll
      for (int j = 0; j < MT2; ++j) {
        const int m = m_out[j];
        half8_t h8[2];
        if constexpr (FOLD) relu_acc16(acc[i][j], h8);
        else bn_relu_acc16(acc[i][j], sc, sh, h8);
        char* rowp = smem + m * ROWB;
        const int cb = (2 * wcol + i) * 4 + 2 * lhi;
#pragma unroll
        for (int h = 0; h < 2; ++h) *reinterpret_cast<half8_t*>(rowp + (((cb + h) ^ (m & 15)) << 4)) = h8[h];
      }
    }
  }
  zero_acc();
  BNS_TS(4);

  // ---- phase 3: four quarters of P output channels, K = P -------------------------------------------------------------
  {
    // direct form: lane -> 32-byte runs of its own pixel; staged form: thread -> 16-byte chunks of whole pixel rows
    unsigned y_voff[MT2];
#pragma unroll
    for (int j = 0; j < MT2; ++j) {
      const int m = m_out[j];
      y_voff[j] = m < npix_out ? (unsigned)((((n * p.H + y0) * W + m) * p.y_cstride + p.y_coff + (2 * wcol) * 32 + 16 * lhi) * 2) : kOOB;
    }
    constexpr int CPR = ROWB / 16;                   // 16-byte chunks per staging row
    constexpr int NSTG = NOUT * CPR / 256;           // chunks per thread
    unsigned s_voff[STAGED ? NSTG : 1];
    int s_off[STAGED ? NSTG : 1];
    if constexpr (STAGED) {
#pragma unroll
      for (int k = 0; k < NSTG; ++k) {
        const int idx = tid + 256 * k, m = idx / CPR, ch = idx % CPR;
        s_voff[k] = m < npix_out ? (unsigned)((((n * p.H + y0) * W + m) * p.y_cstride + p.y_coff + ch * 8) * 2) : kOOB;
        s_off[k] = m * ROWB + ((ch ^ (m & 15)) << 4);
      }
    }
    int rb[MT2];
    row_bases(0, 0, 0, rb);
    pstart(G::G3, G::G3 % 3, rb, 2);
    bns_unroll<4>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      bns_unroll<KC>([&](auto kcc) {
        constexpr int kc = decltype(kcc)::value;
        constexpr int g = G::G3 + q * KC + kc;
        constexpr bool last_of_q = kc == KC - 1;
        int rbn[MT2];
        row_bases(0, last_of_q ? 0 : kc + 1, 0, rbn);
        // the table of the NEXT quarter's epilogue follows the barrier of the quarter's first step
        pstep(g, g % 3, rb, g + 1 < G::GEND, rbn, (kc == 0 && q > 0) ? 2 + q : -1, STAGED && P == 256 && last_of_q);
#pragma unroll
        for (int j = 0; j < MT2; ++j) rb[j] = rbn[j];
      });
      if constexpr (q == 3) {
        // the last table: no later hand-over waits for it, and every wave loaded only its share of it
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        BNS_BARRIER();
      }
      constexpr int glast = G::G3 + q * KC + KC - 1;
      char* stg = smem + (P == 128 ? G::STG : G::WBASE + (glast % 3) * WSTEP);
      [[maybe_unused]] const float* tb = reinterpret_cast<const float*>(smem + G::TAB);
      if constexpr (FOLD) {
        // shift3 of the quarter and the residual join the accumulators as three MFMAs per tile
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < MT2; ++j) bns_fold_tail(acc[i][j], shp[2 + q][i], onesB, permA, res[q][i][j]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        [[maybe_unused]] const int ch = (2 * wcol + i) * 32 + 16 * lhi;
        [[maybe_unused]] float4_t sc[4], sh[4];
        if constexpr (!FOLD) {
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            sc[g4] = *reinterpret_cast<const float4_t*>(tb + ch + g4 * 4);
            sh[g4] = *reinterpret_cast<const float4_t*>(tb + P + ch + g4 * 4);
          }
        }
#pragma unroll
        for (int j = 0; j < MT2; ++j) {
          [[maybe_unused]] half8_t o8[2];
          if constexpr (FOLD) relu_acc16(acc[i][j], o8);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            half8_t o;
            if constexpr (FOLD) {
              o = o8[h];
            } else {
              const half8_t rs = __builtin_bit_cast(half8_t, res[q][i][j][h]);
              // (scalar on purpose: the packed form, bn_res_relu_acc8, needs aligned register pairs and made <128,4,3> spill)
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const int r = h * 8 + e;
                o[e] = (half_t)__builtin_fmaxf(acc[i][j][r] * sc[r >> 2][r & 3] + sh[r >> 2][r & 3] + (float)rs[e], 0.f);
              }
            }
            if constexpr (STAGED) {
              const int m = m_out[j];
              *reinterpret_cast<half8_t*>(stg + m * ROWB + ((((2 * wcol + i) * 4 + 2 * lhi + h) ^ (m & 15)) << 4)) = o;
            } else if (!(p.dbg & 4)) {
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4_t, o), rsrc_y, y_voff[j] + (unsigned)((q * P + i * 32 + h * 8) * 2), 0, FT_YSTORE_BUF_AUX);
            }
          }
        }
      }
      zero_acc();
      if constexpr (STAGED) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        BNS_BARRIER();
#pragma unroll
        for (int k = 0; k < NSTG; ++k) {
          const uint4_t v = *reinterpret_cast<const uint4_t*>(stg + s_off[k]);
          if (!(p.dbg & 4)) __builtin_amdgcn_raw_buffer_store_b128(v, rsrc_y, s_voff[k] + (unsigned)(q * P * 2), 0, FT_YSTORE_BUF_AUX);
        }
        if constexpr (P == 256 && q < 3) {
          // the staging tile sat in a weight buffer: hand it back (its refill with step glast + 3 was deferred)
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          BNS_BARRIER();
          if constexpr (glast + 3 < G::GEND) issue_w(glast + 3, glast % 3);
        }
      }
    });
  }
  BNS_TS_TAIL();
#endif
}

// ---- 256 planes, weights straight to registers -----------------------------------------------------------------------
// At 256 planes every wave owns its own two output-channel tiles, so no weight fragment is shared between waves: the
// LDS round trip of the weight stream (DMA write + ds_read, competing with the pixel-operand reads for the LDS port) is
// pure overhead.  Here each wave loads ITS fragments of a step (8 x 1 KiB, contiguous in the fragment-ordered stream)
// straight into VGPRs two steps ahead; only the pixel operand (x chunks, T1, T2) lives in LDS.  No ring, no ring
// barriers: the waves only meet at the phase transitions.  tools/dev/ubench/stream_ring.hip: 447 vs ~680 ns per 32-KiB
// step on the 2 x 2 micro-tile at 256 workgroups (30 vs 20 B/clk/CU of weights beside the matrix pipe).
// LDS: [0, 48 K) x-chunk buffers / [0, 60 K) T1 then T2, zero row at 60 K, all six folded-BN tables at 64 K (loaded
// once), two output staging tiles from 80 K.
// XH = column-split form for small batches (R101 384x288 at 16 crops per GPU gives 128 full-width strips for 256 CUs): a
// workgroup takes TWc of the W columns of its rows and carries its own x-halo — the T1 patch is (TH + 2) x (TWc + 2) with
// out-of-image columns zeroed like out-of-image rows, so every 3x3 tap is a plain shift inside the patch (no lane masks)
// and twice as many, half as long workgroups fill the chip.  conv1 is recomputed on the halo columns as on the halo rows.
// NS = weight-step register slots (prefetch distance NS - 1 steps of 8 KiB per wave): inside a network every block's 2.2 MB
// of weights arrive cold (from the MALL, not the XCD's L2); the column-split form has the registers for a deeper ring.
// HEADC > 0 = the stride-2 HEAD of a stage's entry block (conv1 1x1 + bn1 + relu -> conv2 3x3 / stride 2 + bn2 + relu,
// blocks.py:105-112 with stride on conv2, resnet.py:44-49): x has 64 * HEADC channels, the strip's t1 is kept at full input
// resolution (2 TH + 1 rows), the taps of output pixel (r, c) sit at T1 row (2r + ky) W + 2c - 1 + kx (only the left border
// needs the zero row: W is even), and the kernel ends behind conv2: t2 [N, H/2, W/2, P] leaves through the T2 tile.
// NW = waves per workgroup (round 5).  4: a wave owns TWO output-channel tiles (one wave per SIMD).  8: a wave owns ONE tile and
// two waves share a SIMD: every weight byte still reaches the CU once (the waves split the CHANNEL tiles, not the pixels), but
// while one wave of a SIMD is held at its issue port by its weight loads (a buffer_load_b128 holds it ~40 cycles: a step of the
// 4-wave form costs its MFMA time + ~335 cycles for its eight loads, tools/dev/ubench/l2_burst.hip) the other one multiplies.
// FOLD (round 6) = the folded operands: the BatchNorm scales are in the fp16 weights (one rounding, like the plain weights),
// p.tab holds the shifts as (hi, lo) fp16 pairs, uint32 [P + P + C].  A shift enters its accumulator as ONE extra MFMA per tile (A row
// = {hi, lo, 0 ..}, B = ones at k = 0, 1), the identity residual as TWO (A = the 0/1 matrix that maps the registers the residual was
// picked up in — 16 consecutive channels per lane — onto the tile's MFMA rows), and every epilogue shrinks to fp16(relu(acc)):
// per quarter of phase 3 ~190 vector instructions + 32 table reads become 12 MFMAs + 64 (ft_common.h: relu_acc16).
template <int MT1, int MT2, bool XH, int NS, int HEADC = 0, int NW = 4, bool FOLD = false>
__global__ __launch_bounds__(64 * NW, NW / 4) void bottleneck_stream_direct_kernel(const BnsParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int P = 256;
  using G = BnsGeom<P>;
  constexpr bool HEAD = HEADC > 0;
  static_assert(!(HEAD && XH), "the head form uses full-width strips");
  constexpr int NCT = G::NCT, NC1 = HEAD ? HEADC : G::NC1, KC = G::KC, WSTEP = G::WSTEP, ROWB = G::ROWB;
  constexpr int G2 = NC1, G3 = G2 + 9 * KC, GEND = HEAD ? G3 : G3 + 4 * KC;
  static_assert(NW == 4 || NW == 8, "waves per workgroup");
  constexpr int CTW = 8 / NW, NT = 64 * NW;                  // output-channel tiles per wave, threads
  constexpr int XROWS = MT1 * 32, LX = (MT1 * 4 + NW - 1) / NW;   // x-chunk wave loads (8 rows each) per wave
  static_assert(LX * NW * 8 * 128 <= G::XSTRIDE, "x-chunk buffer");
  constexpr int NOUT = MT2 * 32;
  constexpr int ZROW = 61440, TABS = 65536, STG = 81920, STGB = NOUT * ROWB;   // [76 K, 77 K): scratch of the L2 touch loads
  constexpr int LDS_BYTES = STG + 2 * STGB;
  static_assert(XROWS * 128 <= G::XSTRIDE && NOUT * ROWB <= 61440 && LDS_BYTES <= 163840, "LDS map");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using c0 = std::integral_constant<int, 0>;
  using c1 = std::integral_constant<int, 1>;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wcol = wave;
  const int l31 = lane & 31, lhi = lane >> 5;

  const int logical = xcd_logical_wg(p.total);
  const int n = logical / p.ppi;
  const int W = p.W;
  const int TWc = XH ? p.TWc : (HEAD ? p.Wo : W);   // output columns of this workgroup; output pixel m = r * TWc + c
  const int PW = XH ? TWc + 2 : W;            // row pitch of the x-chunk / T1 patch
  int y0, x0 = 0;
  {
    const int li = logical - n * p.ppi;
    if constexpr (XH) {
      const int st = li / p.csplit;
      x0 = (li - st * p.csplit) * TWc;
      y0 = st * p.TH;
    } else {
      y0 = li * p.TH;
    }
  }
  const int Hout = HEAD ? p.Ho : p.H;
  const int rows_out = Hout - y0 < p.TH ? Hout - y0 : p.TH;
  const int cols_out = HEAD ? TWc : (W - x0 < TWc ? W - x0 : TWc);
  const int npix_out = rows_out * TWc;
  const int npix_halo = (HEAD ? 2 * p.TH + 1 : p.TH + 2) * PW;
  const int iy0 = HEAD ? 2 * y0 - 1 : y0 - 1;          // input row of the patch's first row

  const __amdgpu_buffer_rsrc_t rsrc_x = bns_rsrc(p.x, p.x_bytes), rsrc_y = bns_rsrc(p.y, p.y_bytes), rsrc_w = bns_rsrc(p.ws, p.ws_bytes);
  const __amdgpu_buffer_rsrc_t rsrc_t = bns_rsrc(p.tab, FOLD ? (2 * P + G::C) * 4 : 6 * G::TABB);
  constexpr unsigned kOOB = 0x80000000u;

  // (own copy of the x_voff set-up: NW waves, the column-split form's patch pitch and x-halo, the head form's first row)
  unsigned x_voff[LX];
#pragma unroll
  for (int t = 0; t < LX; ++t) {
    const int hp = (t * NW + wave) * 8 + (lane >> 3);
    const int hr = hp / PW, hc = hp - hr * PW;
    const int iy = iy0 + hr, ix = XH ? x0 - 1 + hc : hc;
    unsigned v = kOOB;
    if (hp < npix_halo && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)W)
      v = (unsigned)((((n * p.H + iy) * W + ix) * p.x_cstride + p.x_coff) * 2 + (((lane & 7) ^ BNS_XKEY(hp)) << 4));
    x_voff[t] = v;
  }
  const unsigned lane16 = (unsigned)lane * 16u;
  auto issue_x = [&](int c, int buf) { bns_issue_x<NW>(rsrc_x, smem + buf * G::XSTRIDE, wave, x_voff, c); };
  // the weight fragments of step g for this wave: (kk, tile 2*wcol + i) at g * WSTEP + (kk * NCT + 2*wcol + i) KiB
  static_assert(NS >= 3 && 12 % NS == 0, "ring phase of the unrolled phase-2 body (12 steps per kernel row)");
  constexpr int D = NS - 1;
  uint4_t areg[NS][4][CTW];
  auto load_a = [&](auto slotc, int g) {        // past the end of the stream: out of range, zeros, never multiplied
    constexpr int SL = decltype(slotc)::value;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int i = 0; i < CTW; ++i) {
#if FT_BNSD_ABL & 32
        if (g >= NC1) { uint4_t z{0u, 0u, 0u, 0u}; asm volatile("" : "+v"(z)); areg[SL][kk][i] = z; continue; }
#endif
        areg[SL][kk][i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, lane16, g * WSTEP + (kk * NCT + CTW * wcol + i) * 1024, 0);
      }
  };

  auto load_a_half = [&](auto slotc, int g, auto halfc) {   // K16 slices {0, 1} or {2, 3} of the step
    constexpr int SL = decltype(slotc)::value, HF = decltype(halfc)::value;
#pragma unroll
    for (int kk = 2 * HF; kk < 2 * HF + 2; ++kk)
#pragma unroll
      for (int i = 0; i < CTW; ++i) {
#if FT_BNSD_ABL & 16
        { uint4_t z{0u, 0u, 0u, 0u}; asm volatile("" : "+v"(z)); areg[SL][kk][i] = z; continue; }
#endif
        areg[SL][kk][i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, lane16, g * WSTEP + (kk * NCT + CTW * wcol + i) * 1024, 0);
      }
  };
  unsigned long long ts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  BNS_TS(0);
  // Inside a network the block's weights are not in this XCD's L2 when the kernel starts, and every workgroup of the XCD
  // asks for the same lines at the same moment: the stream then costs 17 us of a 46-us block (FT_BNS_DBG=64 in situ).  The
  // first round of workgroups on an XCD therefore TOUCHES the whole stream once, each its own 1/n-th (one dword per
  // 128-byte line, results discarded): the lines are on their way into the L2 before the lock-step demand loads reach them.
  // (as LDS-DMA into a scratch corner: no destination register whose reuse the compiler would have to guard.)  Round 6: EXACTLY
  // kTouch loads per thread (lines past the share: out of range, no traffic), issued BEHIND x chunk 0 and the weights of step 0 —
  // the touch used to lead every wave's in-order load queue, so the first chunk waited for 100 KB of line fetches per CU (start-up
  // 5.4 k cycles of a 71 k-cycle workgroup, tools/dev/bns_phases.py) — and counted by the first hand-counted wait.
  constexpr int kTouch = 6;
  auto issue_touch = [&]() {
    const bool on = blockIdx.x < 256 && !(p.dbg & 512);
    const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    const int first = p.total < 256 ? p.total : 256;
    const int nloc = (first - xcd + 7) >> 3;                       // workgroups of the first round on this XCD
    const unsigned lines = (p.ws_bytes + 127u) >> 7;
    const unsigned per = (lines + nloc - 1) / nloc;
    const unsigned lo = loc * per, hi = lo + per < lines ? lo + per : lines;
#pragma unroll
    for (int k = 0; k < kTouch; ++k) {
      const unsigned l = lo + tid + (unsigned)(NT * k);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (lds_ptr)(smem + 77824 + wave * 256), 4, (on && l < hi) ? l << 7 : kOOB, 0, 0, 0);
    }
  };
  // prologue: all six tables (12 KiB, 3 x 256-byte pieces per wave ... 48 pieces), x chunks 0..2, weights of steps 0 and 1, zero row
  // folded form: no tables in LDS; the shift pair of MFMA row l31 of every (epilogue, channel tile) of this wave sits in a register
  // (lanes 32..63 hold k = 8..15 of the shift slice: zeros, fetched out of range), and the two residual slices' 0/1 matrix is built here:
  // accumulator register k of lane (pixel, half) is channel 16 half + k (bns_sigma), the residual registers hold channels
  // 16 half + 8 h + e as element e of slice h, which the MFMA reads as k = 8 half + e: row r takes slice (sigma(r) >> 3) & 1, k = 8 (sigma(r) >> 4) + (sigma(r) & 7)
  [[maybe_unused]] unsigned shp[6][CTW];
  [[maybe_unused]] uint4_t permA[2];
  [[maybe_unused]] const uint4_t onesB = uint4_t{0x3C003C00u, 0u, 0u, 0u};
  if constexpr (FOLD) {
    const int sg = bns_sigma(l31);
    const bool on = lhi == (sg >> 4);
    const int ph = (sg >> 3) & 1, pe = sg & 7;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      unsigned w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = (on && ph == hh && (pe >> 1) == k) ? (0x3C00u << (16 * (pe & 1))) : 0u;
      permA[hh] = uint4_t{w[0], w[1], w[2], w[3]};
    }
  }
  constexpr int kTabLoads = FOLD ? 6 * CTW : 48 / NW;
  auto load_tables = [&]() {
    if constexpr (FOLD) {
      bns_load_shp<P>(shp, rsrc_t, l31, lhi, CTW * wcol, 0, 6);
    } else {
#pragma unroll
      for (int t = 0; t < 48 / NW; ++t)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_t, (lds_ptr)(smem + TABS + (t * NW + wave) * 256), 4, (unsigned)lane * 4u, (t * NW + wave) * 256, 0, 0);
    }
  };
  // order of every wave's (in-order) load queue: x chunk 0, the weights of step 0, the L2 touch, the tables / shift pairs, x chunks 1
  // and 2, the weights of steps 1 .. D-1
  // (the first wait counts them: compiler fences on both sides of the touch / table group, so that the count does not rest on one
  // compiler build's schedule)
  issue_x(0, 0);
  load_a(std::integral_constant<int, 0>{}, 0);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  issue_touch();
  load_tables();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  issue_x(1, 1);
  issue_x(2, 2);
  bns_unroll<D - 1>([&](auto sc) { load_a(std::integral_constant<int, decltype(sc)::value + 1>{}, decltype(sc)::value + 1); });
  if (tid < ROWB / 16) *reinterpret_cast<uint4_t*>(smem + ZROW + tid * 16) = uint4_t{0u, 0u, 0u, 0u};

  uint4_t res[4][CTW][MT2][2];
  int m_out[MT2], hp_out[MT2];          // output pixel of the lane in tile j, and its index in the halo patch
#pragma unroll
  for (int j = 0; j < MT2; ++j) {
    m_out[j] = j * 32 + l31;
    if constexpr (XH) {
      const int r = m_out[j] / TWc;
      hp_out[j] = (r + 1) * PW + (m_out[j] - r * TWc) + 1;
    } else if constexpr (HEAD) {
      const int r = m_out[j] / TWc;
      hp_out[j] = (2 * r + 1) * W + 2 * (m_out[j] - r * TWc);      // the pixel's centre tap in the T1 patch
    } else {
      hp_out[j] = m_out[j] + W;
    }
  }

  // ================= phase 1 ============================================================================================
  float16_t acc1[CTW][MT1];
#pragma unroll
  for (int i = 0; i < CTW; ++i)
#pragma unroll
    for (int j = 0; j < MT1; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[i][j][r] = 0.f;
  int b1_off[MT1];
#pragma unroll
  for (int j = 0; j < MT1; ++j) {
    const int hp = j * 32 + l31;
    b1_off[j] = hp * 128 + ((lhi ^ BNS_XKEY(hp)) << 4);
  }
  {
    uint4_t fx[2][MT1];
    auto ldx = [&](auto setc, int buf, int kk) {
      constexpr int S = decltype(setc)::value;
      const char* xb = smem + buf * G::XSTRIDE;
#pragma unroll
      for (int j = 0; j < MT1; ++j) {
#if FT_BNSD_ABL & 8
        { uint4_t z{0u, 0u, 0u, 0u}; asm volatile("" : "+v"(z)); fx[S][j] = z; continue; }
#endif
        fx[S][j] = *reinterpret_cast<const uint4_t*>(xb + (b1_off[j] ^ (kk << 5)));
      }
    };
    auto mma1 = [&](auto setc, auto slotc, auto kkc) {
      constexpr int S = decltype(setc)::value, SL = decltype(slotc)::value, kk = decltype(kkc)::value;
#pragma unroll
      for (int i = 0; i < CTW; ++i)
#pragma unroll
        for (int j = 0; j < MT1; ++j)
          acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, areg[SL][kk][i]),
                                                              __builtin_bit_cast(half8_t, fx[S][j]), acc1[i][j], 0, 0, 0);
    };
    // x chunk 0 has landed (this wave's share): behind it chunks 1, 2 and the two weight steps (8 loads each) may fly
    static_assert(2 * LX + 4 * CTW * D + kTouch + kTabLoads <= 63, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * LX + 4 * CTW * D + kTouch + kTabLoads) : "memory");
    BNS_BARRIER();
    BNS_TS(7);             // start-up: x chunk 0 of every wave has landed
    ldx(c0{}, 0, 0);
    bns_unroll<NC1>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      constexpr int buf = c % 3;
      using slot = std::integral_constant<int, c % NS>;
      // The wave-uniform branch below (residual pick-up) splits the chunk into two scheduling regions; each gets half of the
      // step's weight loads and a pinned issue order (see dstep): one vector-memory load and the LDS reads behind every two
      // MFMAs instead of hipcc's clusters of 6-8 loads with the matrix pipe drained behind them.
      load_a_half(std::integral_constant<int, (c + D) % NS>{}, c + D, c0{});
      ldx(c1{}, buf, 1);
      mma1(c0{}, slot{}, std::integral_constant<int, 0>{});
      ldx(c0{}, buf, 2);
      if constexpr (NW == 4) {
        // region: [x chunk c+2 DMA, slice-0 reads of this chunk, slice 3 of chunk c-1] (behind the last barrier) + the above
        __builtin_amdgcn_sched_group_barrier(0x020, LX, 0);
        bns_unroll<3>([&](auto) {
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, (2 * MT1 + 2) / 3, 0);
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        });
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, (MT1 + 2) / 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        bns_unroll<MT1 - 1>([&](auto) {
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, (MT1 + 2) / 3, 0);
        });
      }
      // (own copy of the residual pick-up: CTW tiles per wave, so the piece index goes by the tile's parity, and hp_out[] of the patch)
      if (!HEAD && !(FT_BNSD_ABL & 2) && c % 4 == (CTW * wcol) / 2) {  // this chunk holds the channels of this wave column for quarter c / 4
        constexpr int q = c / 4;
        const char* xb = smem + buf * G::XSTRIDE;
#pragma unroll
        for (int j = 0; j < MT2; ++j) {
          const int hp = hp_out[j];
          const char* rowp = xb + hp * 128;
#pragma unroll
          for (int i = 0; i < CTW; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h)
              res[q][i][j][h] = *reinterpret_cast<const uint4_t*>(rowp + (((4 * ((CTW * wcol + i) & 1) + 2 * lhi + h) ^ BNS_XKEY(hp)) << 4));
        }
      }
      mma1(c1{}, slot{}, std::integral_constant<int, 1>{});
      load_a_half(std::integral_constant<int, (c + D) % NS>{}, c + D, c1{});
      ldx(c1{}, buf, 3);
      mma1(c0{}, slot{}, std::integral_constant<int, 2>{});
      if constexpr (NW == 4) {
        bns_unroll<MT1>([&](auto) {
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        });
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 4 - MT1 > 0 ? 4 - MT1 : 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4 * MT1 - 2 * MT1 - 2, 0);
      }
      if constexpr (c + 1 < NC1) {
        // x chunk c+1 has landed and every read of chunk c's buffer is complete: refill it with chunk c+3.  Younger than x
        // chunk c+1 are the weights of step c+1 (needed next anyway), x chunk c+2 and the weights of step c+2.
        // (with a prefetch distance of three or more steps the weights of step c+1 are OLDER than x chunk c+1: two weight
        // steps may stay in flight)
#if FT_BNSD_ABL & 4
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#elif !(FT_BNSD_ABL & 16)
        if constexpr (c + 2 < NC1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LX + (D == 2 ? 4 * CTW : 8 * CTW)) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(D == 2 ? 4 * CTW : 8 * CTW) : "memory");
#else
        if constexpr (c + 2 < NC1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LX) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
#if !(FT_BNSD_ABL & 1)
        BNS_BARRIER();
#endif
        if constexpr (c + 3 < NC1 && !(FT_BNSD_ABL & 4)) issue_x(c + 3, buf);
        ldx(c0{}, (c + 1) % 3, 0);
      }
      mma1(c1{}, slot{}, std::integral_constant<int, 3>{});
    });
  }
  BNS_TS(1);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();          // every wave is past its last x-chunk read: the x buffers become T1
  {
    if constexpr (FOLD) bns_add_shift(acc1, shp[0]);
    [[maybe_unused]] const float* tb = reinterpret_cast<const float*>(smem + TABS);
#pragma unroll
    for (int i = 0; i < CTW; ++i) {
      [[maybe_unused]] const int ch = (CTW * wcol + i) * 32 + 16 * lhi;
      [[maybe_unused]] float4_t sc[4], sh[4];
      if constexpr (!FOLD) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          sc[g4] = *reinterpret_cast<const float4_t*>(tb + ch + g4 * 4);
          sh[g4] = *reinterpret_cast<const float4_t*>(tb + P + ch + g4 * 4);
        }
      }
#pragma unroll
      for (int j = 0; j < MT1; ++j) {
        const int hp = j * 32 + l31;
        const int hr = hp / PW;
        const int iy = iy0 + hr, ix = XH ? x0 - 1 + (hp - hr * PW) : 0;
        const bool inside = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)W;
        half8_t h8[2];
        if constexpr (FOLD) relu_acc16(acc1[i][j], h8);
        else bn_relu_acc16(acc1[i][j], sc, sh, h8);
#pragma unroll
        for (int h = 0; h < 2; ++h) h8[h] = bns_keep_if(h8[h], inside);
        if (hp < npix_halo) {
          char* rowp = smem + hp * ROWB;
          const int cb = (CTW * wcol + i) * 4 + 2 * lhi;
#pragma unroll
          for (int h = 0; h < 2; ++h)
            *reinterpret_cast<half8_t*>(rowp + (((cb + h) ^ (hp & 15)) << 4)) = h8[h];
        }
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();          // T1 complete
  BNS_TS(2);

  // ================= phases 2 + 3 =======================================================================================
  float16_t acc[CTW][MT2];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < CTW; ++i)
#pragma unroll
      for (int j = 0; j < MT2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  };
  zero_acc();
  int edge[MT2];
#pragma unroll
  for (int j = 0; j < MT2; ++j) {
    const int ox = m_out[j] % TWc;
    edge[j] = XH ? 0 : (HEAD ? (ox == 0 ? 1 : 0) : (ox == 0 ? 1 : 0) | (ox == W - 1 ? 2 : 0));
  }
  // T1 / T2 row of the pixel operand: `off` relative to the lane's own row; full-width strips mask the two x-border taps
  // (bad), the column-split form reads its zeroed halo columns instead
  auto row_bases = [&](int off, int kc, int bad, int (&rb)[MT2], bool t1) {
#pragma unroll
    for (int j = 0; j < MT2; ++j) {
      const int row = ((XH && t1) ? hp_out[j] - PW - 1 : ((HEAD && t1) ? hp_out[j] - W - 1 : m_out[j])) + off;
      const int v = row * ROWB + (((row & 15) ^ lhi) << 4);
      rb[j] = ((edge[j] & bad) ? ZROW + (lhi << 4) : v) ^ (kc << 7);
    }
  };
  auto tap_off = [&](int ky, int kx) { return (XH || HEAD) ? ky * PW + kx : ky * W + kx - 1; };
  uint4_t fb[2][MT2];
  auto ldb = [&](auto setc, int kk, const int (&rb)[MT2]) {
    constexpr int S = decltype(setc)::value;
#pragma unroll
    for (int j = 0; j < MT2; ++j) {
#if FT_BNSD_ABL & 64
      { uint4_t z{0u, 0u, 0u, 0u}; asm volatile("" : "+v"(z)); fb[S][j] = z; continue; }
#endif
      fb[S][j] = *reinterpret_cast<const uint4_t*>(smem + (rb[j] ^ (kk << 5)));
    }
  };
  auto mma2 = [&](auto setc, auto slotc, auto kkc, float16_t (&A)[CTW][MT2]) {
    constexpr int S = decltype(setc)::value, SL = decltype(slotc)::value, kk = decltype(kkc)::value;
#pragma unroll
    for (int i = 0; i < CTW; ++i)
#pragma unroll
      for (int j = 0; j < MT2; ++j)
        A[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, areg[SL][kk][i]),
                                                         __builtin_bit_cast(half8_t, fb[S][j]), A[i][j], 0, 0, 0);
  };
  // one weight step g (ring slot SL = g % 3): slice 0 of the pixel operand already sits in register set 0; `rbn` = row
  // bases of the next step
  auto dstep = [&](auto slotc, int g, const int (&rb)[MT2], bool has_next, const int (&rbn)[MT2], float16_t (&A)[CTW][MT2]) {
    constexpr int SL = decltype(slotc)::value;
    using slot = std::integral_constant<int, SL>;
    load_a(std::integral_constant<int, (SL + D) % NS>{}, g + D);
    ldb(c1{}, 1, rb);
    mma2(c0{}, slot{}, std::integral_constant<int, 0>{}, A);
    ldb(c0{}, 2, rb);
    mma2(c1{}, slot{}, std::integral_constant<int, 1>{}, A);
    ldb(c1{}, 3, rb);
    mma2(c0{}, slot{}, std::integral_constant<int, 2>{}, A);
    if (has_next) ldb(c0{}, 0, rbn);
    mma2(c1{}, slot{}, std::integral_constant<int, 3>{}, A);
    // Issue order of the step: one weight load and the pixel-operand reads after every MT2 MFMAs.  A buffer_load_b128 holds
    // the wave's issue port for ~40 cycles (tools/dev/ubench/l2_burst.hip: a step costs its compute time + 335 cycles for its
    // eight loads, whatever the prefetch depth); clustered as hipcc places them, the matrix pipe drains behind them.
    if constexpr (NW == 4) {
      bns_unroll<8>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        __builtin_amdgcn_sched_group_barrier(0x008, MT2, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, (i & 1) ? (MT2 + 1) / 2 : MT2 / 2, 0);
      });
    }
  };

  // ---- phase 2: nine taps x KC chunks, three taps per loop trip (12 steps: a multiple of the register ring period) -------
  {
    static_assert((3 * KC) % NS == 0, "ring phase of the unrolled body");
    int rb[MT2], rbn[MT2];
    row_bases(tap_off(0, 0), 0, 1, rb, true);
    ldb(c0{}, 0, rb);
    for (int ky = 0; ky < 3; ++ky) {
      bns_unroll<3 * KC>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        constexpr int kx = s / KC, kc = s % KC;
        constexpr int nkc = (kc + 1) % KC, nkx = kc + 1 == KC ? (kx + 1) % 3 : kx;
        const int nky = (kc + 1 == KC && kx == 2) ? ky + 1 : ky;
        row_bases(tap_off(nky, nkx), nkc, nkx == 0 ? 1 : (nkx == 2 ? 2 : 0), rbn, true);
        dstep(std::integral_constant<int, (G2 + s) % NS>{}, G2 + 3 * KC * ky + s, rb, !(ky == 2 && s == 3 * KC - 1), rbn, acc);
#pragma unroll
        for (int j = 0; j < MT2; ++j) rb[j] = rbn[j];
      });
    }
  }
  BNS_TS(3);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();          // every wave is past its last T1 read: T2 overwrites T1
  {
    if constexpr (FOLD) bns_add_shift(acc, shp[1]);
    [[maybe_unused]] const float* tb = reinterpret_cast<const float*>(smem + TABS + G::TABB);
#pragma unroll
    for (int i = 0; i < CTW; ++i) {
      [[maybe_unused]] const int ch = (CTW * wcol + i) * 32 + 16 * lhi;
      [[maybe_unused]] float4_t sc[4], sh[4];
      if constexpr (!FOLD) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          sc[g4] = *reinterpret_cast<const float4_t*>(tb + ch + g4 * 4);
          sh[g4] = *reinterpret_cast<const float4_t*>(tb + P + ch + g4 * 4);
        }
      }
#pragma unroll
      for (int j = 0; j < MT2; ++j) {
        const int m = m_out[j];
        half8_t h8[2];
        if constexpr (FOLD) relu_acc16(acc[i][j], h8);
        else bn_relu_acc16(acc[i][j], sc, sh, h8);
        char* rowp = smem + m * ROWB;
        const int cb = (CTW * wcol + i) * 4 + 2 * lhi;
#pragma unroll
        for (int h = 0; h < 2; ++h) *reinterpret_cast<half8_t*>(rowp + (((cb + h) ^ (m & 15)) << 4)) = h8[h];
      }
    }
  }
  zero_acc();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();          // T2 complete
  BNS_TS(4);
  if constexpr (HEAD) {
    // the head form ends here: the T2 tile (rows = output pixels, 16-byte chunk ^= row & 15) leaves as whole lines
    constexpr int CPRH = ROWB / 16, NSTH = NOUT * CPRH / NT;
#pragma unroll
    for (int k = 0; k < NSTH; ++k) {
      const int idx = tid + NT * k, m = idx / CPRH, ch = idx % CPRH;
      const int r = m / TWc, c = m - r * TWc;
      const unsigned vo = m < npix_out ? (unsigned)((((n * p.Ho + y0 + r) * p.Wo + c) * p.y_cstride + p.y_coff + ch * 8) * 2) : kOOB;
      const uint4_t v = *reinterpret_cast<const uint4_t*>(smem + m * ROWB + ((ch ^ (m & 15)) << 4));
      if (!(p.dbg & 4)) __builtin_amdgcn_raw_buffer_store_b128(v, rsrc_y, vo, 0, FT_YSTORE_BUF_AUX);
    }
    return;
  }

  // ---- phase 3: four quarters of P output channels; the tile of a quarter leaves through one of two LDS staging tiles ----
  {
    // WSTG: the wave's own [NOUT pixels][128 bytes = its 64 channels of the quarter] tile, 16-byte chunk c of pixel m at chunk
    // c ^ (m & 7): the eight lanes of a ds_write_b128 group (eight pixels, one chunk) and the sixteen of a ds_read_b128 group
    // (two pixels x eight chunks ...) cover distinct bank groups.  Read-out: lane -> pixel lane / 8 + 8 k, chunk lane % 8.
    constexpr bool WSTG = CTW == 2;
    constexpr int CPR = ROWB / 16, NSTG = WSTG ? NOUT / 8 : NOUT * CPR / NT;
    unsigned s_voff[NSTG];
    int s_off[NSTG];
#pragma unroll
    for (int k = 0; k < NSTG; ++k) {
      if constexpr (WSTG) {
        const int m = (lane >> 3) + 8 * k, ch = lane & 7;
        const int r = m / TWc, c = m - r * TWc;
        s_voff[k] = (m < npix_out && c < cols_out)
                        ? (unsigned)((((n * p.H + y0 + r) * W + x0 + c) * p.y_cstride + p.y_coff + wcol * 64 + ch * 8) * 2) : kOOB;
        s_off[k] = wave * (NOUT * 128) + m * 128 + ((ch ^ (m & 7)) << 4);
      } else {
        const int idx = tid + NT * k, m = idx / CPR, ch = idx % CPR;
        const int r = m / TWc, c = m - r * TWc;
        s_voff[k] = (m < npix_out && c < cols_out) ? (unsigned)((((n * p.H + y0 + r) * W + x0 + c) * p.y_cstride + p.y_coff + ch * 8) * 2) : kOOB;
        s_off[k] = m * ROWB + ((ch ^ (m & 15)) << 4);
      }
    }
    int rb[MT2], rbn[MT2];
    row_bases(0, 0, 0, rb, false);
    ldb(c0{}, 0, rb);
    // epilogue of quarter q, tile (i, j): folded BN + residual + ReLU -> fp16 -> staging tile q & 1
    auto epi_piece = [&](auto qc, int i, int j, float16_t (&A)[CTW][MT2]) {
      constexpr int q = decltype(qc)::value;
      char* stg = smem + STG + (q & 1) * STGB;
      [[maybe_unused]] const float* tb = reinterpret_cast<const float*>(smem + TABS + (2 + q) * G::TABB);
      [[maybe_unused]] const int ch = (CTW * wcol + i) * 32 + 16 * lhi;
      [[maybe_unused]] float4_t sc[4], sh[4];
      [[maybe_unused]] half8_t o8[2];
      if constexpr (FOLD) {
        relu_acc16(A[i][j], o8);
      } else {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          sc[g4] = *reinterpret_cast<const float4_t*>(tb + ch + g4 * 4);
          sh[g4] = *reinterpret_cast<const float4_t*>(tb + P + ch + g4 * 4);
        }
      }
      const int m = m_out[j];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        half8_t o;
        if constexpr (FOLD) o = o8[h];
        else o = bn_res_relu_acc8(A[i][j], h, sc, sh, __builtin_bit_cast(half8_t, res[q][i][j][h]));
        if constexpr (WSTG) *reinterpret_cast<half8_t*>(stg + wave * (NOUT * 128) + m * 128 + (((i * 4 + 2 * lhi + h) ^ (m & 7)) << 4)) = o;
        else *reinterpret_cast<half8_t*>(stg + m * ROWB + ((((CTW * wcol + i) * 4 + 2 * lhi + h) ^ (m & 15)) << 4)) = o;
      }
    };
    // folded form: shift3 of the quarter and the residual join tile (i, j)'s accumulator as three MFMAs
    [[maybe_unused]] auto fold_tail = [&](auto qc, int i, int j, float16_t (&A)[CTW][MT2]) {
      constexpr int q = decltype(qc)::value;
      bns_fold_tail(A[i][j], shp[2 + q][i], onesB, permA, res[q][i][j]);
    };
    auto readout = [&](auto qc) {
      constexpr int q = decltype(qc)::value;
      const char* stg = smem + STG + (q & 1) * STGB;
#pragma unroll
      for (int k = 0; k < NSTG; ++k) {
        const uint4_t v = *reinterpret_cast<const uint4_t*>(stg + s_off[k]);
        if (!(p.dbg & 4)) __builtin_amdgcn_raw_buffer_store_b128(v, rsrc_y, s_voff[k] + (unsigned)(q * P * 2), 0, FT_YSTORE_BUF_AUX);
      }
    };
    // (hiding a quarter's epilogue inside the next quarter's weight steps was tried: it spills.  profiles/HISTORY.md)
    bns_unroll<4>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      bns_unroll<KC>([&](auto kcc) {
        constexpr int kc = decltype(kcc)::value;
        constexpr int g = G3 + q * KC + kc;
        row_bases(0, (kc + 1) % KC, 0, rbn, false);
        dstep(std::integral_constant<int, g % NS>{}, g, rb, g + 1 < GEND, rbn, acc);
#pragma unroll
        for (int j = 0; j < MT2; ++j) rb[j] = rbn[j];
      });
      if constexpr (FOLD) {
#pragma unroll
        for (int i = 0; i < CTW; ++i)
#pragma unroll
          for (int j = 0; j < MT2; ++j) fold_tail(qc, i, j, acc);
      }
#pragma unroll
      for (int i = 0; i < CTW; ++i)
#pragma unroll
        for (int j = 0; j < MT2; ++j) epi_piece(qc, i, j, acc);
      zero_acc();
      // the two staging tiles alternate: a tile's previous readers (quarter q-2) are two barriers behind
      // (wave-private pieces: a wave reads back only what it wrote itself, its LDS operations execute in order: no barrier)
      if constexpr (!WSTG) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        BNS_BARRIER();
      } else {
        asm volatile("" ::: "memory");       // compiler fence only: the read-out must stay behind the tile's writes in program order
      }
      readout(qc);
    });
  }
  BNS_TS_TAIL();
#endif
}

// ---- 256 planes, 16-pixel MFMA tiles (weights straight to registers, folded operands, four waves) ----------------------------
// The full-width-strip form of bottleneck_stream_direct_kernel<3, 2, false, NS, 0, 4, true> on v_mfma_f32_16x16x32_f16: the R50
// layer3 strip is 4 x 12 = 48 output pixels on a 6 x 12 = 72-pixel halo, which the 32-pixel tiles of the direct kernel run as 64
// and 96 (a quarter of every phase multiplies zero rows).  With 16-pixel tiles the strip is 3 tiles and its halo 5 (80): per wave
// 4 channel tiles x {5, 3, 3} pixel tiles x {32, 72, 32} K32 steps x 16 cycles = 30.7 k MFMA cycles instead of 40.8 k.
// Same plan as the direct kernel: x-chunk ring -> T1 -> T2 in LDS, the wave's weight fragments of a 64-wide K step (8 x 1 KiB,
// two K32 slices x four channel tiles) straight to registers NS - 1 steps ahead, L2 touch behind x chunk 0, wave-private output
// staging.  Fragment maps (lane l, p = l & 15, h = l >> 4):
//   A (weights)  row p of a 16-channel tile, k = 8 h .. 8 h + 7 of the K32 slice.  Row r of tile t of a wave is channel
//                16 (r >> 2) + 4 t + (r & 3) of the wave's 64 (bns_pack16_kernel), so that
//   C / D        pixel p, rows 4 h + reg: the lane's 4 tiles x 4 registers are the 16 CONSECUTIVE channels 16 h + 4 t + reg: T1 / T2 /
//                the output leave as two 16-byte pieces per lane and pixel tile, the residual arrives as two.
//   B (pixels)   pixel p, the same k: one ds_read_b128 at 16-byte piece h (+ 4 for the odd slice) of the pixel's 128 bytes of the
//                chunk; the sixteen lanes of a piece read sixteen consecutive rows, which BNS_XKEY (x chunks: two rows per bank row)
//                and row & 15 (T1 / T2: 512-byte rows) spread over all banks.
//   shift        one MFMA per tile: A row = {hi, lo, 0 ..} in the lanes with h = 0, B = ones at k = 0, 1.
//   residual     one MFMA per tile: B = the lane's residual piece t >> 1 (channels 16 h + 8 (t >> 1) + e as k = 8 h + e), A = the 0/1 matrix
//                with row 4 h' + reg at k = 8 h' + 4 (t & 1) + reg (two matrices, by t & 1).
template <int NS>
__global__ __launch_bounds__(256, 1) void bottleneck_stream_tile16_kernel(const BnsParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int P = 256;
  using G = BnsGeom<P>;
  constexpr int NC1 = G::NC1, KC = G::KC, WSTEP = G::WSTEP, ROWB = G::ROWB;
  constexpr int G2 = NC1, G3 = G2 + 9 * KC, GEND = G3 + 4 * KC;
  constexpr int CT = 4, MT1 = 5, MT2 = 3, NT = 256;             // channel tiles per wave, halo / output pixel tiles of 16
  constexpr int LX = (MT1 * 2 + 3) / 4;                         // x-chunk wave loads (8 rows each) per wave
  constexpr int NOUT = MT2 * 16;
  constexpr int ZROW = 61440, TOUCH = 77824, STG = 81920, STGB = 4 * NOUT * 128;
  static_assert(LX * 4 * 8 * 128 <= G::XSTRIDE && MT1 * 16 * ROWB <= ZROW && STG + 2 * STGB <= 163840, "LDS map");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using c0 = std::integral_constant<int, 0>;
  using c1 = std::integral_constant<int, 1>;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lq = lane >> 4;

  const int logical = xcd_logical_wg(p.total);
  const int n = logical / p.ppi;
  const int W = p.W;
  const int y0 = (logical - n * p.ppi) * p.TH;
  const int rows_out = p.H - y0 < p.TH ? p.H - y0 : p.TH;
  const int npix_out = rows_out * W;
  const int npix_halo = (p.TH + 2) * W;
  const int iy0 = y0 - 1;

  const __amdgpu_buffer_rsrc_t rsrc_x = bns_rsrc(p.x, p.x_bytes), rsrc_y = bns_rsrc(p.y, p.y_bytes), rsrc_w = bns_rsrc(p.ws, p.ws_bytes);
  const __amdgpu_buffer_rsrc_t rsrc_t = bns_rsrc(p.tab, (2 * P + G::C) * 4);
  constexpr unsigned kOOB = 0x80000000u;

  unsigned x_voff[LX];
#pragma unroll
  for (int t = 0; t < LX; ++t) {
    const int hp = (t * 4 + wave) * 8 + (lane >> 3);
    const int hr = hp / W, hc = hp - hr * W;
    const int iy = iy0 + hr;
    unsigned v = kOOB;
    if (hp < npix_halo && (unsigned)iy < (unsigned)p.H)
      v = (unsigned)((((n * p.H + iy) * W + hc) * p.x_cstride + p.x_coff) * 2 + (((lane & 7) ^ BNS_XKEY(hp)) << 4));
    x_voff[t] = v;
  }
  const unsigned lane16 = (unsigned)lane * 16u;
  auto issue_x = [&](int c, int buf) { bns_issue_x<4>(rsrc_x, smem + buf * G::XSTRIDE, wave, x_voff, c); };
  // the weight fragments of step g for this wave: (slice ks, tile 4 * wave + t) at g * WSTEP + (ks * 16 + 4 * wave + t) KiB
  static_assert(NS >= 3 && 12 % NS == 0, "ring phase of the unrolled phase-2 body (12 steps per kernel row)");
  constexpr int D = NS - 1;
  uint4_t areg[NS][2][CT];
  auto load_a_slice = [&](auto slotc, int g, auto ksc) {   // past the end of the stream: out of range, zeros, never multiplied
    constexpr int SL = decltype(slotc)::value, ks = decltype(ksc)::value;
#pragma unroll
    for (int t = 0; t < CT; ++t)
      areg[SL][ks][t] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, lane16, g * WSTEP + (ks * 16 + CT * wave + t) * 1024, 0);
  };
  auto load_a = [&](auto slotc, int g) {
    load_a_slice(slotc, g, c0{});
    load_a_slice(slotc, g, c1{});
  };
  unsigned long long ts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  BNS_TS(0);
  // the L2 touch of the direct kernel: exactly kTouch loads per thread, behind x chunk 0 and the weights of step 0
  constexpr int kTouch = 6;
  auto issue_touch = [&]() {
    const bool on = blockIdx.x < 256 && !(p.dbg & 512);
    const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    const int first = p.total < 256 ? p.total : 256;
    const int nloc = (first - xcd + 7) >> 3;                       // workgroups of the first round on this XCD
    const unsigned lines = (p.ws_bytes + 127u) >> 7;
    const unsigned per = (lines + nloc - 1) / nloc;
    const unsigned lo = loc * per, hi = lo + per < lines ? lo + per : lines;
#pragma unroll
    for (int k = 0; k < kTouch; ++k) {
      const unsigned l = lo + tid + (unsigned)(NT * k);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (lds_ptr)(smem + TOUCH + wave * 256), 4, (on && l < hi) ? l << 7 : kOOB, 0, 0, 0);
    }
  };
  // the shift pair of MFMA row l15 of every (epilogue, channel tile) of this wave (lanes 16..63 hold k = 8..31 of the shift slice: zeros,
  // fetched out of range; those of phase 3 are fetched behind phase 1, where its registers are free), and the two 0/1 matrices of the
  // residual MFMAs.  (own copies: rows of 16-channel tiles, not bns_sigma's order)
  unsigned shp[6][CT];
  uint4_t permA[2];
  {
    const bool on = lq == (l15 >> 2);
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int pe = 4 * o + (l15 & 3);
      unsigned w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = (on && (pe >> 1) == k) ? (0x3C00u << (16 * (pe & 1))) : 0u;
      permA[o] = uint4_t{w[0], w[1], w[2], w[3]};
    }
  }
  constexpr int kTabLoads = 2 * CT;
  auto load_tables = [&](int e0, int e1) {
    const unsigned so = lq == 0 ? 4u * (unsigned)(16 * (l15 >> 2) + (l15 & 3)) : kOOB;
#pragma unroll
    for (int e = e0; e < e1; ++e)
#pragma unroll
      for (int t = 0; t < CT; ++t)
        shp[e][t] = __builtin_amdgcn_raw_buffer_load_b32(rsrc_t, so, 4 * (e * P + 64 * wave + 4 * t), 0);
  };
  // order of every wave's (in-order) load queue: x chunk 0, the weights of step 0, the L2 touch, the shift pairs, x chunks 1 and 2,
  // the weights of steps 1 .. D-1.  The first wait below counts them: nothing may move across the touch / shift-pair group.
  issue_x(0, 0);
  load_a(c0{}, 0);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  issue_touch();
  load_tables(0, 2);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  issue_x(1, 1);
  issue_x(2, 2);
  bns_unroll<D - 1>([&](auto sc) { load_a(std::integral_constant<int, decltype(sc)::value + 1>{}, decltype(sc)::value + 1); });
  if (tid < ROWB / 16) *reinterpret_cast<uint4_t*>(smem + ZROW + tid * 16) = uint4_t{0u, 0u, 0u, 0u};

  uint4_t res[4][MT2][2];
  int m_out[MT2], hp_out[MT2];          // output pixel of the lane in tile j, and its index in the halo strip
#pragma unroll
  for (int j = 0; j < MT2; ++j) {
    m_out[j] = j * 16 + l15;
    hp_out[j] = m_out[j] + W;
  }

  // ================= phase 1 ============================================================================================
  float4_t acc1[CT][MT1];
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int j = 0; j < MT1; ++j) acc1[t][j] = float4_t{0.f, 0.f, 0.f, 0.f};
  int b1_off[MT1];
#pragma unroll
  for (int j = 0; j < MT1; ++j) {
    const int hp = j * 16 + l15;
    b1_off[j] = hp * 128 + ((lq ^ BNS_XKEY(hp)) << 4);
  }
  {
    uint4_t fx[2][MT1];
    auto ldx = [&](auto setc, int buf, int ks) {
      constexpr int S = decltype(setc)::value;
      const char* xb = smem + buf * G::XSTRIDE;
#pragma unroll
      for (int j = 0; j < MT1; ++j) fx[S][j] = *reinterpret_cast<const uint4_t*>(xb + (b1_off[j] ^ (ks << 6)));
    };
    auto mma1 = [&](auto setc, auto slotc, auto ksc) {
      constexpr int S = decltype(setc)::value, SL = decltype(slotc)::value, ks = decltype(ksc)::value;
#pragma unroll
      for (int j = 0; j < MT1; ++j)
#pragma unroll
        for (int t = 0; t < CT; ++t)
          acc1[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, areg[SL][ks][t]),
                                                              __builtin_bit_cast(half8_t, fx[S][j]), acc1[t][j], 0, 0, 0);
    };
    // x chunk 0 has landed (this wave's share): behind it the touch, the shift pairs, chunks 1, 2 and D weight steps may fly
    static_assert(2 * LX + 2 * CT * D + kTouch + kTabLoads <= 63, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * LX + 2 * CT * D + kTouch + kTabLoads) : "memory");
    BNS_BARRIER();
    BNS_TS(7);             // start-up: x chunk 0 of every wave has landed
    ldx(c0{}, 0, 0);
    bns_unroll<NC1>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      constexpr int buf = c % 3;
      using slot = std::integral_constant<int, c % NS>;
      using nslot = std::integral_constant<int, (c + D) % NS>;
      // The wave-uniform branch below (residual pick-up) splits the chunk into two scheduling regions, each with one slice's weight
      // loads of step c + D.  Region 1: [x chunk c+2 DMA, slice-0 reads of this chunk, slice 1 of chunk c-1] (behind the last
      // barrier) + slice 0 of this chunk: one LDS read or one weight load behind every two MFMAs.
      load_a_slice(nslot{}, c + D, c0{});
      ldx(c1{}, buf, 1);
      mma1(c0{}, slot{}, c0{});
      __builtin_amdgcn_sched_group_barrier(0x020, LX, 0);
      bns_unroll<MT1>([&](auto) {
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      });
      bns_unroll<CT>([&](auto) {
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      });
      __builtin_amdgcn_sched_group_barrier(0x008, CT * MT1 - 2 * MT1 - 2 * CT, 0);
      bns_unroll<MT1>([&](auto) {
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      });
      if (c % 4 == wave) {  // this chunk holds the channels of this wave for quarter c / 4: the lane's own 16 channels, two pieces
        constexpr int q = c / 4;
        const char* xb = smem + buf * G::XSTRIDE;
#pragma unroll
        for (int j = 0; j < MT2; ++j) {
          const int hp = hp_out[j];
          const char* rowp = xb + hp * 128;
#pragma unroll
          for (int h = 0; h < 2; ++h)
            res[q][j][h] = *reinterpret_cast<const uint4_t*>(rowp + (((2 * lq + h) ^ BNS_XKEY(hp)) << 4));
        }
      }
      load_a_slice(nslot{}, c + D, c1{});
      if constexpr (c + 1 < NC1) {
        // x chunk c+1 has landed and every read of chunk c's buffer is complete: refill it with chunk c+3.  Younger than x chunk
        // c+1 are the weights of steps c+D-1 and c+D and x chunk c+2 (the weights of step c+1 are older: D >= 2 steps ahead)
        if constexpr (c + 2 < NC1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LX + 4 * CT) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(4 * CT) : "memory");
        BNS_BARRIER();
        if constexpr (c + 3 < NC1) issue_x(c + 3, buf);
        ldx(c0{}, (c + 1) % 3, 0);
      }
      mma1(c1{}, slot{}, c1{});
    });
  }
  BNS_TS(1);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();          // every wave is past its last x-chunk read: the x buffers become T1
  // the lane's 16 consecutive channels of pixel tile j as two 16-byte pieces: fp16(relu(acc))
  auto pieces = [&](auto& A, int j, half8_t (&h8)[2]) {
    h8[0] = relu_acc4x2(A[0][j], A[1][j]);
    h8[1] = relu_acc4x2(A[2][j], A[3][j]);
  };
  {
    bns_add_shift(acc1, shp[0]);
#pragma unroll
    for (int j = 0; j < MT1; ++j) {
      const int hp = j * 16 + l15;
      const int iy = iy0 + hp / W;
      const bool inside = (unsigned)iy < (unsigned)p.H;
      half8_t h8[2];
      pieces(acc1, j, h8);
#pragma unroll
      for (int h = 0; h < 2; ++h) h8[h] = bns_keep_if(h8[h], inside);
      if (hp < npix_halo) {
        char* rowp = smem + hp * ROWB;
        const int cb = wave * 8 + 2 * lq;
#pragma unroll
        for (int h = 0; h < 2; ++h) *reinterpret_cast<half8_t*>(rowp + (((cb + h) ^ (hp & 15)) << 4)) = h8[h];
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();          // T1 complete
  BNS_TS(2);
  load_tables(2, 6);

  // ================= phases 2 + 3 =======================================================================================
  float4_t acc[CT][MT2];
  auto zero_acc = [&]() {
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
      for (int j = 0; j < MT2; ++j) acc[t][j] = float4_t{0.f, 0.f, 0.f, 0.f};
  };
  zero_acc();
  int edge[MT2];
#pragma unroll
  for (int j = 0; j < MT2; ++j) edge[j] = bns_edge(m_out[j] % W, W);
  // T1 / T2 row of the pixel operand: `off` relative to the lane's own row; the two x-border taps (bad) read the zero row
  auto row_bases = [&](int off, int kc, int bad, int (&rb)[MT2]) {
#pragma unroll
    for (int j = 0; j < MT2; ++j) {
      const int row = m_out[j] + off;
      const int v = row * ROWB + (((row & 15) ^ lq) << 4);
      rb[j] = ((edge[j] & bad) ? ZROW + (lq << 4) : v) ^ (kc << 7);
    }
  };
  uint4_t fb[2][MT2];
  auto ldb = [&](auto setc, int ks, const int (&rb)[MT2]) {
    constexpr int S = decltype(setc)::value;
#pragma unroll
    for (int j = 0; j < MT2; ++j) fb[S][j] = *reinterpret_cast<const uint4_t*>(smem + (rb[j] ^ (ks << 6)));
  };
  auto mma2 = [&](auto setc, auto slotc, auto ksc) {
    constexpr int S = decltype(setc)::value, SL = decltype(slotc)::value, ks = decltype(ksc)::value;
#pragma unroll
    for (int j = 0; j < MT2; ++j)
#pragma unroll
      for (int t = 0; t < CT; ++t)
        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, areg[SL][ks][t]),
                                                           __builtin_bit_cast(half8_t, fb[S][j]), acc[t][j], 0, 0, 0);
  };
  // one weight step g (ring slot SL): slice 0 of the pixel operand already sits in register set 0; `rbn` = row bases of the next step.
  // Issue order: an LDS read, three MFMAs, a weight load — eight times (a buffer_load_b128 holds the wave's issue port for ~40 cycles;
  // clustered as hipcc places them, the matrix pipe drains behind them)
  auto dstep = [&](auto slotc, int g, const int (&rb)[MT2], bool has_next, const int (&rbn)[MT2]) {
    constexpr int SL = decltype(slotc)::value;
    using slot = std::integral_constant<int, SL>;
    load_a(std::integral_constant<int, (SL + D) % NS>{}, g + D);
    ldb(c1{}, 1, rb);
    mma2(c0{}, slot{}, c0{});
    if (has_next) ldb(c0{}, 0, rbn);
    mma2(c1{}, slot{}, c1{});
    bns_unroll<8>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      __builtin_amdgcn_sched_group_barrier(0x100, (i & 3) < MT2 ? 1 : 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, CT * MT2 / 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    });
  };

  // ---- phase 2: nine taps x KC chunks, three taps per loop trip (12 steps: a multiple of the register ring period) -------
  {
    static_assert((3 * KC) % NS == 0, "ring phase of the unrolled body");
    int rb[MT2], rbn[MT2];
    row_bases(-1, 0, 1, rb);
    ldb(c0{}, 0, rb);
    for (int ky = 0; ky < 3; ++ky) {
      bns_unroll<3 * KC>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        constexpr int kx = s / KC, kc = s % KC;
        constexpr int nkc = (kc + 1) % KC, nkx = kc + 1 == KC ? (kx + 1) % 3 : kx;
        const int nky = (kc + 1 == KC && kx == 2) ? ky + 1 : ky;
        row_bases(nky * W + nkx - 1, nkc, nkx == 0 ? 1 : (nkx == 2 ? 2 : 0), rbn);
        // (the last step's look-ahead read lands inside LDS and is never multiplied: no branch in the step)
        dstep(std::integral_constant<int, (G2 + s) % NS>{}, G2 + 3 * KC * ky + s, rb, true, rbn);
#pragma unroll
        for (int j = 0; j < MT2; ++j) rb[j] = rbn[j];
      });
    }
  }
  BNS_TS(3);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();          // every wave is past its last T1 read: T2 overwrites T1
  {
    bns_add_shift(acc, shp[1]);
#pragma unroll
    for (int j = 0; j < MT2; ++j) {
      const int m = m_out[j];
      half8_t h8[2];
      pieces(acc, j, h8);
      char* rowp = smem + m * ROWB;
      const int cb = wave * 8 + 2 * lq;
#pragma unroll
      for (int h = 0; h < 2; ++h) *reinterpret_cast<half8_t*>(rowp + (((cb + h) ^ (m & 15)) << 4)) = h8[h];
    }
  }
  zero_acc();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();          // T2 complete
  BNS_TS(4);

  // ---- phase 3: four quarters of P output channels; a quarter leaves through one of the wave's two private staging tiles ----------
  {
    // the wave's own [NOUT pixels][128 bytes = its 64 channels of the quarter] tile, 16-byte piece c of pixel m at piece c ^ (m & 7);
    // read-out: lane -> pixel lane / 8 + 8 k, piece lane % 8 (whole 128-byte lines per pixel)
    constexpr int NSTG = NOUT / 8;
    unsigned s_voff[NSTG];
    int s_off[NSTG];
#pragma unroll
    for (int k = 0; k < NSTG; ++k) {
      const int m = (lane >> 3) + 8 * k, ch = lane & 7;
      s_voff[k] = m < npix_out ? (unsigned)((((n * p.H + y0) * W + m) * p.y_cstride + p.y_coff + wave * 64 + ch * 8) * 2) : kOOB;
      s_off[k] = wave * (NOUT * 128) + m * 128 + ((ch ^ (m & 7)) << 4);
    }
    int rb[MT2], rbn[MT2];
    row_bases(0, 0, 0, rb);
    ldb(c0{}, 0, rb);
    bns_unroll<4>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      bns_unroll<KC>([&](auto kcc) {
        constexpr int kc = decltype(kcc)::value;
        constexpr int g = G3 + q * KC + kc;
        row_bases(0, (kc + 1) % KC, 0, rbn);
        dstep(std::integral_constant<int, g % NS>{}, g, rb, g + 1 < GEND, rbn);
#pragma unroll
        for (int j = 0; j < MT2; ++j) rb[j] = rbn[j];
      });
      // shift3 of the quarter and the residual join every tile's accumulator as two MFMAs
      bns_add_shift(acc, shp[2 + q]);
#pragma unroll
      for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int j = 0; j < MT2; ++j)
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, permA[t & 1]),
                                                             __builtin_bit_cast(half8_t, res[q][j][t >> 1]), acc[t][j], 0, 0, 0);
      char* stg = smem + STG + (q & 1) * STGB + wave * (NOUT * 128);
#pragma unroll
      for (int j = 0; j < MT2; ++j) {
        const int m = m_out[j];
        half8_t h8[2];
        pieces(acc, j, h8);
#pragma unroll
        for (int h = 0; h < 2; ++h) *reinterpret_cast<half8_t*>(stg + m * 128 + (((2 * lq + h) ^ (m & 7)) << 4)) = h8[h];
      }
      zero_acc();
      // wave-private pieces: a wave reads back only what it wrote itself, its LDS operations execute in order: no barrier, only a
      // compiler fence (the read-out must stay behind the tile's writes in program order)
      asm volatile("" ::: "memory");
#pragma unroll
      for (int k = 0; k < NSTG; ++k) {
        const uint4_t v = *reinterpret_cast<const uint4_t*>(smem + STG + (q & 1) * STGB + s_off[k]);
        if (!(p.dbg & 4)) __builtin_amdgcn_raw_buffer_store_b128(v, rsrc_y, s_voff[k] + (unsigned)(q * P * 2), 0, FT_YSTORE_BUF_AUX);
      }
    });
  }
  BNS_TS_TAIL();
#endif
}

// ---- 128 planes, weights straight to registers (folded operands, four waves) ---------------------------------------------------
// bottleneck_stream_kernel<128, MT1, MT2, true> with the weight path of bottleneck_stream_direct_kernel.  At 128 planes the waves are
// WCOLS 2 x WPG 2: the two pixel groups of a wave column multiply the SAME weight fragments, which is why the ring kernel shares them
// through LDS — and pays for it with (2 A + 3 B) ds_read_b128 per 6 MFMAs at one wave per SIMD and a workgroup barrier at every 16-KiB
// weight step (34 per strip).  Here every wave loads its own 8 x 1 KiB of a step (kk, tile 2 wcol + i at g * WSTEP + (kk * NCT + 2 wcol
// + i) KiB of the unchanged bns_pack_kernel<128> stream) straight into VGPRs NS - 1 steps ahead: the stream reaches a CU twice (32 KiB
// per step, half of what the 256-plane direct kernels pull through the same path per MFMA cycle), the A operand never crosses LDS, the
// ring barriers are gone (phases 2 and 3 meet only at the phase transitions and at the output tile of a quarter) and the 48 KiB of the
// ring hold a second output staging tile, so that the write of quarter q + 1 never waits behind the stores of quarter q.
// Everything else is the ring kernel's plan: x-chunk ring -> T1 -> T2, zero row, x-border lane masks, residual picked out of the x
// chunks, shift and residual MFMAs, relu_acc16 epilogues, whole-line stores.  Every accumulator sees the same MFMAs on the same fp16
// operands in the same order as in the ring kernel: the two forms are bit-identical.
// LDS (160 KiB): [0, 96 K) x-chunk buffers / [0, 64 K) T1 / [0, 48 K) T2, staging tile 0 at 48 K (phase 3), zero row at 97 K, scratch
// of the L2 touch at 100 K, staging tile 1 at 112 K.
// Registers decide the shape (residual 64 MT2, phase 1's accumulators 32 MT1, 32 per weight slot, 8 MT1 for the x fragments):
//   <4, 3, NS = 2>  504 registers, 160 KiB of LDS, scratch 0.  NS = 3 spills (512 registers + 180 B of scratch; 132 B with the shift pairs
//                   of epilogues 1 .. 5 loaded behind phase 1 as they are now; the same 132 B with phase 1's x fragments single-buffered),
//                   so the large strips prefetch ONE step ahead: a step is 768-1024 MFMA cycles, an L2 hit ~500.
//   <3, 2, NS = 3>  422 registers, 160 KiB of LDS, scratch 0.
template <int MT1, int MT2, int NS>
__global__ __launch_bounds__(256, 1) void bottleneck_stream_direct128_kernel(const BnsParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int P = 128;
  using G = BnsGeom<P>;
  constexpr int NCT = G::NCT, WCOLS = G::WCOLS, WPG = G::WPG, NC1 = G::NC1, KC = G::KC, WSTEP = G::WSTEP, ROWB = G::ROWB;
  constexpr int G2 = G::G2, G3 = G::G3, GEND = G::GEND;
  constexpr int XROWS = WPG * MT1 * 32, LX = WPG * MT1;     // rows of an x chunk buffer; 1-KiB x loads per wave per chunk
  constexpr int NOUT = WPG * MT2 * 32;                       // output pixels of the strip (padded)
  constexpr int STG0 = G::STG, STG1 = G::WBASE, STGB = NOUT * ROWB, SCR = 102400;
  static_assert(XROWS * 128 <= G::XSTRIDE && XROWS * ROWB <= G::TAB && STGB <= STG0 && STG0 + STGB <= G::TAB, "LDS map: T1, T2, staging tile 0");
  static_assert(SCR >= G::ZROW + ROWB && SCR + 1024 <= STG1 && STG1 + STGB <= G::LDS_BYTES, "LDS map: scratch, staging tile 1");
  static_assert(NS >= 2 && (3 * KC) % NS == 0, "ring phase of the unrolled phase-2 body");
  constexpr int D = NS - 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using c0 = std::integral_constant<int, 0>;
  using c1 = std::integral_constant<int, 1>;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wcol = wave % WCOLS, pg = wave / WCOLS;
  const int l31 = lane & 31, lhi = lane >> 5;

  const int logical = xcd_logical_wg(p.total);
  const int n = logical / p.ppi;
  const int y0 = (logical - n * p.ppi) * p.TH;
  const int W = p.W;
  const int rows_out = p.H - y0 < p.TH ? p.H - y0 : p.TH;
  const int npix_out = rows_out * W;
  const int npix_halo = (p.TH + 2) * W;

  const __amdgpu_buffer_rsrc_t rsrc_x = bns_rsrc(p.x, p.x_bytes), rsrc_y = bns_rsrc(p.y, p.y_bytes), rsrc_w = bns_rsrc(p.ws, p.ws_bytes);
  const __amdgpu_buffer_rsrc_t rsrc_t = bns_rsrc(p.tab, (2 * P + G::C) * 4);
  constexpr unsigned kOOB = 0x80000000u;

  // x chunk: row = halo pixel, 128 bytes (64 channels); see the ring kernel
  unsigned x_voff[LX];
#pragma unroll
  for (int t = 0; t < LX; ++t) {
    const int hp = (t * 4 + wave) * 8 + (lane >> 3);
    const int hr = hp / W, hc = hp - hr * W;
    const int iy = y0 - 1 + hr;
    unsigned v = kOOB;
    if (hp < npix_halo && (unsigned)iy < (unsigned)p.H)
      v = (unsigned)((((n * p.H + iy) * W + hc) * p.x_cstride + p.x_coff) * 2 + (((lane & 7) ^ BNS_XKEY(hp)) << 4));
    x_voff[t] = v;
  }
  const unsigned lane16 = (unsigned)lane * 16u;
  auto issue_x = [&](int c, int buf) { bns_issue_x<4>(rsrc_x, smem + buf * G::XSTRIDE, wave, x_voff, c); };
  // the weight fragments of step g for this wave: (kk, tile 2*wcol + i) at g * WSTEP + (kk * NCT + 2*wcol + i) KiB; both pixel groups of a
  // wave column load the same ones.  Steps past the end of the stream: out of range by the lane offset, zeros, never multiplied.
  uint4_t areg[NS][4][2];
  auto load_a_half = [&](auto slotc, int g, auto halfc) {   // K16 slices {0, 1} or {2, 3} of the step
    constexpr int SL = decltype(slotc)::value, HF = decltype(halfc)::value;
    const unsigned vo = g < GEND ? lane16 : kOOB;
#pragma unroll
    for (int kk = 2 * HF; kk < 2 * HF + 2; ++kk)
#pragma unroll
      for (int i = 0; i < 2; ++i)
        areg[SL][kk][i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, vo, g * WSTEP + (kk * NCT + 2 * wcol + i) * 1024, 0);
  };
  auto load_a = [&](auto slotc, int g) {
    load_a_half(slotc, g, c0{});
    load_a_half(slotc, g, c1{});
  };
  unsigned long long ts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  BNS_TS(0);
  // the first round of workgroups on an XCD pulls the block's weight stream into that XCD's L2 (see the direct kernel): EXACTLY kTouch
  // loads per thread, issued behind x chunk 0 and the weights of step 0 and counted by the first hand-counted wait
  constexpr int kTouch = 6;
  auto issue_touch = [&]() {
    const bool on = blockIdx.x < 256 && !(p.dbg & 512);
    const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    const int first = p.total < 256 ? p.total : 256;
    const int nloc = (first - xcd + 7) >> 3;
    const unsigned lines = (p.ws_bytes + 127u) >> 7;
    const unsigned per = (lines + nloc - 1) / nloc;
    const unsigned lo = loc * per, hi = lo + per < lines ? lo + per : lines;
#pragma unroll
    for (int k = 0; k < kTouch; ++k) {
      const unsigned l = lo + tid + 256u * k;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (lds_ptr)(smem + SCR + wave * 256), 4, (on && l < hi) ? l << 7 : kOOB, 0, 0, 0);
    }
  };
  // folded operands: the shift pair of MFMA row l31 of every (epilogue, channel tile) of this wave and the residual's 0/1 matrix (see
  // the direct kernel)
  unsigned shp[6][2];
  uint4_t permA[2];
  const uint4_t onesB = uint4_t{0x3C003C00u, 0u, 0u, 0u};
  {
    const int sg = bns_sigma(l31);
    const bool on = lhi == (sg >> 4);
    const int ph = (sg >> 3) & 1, pe = sg & 7;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      unsigned w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = (on && ph == hh && (pe >> 1) == k) ? (0x3C00u << (16 * (pe & 1))) : 0u;
      permA[hh] = uint4_t{w[0], w[1], w[2], w[3]};
    }
  }
  // (the pairs of epilogue 0 in the prologue, those of epilogues 1 .. 5 behind phase 1's loop, where the registers are free again)
  constexpr int kTabLoads = 2;
  auto load_shp = [&](int e0, int e1) { bns_load_shp<P>(shp, rsrc_t, l31, lhi, 2 * wcol, e0, e1); };
  // order of every wave's (in-order) load queue: x chunk 0, the weights of step 0, the L2 touch, the shift pairs, x chunk 1, the weights
  // of steps 1 .. D-1, x chunk 2 (the order of the steady state: weights of step c+1 between x chunks c+1 and c+2).  The first wait
  // counts them: compiler fences on both sides of the touch / shift group.
  issue_x(0, 0);
  load_a(c0{}, 0);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  issue_touch();
  load_shp(0, 1);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  issue_x(1, 1);
  bns_unroll<D - 1>([&](auto sc) { load_a(std::integral_constant<int, decltype(sc)::value + 1>{}, decltype(sc)::value + 1); });
  issue_x(2, 2);
  if (tid < ROWB / 16) *reinterpret_cast<uint4_t*>(smem + G::ZROW + tid * 16) = uint4_t{0u, 0u, 0u, 0u};

  // residual = the block input at the strip's own pixels, in phase 3's accumulator layout: [quarter][tile i][pixel tile j][half]
  uint4_t res[4][2][MT2][2];
  int m_out[MT2];       // output pixel (strip-relative, row-major at width W) of this lane per pixel tile
#pragma unroll
  for (int j = 0; j < MT2; ++j) m_out[j] = (pg * MT2 + j) * 32 + l31;

  // ================= phase 1: t1 = relu(W1' . x + shift1) on the halo strip ===========================================================
  float16_t acc1[2][MT1];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < MT1; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[i][j][r] = 0.f;
  int b1_off[MT1];
#pragma unroll
  for (int j = 0; j < MT1; ++j) {
    const int hp = (pg * MT1 + j) * 32 + l31;
    b1_off[j] = hp * 128 + ((lhi ^ BNS_XKEY(hp)) << 4);
  }
  {
    uint4_t fx[2][MT1];
    auto ldx = [&](auto setc, int buf, int kk) {
      constexpr int S = decltype(setc)::value;
      const char* xb = smem + buf * G::XSTRIDE;
#pragma unroll
      for (int j = 0; j < MT1; ++j) fx[S][j] = *reinterpret_cast<const uint4_t*>(xb + (b1_off[j] ^ (kk << 5)));
    };
    auto mma1 = [&](auto setc, auto slotc, auto kkc) {
      constexpr int S = decltype(setc)::value, SL = decltype(slotc)::value, kk = decltype(kkc)::value;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < MT1; ++j)
          acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, areg[SL][kk][i]),
                                                              __builtin_bit_cast(half8_t, fx[S][j]), acc1[i][j], 0, 0, 0);
    };
    // x chunk 0 has landed (this wave's share): behind it the weights of steps 0 .. D-1 (8 loads each), the touch, the shift pairs and
    // x chunks 1 and 2 may fly
    static_assert(2 * LX + 8 * D + kTouch + kTabLoads <= 63, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * LX + 8 * D + kTouch + kTabLoads) : "memory");
    BNS_BARRIER();
    BNS_TS(7);             // start-up: x chunk 0 of every wave has landed
    ldx(c0{}, 0, 0);
    bns_unroll<NC1>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      constexpr int buf = c % 3;
      using slot = std::integral_constant<int, c % NS>;
      // two scheduling regions per chunk (the wave-uniform branch of the residual pick-up splits it), each with half of the step's
      // weight loads and the direct kernel's pinned issue order: one vector-memory load and the LDS reads behind every two MFMAs
      load_a_half(std::integral_constant<int, (c + D) % NS>{}, c + D, c0{});
      ldx(c1{}, buf, 1);
      mma1(c0{}, slot{}, std::integral_constant<int, 0>{});
      ldx(c0{}, buf, 2);
      __builtin_amdgcn_sched_group_barrier(0x020, LX, 0);
      bns_unroll<3>([&](auto) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, (2 * MT1 + 2) / 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      });
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, (MT1 + 2) / 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      bns_unroll<MT1 - 1>([&](auto) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, (MT1 + 2) / 3, 0);
      });
      if (c % WCOLS == wcol) {       // this chunk holds the channels of this wave column for quarter c / WCOLS
        constexpr int q = c / WCOLS;
        const char* xb = smem + buf * G::XSTRIDE;
#pragma unroll
        for (int j = 0; j < MT2; ++j) {
          const int hp = m_out[j] + W;
          const char* rowp = xb + hp * 128;
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h)
              res[q][i][j][h] = *reinterpret_cast<const uint4_t*>(rowp + (((4 * i + 2 * lhi + h) ^ BNS_XKEY(hp)) << 4));
        }
      }
      mma1(c1{}, slot{}, std::integral_constant<int, 1>{});
      load_a_half(std::integral_constant<int, (c + D) % NS>{}, c + D, c1{});
      ldx(c1{}, buf, 3);
      mma1(c0{}, slot{}, std::integral_constant<int, 2>{});
      bns_unroll<MT1>([&](auto) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      });
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 4 - MT1 > 0 ? 4 - MT1 : 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4 * MT1 - 2 * MT1 - 2, 0);
      if constexpr (c + 1 < NC1) {
        // x chunk c+1 has landed and every read of chunk c's buffer is complete: refill it with chunk c+3.  Younger than x chunk c+1 are the weights of step c+1 (D = 2: needed next anyway, waited for), x
        // chunk c+2 and the weights of step c+D (8 loads); with D = 3 the weights of step c+2 sit in between and stay in flight too.
        if constexpr (c + 2 < NC1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LX + (D <= 2 ? 8 : 16)) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(D <= 2 ? 8 : 16) : "memory");
        BNS_BARRIER();
        if constexpr (c + 3 < NC1) issue_x(c + 3, buf);
        ldx(c0{}, (c + 1) % 3, 0);
      }
      mma1(c1{}, slot{}, std::integral_constant<int, 3>{});
    });
  }
  BNS_TS(1);
  load_shp(1, 6);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();          // every wave is past its last x-chunk read: the x buffers become T1
  {
    bns_add_shift(acc1, shp[0]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < MT1; ++j) {
        const int hp = (pg * MT1 + j) * 32 + l31;
        const int hr = hp / W;
        const int iy = y0 - 1 + hr;
        const bool inside = (unsigned)iy < (unsigned)p.H;     // out-of-image halo rows are conv2's zero padding
        half8_t h8[2];
        relu_acc16(acc1[i][j], h8);
#pragma unroll
        for (int h = 0; h < 2; ++h) h8[h] = bns_keep_if(h8[h], inside);
        if (hp < npix_halo) {
          char* rowp = smem + hp * ROWB;
          const int cb = (2 * wcol + i) * 4 + 2 * lhi;
#pragma unroll
          for (int h = 0; h < 2; ++h)
            *reinterpret_cast<half8_t*>(rowp + (((cb + h) ^ (hp & 15)) << 4)) = h8[h];
        }
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();          // T1 complete
  BNS_TS(2);

  // ================= phases 2 + 3: weight steps G2 .. GEND-1, pixel operand from T1 / T2 ==============================================
  float16_t acc[2][MT2];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < MT2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  };
  zero_acc();
  // x-border flags of this lane's output pixels: bit 0 = first column (tap kx = 0 is padding), bit 1 = last column
  int edge[MT2];
#pragma unroll
  for (int j = 0; j < MT2; ++j) edge[j] = bns_edge(m_out[j] % W, W);
  auto row_bases = [&](int off, int kc, int bad, int (&rb)[MT2]) {
#pragma unroll
    for (int j = 0; j < MT2; ++j) {
      const int row = m_out[j] + off;
      const int v = row * ROWB + (((row & 15) ^ lhi) << 4);
      rb[j] = ((edge[j] & bad) ? G::ZROW + (lhi << 4) : v) ^ (kc << 7);
    }
  };
  uint4_t fb[2][MT2];
  auto ldb = [&](auto setc, int kk, const int (&rb)[MT2]) {
    constexpr int S = decltype(setc)::value;
#pragma unroll
    for (int j = 0; j < MT2; ++j) fb[S][j] = *reinterpret_cast<const uint4_t*>(smem + (rb[j] ^ (kk << 5)));
  };
  auto mma2 = [&](auto setc, auto slotc, auto kkc) {
    constexpr int S = decltype(setc)::value, SL = decltype(slotc)::value, kk = decltype(kkc)::value;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < MT2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, areg[SL][kk][i]),
                                                           __builtin_bit_cast(half8_t, fb[S][j]), acc[i][j], 0, 0, 0);
  };
  // one weight step g (register slot SL = g % NS): slice 0 of the pixel operand already sits in register set 0; `rbn` = row bases of
  // the next step.  Issue order as in the direct kernel: one weight load and the pixel-operand reads after every MT2 MFMAs.
  auto dstep = [&](auto slotc, int g, const int (&rb)[MT2], bool has_next, const int (&rbn)[MT2]) {
    constexpr int SL = decltype(slotc)::value;
    using slot = std::integral_constant<int, SL>;
    load_a(std::integral_constant<int, (SL + D) % NS>{}, g + D);
    ldb(c1{}, 1, rb);
    mma2(c0{}, slot{}, std::integral_constant<int, 0>{});
    ldb(c0{}, 2, rb);
    mma2(c1{}, slot{}, std::integral_constant<int, 1>{});
    ldb(c1{}, 3, rb);
    mma2(c0{}, slot{}, std::integral_constant<int, 2>{});
    if (has_next) ldb(c0{}, 0, rbn);
    mma2(c1{}, slot{}, std::integral_constant<int, 3>{});
    bns_unroll<8>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      __builtin_amdgcn_sched_group_barrier(0x008, MT2, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, (i & 1) ? (MT2 + 1) / 2 : MT2 / 2, 0);
    });
  };

  // ---- phase 2: nine taps x KC chunks, three taps per loop trip (6 steps: a multiple of the register ring period) --------------------
  {
    int rb[MT2], rbn[MT2];
    row_bases(-1, 0, 1, rb);                         // tap (0, 0), chunk 0
    ldb(c0{}, 0, rb);
    for (int ky = 0; ky < 3; ++ky) {
      bns_unroll<3 * KC>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        constexpr int kx = s / KC, kc = s % KC;
        constexpr int nkc = (kc + 1) % KC, nkx = kc + 1 == KC ? (kx + 1) % 3 : kx;
        const int nky = (kc + 1 == KC && kx == 2) ? ky + 1 : ky;
        row_bases(nky * W + nkx - 1, nkc, nkx == 0 ? 1 : (nkx == 2 ? 2 : 0), rbn);
        dstep(std::integral_constant<int, (G2 + s) % NS>{}, G2 + 3 * KC * ky + s, rb, !(ky == 2 && s == 3 * KC - 1), rbn);
#pragma unroll
        for (int j = 0; j < MT2; ++j) rb[j] = rbn[j];
      });
    }
  }
  BNS_TS(3);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();          // every wave is past its last T1 read: T2 overwrites T1
  {
    bns_add_shift(acc, shp[1]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < MT2; ++j) {
        const int m = m_out[j];
        half8_t h8[2];
        relu_acc16(acc[i][j], h8);
        char* rowp = smem + m * ROWB;
        const int cb = (2 * wcol + i) * 4 + 2 * lhi;
#pragma unroll
        for (int h = 0; h < 2; ++h) *reinterpret_cast<half8_t*>(rowp + (((cb + h) ^ (m & 15)) << 4)) = h8[h];
      }
    }
  }
  zero_acc();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNS_BARRIER();          // T2 complete
  BNS_TS(4);

  // ---- phase 3: four quarters of P output channels, K = P; the tile of a quarter leaves through one of two LDS staging tiles ---------
  {
    // read-out: thread -> 16-byte chunk tid % 16 of the whole 256-byte lines of pixels tid / 16 + 16 k (the row key m & 15 is the same
    // for every k, so the LDS offsets and the output offsets are one base each plus a constant / wave-uniform step)
    constexpr int CPR = ROWB / 16, NSTG = NOUT * CPR / 256;
    static_assert(CPR == 16, "read-out map");
    const int m0 = tid >> 4, sch = tid & 15;
    const unsigned y_base = (unsigned)((((n * p.H + y0) * W + m0) * p.y_cstride + p.y_coff + sch * 8) * 2);
    const unsigned y_step = (unsigned)(16 * p.y_cstride * 2);
    const int s_off0 = m0 * ROWB + ((sch ^ (m0 & 15)) << 4);
    int rb[MT2], rbn[MT2];
    row_bases(0, 0, 0, rb);
    ldb(c0{}, 0, rb);
    bns_unroll<4>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      bns_unroll<KC>([&](auto kcc) {
        constexpr int kc = decltype(kcc)::value;
        constexpr int g = G3 + q * KC + kc;
        row_bases(0, (kc + 1) % KC, 0, rbn);
        dstep(std::integral_constant<int, g % NS>{}, g, rb, g + 1 < GEND, rbn);
#pragma unroll
        for (int j = 0; j < MT2; ++j) rb[j] = rbn[j];
      });
      char* stg = smem + ((q & 1) ? STG1 : STG0);
      // shift3 of the quarter and the residual join the accumulators as three MFMAs per tile
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < MT2; ++j) bns_fold_tail(acc[i][j], shp[2 + q][i], onesB, permA, res[q][i][j]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < MT2; ++j) {
          half8_t o8[2];
          relu_acc16(acc[i][j], o8);
          const int m = m_out[j];
#pragma unroll
          for (int h = 0; h < 2; ++h)
            *reinterpret_cast<half8_t*>(stg + m * ROWB + ((((2 * wcol + i) * 4 + 2 * lhi + h) ^ (m & 15)) << 4)) = o8[h];
        }
      zero_acc();
      // the two staging tiles alternate: the readers of this tile's previous content (quarter q-2) passed the barrier of quarter q-1
      // with their LDS reads complete, so ONE barrier per quarter (tile complete) is all the hand-over needs
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      BNS_BARRIER();
#pragma unroll
      for (int k = 0; k < NSTG; ++k) {
        const uint4_t v = *reinterpret_cast<const uint4_t*>(stg + s_off0 + k * 16 * ROWB);
        const unsigned vo = m0 + 16 * k < npix_out ? y_base + (unsigned)k * y_step + (unsigned)(q * P * 2) : kOOB;
        if (!(p.dbg & 4)) __builtin_amdgcn_raw_buffer_store_b128(v, rsrc_y, vo, 0, FT_YSTORE_BUF_AUX);
      }
    });
  }
  BNS_TS_TAIL();
#endif
}

// ---- weight stream packing -------------------------------------------------------------------------------------------
// w1 [P][C], w2 [P][9P] (k = tap * P + ci), w3 [C][P]: the K-major layouts of ft_conv_pack_geometry.  One thread per
// 16-byte piece of the stream: step g, slice kk, channel tile i, lane -> 8 consecutive k of one output channel.
template <int P>
__global__ __launch_bounds__(256) void bns_pack_kernel(const half_t* __restrict__ w1, const half_t* __restrict__ w2,
                                                       const half_t* __restrict__ w3, uint4_t* __restrict__ out) {
  using G = BnsGeom<P>;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= G::GEND * G::WSTEP / 16) return;
  const int lane = idx & 63, frag = idx >> 6;
  const int per_step = 4 * G::NCT;
  const int g = frag / per_step, f = frag - g * per_step;
  const int kk = f / G::NCT, i = f - kk * G::NCT;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int co_t = 32 * i + bns_sigma(l31);
  const int k_t = 16 * kk + 8 * lhi;
  const half_t* src;
  if (g < G::G2) {
    src = w1 + (size_t)co_t * G::C + 64 * g + k_t;
  } else if (g < G::G3) {
    const int s = g - G::G2, tap = s / G::KC, kc = s - tap * G::KC;
    src = w2 + (size_t)co_t * (9 * P) + tap * P + 64 * kc + k_t;
  } else {
    const int s = g - G::G3, q = s / G::KC, kc = s - q * G::KC;
    src = w3 + (size_t)(q * P + co_t) * P + 64 * kc + k_t;
  }
  out[idx] = *reinterpret_cast<const uint4_t*>(src);
}

// The stream of bottleneck_stream_tile16_kernel (P = 256, layout 1): same steps of 64 k, a step = two K32 slices x sixteen 16-channel
// tiles x 1 KiB; lane l of a fragment holds row l & 15, k = 8 (l >> 4) .. + 7 of the slice, row r of tile t = channel
// 64 (t >> 2) + 16 (r >> 2) + 4 (t & 3) + (r & 3).  A wave's four tiles of a slice are 4 contiguous KiB.
__global__ __launch_bounds__(256) void bns_pack16_kernel(const half_t* __restrict__ w1, const half_t* __restrict__ w2,
                                                         const half_t* __restrict__ w3, uint4_t* __restrict__ out) {
  using G = BnsGeom<256>;
  constexpr int P = 256;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= G::GEND * G::WSTEP / 16) return;
  const int lane = idx & 63, frag = idx >> 6;
  const int g = frag >> 5, f = frag & 31;
  const int ks = f >> 4, t = f & 15;
  const int r = lane & 15;
  const int co_t = 64 * (t >> 2) + 16 * (r >> 2) + 4 * (t & 3) + (r & 3);
  const int k_t = 32 * ks + 8 * (lane >> 4);
  const half_t* src;
  if (g < G::G2) {
    src = w1 + (size_t)co_t * G::C + 64 * g + k_t;
  } else if (g < G::G3) {
    const int s = g - G::G2, tap = s / G::KC, kc = s - tap * G::KC;
    src = w2 + (size_t)co_t * (9 * P) + tap * P + 64 * kc + k_t;
  } else {
    const int s = g - G::G3, q = s / G::KC, kc = s - q * G::KC;
    src = w3 + (size_t)(q * P + co_t) * P + 64 * kc + k_t;
  }
  out[idx] = *reinterpret_cast<const uint4_t*>(src);
}

// the head form's stream (P = 256): NC1 = C / 64 steps of w1 [P][C], then nine taps x KC steps of w2; same piece order
__global__ __launch_bounds__(256) void bns_pack_head_kernel(const half_t* __restrict__ w1, const half_t* __restrict__ w2,
                                                            uint4_t* __restrict__ out, int C) {
  using G = BnsGeom<256>;
  const int nc1 = C / 64, gend = nc1 + 9 * G::KC;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= gend * G::WSTEP / 16) return;
  const int lane = idx & 63, frag = idx >> 6;
  const int per_step = 4 * G::NCT;
  const int g = frag / per_step, f = frag - g * per_step;
  const int kk = f / G::NCT, i = f - kk * G::NCT;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int co_t = 32 * i + bns_sigma(l31);
  const int k_t = 16 * kk + 8 * lhi;
  const half_t* src;
  if (g < nc1) {
    src = w1 + (size_t)co_t * C + 64 * g + k_t;
  } else {
    const int sft = g - nc1, tap = sft / G::KC, kc = sft - tap * G::KC;
    src = w2 + (size_t)co_t * (9 * 256) + tap * 256 + 64 * kc + k_t;
  }
  out[idx] = *reinterpret_cast<const uint4_t*>(src);
}

// The forms a plan can take.  The integers are what ft_bottleneck_stream_variant returns and what FT_BNS_VARIANT forces: they stay.
enum BnsVariant {
  BNS_RING128_LARGE = 0,    // bottleneck_stream_kernel<128, 4, 3>
  BNS_RING256 = 1,          // bottleneck_stream_kernel<256, 4, 3>
  BNS_DIRECT256 = 2,        // bottleneck_stream_direct_kernel<3, 2>: 64-pixel strips, weights straight to registers
  BNS_DIRECT256_XSPLIT = 3, // bottleneck_stream_direct_kernel<2, 1, XH>: column-split
  BNS_HEAD = 4,             // bottleneck_stream_direct_kernel<4, 1, HEADC = 8>: stride-2 head of an entry block (its own stream, no folding)
  BNS_RING128_SMALL = 5,    // bottleneck_stream_kernel<128, 3, 2>
  BNS_TILE16 = 6,           // bottleneck_stream_tile16_kernel: 256 planes on 16-pixel tiles (its own stream layout)
  BNS_DIRECT128_LARGE = 7,  // bottleneck_stream_direct128_kernel<4, 3>
  BNS_DIRECT128_SMALL = 8,  // bottleneck_stream_direct128_kernel<3, 2>
};

struct BnsPlan {
  int variant;   // BnsVariant
  int TH, ppi;
  int TWc, csplit;
};

// the rule's choice at 128 planes, per strip size: 1 = bottleneck_stream_direct128_kernel for folded descriptors.  Measured in situ
// (profiles/HISTORY.md): large strips, R50 batch 64: 42.2 -> 38.0 us per block, +1.35 % on the step; small strips, R101 384x288 at 16
// crops: +0.4 % on the step
#ifndef FT_BNS_DIRECT128_LARGE
#define FT_BNS_DIRECT128_LARGE 1
#endif
#ifndef FT_BNS_DIRECT128_SMALL
#define FT_BNS_DIRECT128_SMALL 1
#endif

static int bns_plan(const ft_bottleneck_desc* d, BnsPlan* out) {
  if (!d) return FT_ERR_INVALID_ARG;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0) return FT_ERR_INVALID_ARG;
  if (d->head_only) {
    // conv1 + conv2 / stride 2 of a 256-plane entry block (layer3.0): 512 input channels, even map, <= 120 T1 rows per strip
    if (d->dtype != FT_F16 || d->projection || d->P != 256 || d->C != 512 || d->stride != 2 || (d->H & 1) || (d->W & 1)) return FT_ERR_UNSUPPORTED;
    if (d->x_coff < 0 || d->y_coff < 0 || d->x_coff % 8 || d->y_coff % 8 || d->x_cstride % 8 || d->y_cstride % 8) return FT_ERR_UNSUPPORTED;
    const int Ho = d->H / 2, Wo = d->W / 2;
    if (d->x_cstride < d->x_coff + d->C || d->y_cstride < d->y_coff + d->P) return FT_ERR_INVALID_ARG;
    if ((long long)d->N * d->H * d->W * d->x_cstride * 2 >= (1LL << 31) || (long long)d->N * Ho * Wo * d->y_cstride * 2 >= (1LL << 31))
      return FT_ERR_UNSUPPORTED;
    int th = (120 / d->W - 1) / 2;
    const int th2 = 32 / Wo;
    th = th < th2 ? th : th2;
    if (th < 1) return FT_ERR_UNSUPPORTED;
    th = th < Ho ? th : Ho;
    th = ceil_div(Ho, ceil_div(Ho, th));
    *out = BnsPlan{BNS_HEAD, th, ceil_div(Ho, th), d->W, 1};
    return FT_OK;
  }
  if (d->dtype != FT_F16 || d->projection || (d->P != 128 && d->P != 256) || d->C != 4 * d->P || d->stride > 1) return FT_ERR_UNSUPPORTED;
  if (d->x_coff < 0 || d->y_coff < 0 || d->x_coff % 8 || d->y_coff % 8 || d->x_cstride % 8 || d->y_cstride % 8) return FT_ERR_UNSUPPORTED;
  if (d->x_cstride < d->x_coff + d->C || d->y_cstride < d->y_coff + d->C) return FT_ERR_INVALID_ARG;
  if ((long long)d->N * d->H * d->W * d->x_cstride * 2 >= (1LL << 31) || (long long)d->N * d->H * d->W * d->y_cstride * 2 >= (1LL << 31))
    return FT_ERR_UNSUPPORTED;
  auto rows = [&](int outcap, int halocap) {
    int th = outcap / d->W;
    const int th2 = halocap / d->W - 2;
    th = th < th2 ? th : th2;
    if (th < 1) return 0;
    th = th < d->H ? th : d->H;
    return ceil_div(d->H, ceil_div(d->H, th));     // same strip count, balanced rows
  };
  const int force = dev_env_int("FT_BNS_VARIANT", -1);   // dev / tests: 1, 2, 3 or 6 (read per call)
  if (d->P == 128) {
    // strips of <= 192 output pixels on <= 256 halo pixels (<128, 4, 3>), or of <= 128 on <= 192 (<128, 3, 2>, round 4) where the
    // large strips leave CUs idle: ResNet-101 at 384 x 288 with 16 crops per GPU has 160 large strips for 256 CUs (48 x 36 maps,
    // 5 rows each) and exactly 256 small ones (3 rows).  Cost = rounds of 256 workgroups x MFMAs per wave: 32 K16 steps of conv1
    // on MT1 halo tiles + (72 + 32) steps on MT2 output tiles, per pair of channel tiles.
    const int th_b = rows(192, 256), th_s = rows(128, 192);
    if (th_b < 1 && th_s < 1) return FT_ERR_UNSUPPORTED;
    // dev / tests (read per call): 1 ring kernel on large strips, 2 ring on small, 3 direct kernel on large, 4 direct on small
    const int force128 = dev_env_int("FT_BNS_VARIANT128", 0);
    auto cost = [&](int th, int mt1, int mt2) {
      const long long wg = (long long)d->N * ceil_div(d->H, th);
      return ((wg + 255) / 256) * (long long)(32 * mt1 + 104 * mt2);
    };
    bool small = th_b < 1 || (th_s >= 1 && cost(th_s, 3, 2) < cost(th_b, 4, 3));
    if ((force128 == 1 || force128 == 3) && th_b >= 1) small = false;
    if ((force128 == 2 || force128 == 4) && th_s >= 1) small = true;
    // the direct form (folded fp16 operands only; table-form descriptors keep the ring kernels) where it was measured faster in situ
    bool direct = d->folded && (small ? FT_BNS_DIRECT128_SMALL : FT_BNS_DIRECT128_LARGE);
    if (force128 == 1 || force128 == 2) direct = false;
    if (force128 == 3 || force128 == 4) direct = d->folded != 0;
    const int th = small ? th_s : th_b;
    *out = BnsPlan{direct ? (small ? BNS_DIRECT128_SMALL : BNS_DIRECT128_LARGE) : (small ? BNS_RING128_SMALL : BNS_RING128_LARGE), th, ceil_div(d->H, th), d->W, 1};
    return FT_OK;
  }
  const int th_big = rows(96, 120), th_small = rows(64, 96);
  // column-split form: <= 32 output pixels on a <= 64-pixel patch with its own x-halo; the fewest parts that fit
  int xs = 0, x_tw = 0, x_th = 0;
  for (int cs = 2; cs <= 4 && !xs; ++cs) {
    const int tw = ceil_div(d->W, cs);
    int th = 32 / tw;
    const int th2 = 64 / (tw + 2) - 2;
    th = th < th2 ? th : th2;
    if (th < 1 || tw * (cs - 1) >= d->W) continue;
    th = th < d->H ? th : d->H;
    xs = cs; x_tw = tw; x_th = ceil_div(d->H, ceil_div(d->H, th));
  }
  if (th_big < 1 && th_small < 1 && !xs) return FT_ERR_UNSUPPORTED;
  // 16-pixel tiles: <= 48 output pixels on <= 80 halo pixels; folded operands and four waves only
  const int th_16 = d->folded ? rows(48, 80) : 0;
  int pick;
  if (force == BNS_RING256 || force == BNS_DIRECT256 || (force == BNS_DIRECT256_XSPLIT && xs) || (force == BNS_TILE16 && th_16 >= 1)) pick = force;
  else {
    // Both variants run one workgroup per CU at the matrix pipe's pace (the FT_BNS_DBG=64/128 ablation: same phase times
    // with every load out of range), so the cost of a launch is rounds of 256 workgroups x MFMAs per workgroup:
    // 64 K-steps on MT1 halo tiles + (144 + 64) K-steps on MT2 output tiles, per wave and pair of channel tiles.
    auto cost = [&](int th, int mt1, int mt2) {
      const long long wg = (long long)d->N * ceil_div(d->H, th);
      return ((wg + 255) / 256) * (long long)(64 * mt1 + 208 * mt2);
    };
    if (th_big < 1) pick = BNS_DIRECT256;
    else if (th_small < 1) pick = BNS_RING256;
    else pick = cost(th_big, 4, 3) <= cost(th_small, 3, 2) ? BNS_RING256 : BNS_DIRECT256;
    if (pick == BNS_RING256 && th_big < 1) pick = BNS_DIRECT256;
    if (pick == BNS_DIRECT256 && th_small < 1) pick = th_big >= 1 ? BNS_RING256 : BNS_DIRECT256_XSPLIT;
    long long cf = pick == BNS_RING256 ? cost(th_big, 4, 3) : (pick == BNS_DIRECT256 ? cost(th_small, 3, 2) : -1);
    // the 16-pixel tiles in the same unit (one 32-pixel tile of a pair of channel tiles for a K16 step = 64 MFMA cycles = two 16-pixel
    // tiles of four channel tiles for half a K32 step): 5 halo and 3 output tiles count as 2.5 and 1.5.  Not under FT_BNS_WAVES=8
    // (the eight-wave forms are 32-pixel kernels).
    if (th_16 >= 1 && dev_env_int("FT_BNS_WAVES", 4) != 8) {
      const long long wg = (long long)d->N * ceil_div(d->H, th_16);
      const long long c16 = ((wg + 255) / 256) * (long long)(32 * 5 + 104 * 3);
      if (cf < 0 || c16 < cf) { pick = BNS_TILE16; cf = c16; }
    }
    if (xs && pick != BNS_DIRECT256_XSPLIT) {
      // the column-split form only where it needs no more rounds of 256 workgroups than it saves in work per workgroup
      const long long wgx = (long long)d->N * ceil_div(d->H, x_th) * xs;
      const long long cx = ((wgx + 255) / 256) * (long long)(64 * 2 + 208 * 1);
      if (cx < cf) pick = BNS_DIRECT256_XSPLIT;
    }
  }
  if (pick == BNS_TILE16) {
    *out = BnsPlan{BNS_TILE16, th_16, ceil_div(d->H, th_16), d->W, 1};
    return FT_OK;
  }
  if (pick == BNS_RING256 && th_big < 1) pick = BNS_DIRECT256;
  if (pick == BNS_DIRECT256 && th_small < 1) pick = th_big >= 1 ? BNS_RING256 : BNS_DIRECT256_XSPLIT;
  if (pick == BNS_DIRECT256_XSPLIT) {
    *out = BnsPlan{BNS_DIRECT256_XSPLIT, x_th, ceil_div(d->H, x_th) * xs, x_tw, xs};
    return FT_OK;
  }
  const int th = pick == BNS_RING256 ? th_big : th_small;
  *out = BnsPlan{pick, th, ceil_div(d->H, th), d->W, 1};
  return FT_OK;
}

// One launch of a stream kernel, one workgroup per strip.  The kernel is a template argument: the LDS opt-in of FT_RAISE_LDS is kept
// per kernel (and per device).
template <void (*kernel)(BnsParams)>
static int bns_run(int threads, int lds, const char* name, const BnsParams& p, hipStream_t s) {
  FT_RAISE_LDS(kernel, lds);
  hipLaunchKernelGGL(kernel, dim3(p.total), dim3(threads), lds, s, p);
  FT_LAUNCH_CHECK(name);
  return FT_OK;
}

template <int P, int MT1, int MT2, bool FOLD = false>
static int bns_launch(const BnsParams& p, hipStream_t s) {
  return bns_run<bottleneck_stream_kernel<P, MT1, MT2, FOLD>>(256, BnsGeom<P>::LDS_BYTES, "bottleneck_stream_kernel", p, s);
}

#ifndef FT_BNS_SLOTS
#define FT_BNS_SLOTS 4        // weight-step register slots of the full-width strips: 3 -> 4 = +0.9-1.2 % on the R50 batch-64 step (56.25 / 56.34 -> 56.74 / 57.01 k crops/s same box), 6: -4.5 %; the column-split form: no difference at 3 / 4 / 6 (tools/dev/ab/ns_ab.sh)
#endif
#ifndef FT_BNS_XH_SLOTS
#define FT_BNS_XH_SLOTS 3
#endif
template <int MT1, int MT2, bool XH, int HEADC = 0, int NW = 4, bool FOLD = false>
static int bns_launch_direct(const BnsParams& p, hipStream_t s) {
  return bns_run<bottleneck_stream_direct_kernel<MT1, MT2, XH, XH ? FT_BNS_XH_SLOTS : FT_BNS_SLOTS, HEADC, NW, FOLD>>(
      64 * NW, 81920 + 2 * MT2 * 32 * 512, "bottleneck_stream_direct_kernel", p, s);
}

#ifndef FT_BNS_SLOTS128
#define FT_BNS_SLOTS128 2     // weight-step register slots of the 128-plane direct kernel on large strips: 3 spills (132 B of scratch)
#endif
template <int MT1, int MT2>
static int bns_launch_direct128(const BnsParams& p, hipStream_t s) {
  return bns_run<bottleneck_stream_direct128_kernel<MT1, MT2, MT1 == 4 ? FT_BNS_SLOTS128 : 3>>(256, BnsGeom<128>::LDS_BYTES,
                                                                                             "bottleneck_stream_direct128_kernel", p, s);
}

static int bns_launch_tile16(const BnsParams& p, hipStream_t s) {
  return bns_run<bottleneck_stream_tile16_kernel<FT_BNS_SLOTS>>(256, 81920 + 2 * 4 * 48 * 128, "bottleneck_stream_tile16_kernel", p, s);
}

}  // namespace
}  // namespace ft

extern "C" int ft_bottleneck_stream_supported(const ft_bottleneck_desc* d) {
  ft::BnsPlan pl;
  return ft::bns_plan(d, &pl);
}

extern "C" int ft_bottleneck_stream_folds(const ft_bottleneck_desc* d) {
  ft::BnsPlan pl;
  if (ft::bns_plan(d, &pl) != FT_OK) return 0;
  return pl.variant != ft::BNS_HEAD;
}

extern "C" int ft_bottleneck_stream_layout(const ft_bottleneck_desc* d) {
  ft::BnsPlan pl;
  if (ft::bns_plan(d, &pl) != FT_OK) return -1;
  return pl.variant == ft::BNS_TILE16 ? 1 : 0;
}

extern "C" int ft_bottleneck_stream_variant(const ft_bottleneck_desc* d) {
  ft::BnsPlan pl;
  if (ft::bns_plan(d, &pl) != FT_OK) return -1;
  return pl.variant;
}

extern "C" long long ft_bottleneck_stream_weight_bytes(const ft_bottleneck_desc* d) {
  ft::BnsPlan pl;
  if (ft::bns_plan(d, &pl) != FT_OK) return 0;
  if (pl.variant == ft::BNS_HEAD) return (long long)(d->C / 64 + 9 * ft::BnsGeom<256>::KC) * ft::BnsGeom<256>::WSTEP;
  return d->P == 128 ? (long long)ft::BnsGeom<128>::GEND * ft::BnsGeom<128>::WSTEP : (long long)ft::BnsGeom<256>::GEND * ft::BnsGeom<256>::WSTEP;
}

extern "C" int ft_bottleneck_stream_pack(const ft_bottleneck_desc* d, const void* w1, const void* w2, const void* w3, void* wstream,
                                         ft_stream_t stream) {
  using namespace ft;
  BnsPlan pl;
  const int st = bns_plan(d, &pl);
  if (st != FT_OK) return st;
  if (!w1 || !w2 || (!w3 && pl.variant != BNS_HEAD) || !wstream) return FT_ERR_INVALID_ARG;
  hipStream_t s = as_stream(stream);
  const half_t *a = static_cast<const half_t*>(w1), *b = static_cast<const half_t*>(w2), *c = static_cast<const half_t*>(w3);
  if (pl.variant == BNS_HEAD) {
    const int n16 = (int)(ft_bottleneck_stream_weight_bytes(d) / 16);
    hipLaunchKernelGGL(bns_pack_head_kernel, dim3(ceil_div(n16, 256)), dim3(256), 0, s, a, b, static_cast<uint4_t*>(wstream), d->C);
    FT_LAUNCH_CHECK("bns_pack_head_kernel");
    return FT_OK;
  }
  if (d->P == 128) {
    const int n16 = BnsGeom<128>::GEND * BnsGeom<128>::WSTEP / 16;
    hipLaunchKernelGGL(bns_pack_kernel<128>, dim3(ceil_div(n16, 256)), dim3(256), 0, s, a, b, c, static_cast<uint4_t*>(wstream));
  } else if (pl.variant == BNS_TILE16) {
    const int n16 = BnsGeom<256>::GEND * BnsGeom<256>::WSTEP / 16;
    hipLaunchKernelGGL(bns_pack16_kernel, dim3(ceil_div(n16, 256)), dim3(256), 0, s, a, b, c, static_cast<uint4_t*>(wstream));
  } else {
    const int n16 = BnsGeom<256>::GEND * BnsGeom<256>::WSTEP / 16;
    hipLaunchKernelGGL(bns_pack_kernel<256>, dim3(ceil_div(n16, 256)), dim3(256), 0, s, a, b, c, static_cast<uint4_t*>(wstream));
  }
  FT_LAUNCH_CHECK("bns_pack_kernel");
  return FT_OK;
}

extern "C" int ft_bottleneck_stream_fwd(const ft_bottleneck_desc* d, const void* x, const void* wstream, const float* tables, void* y,
                                        ft_stream_t stream) {
  using namespace ft;
  BnsPlan pl;
  const int st = bns_plan(d, &pl);
  if (st != FT_OK) return st;
  if (!x || !wstream || !tables || !y || x == y) return FT_ERR_INVALID_ARG;
  if (d->folded && pl.variant == BNS_HEAD) return FT_ERR_UNSUPPORTED;      // the stride-2 head keeps its tables (ft_bottleneck_stream_folds)
  BnsParams p{};
  p.x = static_cast<const char*>(x);
  p.y = static_cast<char*>(y);
  p.ws = static_cast<const char*>(wstream);
  p.tab = reinterpret_cast<const char*>(tables);
  p.H = d->H; p.W = d->W; p.TH = pl.TH; p.ppi = pl.ppi;
  p.TWc = pl.TWc; p.csplit = pl.csplit;
  if (pl.variant == BNS_HEAD) { p.Ho = d->H / 2; p.Wo = d->W / 2; }
  p.total = d->N * pl.ppi;
  p.x_cstride = d->x_cstride; p.x_coff = d->x_coff; p.y_cstride = d->y_cstride; p.y_coff = d->y_coff;
  p.x_bytes = (unsigned)((size_t)d->N * d->H * d->W * d->x_cstride * 2);
  p.y_bytes = (unsigned)((size_t)d->N * d->H * d->W * d->y_cstride * 2);
  p.ws_bytes = (unsigned)ft_bottleneck_stream_weight_bytes(d);
  if (pl.variant == BNS_HEAD) p.y_bytes = (unsigned)((size_t)d->N * p.Ho * p.Wo * d->y_cstride * 2);
  static const int dbg = dev_env_int("FT_BNS_DBG", 0);
  p.dbg = dbg;
  if (dbg & 64) p.ws_bytes = 0;     // dev: every weight load out of range (returns 0, no L2 access): the kernel's time without its weight stream
  if (dbg & 128) p.x_bytes = 0;     // dev: likewise the input
  hipStream_t s = as_stream(stream);
  // FT_BNS_WAVES=4|8 (read per call: dev A/B and tests): waves per workgroup of the direct (256-plane) kernels.  Default: eight
  // for the column-split form (R101 384x288 at 16 crops: 34.4 -> 33.3 us per block, R50 at 16 crops 30.0 -> 28.5), four for the
  // full-width strips (batch 64: 46.1 vs 46.0 us — the eight-wave form gains in phases 1 and 3 what its doubled pixel-operand
  // reads cost in phase 2; both forms sit on the CU's 64 B/clk weight path: 32 KiB of fragments per 16-MFMA step)
  const bool waves8 = dev_env_int("FT_BNS_WAVES", pl.variant == BNS_DIRECT256_XSPLIT ? 8 : 4) == 8;
  if (d->folded) {
    switch (pl.variant) {
      case BNS_RING128_LARGE: return bns_launch<128, 4, 3, true>(p, s);
      case BNS_RING128_SMALL: return bns_launch<128, 3, 2, true>(p, s);
      case BNS_DIRECT128_LARGE: return bns_launch_direct128<4, 3>(p, s);
      case BNS_DIRECT128_SMALL: return bns_launch_direct128<3, 2>(p, s);
      case BNS_RING256: return bns_launch<256, 4, 3, true>(p, s);
      case BNS_TILE16: return bns_launch_tile16(p, s);
      case BNS_DIRECT256_XSPLIT: return waves8 ? bns_launch_direct<2, 1, true, 0, 8, true>(p, s) : bns_launch_direct<2, 1, true, 0, 4, true>(p, s);
      default: return waves8 ? bns_launch_direct<3, 2, false, 0, 8, true>(p, s) : bns_launch_direct<3, 2, false, 0, 4, true>(p, s);
    }
  }
  switch (pl.variant) {
    case BNS_RING128_LARGE: return bns_launch<128, 4, 3>(p, s);
    case BNS_RING128_SMALL: return bns_launch<128, 3, 2>(p, s);
    case BNS_RING256: return bns_launch<256, 4, 3>(p, s);
    case BNS_DIRECT256_XSPLIT: return waves8 ? bns_launch_direct<2, 1, true, 0, 8>(p, s) : bns_launch_direct<2, 1, true>(p, s);
    case BNS_HEAD: return waves8 ? bns_launch_direct<4, 1, false, 8, 8>(p, s) : bns_launch_direct<4, 1, false, 8>(p, s);
    default:     // 64-pixel strips at 256 planes: weights straight to registers
      return waves8 ? bns_launch_direct<3, 2, false, 0, 8>(p, s) : bns_launch_direct<3, 2, false>(p, s);
  }
}
