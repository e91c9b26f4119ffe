// Whole-bottleneck fusion for the HBM-bound first ResNet stage (fp16): conv1 1x1 + bn1 + relu -> conv2 3x3 + bn2 + relu
// -> conv3 1x1 + bn3 + identity residual + relu in ONE launch (reference: Bottleneck.forward, lib/pose/models/blocks.py:
// 105-120, the blocks without a projection shortcut, layer1.1 / layer1.2 of resnet.py:29-36).
//
// Why: at 64x48 x 256 channels the three launches move 6.1 MB per crop through HBM (read x, write/read t1, write/read
// t2, read the residual, write y) for 27 MFLOP/KB — they run at the HBM roof (134 us per block at batch 64, of which
// the matrix pipe needs ~45).  Fused, a block reads x once and writes y once (3.0 MB per crop): t1 and t2 only ever
// exist in LDS.
//
// One 256-thread workgroup owns an 8x16 (or 16x8) patch of output pixels of one image:
//   phase 1  t1 = relu(bn1(W1 . x)) on the 10x18 HALO patch (180 pixels padded to 192; out-of-image pixels forced to 0 =
//            conv2's zero padding): GEMM [64 co] x [192 px] x K=256.  x streams HBM -> LDS in four 64-channel chunks
//            (whole 128-byte lines per pixel) through two DMA stages together with the matching K-slice of W1; the
//            residual (the patch's own 128 pixels) is picked out of the same stages in phase 3's register layout;
//            result -> fp16 T1 in LDS (24 KiB).
//   phase 2  t2 = relu(bn2(W2 * t1)): GEMM [64 co] x [128 px] x K=9*64; the pixel operand of every tap is read from T1
//            at the tap's offset (the conv_halo_kernel idea), only W2 streams (one tap = 8 KiB per K-step, 4-slot ring,
//            W3's quarters follow the taps through the same ring) -> fp16 T2 (16 KiB).
//   phase 3  y = relu(bn3(W3 . t2) + x): four 64-channel quarters, GEMM [64 co] x [128 px] x K=64 each, nothing is loaded
//            from memory any more; the fp16 tile is transposed through two alternating LDS buffers for 16-byte
//            coalesced stores (one barrier per quarter, no wait on the stores).
// 75 KiB of LDS -> two workgroups per CU.  The halo makes phase 1 do 1.4x the 1x1's MACs (0.9 GMAC of 13.7 per block at
// batch 64): cheap next to 3 MB of HBM.
// Measured (batch 64, 64x48): 134 us for the three launches -> 64 us.  The phases above describe the LDS-RING form (wfrag = 0): per
// patch 232 KB go L2 -> LDS (96 x, 136 weights), every hand-over is a workgroup barrier (22 per patch).  Its weight traffic alone is
// worth 6-11 us of a 55-73-us launch (FT_BNK_DBG=64: no weight loads; profiles/HISTORY.md, "fragment stream"); tools/dev/
// bnk_phases.py (phase timestamps) and the FT_BNK_DBG ablations in bnk_bench.py are the instruments; deeper rings, 64- vs
// 128-byte rows, an L2 warm-up of the later chunks and staggering the co-resident workgroups changed nothing.  The whole-block forms
// now run the fragment-stream form (WFRAG below): the weights skip LDS, 12-13 barriers per patch.
#include <stdlib.h>

#include <type_traits>

#include "ft_common.h"

// cache-policy bits of the block input's LDS-DMA loads (read once per workgroup + its halo neighbours): 0 = default, 2 = nt (A/B
// builds: tools/dev/build_variant.sh bnknt -DFT_BNK_XLOAD_AUX=2)
#ifndef FT_BNK_XLOAD_AUX
#define FT_BNK_XLOAD_AUX 0
#endif
namespace ft {
namespace {

struct BnkParams {
  const char* x;
  char* y;
  const char *w1, *w2, *w3;
  const char* tab;   // float [s1 64 | b1 64 | s2 64 | b2 64 | s3 256 | b3 256]
  int N, H, W;
  int x_cstride, x_coff, y_cstride, y_coff;
  unsigned x_bytes;
  int tx, ty;      // patches per image along x / y
  int total;       // workgroups
  int w3_pitch;    // bytes per output-channel row of w3: 128 (W3 [256][64]); 256 at a projection block ([256][W3' 64 | Wd' 64])
  int dbg;         // FT_BNK_DBG (dev): 1 no x loads, 4 no stores, 16 x loads from images 0..7 only (L2-resident), 32 phase timestamps
};
// the exit form's extra arguments (a type of its own: the kernel argument block of the other forms stays what it was)
struct BnkExitParams : BnkParams {
  const char* tw;      // tail weights [128][256] in fragment order (bnk_tail_pack_kernel)
  const float* tscale; // folded BN of the tail conv, 128 + 128 floats
  const float* tshift;
  char* t1;            // tail output [N,H,W,128] view
  int t1_cstride, t1_coff;
  int y_mode;          // FT_BNK_Y_FULL / _EVEN / _NONE
  unsigned y_bytes, t1_bytes;   // extents of the two outputs (buffer stores: a lane with nothing to store points out of range)
};

template <int N, int I = 0, typename F>
__device__ __forceinline__ void unroll_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    unroll_for<N, I + 1>(f);
  }
}

// s_barrier with a memory clobber: the builtin is IntrNoMem, LDS reads may be hoisted above it (see conv_igemm.hip)
#define BNK_BARRIER() asm volatile("s_barrier" ::: "memory")
// XOR key of the 16-byte chunk position inside a 128-byte LDS row.  A 256-byte bank row holds TWO such rows, so the sixteen
// consecutive rows a ds_read_b128 services together hit sixteen distinct 16-byte slots only if the key changes every second
// row: with `row & 7` rows r and r + 8 collided.  PMC (profiles/r02_lds_wait_counters.txt): bank-conflict cycles were 43-47 % of
// this kernel's LDS-active cycles before and are 30-33 % after — the fragment reads this key governs are fixed (the same change
// takes conv_direct's ring reads from 27-44 % to 0), but a third of the LDS time here is STILL conflicts.  Not tracked down;
// candidates are the 8-byte accesses (T1 / T2 / staging epilogue writes, the residual pick-up), where the two lanes of a pixel
// write the halves of one 16-byte chunk.  60.4 -> 57.3 us per block came from the part that is fixed.
#define BNK_KEY(r) (((r) >> 1) & 7)
// T1 (the 18- or 10-pixel-wide halo patch conv2's taps read at a row / column shift): ds_read_b128 serves lanes {0-3, 12-15,
// 20-27} together = with 16-pixel tile rows: columns 0-3 and 12-15 of one patch row and 4-11 of the next.  Keyed by the linear
// index (r >> 1 = 9 * row + column / 2) columns 12-13 of a row and 10-11 of the next share key AND 128-byte half: a 2-way
// conflict in every such read (+1 LDS cycle on 4: the 30-33 % conflict cycles the PMC kept showing).  Keyed by the COLUMN pair
// alone the sixteen lanes cover the sixteen slots.  (8-pixel tile rows: four rows x four columns per group; the old key stays.)
template <int TW> __device__ __forceinline__ int bnk_t1_key(int r, int pc) { return TW == 16 ? ((pc >> 1) & 7) : BNK_KEY(r); }

constexpr int kC = 256, kP = 64;                 // block width / planes this kernel is written for
// LDS map (bytes).  Phase 1: two 32-KiB stages (64-channel x chunk 24 KiB + W1 K-slice 8 KiB) at 0 .. 64 Ki.
// Phase 2: T1 at 0 (24 KiB), W2 ring slots 1..3 at 24 / 32 / 40 Ki and slot 0 at 64 Ki, T2 at 48 Ki (16 KiB).
// Phase 3: W3 quarters in the ring slots, output staging A at 0 and B at 48 Ki (16 KiB each).  Folded-BN table at 72 Ki.
[[maybe_unused]] constexpr int kStage1 = 32768, kXChunk = 24576;
[[maybe_unused]] constexpr int kOffT1 = 0, kOffT2 = 49152, kOffOutA = 0, kOffOutB = 49152, kOffTab = 73728;
constexpr int kLdsBytes = 76800;
__device__ __forceinline__ constexpr int ring_slot(int i) { return i == 0 ? 65536 : 24576 + (i - 1) * 8192; }
// The fragment stream of the WFRAG forms, in 1-KiB fragments (64 lanes x 16 bytes: lane -> weight row 32 * tile + lane % 32, eight
// consecutive k from 16 * slice + 8 * (lane / 32)), in the order a wave reads them.  nch = 64-channel chunks of the block input:
//   W1  [chunk nch][channel tile 2][K16 slice 4]
//   W2  [tap 9][channel tile 2][K16 slice 4]
//   W3  [quarter 4][channel tile 2][K16 slice 4]; projection form [quarter 4][channel tile 2][8]: slices 0-3 of W3', then 0-3 of Wd'
__host__ __device__ constexpr int frag_w2(int nch) { return nch * 8; }
__host__ __device__ constexpr int frag_w3(int nch) { return nch * 8 + 72; }
__host__ __device__ constexpr int frag_count(int nch, bool proj) { return nch * 8 + 72 + (proj ? 64 : 32); }

// NCH = 64-channel chunks of the block input (4: the 256-wide identity blocks, 1: the stage's entry block, 64 in).
// FULL = false stops after phase 2 and writes t2 (the entry block's conv3 is K-concatenated with its projection shortcut
// in ft_conv2d_fwd's x2_* path; here only its conv1 + conv2 pair is fused).
// PROJ = the entry block WHOLE (64 -> 64 -> 64 -> 256 with its projection shortcut, blocks.py:104-119): phase 3 is the GEMM
// over K = [t2 | x] of FusedShortcutConv (both BatchNorms folded into the weights, the shifts added): W3' quarters come through
// the ring as before, the x fragments of the patch's own pixels are picked out of the phase-1 stage in the B-operand layout
// and the shortcut weights Wd' (32 KiB per workgroup, L2-resident) go straight to registers at kernel start.
// EXIT = the stage's LAST identity block together with the 1x1 conv that opens the next stage (layer2.0.conv1, 256 -> 128 + bn + relu,
// resnet.py:37-43): nothing but that conv and the stride-2 shortcut reads the block's output, so a fourth phase multiplies every
// activated quarter of y, as it sits in its staging buffer ([128 px][64 ch] = the pixel-operand layout T2 is read in), by the
// K-slice [128 co][64 ci] of the tail weights into a persistent 128 x 128 fp32 accumulator (wave: ONE 32-channel tile x all four pixel
// tiles = 64 registers: no two waves fetch the same weights, 64 KiB per patch from L2; 2 x 2 tiles per wave fetch 128 KiB and read
// half the pixel fragments from LDS: measured alone the two layouts take the same time, profiles/HISTORY.md).  The tail weights come
// straight from L2 to registers in fragment order, a quarter's 4 KiB per wave one quarter ahead (two register sets); the outputs go
// through buffer stores, which the compiler counts: no wait on a weight fragment also waits for stores.  t1 leaves from the
// accumulator layout (a lane owns 16 consecutive channels, as in conv1x1_stream_kernel) and y is written whole, at its even pixels
// only (compact [N, H/2, W/2, 256]: what the stride-2 shortcut reads) or not at all.  250 registers, 76 800 B of LDS, no scratch.
//
// WFRAG = the weights come as ONE fragment-ordered stream (bnk_frag_pack_kernel, ft_bottleneck_desc.wfrag = 1; p.w1 is the stream,
// p.w2 / p.w3 are not read) and go from L2 straight to registers, every wave load one contiguous 1 KiB in the A-operand layout of
// mfma_f32_32x32x16_f16; both pixel groups of a channel tile load the same fragments (as bottleneck_stream_direct128_kernel):
//   phase 1  the W1 K-slice of a chunk (4 fragments per wave) one chunk ahead in two register sets; the stages hold x only, so there
//            are THREE of them (3 x 24 KiB): chunks 0..2 are in flight from the start and chunk 3 refills stage 0 — one refill
//            barrier per patch instead of two, 72 KiB per workgroup in flight against HBM.
//   phase 2  a tap's four fragments two taps ahead in three register sets; T1 is static in LDS, so the nine taps run with NO
//            workgroup barrier between them and the T1 fragment reads of tap t + 1 are issued under tap t's MFMAs.
//   phase 3  a W3 quarter's four fragments one quarter ahead (projection form: eight, W3' | Wd' — the shortcut weights stream with
//            them instead of sitting in 64 registers from kernel start).  The barrier per quarter guards the staging tiles only.
//            EXIT form: phases 3 / 4 have no registers left (acc4 + fw4), so its four W3 quarters go to LDS in one go behind
//            phase 1 (8 LDS-DMA loads per wave into the space the old ring slots had: free during phase 2) and are read as before.
//            The other forms write y with buffer stores the compiler can count: a wait on a W3 fragment leaves the stores in flight.
// The ring, its slots and 10 of the 22 barriers per patch are gone (12 left: 4 chunk + 1 refill + 1 stage hand-over, T1, T2,
// 4 quarters; + 1 in front of the quarters in the exit form).  The MFMA operand values and the accumulation order are those of the
// ring form: every output is bit-identical (tests/test_bottleneck_frag_gpu.py).  The head-only form (FULL = false) has no stream form.
template <int TW, int NCH, bool FULL, bool PROJ = false, bool EXIT = false, bool WFRAG = false>
__global__ __launch_bounds__(256, 2) void bottleneck_fused_kernel(const std::conditional_t<EXIT, BnkExitParams, BnkParams> p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int TH = 128 / TW, PW = TW + 2, PH = TH + 2, NPIX = PW * PH;
  static_assert(NPIX <= 192, "halo patch");
  static_assert(!PROJ || (FULL && NCH == 1), "projection form: 64-channel input, whole block");
  static_assert(!EXIT || (FULL && NCH == 4 && !PROJ), "exit form: the 256-wide identity block");
  static_assert(!WFRAG || FULL, "the fragment stream: whole blocks only");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) void* lds_ptr;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;

  // XCD-aware order: each XCD gets one contiguous range of patches (neighbouring patches share their halo rows through that
  // XCD's L2)
  const int logical = xcd_logical_wg(p.total);
  const int tiles_per_img = p.tx * p.ty;
  const int n = logical / tiles_per_img;
  const int trem = logical - n * tiles_per_img;
  const int tyi = trem / p.tx, txi = trem - tyi * p.tx;
  const int qy0 = tyi * TH, qx0 = txi * TW;

  const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.x), 0, p.x_bytes, 0x00020000);
  // (dbg & 64, dev: every weight load out of range = no traffic, zeros: the kernel's time without its 136 KB of weights per patch)
  const bool now = p.dbg & 64;
  const __amdgpu_buffer_rsrc_t rsrc_w1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.w1), 0, now ? 0 : kP * NCH * 128, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_w2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.w2), 0, now ? 0 : kP * 9 * kP * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_w3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.w3), 0, (FULL && !now) ? kC * kP * (PROJ ? 4 : 2) : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_tab = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.tab), 0, FULL ? 3072 : 1024, 0x00020000);
  constexpr unsigned kOOB = 0x80000000u;
  // WFRAG: the one stream behind p.w1; fragment f of it into a register quad (the fragment index is wave-uniform: the scalar offset)
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t rsrc_ws =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.w1), 0, (WFRAG && !now) ? frag_count(NCH, PROJ) * 1024 : 0, 0x00020000);
  [[maybe_unused]] const unsigned lane16 = (unsigned)(lane * 16);
  [[maybe_unused]] auto ld_frag = [&](int f) { return __builtin_amdgcn_raw_buffer_load_b128(rsrc_ws, lane16, f * 1024, 0); };

  // ---- loader lanes --------------------------------------------------------------------------------------------
  // every LDS tile here has 128-byte rows (64 fp16): a 1-KiB wave load covers 8 rows, lane -> (row = lane / 8, 16-byte
  // position = lane % 8) — whole 128-byte lines per row for the texture path (64-byte rows cost twice the requests per
  // byte: the phase-1 stream was request-bound with them).  The LDS image is lane-linear, so the XOR swizzle
  // (position ^= BNK_KEY(row)) is applied to the SOURCE position.
  const int lrow = lane >> 3, lpos = lane & 7;
  unsigned x_voff[6];
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const int pp = (t * 4 + wave) * 8 + lrow;           // halo pixel
    const int pr = pp / PW, pc = pp - pr * PW;
    const int iy = qy0 - 1 + pr, ix = qx0 - 1 + pc;
    unsigned v = kOOB;
    if (pp < NPIX && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W && !(p.dbg & 1))
      v = (unsigned)(((((p.dbg & 16 ? (n & 7) : n) * p.H + iy) * p.W + ix) * p.x_cstride + p.x_coff) * 2 + ((lpos ^ BNK_KEY(pp)) << 4));
    x_voff[t] = v;
  }
  unsigned w1_voff[2], w2_voff[2], w3_voff[2];           // rows (t * 4 + wave) * 8 + lrow of a 64-row weight block
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int wr = (t * 4 + wave) * 8 + lrow;
    const unsigned lc = (unsigned)((lpos ^ BNK_KEY(wr)) << 4);
    w1_voff[t] = (unsigned)(wr * NCH * 128) + lc;        // W1 [64][64 * NCH]
    w2_voff[t] = (unsigned)(wr * 9 * kP * 2) + lc;       // W2 [64][576]
    w3_voff[t] = (unsigned)(wr * p.w3_pitch) + lc;       // W3 [256][64] (or the first half of [256][128]), + quarter * 64 rows
  }

  auto load_stage1 = [&](int slot, int c) {              // chunk c: channels 64c .. 64c+63 of the halo patch + W1's K-slice
    char* st = smem + slot * kStage1;
#pragma unroll
    for (int t = 0; t < 6; ++t)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (lds_ptr)(st + (t * 4 + wave) * 1024), 16, x_voff[t],
                                               x_voff[t] == kOOB ? 0 : c * 128, 0, FT_BNK_XLOAD_AUX);
#pragma unroll
    for (int t = 0; t < 2; ++t)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w1, (lds_ptr)(st + kXChunk + (t * 4 + wave) * 1024), 16, w1_voff[t], c * 128, 0, 0);
  };
  // ring items 0..8 = the nine taps of W2 ([64 co][64 ci] = 128-byte rows), items 9..12 = the quarters of W3
  auto load_item = [&](int item) {
    char* st = smem + ring_slot(item & 3);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (item < 9)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w2, (lds_ptr)(st + (t * 4 + wave) * 1024), 16, w2_voff[t], item * 128, 0, 0);
      else    // !FULL: rsrc_w3 is empty, every lane is out of range -> zero fill, no traffic, same load count for the waits
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w3, (lds_ptr)(st + (t * 4 + wave) * 1024), 16, w3_voff[t], (item - 9) * 64 * p.w3_pitch, 0, 0);
    }
  };

  // oldest loads of every wave: the folded-BN table (3 KiB, waves 0..2) and W2's first tap (its ring slot lies outside the
  // phase-1 stages) — both land long before they are needed and sit in front of every counted wait below
  // projection form: the shortcut weights of this wave's channel tile, all four quarters x four 16-channel K slices, straight
  // to registers (the oldest loads of the wave: every counted wait below covers them)
  uint4_t fad[PROJ ? 4 : 1][4];
  if constexpr (PROJ && !WFRAG) {
    const int wc2_ = wave >> 1;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4)
        fad[q][k4] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w3, (unsigned)((q * 64 + wc2_ * 32 + l31) * 256 + 128 + (k4 * 2 + lhi) * 16), 0, 0);
  }
  if (wave < (FULL ? 3 : 1))
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_tab, (lds_ptr)(smem + kOffTab + wave * 1024), 16, (unsigned)(lane * 16), wave * 1024, 0, 0);
  if constexpr (!WFRAG) load_item(0);
  const float* tab =reinterpret_cast<const float*>(smem + kOffTab);
  unsigned long long ts[8];
#define BNK_TS(i) do { if (p.dbg & 32) ts[i] = __builtin_amdgcn_s_memtime(); } while (0)
  BNK_TS(0);

  // ================= phase 1: t1 = relu(bn1(W1 . x)) on the halo patch ==========================================
  // wave -> output-channel tile (wave & 1) x three 32-pixel tiles (wave >> 1)
  const int wc1 = wave & 1, wp1 = wave >> 1;
  const int a1_row = wc1 * 32 + l31;
  const int a1_off = a1_row * 128 + ((lhi ^ BNK_KEY(a1_row)) << 4);       // + (k16 * 2) << 4 by XOR: 16-channel slice k16
  int b1_off[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int r = (wp1 * 3 + j) * 32 + l31;
    b1_off[j] = r * 128 + ((lhi ^ BNK_KEY(r)) << 4);
  }
  float16_t acc1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[j][r] = 0.f;

  // residual = the block input at the patch's own 128 pixels, picked up in the ACCUMULATOR layout of phase 3 (lane ->
  // pixel wp2*64 + j*32 + l31, channels q*64 + wc2*32 + g*8 + lhi*4 .. +3) from the phase-1 stages as they pass through
  // LDS: chunk c = quarter c.  No second trip to L2 for them.
  const int wc2 = wave >> 1, wp2 = wave & 1;
  int rc_off[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = wp2 * 64 + j * 32 + l31;
    const int rc = (m / TW + 1) * PW + (m % TW + 1);
    rc_off[j] = rc * 128 + lhi * 8 + (((wc2 * 4) ^ BNK_KEY(rc)) << 4);    // 16-byte chunk wc2*4 + g sits at (.. ^ g) << 4
  }
  half4_t res[FULL && !PROJ ? 4 : 1][2][4];
  uint4_t fbx[PROJ ? 2 : 1][2][2];      // projection form: the block input at the patch's own pixels as phase 3's pixel operand

  // WFRAG: register sets of the weight stream.  W1's K-slice of chunk c sits in wa[c & 1], W2's tap t in w2r[t % 3], W3's quarter q
  // in w3r[q & 1] (projection form: W3' in [0..3], Wd' in [4..7])
  constexpr int NW3 = PROJ ? 8 : 4;
  uint4_t wa[WFRAG ? 2 : 1][4], w2r[WFRAG ? 3 : 1][4], w3r[WFRAG && !EXIT ? 2 : 1][NW3];
  [[maybe_unused]] auto load_w1 = [&](int c) __attribute__((always_inline)) {
#pragma unroll
    for (int k16 = 0; k16 < 4; ++k16) wa[c & 1][k16] = ld_frag((c * 2 + wc1) * 4 + k16);
  };
  [[maybe_unused]] auto load_w2 = [&](int tap) __attribute__((always_inline)) {
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) w2r[tap % 3][kq] = ld_frag(frag_w2(NCH) + (tap * 2 + wc2) * 4 + kq);
  };
  [[maybe_unused]] auto load_w3 = [&](int q) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NW3; ++i) w3r[q & 1][i] = ld_frag(frag_w3(NCH) + (q * 2 + wc2) * NW3 + i);
  };
  [[maybe_unused]] auto load_x = [&](int slot, int c) __attribute__((always_inline)) {   // WFRAG: a stage is the 24-KiB x chunk alone
    char* st = smem + slot * kXChunk;
#pragma unroll
    for (int t = 0; t < 6; ++t)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (lds_ptr)(st + (t * 4 + wave) * 1024), 16, x_voff[t],
                                               x_voff[t] == kOOB ? 0 : c * 128, 0, FT_BNK_XLOAD_AUX);
  };

  // ring form: two 32-KiB stages: chunk c+1 streams while chunk c is multiplied; a stage is refilled (chunk c+2) once every wave is
  // past its reads — a second barrier per chunk, four chunks.
  // WFRAG: three x stages, chunks 0..2 in flight from the start.  Vector-memory order of a wave: [table] W1.0 (4) x.0 (6) W1.1 (4)
  // x.1 (6) x.2 (6) | chunk 0 | W1.2 (4) x.3 (6, behind the refill barrier) | chunk 1 | W1.3 (4) | chunk 2 | chunk 3, W2 taps 0, 1 —
  // the counted waits below leave in flight what is younger than the chunk's x AND its W1 slice.
  if constexpr (WFRAG) {
    load_w1(0);
    asm volatile("" ::: "memory");    // compiler fences: the counts below need this issue order
    load_x(0, 0);
    if constexpr (NCH > 1) {
      asm volatile("" ::: "memory");
      load_w1(1);
      asm volatile("" ::: "memory");
      load_x(1, 1);
      load_x(2, 2);
    }
  } else {
    load_stage1(0, 0);
    if constexpr (NCH > 1) load_stage1(1, 1);
  }
  unroll_for<NCH>([&](auto cc) {
    constexpr int c = decltype(cc)::value;
    if constexpr (WFRAG) {
      static_assert(NCH == 1 || NCH == 4, "counted waits");
      if constexpr (c + 1 == NCH) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      else if constexpr (c < 2) asm volatile("s_waitcnt vmcnt(16) lgkmcnt(0)" ::: "memory");   // c = 0: W1.1 x.1 x.2; c = 1: x.2 W1.2 x.3
      else asm volatile("s_waitcnt vmcnt(10) lgkmcnt(0)" ::: "memory");                        // c = 2: x.3 W1.3
    } else {
      if constexpr (c < NCH - 1) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");   // chunk c landed; c+1 (8 loads) may fly
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    BNK_BARRIER();
    if constexpr (WFRAG && c + 1 == NCH) {     // W2's first two taps fly under the last chunk's MFMAs and epilogue 1
      load_w2(0);
      load_w2(1);
    }
    const char* st = smem + (WFRAG ? (c % 3) * kXChunk : (c & 1) * kStage1);
    uint4_t fa[4], fb[4][3];
#pragma unroll
    for (int k16 = 0; k16 < 4; ++k16) {
      if constexpr (WFRAG) fa[k16] = wa[c & 1][k16];
      else fa[k16] = *reinterpret_cast<const uint4_t*>(st + kXChunk + (a1_off ^ (k16 << 5)));
#pragma unroll
      for (int j = 0; j < 3; ++j) fb[k16][j] = *reinterpret_cast<const uint4_t*>(st + (b1_off[j] ^ (k16 << 5)));
    }
    if constexpr (FULL && !PROJ) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) res[c][j][g] = *reinterpret_cast<const half4_t*>(st + (rc_off[j] ^ (g << 4)));
    }
    if constexpr (PROJ) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int m = wp2 * 64 + j * 32 + l31;
        const int rc = (m / TW + 1) * PW + (m % TW + 1);
        const int lsw = lhi ^ BNK_KEY(rc);
#pragma unroll
        for (int sl = 0; sl < 2; ++sl)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk)
            fbx[sl][kk][j] = *reinterpret_cast<const uint4_t*>(st + rc * 128 + ((lsw ^ (sl * 4 + kk * 2)) << 4));
      }
    }
#pragma unroll
    for (int k16 = 0; k16 < 4; ++k16)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        acc1[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, fa[k16]),
                                                         __builtin_bit_cast(half8_t, fb[k16][j]), acc1[j], 0, 0, 0);
    if constexpr (WFRAG) {
      if constexpr (c + 2 < NCH) load_w1(c + 2);      // into the set this chunk's MFMAs were the last readers of
      if constexpr (c == 0 && NCH > 3) {              // the one refill: chunk 3 into stage 0
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        BNK_BARRIER();
        load_x(0, 3);
      }
    } else if constexpr (c + 2 < NCH) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      BNK_BARRIER();
      load_stage1(c & 1, c + 2);
    }
  });
  // the last chunk had vmcnt(0): no LDS-DMA load of this wave is in flight.  Every wave is past its last stage read once it
  // reaches this barrier: the stage region becomes T1 + the W2 ring (WFRAG, exit form: + the four W3 quarters).
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNK_BARRIER();
  BNK_TS(1);
  if constexpr (!WFRAG) {
    load_item(1);
    load_item(2);
  } else if constexpr (EXIT) {
    // W3 whole, from the fragment stream into the row-major swizzled image phase 3 reads (quarter q at ring_slot(q + 1)): LDS row
    // wr, 16-byte position lpos holds chunk lc = lpos ^ key of that row = lane 32 * (lc & 1) + wr % 32 of fragment
    // (q, wr / 32, lc / 2); eight rows of a wave load = eight 128-byte runs of the stream
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int wr = (t * 4 + wave) * 8 + lrow, lc = lpos ^ BNK_KEY(wr);
        const unsigned vo = (unsigned)((((wr >> 5) * 4 + (lc >> 1)) * 64 + (lc & 1) * 32 + (wr & 31)) * 16);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_ws, (lds_ptr)(smem + ring_slot((q + 1) & 3) + (t * 4 + wave) * 1024), 16, vo,
                                                 (frag_w3(NCH) + q * 8) * 1024, 0, 0);
      }
  }
  {
    char* t1 = smem + kOffT1;
    float4_t sc[4], sh[4];               // read once: the compiler cannot hoist LDS reads over the T1 writes itself
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      sc[g] = *reinterpret_cast<const float4_t*>(tab + wc1 * 32 + g * 8 + lhi * 4);
      sh[g] = *reinterpret_cast<const float4_t*>(tab + 64 + wc1 * 32 + g * 8 + lhi * 4);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int r = (wp1 * 3 + j) * 32 + l31;
      const int pr = r / PW, pc = r - pr * PW;
      const int iy = qy0 - 1 + pr, ix = qx0 - 1 + pc;
      const bool inside = r < NPIX && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      char* rowp = t1 + r * 128 + lhi * 8;
      const int rsw = bnk_t1_key<TW>(r, pc) << 4;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        half4_t h;
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const half2_t o = bn_relu_pk(acc1[j][g * 4 + e], acc1[j][g * 4 + e + 1], sc[g][e], sc[g][e + 1], sh[g][e], sh[g][e + 1]);
          h[e] = o[0];
          h[e + 1] = o[1];
        }
        uint2 hb = __builtin_bit_cast(uint2, h);
        hb.x = inside ? hb.x : 0u;       // out-of-image halo pixels are conv2's zero padding, not relu(bn1(0))
        hb.y = inside ? hb.y : 0u;
        *reinterpret_cast<uint2*>(rowp + ((((wc1 * 4 + g) << 4)) ^ rsw)) = hb;
      }
    }
  }
  BNK_TS(2);
  // ================= phase 2: t2 = relu(bn2(W2 * t1)), pixel operand from T1 ======================================
  // wave -> output-channel tile wc2 = wave >> 1 x two 32-pixel tiles (wp2 = wave & 1)
  const int a2_row = wc2 * 32 + l31;
  const int a2_off = a2_row * 128 + ((lhi ^ BNK_KEY(a2_row)) << 4);
  int r0[2], c0[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = wp2 * 64 + j * 32 + l31;
    r0[j] = (m / TW) * PW + (m % TW);
    c0[j] = m % TW;
  }
  float16_t acc2[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[j][r] = 0.f;

  if constexpr (WFRAG) {
    // T1 written by every wave; from here to T2 no barrier: the weights are this wave's own registers
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    BNK_BARRIER();
    const char* t1 = smem + kOffT1;
    uint4_t fbt[2][2][2][2];             // [tap & 1][sl][kk][j]: tap t + 1's pixel fragments are read under tap t's MFMAs
    auto read_t1 = [&](int tap) __attribute__((always_inline)) {
      const int ky = tap / 3, kx = tap % 3;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = r0[j] + ky * PW + kx;
        const int lsw = lhi ^ bnk_t1_key<TW>(r, c0[j] + kx);
        const char* rowp = t1 + r * 128;
#pragma unroll
        for (int sl = 0; sl < 2; ++sl)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk)
            fbt[tap & 1][sl][kk][j] = *reinterpret_cast<const uint4_t*>(rowp + ((lsw ^ (sl * 4 + kk * 2)) << 4));
      }
    };
    read_t1(0);
    unroll_for<9>([&](auto tc) {
      constexpr int tap = decltype(tc)::value;
      // (scheduling barriers: left alone, hipcc sinks every weight load to two MFMAs in front of its first use — the look-ahead is gone)
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (tap + 2 < 9) load_w2(tap + 2);                 // two taps ahead
      else if constexpr (tap == 7 && !EXIT) load_w3(0);            // then W3's first quarter
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (tap + 1 < 9) read_t1(tap + 1);
#pragma unroll
      for (int sl = 0; sl < 2; ++sl)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, w2r[tap % 3][sl * 2 + kk]),
                                                             __builtin_bit_cast(half8_t, fbt[tap & 1][sl][kk][j]), acc2[j], 0, 0, 0);
    });
  } else
  unroll_for<9>([&](auto tc) {
    constexpr int tap = decltype(tc)::value;
    constexpr int ky = tap / 3, kx = tap % 3;
    // item `tap` has landed; the two younger items (2 loads per wave each) stay in flight.  (tap 0: also T1 written)
    asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
    BNK_BARRIER();
    load_item(tap + 3);                                  // taps 3..8, then quarters 0..2 of W3
    const char* st = smem + ring_slot(tap & 3);
    const char* t1 = smem + kOffT1;
    uint4_t fa[2][2], fb[2][2][2];
#pragma unroll
    for (int sl = 0; sl < 2; ++sl)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) fa[sl][kk] = *reinterpret_cast<const uint4_t*>(st + (a2_off ^ ((sl * 2 + kk) << 5)));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = r0[j] + ky * PW + kx;
      const int lsw = lhi ^ bnk_t1_key<TW>(r, c0[j] + kx);
      const char* rowp = t1 + r * 128;
#pragma unroll
      for (int sl = 0; sl < 2; ++sl)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          fb[sl][kk][j] = *reinterpret_cast<const uint4_t*>(rowp + ((lsw ^ (sl * 4 + kk * 2)) << 4));
    }
#pragma unroll
    for (int sl = 0; sl < 2; ++sl)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc2[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, fa[sl][kk]),
                                                           __builtin_bit_cast(half8_t, fb[sl][kk][j]), acc2[j], 0, 0, 0);
  });

  // exit form: the tail weights of quarter 0 (this wave's one 32-channel tile x four K16 slices).  Issued behind the last
  // counted wait of the ring; the vmcnt(0) in front of phase 3 covers them.
  uint4_t fw4[EXIT ? 2 : 1][4];        // [quarter & 1][K16 slice] of channel tile `wave`
  float16_t acc4[EXIT ? 4 : 1];        // [pixel tile]
  [[maybe_unused]] auto load_tail = [&](int q) {
    if constexpr (EXIT) {
      const __amdgpu_buffer_rsrc_t rsrc_tw = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.tw), 0, 128 * kC * 2, 0x00020000);
#pragma unroll
      for (int k16 = 0; k16 < 4; ++k16)
        fw4[q & 1][k16] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_tw, (unsigned)(lane * 16), ((q * 4 + wave) * 4 + k16) * 1024, 0);
    }
  };
  if constexpr (EXIT) load_tail(0);
  BNK_TS(3);
  {
    char* t2 = smem + kOffT2;            // the T2 region held only a phase-1 stage, dead since the barrier after phase 1
    float4_t sc[4], sh[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      sc[g] = *reinterpret_cast<const float4_t*>(tab + 128 + wc2 * 32 + g * 8 + lhi * 4);
      sh[g] = *reinterpret_cast<const float4_t*>(tab + 192 + wc2 * 32 + g * 8 + lhi * 4);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = wp2 * 64 + j * 32 + l31;
      char* rowp = t2 + m * 128 + lhi * 8;
      const int msw = BNK_KEY(m) << 4;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        half4_t h;
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const half2_t o = bn_relu_pk(acc2[j][g * 4 + e], acc2[j][g * 4 + e + 1], sc[g][e], sc[g][e + 1], sh[g][e], sh[g][e + 1]);
          h[e] = o[0];
          h[e + 1] = o[1];
        }
        *reinterpret_cast<half4_t*>(rowp + (((wc2 * 4 + g) << 4) ^ msw)) = h;
      }
    }
  }
  // T2 complete, T1 and the last tap's slot dead once every wave is here: the last quarter of W3 goes into that slot
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BNK_BARRIER();
  BNK_TS(4);
  if constexpr (!FULL) {     // entry block: t2 is the result — 128 pixels x 128 bytes, 16 bytes per lane
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the ring's trailing (empty) loads must not outlive the workgroup's LDS
    const char* t2 = smem + kOffT2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + 256 * i, m = idx >> 3, ch = idx & 7;
      const int oy = qy0 + m / TW, ox = qx0 + m % TW;
      const uint4_t v = *reinterpret_cast<const uint4_t*>(t2 + m * 128 + ((ch ^ BNK_KEY(m)) << 4));
      if (oy < p.H && ox < p.W && !(p.dbg & 4))
        store_out16(p.y + ((((long long)n * p.H + oy) * p.W + ox) * p.y_cstride + p.y_coff + ch * 8) * 2, v);
    }
    return;
  }
  if constexpr (!WFRAG) load_item(12);

  // ================= phase 3: y = relu(bn3(W3 . t2) + x), four quarters of 64 output channels ====================
  // exit form: 64 more accumulator registers live through phase 3, so T2's fragments are read again in every quarter instead of
  // held (32 registers); staging B then cannot reuse the T2 region and lies at 16 .. 32 Ki (8 KiB that T1 left + ring slot 1,
  // whose W3 quarter 0 every wave is done with at quarter 0's barrier, before quarter 1 writes B for the first time)
  constexpr int kOutB = EXIT ? 16384 : kOffOutB;
  uint4_t fb3[2][2][2];
#define BNK_LOAD_FB3()                                                                                                       \
  {                                                                                                                          \
    const char* t2 = smem + kOffT2;                                                                                          \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                                          \
      const int m = wp2 * 64 + j * 32 + l31;                                                                                 \
      const int lsw = lhi ^ BNK_KEY(m);                                                                                      \
      _Pragma("unroll") for (int sl = 0; sl < 2; ++sl)                                                                       \
        _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                                                                     \
          fb3[sl][kk][j] = *reinterpret_cast<const uint4_t*>(t2 + m * 128 + ((lsw ^ (sl * 4 + kk * 2)) << 4));               \
    }                                                                                                                        \
  }
  if constexpr (!EXIT) BNK_LOAD_FB3();
  long long spix[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = (tid + 256 * i) >> 3;
    const int oy = qy0 + m / TW, ox = qx0 + m % TW;
    spix[i] = (oy < p.H && ox < p.W) ? ((long long)n * p.H + oy) * p.W + ox : -1;
    if constexpr (EXIT) {    // patch origins are even: parity is local.  H and W are even here (supported())
      if (p.y_mode == FT_BNK_Y_EVEN)
        spix[i] = (oy < p.H && ox < p.W && !((oy | ox) & 1)) ? ((long long)n * (p.H >> 1) + (oy >> 1)) * (p.W >> 1) + (ox >> 1) : -1;
      else if (p.y_mode == FT_BNK_Y_NONE) spix[i] = -1;
    }
  }
  // every W3 quarter and the residuals have landed; every wave holds its T2 fragments (staging B reuses the T2 region).
  // WFRAG, not the exit form: W3 is in this wave's registers and nothing waits here — staging A is the T1 region, dead since the
  // barrier above, and staging B is first written behind quarter 0's barrier, which every wave reaches with its T2 fragments read.
  if constexpr (!WFRAG || EXIT) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    BNK_BARRIER();
  }
  BNK_TS(5);

  unroll_for<4>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    [[maybe_unused]] const char* wq = smem + ring_slot((q + 1) & 3);
    float16_t acc3[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc3[j][r] = 0.f;
    if constexpr (EXIT) {
      if constexpr (q < 3) load_tail(q + 1);
      BNK_LOAD_FB3();
    }
    if constexpr (WFRAG && !EXIT && q < 3) {                     // one quarter ahead
      __builtin_amdgcn_sched_barrier(0);
      load_w3(q + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int sl = 0; sl < 2; ++sl)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        uint4_t fa;
        if constexpr (WFRAG && !EXIT) fa = w3r[q & 1][sl * 2 + kk];
        else fa = *reinterpret_cast<const uint4_t*>(wq + (a2_off ^ ((sl * 2 + kk) << 5)));
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc3[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, fa),
                                                           __builtin_bit_cast(half8_t, fb3[sl][kk][j]), acc3[j], 0, 0, 0);
      }
    if constexpr (PROJ) {
#pragma unroll
      for (int sl = 0; sl < 2; ++sl)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            uint4_t fd;
            if constexpr (WFRAG) fd = w3r[q & 1][4 + sl * 2 + kk];
            else fd = fad[q][sl * 2 + kk];
            acc3[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, fd),
                                                             __builtin_bit_cast(half8_t, fbx[sl][kk][j]), acc3[j], 0, 0, 0);
          }
    }
    char* so = smem + ((q & 1) ? kOutB : kOffOutA);
    float4_t sc[4], sh[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      sc[g] = *reinterpret_cast<const float4_t*>(tab + 256 + q * 64 + wc2 * 32 + g * 8 + lhi * 4);
      sh[g] = *reinterpret_cast<const float4_t*>(tab + 512 + q * 64 + wc2 * 32 + g * 8 + lhi * 4);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = wp2 * 64 + j * 32 + l31;
      char* rowp = so + m * 128 + lhi * 8;
      const int msw = BNK_KEY(m) << 4;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        half4_t h;
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          half2_t o;
          if constexpr (PROJ) o = bn_relu_pk(acc3[j][g * 4 + e], acc3[j][g * 4 + e + 1], sc[g][e], sc[g][e + 1], sh[g][e], sh[g][e + 1]);
          else o = bn_res_relu_pk(acc3[j][g * 4 + e], acc3[j][g * 4 + e + 1], sc[g][e], sc[g][e + 1], sh[g][e], sh[g][e + 1],
                                  res[PROJ ? 0 : q][j][g][e], res[PROJ ? 0 : q][j][g][e + 1]);
          h[e] = o[0];
          h[e + 1] = o[1];
        }
        *reinterpret_cast<half4_t*>(rowp + (((wc2 * 4 + g) << 4) ^ msw)) = h;
      }
    }
    // one barrier per quarter: the two staging buffers alternate, a buffer's previous readers are two barriers behind
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    BNK_BARRIER();
    if constexpr (WFRAG && !EXIT) {
      // buffer stores, which the compiler counts (store_out16 is opaque to it): its waits on the W3 fragments of the next quarter,
      // loaded in front of these stores, then leave the stores in flight.  32-bit offsets: supported() bounds y for wfrag.
      const __amdgpu_buffer_rsrc_t rsrc_y = __builtin_amdgcn_make_buffer_rsrc(
          p.y, 0, (p.dbg & 4) ? 0 : (unsigned)((size_t)p.N * p.H * p.W * p.y_cstride * 2), 0x00020000);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, m = idx >> 3, ch = idx & 7;
        const uint4_t v = *reinterpret_cast<const uint4_t*>(so + m * 128 + ((ch ^ BNK_KEY(m)) << 4));
        const unsigned vo = spix[i] >= 0 ? (unsigned)((spix[i] * p.y_cstride + p.y_coff + q * 64 + ch * 8) * 2) : kOOB;
        __builtin_amdgcn_raw_buffer_store_b128(v, rsrc_y, vo, 0, FT_YSTORE_BUF_AUX);
      }
    } else if constexpr (!EXIT) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, m = idx >> 3, ch = idx & 7;
        const uint4_t v = *reinterpret_cast<const uint4_t*>(so + m * 128 + ((ch ^ BNK_KEY(m)) << 4));
        if (spix[i] >= 0 && !(p.dbg & 4))
          store_out16(p.y + (spix[i] * p.y_cstride + p.y_coff + q * 64 + ch * 8) * 2, v);
      }
    } else {
      const __amdgpu_buffer_rsrc_t rsrc_y = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, (p.dbg & 4) ? 0 : p.y_bytes, 0x00020000);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, m = idx >> 3, ch = idx & 7;
        const uint4_t v = *reinterpret_cast<const uint4_t*>(so + m * 128 + ((ch ^ BNK_KEY(m)) << 4));
        const unsigned vo = spix[i] >= 0 ? (unsigned)((spix[i] * p.y_cstride + p.y_coff + q * 64 + ch * 8) * 2) : kOOB;
        __builtin_amdgcn_raw_buffer_store_b128(v, rsrc_y, vo, 0, FT_YSTORE_BUF_AUX);
      }
      // ---- phase 4, step q: tail accumulator += Wt[:, 64q .. 64q+63] . y quarter (the fp16 values just staged) ------------
      if constexpr (q == 0) {    // the accumulator starts its life here, not in front of phase 3 (registers)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc4[pt][r] = 0.f;
      }
#pragma unroll
      for (int k16 = 0; k16 < 4; ++k16) {
        uint4_t fb4[4];
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
          const int m = pt * 32 + l31;
          fb4[pt] = *reinterpret_cast<const uint4_t*>(so + m * 128 + (((lhi ^ BNK_KEY(m)) ^ (k16 * 2)) << 4));
        }
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
          acc4[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, fw4[q & 1][k16]),
                                                            __builtin_bit_cast(half8_t, fb4[pt]), acc4[pt], 0, 0, 0);
      }
    }
  });
  if constexpr (EXIT) {
    // tail epilogue = conv1x1_stream_kernel's: fp32 scale * acc + shift, ReLU, fp16; register r of the tile = channel 16 lhi + r
    // (the pack kernel permuted the rows), 32 bytes per lane and pixel tile
    const __amdgpu_buffer_rsrc_t rsrc_t1 = __builtin_amdgcn_make_buffer_rsrc(p.t1, 0, (p.dbg & 4) ? 0 : p.t1_bytes, 0x00020000);
    const int ch = wave * 32 + 16 * lhi;
    float4_t sc[4], sh[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      sc[g] = *reinterpret_cast<const float4_t*>(p.tscale + ch + 4 * g);
      sh[g] = *reinterpret_cast<const float4_t*>(p.tshift + ch + 4 * g);
    }
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int m = pt * 32 + l31;
      const int oy = qy0 + m / TW, ox = qx0 + m % TW;
      const unsigned vo = (oy < p.H && ox < p.W) ? (unsigned)(((((long long)n * p.H + oy) * p.W + ox) * p.t1_cstride + p.t1_coff + ch) * 2) : kOOB;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        half8_t o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int r = h * 8 + e;
          const float v = acc4[pt][r] * sc[r >> 2][r & 3] + sh[r >> 2][r & 3];
          o[e] = (half_t)act_mul(v, 0.f);
        }
        // plain, not write-through (as conv1x1_stream_kernel): a 128-byte line of t1 gets its four 32-byte pieces from four lanes of
        // two waves at different times and the L2 merges them; written through, every piece went to memory as a 64-byte write
        // (WRITE_SIZE 125.8 MB per launch at batch 64 where t1 + the even y are 75.5)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4_t, o), rsrc_t1, vo, h * 16, 0);
      }
    }
  }
  if (p.dbg & 32) {       // dev: phase timestamps of wave 0 over the tile's first output pixel (output is garbage then)
    ts[6] = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ts[7] = __builtin_amdgcn_s_memtime();
    if (tid == 0) {
      unsigned long long* o = reinterpret_cast<unsigned long long*>(p.y + ((((long long)n * p.H + qy0) * p.W + qx0) * p.y_cstride + p.y_coff) * 2);
      if constexpr (EXIT)    // the exit form may have no full y map: the stamps go to t1's first pixel of the tile (128 channels = 256 bytes)
        o = reinterpret_cast<unsigned long long*>(p.t1 + ((((long long)n * p.H + qy0) * p.W + qx0) * p.t1_cstride + p.t1_coff) * 2);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = ts[i];
    }
  }
#endif
}

static int supported(const ft_bottleneck_desc* d) {
  if (!d) return FT_ERR_INVALID_ARG;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0) return FT_ERR_INVALID_ARG;
  if (d->dtype != FT_F16 || d->P != kP || d->stride > 1) return FT_ERR_UNSUPPORTED;
  if (d->head_only && d->projection) return FT_ERR_INVALID_ARG;
  if (d->wfrag != 0 && d->wfrag != 1) return FT_ERR_INVALID_ARG;
  if (d->wfrag && d->head_only) return FT_ERR_UNSUPPORTED;      // the head-only form has no fragment-stream kernel
  if (d->wfrag && (long long)d->N * d->H * d->W * d->y_cstride * 2 >= (1LL << 31)) return FT_ERR_UNSUPPORTED;   // its y goes through buffer stores
  if (d->head_only || d->projection ? d->C != 64 : d->C != kC) return FT_ERR_UNSUPPORTED;   // (256-wide head-only: no caller, not instantiated)
  const int yc = d->head_only ? d->P : kC;
  if (d->x_coff < 0 || d->y_coff < 0 || d->x_coff % 8 || d->y_coff % 8 || d->x_cstride % 8 || d->y_cstride % 8) return FT_ERR_UNSUPPORTED;
  if (d->x_cstride < d->x_coff + d->C || d->y_cstride < d->y_coff + yc) return FT_ERR_INVALID_ARG;
  if ((long long)d->N * d->H * d->W * d->x_cstride * 2 >= (1LL << 31)) return FT_ERR_UNSUPPORTED;
  return FT_OK;
}

// fragment-ordered tail weights of the exit form: [quarter 4][channel tile 4][K16 slice 4][lane 64] x 16 bytes from the packed
// [128][256] layout; row r of a tile holds channel cd_sigma(r), so accumulator register r of lane half lhi = channel 16 lhi + r
__global__ __launch_bounds__(256) void bnk_tail_pack_kernel(const half_t* __restrict__ w, uint4_t* __restrict__ out, int kpad) {
  const int idx = blockIdx.x * 256 + threadIdx.x;      // 4096 = 16 blocks exactly
  const int lane = idx & 63, f = idx >> 6;
  const int k16 = f & 3, tl = (f >> 2) & 3, q = f >> 4;
  const int r = lane & 31;
  const int co = tl * 32 + 16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3), k = q * 64 + k16 * 16 + 8 * (lane >> 5);
  out[idx] = *reinterpret_cast<const uint4_t*>(w + (size_t)co * kpad + k);
}

// the fragment stream of the WFRAG forms (layout: frag_w2 / frag_w3 above) from the three packed weight blocks: W1 [64][64 nch],
// W2 [64][576], W3 [256][64] (projection form [256][W3' 64 | Wd' 64]).  One thread per 16 bytes; the fp16 values are copied as they are.
__global__ __launch_bounds__(256) void bnk_frag_pack_kernel(const half_t* __restrict__ w1, const half_t* __restrict__ w2,
                                                            const half_t* __restrict__ w3, uint4_t* __restrict__ out, int nch, int proj) {
  const int idx = blockIdx.x * 256 + threadIdx.x;      // frag_count * 64 = a multiple of 256
  const int lane = idx & 63, f = idx >> 6;
  const int l31 = lane & 31, k8 = 8 * (lane >> 5);
  const half_t* src;
  if (f < frag_w2(nch)) {
    const int c = f >> 3, wc = (f >> 2) & 1, k16 = f & 3;
    src = w1 + (size_t)(wc * 32 + l31) * (nch * 64) + c * 64 + k16 * 16 + k8;
  } else if (f < frag_w3(nch)) {
    const int g = f - frag_w2(nch), tap = g >> 3, wc = (g >> 2) & 1, kq = g & 3;
    src = w2 + (size_t)(wc * 32 + l31) * (9 * kP) + tap * 64 + kq * 16 + k8;
  } else if (!proj) {
    const int g = f - frag_w3(nch), q = g >> 3, wc = (g >> 2) & 1, kq = g & 3;
    src = w3 + (size_t)(q * 64 + wc * 32 + l31) * kP + kq * 16 + k8;
  } else {
    const int g = f - frag_w3(nch), q = g >> 4, wc = (g >> 3) & 1, i = g & 7;
    src = w3 + (size_t)(q * 64 + wc * 32 + l31) * (2 * kP) + i * 16 + k8;
  }
  out[idx] = *reinterpret_cast<const uint4_t*>(src);
}

// 0 when the descriptor has no stream form (unsupported, or head-only)
static long long frag_bytes(const ft_bottleneck_desc* d) {
  if (supported(d) != FT_OK || d->head_only) return 0;
  return (long long)frag_count(d->C / 64, d->projection != 0) * 1024;
}

static int exit_supported(const ft_bottleneck_desc* d, int tail_cout, int t1_cstride, int t1_coff, int y_mode) {
  const int st = supported(d);
  if (st != FT_OK) return st;
  if (y_mode != FT_BNK_Y_FULL && y_mode != FT_BNK_Y_EVEN && y_mode != FT_BNK_Y_NONE) return FT_ERR_INVALID_ARG;
  if (d->head_only || d->projection || d->C != kC || tail_cout != 128) return FT_ERR_UNSUPPORTED;
  if ((d->H | d->W) & 1) return FT_ERR_UNSUPPORTED;
  if (t1_coff < 0 || t1_coff % 8 || t1_cstride % 8) return FT_ERR_UNSUPPORTED;
  if (t1_cstride < t1_coff + tail_cout) return FT_ERR_INVALID_ARG;
  if ((long long)d->N * d->H * d->W * t1_cstride * 2 >= (1LL << 31) || (long long)d->N * d->H * d->W * d->y_cstride * 2 >= (1LL << 31))
    return FT_ERR_UNSUPPORTED;      // 32-bit offsets of the buffer stores
  return FT_OK;
}

template <int TW, bool WFRAG = false>
static int launch_exit(const BnkExitParams& p, hipStream_t s) {
  auto k = bottleneck_fused_kernel<TW, 4, true, false, true, WFRAG>;
  FT_RAISE_LDS(k, kLdsBytes);
  hipLaunchKernelGGL(k, dim3(p.total), dim3(256), kLdsBytes, s, p);
  FT_LAUNCH_CHECK("bottleneck_fused_kernel(exit)");
  return FT_OK;
}

template <int TW, int NCH, bool FULL, bool PROJ = false, bool WFRAG = false>
static int launch(const BnkParams& p, hipStream_t s) {
  auto k = bottleneck_fused_kernel<TW, NCH, FULL, PROJ, false, WFRAG>;
  FT_RAISE_LDS(k, kLdsBytes);
  hipLaunchKernelGGL(k, dim3(p.total), dim3(256), kLdsBytes, s, p);
  FT_LAUNCH_CHECK("bottleneck_fused_kernel");
  return FT_OK;
}

static void fill_params(BnkParams& p, const ft_bottleneck_desc* d, const void* x, const void* w1, const void* w2, const void* w3,
                        const float* scale_shift, void* y) {
  p.x = static_cast<const char*>(x);
  p.y = static_cast<char*>(y);
  p.w1 = static_cast<const char*>(w1);
  p.w2 = static_cast<const char*>(w2);
  p.w3 = static_cast<const char*>(w3);
  p.tab = reinterpret_cast<const char*>(scale_shift);
  p.N = d->N; p.H = d->H; p.W = d->W;
  p.x_cstride = d->x_cstride; p.x_coff = d->x_coff; p.y_cstride = d->y_cstride; p.y_coff = d->y_coff;
  p.x_bytes = (unsigned)((size_t)d->N * d->H * d->W * d->x_cstride * 2);
  p.w3_pitch = d->projection ? 256 : 128;
  // 8 rows x 16 columns unless the width only divides by 8 (R101 at 384x288: 96x72 maps -> 16 rows x 8 columns)
  const bool tall = d->W % 16 != 0 && d->W % 8 == 0;
  const int tw = tall ? 8 : 16, th = 128 / tw;
  p.tx = ceil_div(d->W, tw);
  p.ty = ceil_div(d->H, th);
  p.total = d->N * p.tx * p.ty;
  static const int dbg = dev_env_int("FT_BNK_DBG", 0);
  p.dbg = dbg;
}

}  // namespace
}  // namespace ft

extern "C" int ft_bottleneck_supported(const ft_bottleneck_desc* d) { return ft::supported(d); }

extern "C" double ft_bottleneck_flops(const ft_bottleneck_desc* d) {
  if (!d) return 0.0;
  const double cout = 4.0 * d->P;
  if (d->head_only && d->stride == 2)     // conv1 on the input map, conv2 on the halved one
    return 2.0 * d->N * ((double)d->H * d->W * d->C * d->P + (double)(d->H / 2) * (d->W / 2) * 9.0 * d->P * d->P);
  return 2.0 * d->N * d->H * d->W * ((double)d->C * d->P + 9.0 * d->P * d->P + (d->head_only ? 0.0 : (double)d->P * cout) +
                                     (d->projection ? (double)d->C * cout : 0.0));
}

extern "C" int ft_bottleneck_fwd(const ft_bottleneck_desc* d, const void* x, const void* w1, const void* w2, const void* w3,
                                 const float* scale_shift, void* y, ft_stream_t stream) {
  using namespace ft;
  const int st = supported(d);
  if (st != FT_OK) return st;
  if (!x || !w1 || !scale_shift || !y) return FT_ERR_INVALID_ARG;
  if (d->wfrag ? (w2 || w3) : (!w2 || (!w3 && !d->head_only))) return FT_ERR_INVALID_ARG;   // wfrag: w1 is the whole stream
  BnkParams p{};
  fill_params(p, d, x, w1, w2, w3, scale_shift, y);
  hipStream_t s = as_stream(stream);
  const bool tall = d->W % 16 != 0 && d->W % 8 == 0;
  if (d->head_only) return tall ? launch<8, 1, false>(p, s) : launch<16, 1, false>(p, s);
  if (d->wfrag) {
    if (d->projection) return tall ? launch<8, 1, true, true, true>(p, s) : launch<16, 1, true, true, true>(p, s);
    return tall ? launch<8, 4, true, false, true>(p, s) : launch<16, 4, true, false, true>(p, s);
  }
  if (d->projection) return tall ? launch<8, 1, true, true>(p, s) : launch<16, 1, true, true>(p, s);
  return tall ? launch<8, 4, true>(p, s) : launch<16, 4, true>(p, s);
}

extern "C" long long ft_bottleneck_frag_bytes(const ft_bottleneck_desc* d) { return d ? ft::frag_bytes(d) : 0; }

extern "C" int ft_bottleneck_frag_pack(const ft_bottleneck_desc* d, const void* w1, const void* w2, const void* w3, void* out,
                                       ft_stream_t stream) {
  using namespace ft;
  const int st = supported(d);
  if (st != FT_OK) return st;
  if (d->head_only) return FT_ERR_UNSUPPORTED;
  if (!w1 || !w2 || !w3 || !out) return FT_ERR_INVALID_ARG;
  const int nch = d->C / 64, proj = d->projection != 0;
  hipLaunchKernelGGL(bnk_frag_pack_kernel, dim3(frag_count(nch, proj) / 4), dim3(256), 0, as_stream(stream), static_cast<const half_t*>(w1),
                     static_cast<const half_t*>(w2), static_cast<const half_t*>(w3), static_cast<uint4_t*>(out), nch, proj);
  FT_LAUNCH_CHECK("bnk_frag_pack_kernel");
  return FT_OK;
}

extern "C" int ft_bottleneck_exit_supported(const ft_bottleneck_desc* d, int tail_cout, int t1_cstride, int t1_coff, int y_mode) {
  return ft::exit_supported(d, tail_cout, t1_cstride, t1_coff, y_mode);
}

extern "C" long long ft_bottleneck_exit_weight_bytes(const ft_bottleneck_desc* d, int tail_cout) {
  return ft::exit_supported(d, tail_cout, tail_cout, 0, FT_BNK_Y_FULL) == FT_OK ? 128LL * ft::kC * 2 : 0;
}

extern "C" int ft_bottleneck_exit_pack(const ft_bottleneck_desc* d, int tail_cout, const void* wt_packed, int kpad, int cout_pad, void* wstream,
                                       ft_stream_t stream) {
  using namespace ft;
  const int st = exit_supported(d, tail_cout, tail_cout, 0, FT_BNK_Y_FULL);
  if (st != FT_OK) return st;
  if (!wt_packed || !wstream || kpad < kC || kpad % 8 || cout_pad < tail_cout) return FT_ERR_INVALID_ARG;
  hipLaunchKernelGGL(bnk_tail_pack_kernel, dim3(16), dim3(256), 0, as_stream(stream), static_cast<const half_t*>(wt_packed),
                     static_cast<uint4_t*>(wstream), kpad);
  FT_LAUNCH_CHECK("bnk_tail_pack_kernel");
  return FT_OK;
}

extern "C" int ft_bottleneck_exit_fwd(const ft_bottleneck_desc* d, const void* x, const void* w1, const void* w2, const void* w3,
                                      const float* scale_shift, void* y, int y_mode, int tail_cout, const void* tail_wstream,
                                      const float* tail_scale, const float* tail_shift, void* t1, int t1_cstride, int t1_coff,
                                      ft_stream_t stream) {
  using namespace ft;
  const int st = exit_supported(d, tail_cout, t1_cstride, t1_coff, y_mode);
  if (st != FT_OK) return st;
  if (!x || !w1 || !scale_shift || (!y && y_mode != FT_BNK_Y_NONE) || !tail_wstream || !tail_scale || !tail_shift || !t1)
    return FT_ERR_INVALID_ARG;
  if (d->wfrag ? (w2 || w3) : (!w2 || !w3)) return FT_ERR_INVALID_ARG;      // wfrag: w1 is the whole stream
  BnkExitParams p{};
  fill_params(p, d, x, w1, w2, w3, scale_shift, y);
  p.tw = static_cast<const char*>(tail_wstream);
  p.tscale = tail_scale;
  p.tshift = tail_shift;
  p.t1 = static_cast<char*>(t1);
  p.t1_cstride = t1_cstride; p.t1_coff = t1_coff;
  p.y_mode = y_mode;
  const size_t ypix = y_mode == FT_BNK_Y_FULL ? (size_t)d->N * d->H * d->W : y_mode == FT_BNK_Y_EVEN ? (size_t)d->N * (d->H / 2) * (d->W / 2) : 0;
  p.y_bytes = (unsigned)(ypix * d->y_cstride * 2);
  p.t1_bytes = (unsigned)((size_t)d->N * d->H * d->W * t1_cstride * 2);
  const bool tall = d->W % 16 != 0 && d->W % 8 == 0;
  if (d->wfrag) return tall ? launch_exit<8, true>(p, as_stream(stream)) : launch_exit<16, true>(p, as_stream(stream));
  return tall ? launch_exit<8>(p, as_stream(stream)) : launch_exit<16>(p, as_stream(stream));
}
