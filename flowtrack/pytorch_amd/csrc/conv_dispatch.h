// Host side of ft_conv2d_fwd, shared by the conv units: the packed-weight geometry, the tile_hint codec, and for every
// kernel family its `*_ok` predicate and `launch_*` entry.  conv_dispatch.hip holds validate / geometry / tile_valid, the
// dispatcher and every extern "C" entry point; the kernels and their launch code live in
//   conv_igemm.hip   conv_igemm_kernel, conv_igemm_dma_kernel (+ the dma tile table), conv_splitk_reduce_kernel,
//                    conv_halo_kernel, conv_stem_kernel, conv_stem_persist_kernel, conv_stem_pool_kernel
//   conv_igemm8.hip  conv_igemm8_kernel
//   conv_fewout.hip  conv_fewout_kernel, conv_pflow_kernel, conv_pflow_mfma_kernel
// Declarations only: nothing here reaches device code.
#pragma once
#include "conv_common.h"

#ifndef FT_DMA_BKB
#define FT_DMA_BKB 64
#endif
#ifndef FT_DMA_STAGES
#define FT_DMA_STAGES 3   // measured on R50 B=64: 2 -> 1.88 ms, 3 -> 1.90, 4 -> 1.98, 5 -> 2.22 (occupancy beats ring depth)
#endif

namespace ft {

constexpr int kBKB = 64;       // generic kernel: bytes of K per tile row per step
constexpr int kBP = 128;       // generic kernel: pixel tile
constexpr int kDmaBKB = FT_DMA_BKB;        // dma kernel: bytes of K per tile row per step (64 -> 32 fp16 / 16 fp32 channels)
constexpr int kDmaStages = FT_DMA_STAGES;  // dma kernel: LDS ring depth

// Packed-weight layout + kernel choice. Everything here depends only on (dtype, Cin, Cout, kernel,
// transposed, x_cstride - x_coff): NOT on the batch / spatial size, so weights are packed once per layer.
struct Geometry {
  int nphases, ntaps, cin_pad, cout_pad, kpad;
  int run_taps, run_cpad;         // row-packed: kernel columns per K-run and their channel stride; else 1, cin_pad
  int dma;                        // 1: conv_igemm_dma_kernel, 0: generic conv_igemm_kernel
  int rowpack;
  int nk, cin_groups, vec, kc;    // K-loop bookkeeping of the chosen kernel
  int cin2_pad, kc2;              // second input (K-concat): its padded K-run and K-steps
};

// ---- tile_hint codec (bit layout: include/flowtrack_hip.h, next to ft_conv_desc.tile_hint) --------------------------
// The cross-workgroup K split is stored as a code: 0..3 = 1, 2, 4, 8 slices (log2), 4..7 = 3, 5, 6, 7 slices (8-phase
// kernel only: 48 tiles x 5 = 240 workgroups fill 256 CUs where x 4 leaves a quarter of them idle).
constexpr int kWide8 = 3;      // ft_conv_tile.wide == 3: the 256 x 256 tile on the 8-phase schedule (conv_igemm8.hip)

inline ft_conv_tile tile_decode(int hint) {
  const int code = (hint >> 21) & 7;
  ft_conv_tile t;
  t.bp = hint & 0xfff;
  t.bc = (hint >> 12) & 0x1ff;
  t.ks = (hint >> 24) & 0xf;
  t.sk = code < 4 ? 1 << code : (code == 4 ? 3 : code);   // 5, 6, 7 are themselves
  t.wide = (hint >> 28) & 3;
  t.halo = (hint >> 30) & 1;
  return t;
}

// the hint, or -FT_ERR_INVALID_ARG for a field that does not fit its bits
inline int tile_encode(const ft_conv_tile& t) {
  if (t.bp < 0 || t.bp > 0xfff || t.bc < 0 || t.bc > 0x1ff || t.ks < 0 || t.ks > 0xf || t.sk < 1 || t.sk > 8 || t.wide < 0 ||
      t.wide > 3 || t.halo < 0 || t.halo > 1)
    return -FT_ERR_INVALID_ARG;
  const int code = t.sk == 1 ? 0 : t.sk == 2 ? 1 : t.sk == 4 ? 2 : t.sk == 8 ? 3 : t.sk == 3 ? 4 : t.sk;
  return t.bp | (t.bc << 12) | (code << 21) | (t.ks << 24) | (t.wide << 28) | (t.halo << 30);
}

// ---- conv_igemm.hip ------------------------------------------------------------------------------------------------
// One row per tile the dma kernel is instantiated for (each with and without the residual prefetch).  `wide` = 1: the
// "wide-K" variants (fp16): 128 bytes of K per tile row per step = whole 128-byte lines per row from L2, half the barriers
// and K-steps; twice the LDS per stage, so fewer stages / workgroups per CU.
struct DmaTile {
  int dtype, bp, bc, ks, wide;
  unsigned ring;                 // bytes of the K-groups' LDS rings (the launch adds bp * 8 for the row table)
  int (*launch)(const ConvParams& p, dim3 grid, hipStream_t s);
};
const DmaTile* dma_tile_at(int i);   // row i of the table, in the order ft_conv_tile_candidates offers them; nullptr past its end
const DmaTile* find_dma_tile(int dtype, int bp, int bc, int ks, int wide);   // nullptr: no such instantiation
int launch_generic(const ConvParams& p, int dtype, int bc, dim3 grid, hipStream_t s);
// sum of the split-K partial tiles in p.ws + the fused epilogue (dma and 8-phase kernels)
int launch_splitk_reduce(const ConvParams& p, int dtype, hipStream_t s);

// ---- conv_igemm8.hip -----------------------------------------------------------------------------------------------
// The 256 x 256 tile on the 8-phase ping-pong schedule, persistent (fp16, Cin % 64 == 0, Cout_pad % 256 == 0, no second
// input, no residual; output = NHWC fp16 in 8-channel-aligned views, the fused tail's map, or split-K partials);
// p.kc / p.nk count 64-channel K-tiles, `tiles` = p.npt * p.nct * p.nph * p.sk; one workgroup of 512 threads per CU walks them.
int launch_igemm8(const ConvParams& p, unsigned tiles, hipStream_t s);

// ---- conv_igemm.hip: halo -----------------------------------------------------------------------------------------------
bool halo_ok(const ft_conv_desc* d, const Geometry& g);
int launch_halo(ConvParams p, const ft_conv_desc* d, const Geometry& g, int bc, hipStream_t s);

// ---- conv_igemm.hip: stem -----------------------------------------------------------------------------------------------
bool stem_ok(const ft_conv_desc* d, const Geometry& g);
bool shift_n_ok(const ft_conv_desc* d, const Geometry& g);
int launch_stem(ConvParams p, const ft_conv_desc* d, const Geometry& g, hipStream_t s);
int launch_stem_pool(ConvParams p, const ft_conv_desc* d, const Geometry& g, hipStream_t s);

// ---- conv_fewout.hip -------------------------------------------------------------------------------------------------------
// The forms for Cout <= 4 (matrix-pipe / LDS-patch predict_flow kernels, the few-output kernel).  Sets *taken and
// returns the launch status where one of them applies; else *taken = false and the caller goes on to the generic kernel.
int launch_fewout_forms(ConvParams p, const ft_conv_desc* d, const Geometry& g, unsigned long long x_bytes, hipStream_t s,
                        bool* taken);

}  // namespace ft
