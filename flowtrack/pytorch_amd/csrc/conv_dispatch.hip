// Host side of ft_conv2d_fwd (no kernel here): descriptor validation, the packed-weight geometry, which tile applies to which
// layer (tile_valid), the tile enumeration for the plan-build-time benchmark, and the dispatcher
//   conv2d_fwd_impl = checks -> fill_params -> the special forms (per-sample shift, pool, fused tail)
//                     -> choose_tile (heuristic, hint, workspace) -> launch_tile | the few-output forms | the generic kernel.
// The kernel families and their launch code: conv_dispatch.h.
#include "conv_dispatch.h"

namespace ft {

static int validate(const ft_conv_desc* d) {
  if (!d) return FT_ERR_INVALID_ARG;
  if (d->dtype != FT_F16 && d->dtype != FT_F32) return FT_ERR_INVALID_ARG;
  if (d->N <= 0 || d->Hi <= 0 || d->Wi <= 0 || d->Cin <= 0 || d->Cout <= 0) return FT_ERR_INVALID_ARG;
  if (d->x_wpitch > 0) {  // row-packed input
    if (d->transposed || d->x_coff != 0 || d->x_cstride % 4 || d->x_cstride < d->Cin) return FT_ERR_INVALID_ARG;
    if (d->x_lpad < d->pad || d->x_wpitch < d->x_lpad + d->Wi) return FT_ERR_INVALID_ARG;
  } else {
    if (d->x_wpitch < 0 || d->x_lpad != 0) return FT_ERR_INVALID_ARG;
    if (d->x_cstride % 8 || d->x_coff % 8 || d->x_coff < 0) return FT_ERR_INVALID_ARG;
    if (d->x_cstride < d->x_coff + round_up(d->Cin, 8)) return FT_ERR_INVALID_ARG;
  }
  if (d->transposed) {
    if (d->kh != 4 || d->kw != 4 || d->stride != 2 || d->pad != 1) return FT_ERR_UNSUPPORTED;
    if (d->Ho != 2 * d->Hi || d->Wo != 2 * d->Wi) return FT_ERR_INVALID_ARG;
  } else {
    if (d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->pad < 0) return FT_ERR_INVALID_ARG;
    if (d->Ho != (d->Hi + 2 * d->pad - d->kh) / d->stride + 1) return FT_ERR_INVALID_ARG;
    if (d->Wo != (d->Wi + 2 * d->pad - d->kw) / d->stride + 1) return FT_ERR_INVALID_ARG;
  }
  if (d->out_layout == FT_LAYOUT_NHWC) {
    if (d->y_cstride % 4 || d->y_coff % 4 || d->y_coff < 0) return FT_ERR_INVALID_ARG;
    if (d->y_cstride < d->y_coff + (d->tail_cout > 0 ? d->tail_cout : d->Cout)) return FT_ERR_INVALID_ARG;
  } else if (d->out_layout != FT_LAYOUT_NCHW_F32) {
    return FT_ERR_INVALID_ARG;
  }
  if (d->has_residual) {
    if (d->res_cstride % 4 || d->res_coff % 4 || d->res_coff < 0) return FT_ERR_INVALID_ARG;
    if (d->res_cstride < d->res_coff + d->Cout) return FT_ERR_INVALID_ARG;
  }
  if (d->act < FT_ACT_NONE || d->act > FT_ACT_LEAKY) return FT_ERR_INVALID_ARG;
  if (d->tail_cout < 0 || d->tail_cout > 32) return FT_ERR_INVALID_ARG;
  if (d->tail_cout > 0) {   // fused tail 1x1 conv: the whole channel dimension of a pixel tile must sit in one workgroup
    if (d->dtype != FT_F16 || d->has_residual || d->x2_cin != 0 || !(d->Cout == 64 || d->Cout == 128 || d->Cout == 256))
      return FT_ERR_UNSUPPORTED;
  }
  if (d->pool != 0 && d->pool != 1) return FT_ERR_INVALID_ARG;
  if (d->x2_cin < 0) return FT_ERR_INVALID_ARG;
  if (d->x2_cin > 0) {   // second input (K-concat): 1x1 / stride 1 or transposed 4x4 / stride 2 main conv, no residual, plain NHWC views
    if (!d->transposed && (d->kh != 1 || d->kw != 1 || d->stride != 1 || d->pad != 0)) return FT_ERR_UNSUPPORTED;
    if (d->has_residual || d->x_wpitch > 0) return FT_ERR_UNSUPPORTED;
    if (d->x2_stride <= 0 || d->x2_hi <= 0 || d->x2_wi <= 0 || d->x2_cstride % 8 || d->x2_coff % 8 || d->x2_coff < 0)
      return FT_ERR_INVALID_ARG;
    if (d->x2_cstride < d->x2_coff + round_up(d->x2_cin, 8)) return FT_ERR_INVALID_ARG;
    // behind a transposed conv x2 is given at the output geometry: every phase reads it at its own output pixels
    if (d->transposed && (d->x2_stride != 1 || d->x2_hi != d->Ho || d->x2_wi != d->Wo)) return FT_ERR_INVALID_ARG;
    if (d->Ho != (d->x2_hi - 1) / d->x2_stride + 1 || d->Wo != (d->x2_wi - 1) / d->x2_stride + 1) return FT_ERR_INVALID_ARG;
  }
  return FT_OK;
}

static int geometry(const ft_conv_desc* d, Geometry* g) {
  int st = validate(d);
  if (st != FT_OK) return st;
  const int esz = d->dtype == FT_F16 ? 2 : 4;
  g->vec = 16 / esz;
  g->nphases = d->transposed ? 4 : 1;
  g->ntaps = d->transposed ? 4 : d->kh * d->kw;
  const int bk = kDmaBKB / esz;
  g->rowpack = 0;
  g->cin2_pad = g->kc2 = 0;
  if (d->x_wpitch > 0) {
    // one K-run = one kernel row: kw taps x x_cstride channels, padded to whole K-steps with zero weights
    if (d->Cout <= 32 || d->kh > 32) return FT_ERR_UNSUPPORTED;
    const int run = round_up(d->kw * d->x_cstride, bk);
    if ((long long)128 * d->kh * run * esz >= (1LL << 31)) return FT_ERR_UNSUPPORTED;
    g->rowpack = g->dma = 1;
    g->ntaps = d->kh;
    g->cin_pad = run;
    g->cout_pad = round_up(d->Cout, d->Cout % 128 == 0 ? 128 : 64);
    g->kc = run / bk;
    g->nk = g->ntaps * g->kc;
    g->kpad = g->ntaps * run;
    g->cin_groups = 0;
    g->run_taps = d->kw;
    g->run_cpad = d->x_cstride;
    return FT_OK;
  }
  const int cin_bk = round_up(d->Cin, bk);
  const long long wbytes = (long long)128 * g->ntaps * cin_bk * esz;  // one co tile of packed weights
  // Cout <= 32 runs on the generic kernel (a 64-wide channel tile would idle half of it) — except 3x3/s1 layers with
  // 16..32 outputs at high resolution (FlowNetFusion inter_conv0/1): channel-aligned layout + LDS-patch (halo) kernel
  // cut their operand traffic so much that the idle half does not matter (inter_conv1: 680 -> 324 us before the patch)
  // (the transposed 16..32-output layers were tried too: fusion deconv0 578 -> 514 us, deconv1 91 -> 103 us: left alone)
  const bool small_3x3 = d->Cout >= 16 && !d->transposed && d->kh == 3 && d->kw == 3 && d->stride == 1;
  g->dma = (d->Cout > 32 || small_3x3) && g->ntaps <= 32 && d->x_cstride >= d->x_coff + cin_bk && wbytes < (1LL << 31);
  if (d->x2_cin > 0) {     // K-concat needs the channel-aligned kernel for both inputs
    const int cin2_bk = round_up(d->x2_cin, bk);
    if (!g->dma || d->x2_cstride < d->x2_coff + cin2_bk || cin_bk / bk < 2) return FT_ERR_UNSUPPORTED;
    g->cin2_pad = cin2_bk;
    g->kc2 = cin2_bk / bk;
  }
  if (g->dma) {
    g->cin_pad = cin_bk;
    g->cout_pad = round_up(d->Cout, d->Cout % 128 == 0 ? 128 : 64);
    g->kc = cin_bk / bk;
    g->nk = g->ntaps * g->kc + g->kc2;
    g->kpad = g->ntaps * cin_bk + g->cin2_pad;
    g->cin_groups = 0;
  } else {
    g->cin_pad = round_up(d->Cin, 8);
    const int bc = d->Cout <= 32 ? 32 : (d->Cout % 128 == 0 ? 128 : 64);
    g->cout_pad = round_up(d->Cout, bc);
    g->cin_groups = g->cin_pad / g->vec;
    const int ch = kBKB / 16;
    g->nk = ceil_div(g->ntaps * g->cin_groups, ch);
    g->kpad = g->nk * ch * g->vec;
    g->kc = 0;
  }
  g->run_taps = 1;
  g->run_cpad = g->cin_pad;
  return FT_OK;
}

// conv_igemm8_kernel: fp16, channel-aligned layout, 64-channel K-tiles (cin_pad % 64 == 0), all-256-channel tiles, no second input
static bool igemm8_ok(const ft_conv_desc* d, const Geometry& g) {
  if (!(g.dma && !g.rowpack && d->dtype == FT_F16 && g.kc2 == 0 && g.kc % 2 == 0 && g.cout_pad % 256 == 0 && g.nk / 2 >= 2)) return false;
  if (d->has_residual) return false;     // results leave straight from the accumulator registers: no residual pick-up
  if ((unsigned long long)g.nphases * g.cout_pad * g.kpad * 2 >= (1ull << 31)) return false;   // one buffer descriptor over all weights
  if (g.cout_pad > 1024) return false;   // folded-BN scale / shift of every output channel sit in 8 KiB of LDS
  if (d->tail_cout > 0) return d->Cout == 256 && d->tail_cout <= 24;   // (the channel halves exchange 12 registers = 24 outputs)
  if (!(d->out_layout == FT_LAYOUT_NHWC && d->Cout % 8 == 0 && d->y_coff % 8 == 0 && d->y_cstride % 8 == 0)) return false;
  return (unsigned long long)d->N * d->Ho * d->Wo * d->y_cstride * 2 < (1ull << 31);
}

static ft_conv_tile tile(int bp, int bc, int ks = 1, int wide = 0, int sk = 1, int halo = 0) {
  ft_conv_tile t;
  t.bp = bp; t.bc = bc; t.ks = ks; t.sk = sk; t.wide = wide; t.halo = halo;
  return t;
}

// Does tile `t` apply to layer `d`?  Which dma tiles exist is the table's business (find_dma_tile); here are only the
// conditions that depend on the layer.
static bool tile_valid(const ft_conv_desc* d, const Geometry& g, const ft_conv_tile& t) {
  const int bp = t.bp, bc = t.bc, ks = t.ks, sk = t.sk, wide = t.wide;
  const bool halo = t.halo != 0;
  if (!g.dma) return false;
  if (wide == kWide8) {
    if (!igemm8_ok(d, g) || bp != 256 || bc != 256 || ks != 1 || halo) return false;
    if (sk != 1) {     // every K slice = ceil(K-tiles / sk) but the last, which must still hold two K-tiles (the kernel's tile hand-over)
      const int nk8 = g.nk / 2, per = (nk8 + sk - 1) / sk;
      if (sk < 2 || sk > 8 || d->tail_cout > 0 || per < 4 || nk8 - (sk - 1) * per < 2) return false;
    }
    return true;
  }
  if (sk != 1) {     // split-K across workgroups: fp32 partial tiles in a workspace + a reduce launch
    if (!(sk == 2 || sk == 4 || sk == 8) || ks != 1 || halo || g.kc2 > 0 || d->tail_cout > 0 || g.rowpack || bp > 128) return false;
    if ((g.nk >> wide) / sk < 4) return false;
  }
  if (g.kc2 > 0) {   // K-concat runs in the lean loop only: no split-K, no halo; wide-K needs whole wide steps of both runs
    if (ks != 1 || halo) return false;
    if (wide && (g.kc2 % 2 != 0 || (g.kc >> 1) < 2)) return false;
  }
  if (halo) return halo_ok(d, g) && bp == 128 && (bc == 64 || (bc == 128 && !g.rowpack)) && g.cout_pad % bc == 0 && ks == 1 && wide == 0;
  if (!find_dma_tile(d->dtype, bp, bc, ks, wide)) return false;
  if (g.cout_pad % bc != 0) return false;
  if (bc == 256 && sk != 1) return false;
  if (wide && g.kc % 2 != 0) return false;     // whole wide K-steps
  if (ks > 1 && g.nk < 2 * ks) return false;   // (wide-K has no intra-workgroup split-K rows)
  return true;
}

// The heuristic tile for `d` (launch-time only; the packed layout does not depend on it), then the caller's benchmarked hint
// where it applies, then the fall-back of a split-K tile without its workspace.  Pure host arithmetic: nothing is launched.
static ft_conv_tile choose_tile(const ft_conv_desc* d, const Geometry& g, int M, const void* workspace, size_t workspace_bytes) {
  // fill the 256 CUs
  int bc = d->Cout % 128 == 0 ? 128 : 64;
  int bp = 128;
  auto blocks = [&](int bp_, int bc_) { return (long long)ceil_div(M, bp_) * (g.cout_pad / bc_) * g.nphases; };
  // The K-loop is bound by operand delivery L2 -> LDS (~10 TB/s chip-wide measured, same as the best GEMMs of
  // the hardware guide): bytes per MAC = (1/BP + 1/BC) * esz, so the largest tile that still fills the chip wins.
  if (d->dtype == FT_F16 && bc == 128 && g.ntaps * g.cin_pad > 512 && blocks(256, 128) >= 2 * 256) bp = 256;
  if (blocks(bp, bc) < 384) bp = 64;
  if (blocks(bp, bc) < 384 && bc == 128) bc = 64;
  // short-K layers (1x1 bottleneck exits) are HBM-bound: smaller pixel tiles = more workgroups per CU =
  // more bytes in flight (measured on MI355X, R50 shapes: 64x128 beats 128x128 by 10-18 % for K <= 512)
  if (g.ntaps * g.cin_pad <= 512 && bc == 128) bp = 64;
  // intra-workgroup split-K (the table's ks rows): few tiles + long K => take the missing waves from K, as long as every
  // workgroup still fits on the chip in ONE round (each K-group brings its own LDS ring)
  int ks = 1;
  {
    const long long nblk = blocks(bp, bc);
    const long long per_cu = (nblk + 255) / 256;
    for (int cand = 4; cand >= 2; cand >>= 1) {
      const DmaTile* row = find_dma_tile(d->dtype, bp, bc, cand, 0);
      if (row && per_cu * ((size_t)row->ring + 2048) <= 160 * 1024 && per_cu * cand * 4 <= 32 && g.nk >= 8 * cand && nblk <= 768) {
        ks = cand;
        break;
      }
    }
  }
  // few workgroups + long K: the K-loop is latency-bound (one barrier per step, <= 2 waves per SIMD), so take
  // 128 bytes of K per step instead of splitting K (measured in situ on R50 / FlowNet2S: 15-25 % on those layers)
  int wide = 0;
  if (d->dtype == FT_F16 && bp <= 128 && g.kc % 2 == 0 && g.ntaps * g.cin_pad >= 512 && blocks(bp, bc) <= 768) {
    wide = 1;
    ks = 1;
  }
  if (g.kc2 > 0) {   // K-concat: lean loop only
    ks = 1;
    if (wide && !tile_valid(d, g, tile(bp, bc, 1, wide))) wide = 0;
  }
  ft_conv_tile t = tile(bp, bc, ks, wide);
  if (d->tile_hint) {      // explicit choice: the caller's benchmarked hint; fields it leaves 0 come from the heuristic
    ft_conv_tile h = tile_decode(d->tile_hint);
    if (!h.ks) h.ks = h.bp || h.bc ? 1 : ks;
    if (!h.bp) h.bp = bp;
    if (!h.bc) h.bc = bc;
    if (tile_valid(d, g, h)) t = h;
  }
  if (t.sk > 1 && (!workspace || workspace_bytes < (size_t)t.sk * g.nphases * M * g.cout_pad * sizeof(float))) t.sk = 1;
  return t;
}

// the 256 x 256 8-phase tile, plain, split-K or with the fused tail
static int launch_igemm8_tile(ConvParams p, const ft_conv_desc* d, const Geometry& g, int sk, void* workspace, hipStream_t s) {
  const bool tail = d->tail_cout > 0;
  p.kc = g.kc >> 1;
  p.nk = g.nk >> 1;
  p.npt = ceil_div(p.M, 256);
  p.nct = g.cout_pad / 256;
  if ((long long)p.npt * p.nct * p.nph * sk > 0x7fffffffLL) return FT_ERR_UNSUPPORTED;
  p.y_bytes = tail ? 0 : (unsigned)((unsigned long long)d->N * d->Ho * d->Wo * d->y_cstride * 2);   // (the tail writes through plain pointers)
  p.w_bytes = (unsigned)((unsigned long long)g.nphases * g.cout_pad * g.kpad * 2);
  if (sk > 1) {
    p.sk = sk;
    p.ws = static_cast<float*>(workspace);
  }
  const int rc8 = launch_igemm8(p, (unsigned)(p.npt * p.nct * p.nph * sk), s);
  if (rc8 != FT_OK) return rc8;
  FT_LAUNCH_CHECK(tail ? "conv_igemm8_kernel (tail)" : "conv_igemm8_kernel");
  return sk > 1 ? launch_splitk_reduce(p, d->dtype, s) : FT_OK;
}

// Launches tile `t` (choose_tile's, or the fused tail's): the LDS-patch kernels, the 8-phase kernel or a row of the dma table.
static int launch_tile(ConvParams p, const ft_conv_desc* d, const Geometry& g, const ft_conv_tile& t, void* workspace, hipStream_t s) {
  if (t.halo) return launch_halo(p, d, g, t.bc, s);
  if (t.wide == kWide8) return launch_igemm8_tile(p, d, g, t.sk, workspace, s);
  const DmaTile* row = find_dma_tile(d->dtype, t.bp, t.bc, t.ks, t.wide);
  if (!row) return FT_ERR_UNSUPPORTED;
  p.kc = g.kc >> t.wide;
  p.kc2 = g.kc2 >> t.wide;
  p.nk = g.nk >> t.wide;
  p.npt = ceil_div(p.M, t.bp);
  p.nct = g.cout_pad / t.bc;
  if ((long long)p.npt * p.nct * p.nph * t.sk > 0x7fffffffLL) return FT_ERR_UNSUPPORTED;
  dim3 grid(p.npt * p.nct * p.nph * t.sk);
  const char* const res_saved = p.res;
  if (t.sk > 1) {          // partial tiles only: the residual belongs to the reduce launch
    p.sk = t.sk;
    p.ws = static_cast<float*>(workspace);
    p.res = nullptr;
  }
  const int rc = row->launch(p, grid, s);
  if (rc != FT_OK) return rc;
  FT_LAUNCH_CHECK(d->tail_cout > 0 ? "conv_igemm_dma_kernel (tail)" : "conv_igemm_dma_kernel");
  if (t.sk == 1) return FT_OK;
  p.res = res_saved;
  return launch_splitk_reduce(p, d->dtype, s);
}

// The kernel parameter block of `d`, as every family starts from it (the launch code sets the tile counts and its own fields).
static int fill_params(const ft_conv_desc* d, const Geometry& g, const void* x, const void* w_packed, const float* scale,
                       const float* shift, const void* residual, void* y, ConvParams* out) {
  ConvParams& p = *out;
  p.x = static_cast<const char*>(x);
  p.w = static_cast<const char*>(w_packed);
  p.scale = scale;
  p.shift = shift;
  p.res = d->has_residual ? static_cast<const char*>(residual) : nullptr;
  p.y = static_cast<char*>(y);
  const int Hq = d->transposed ? d->Hi : d->Ho;
  const int Wq = d->transposed ? d->Wi : d->Wo;
  p.M = d->N * Hq * Wq;
  p.HqWq = Hq * Wq;
  p.Wq = Wq;
  p.Hi = d->Hi;
  p.Wi = d->Wi;
  p.sy = d->transposed ? 1 : d->stride;
  p.x_cstride = d->x_cstride;
  p.x_coff = d->x_coff;
  p.kh = d->transposed ? 2 : d->kh;
  p.kw = d->transposed ? 2 : d->kw;
  p.dmul = d->transposed ? -1 : 1;
  p.pad = d->pad;
  p.pad_x = d->pad;
  p.transposed = d->transposed;
  if (g.rowpack) {      // the kernel sees a (kh x 1)-tap conv over the physically padded rows
    p.kw = 1;
    p.Wi = d->x_wpitch;
    p.pad_x = d->pad - d->x_lpad;
  }
  p.cin_groups = g.cin_groups;
  p.kc = g.kc;
  p.nk = g.nk;
  p.sk = 1;
  p.ws = nullptr;
  p.tail_w = nullptr;
  p.tail_cout = 0;
  p.x2 = nullptr;
  p.kc2 = g.kc2;
  if (g.kc2 > 0) {
    if (!residual) return FT_ERR_INVALID_ARG;
    const unsigned long long x2b = (unsigned long long)d->N * d->x2_hi * d->x2_wi * d->x2_cstride * dtype_size(d->dtype);
    if (x2b >= (1ull << 31)) return FT_ERR_UNSUPPORTED;
    p.x2 = static_cast<const char*>(residual);
    p.x2_bytes = (unsigned)x2b;
    p.x2_hi = d->x2_hi; p.x2_wi = d->x2_wi; p.x2_cstride = d->x2_cstride; p.x2_coff = d->x2_coff; p.x2_stride = d->x2_stride;
  }
  p.Kpad = g.kpad;
  p.Cout = d->Cout;
  p.Cout_pad = g.cout_pad;
  p.Ho = d->Ho;
  p.Wo = d->Wo;
  p.omul = d->transposed ? 2 : 1;
  p.y_cstride = d->y_cstride;
  p.y_coff = d->y_coff;
  p.out_layout = d->out_layout;
  p.res_cstride = d->res_cstride;
  p.res_coff = d->res_coff;
  p.act = d->act;
  p.slope = d->slope;
  p.nph = g.nphases;
  static const int dbg = dev_env_int("FT_CONV_DBG", 0);
  p.dbg = dbg;
  p.shift_n = d->shift_nstride;
  p.x_planar = 0;
  p.x_lpad = d->x_lpad;
  p.x_w = d->Wi;
  p.x_c = d->Cin;
  if (d->x_nchw_f32 != 0 && (!d->pool || !g.rowpack || d->x_cstride != 4 || d->Cin > 3 || d->dtype != FT_F16)) return FT_ERR_UNSUPPORTED;
  p.epi_lds = d->dtype == FT_F16 && d->out_layout == FT_LAYOUT_NHWC && d->Cout % 8 == 0 && d->y_coff % 8 == 0 &&
              d->y_cstride % 8 == 0 && (!d->has_residual || (d->res_coff % 8 == 0 && d->res_cstride % 8 == 0));
  return FT_OK;
}

static int conv2d_fwd_impl(const ft_conv_desc* d, const void* x, const void* w_packed, const float* scale, const float* shift,
                           const void* residual, void* y, void* workspace, size_t workspace_bytes, ft_stream_t stream) {
  Geometry g;
  int st = geometry(d, &g);
  if (st != FT_OK) return st;
  if (!x || !w_packed || !y) return FT_ERR_INVALID_ARG;
  if (d->has_residual && !residual) return FT_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w_packed) |
       reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(residual) |
       reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(shift)) & 15)
    return FT_ERR_INVALID_ARG;

  ConvParams p;
  st = fill_params(d, g, x, w_packed, scale, shift, residual, y, &p);
  if (st != FT_OK) return st;
  hipStream_t s = as_stream(stream);
  const unsigned long long x_bytes =
      (unsigned long long)d->N * d->Hi * (d->x_wpitch > 0 ? d->x_wpitch : d->Wi) * d->x_cstride * dtype_size(d->dtype);

  // ---- the three special forms ----
  if (d->shift_nstride != 0) {      // per-sample shift: straight to the persistent stem, the one kernel that reads it
    if (!shift || !shift_n_ok(d, g)) return FT_ERR_UNSUPPORTED;
    p.x_bytes = (unsigned)x_bytes;
    return launch_stem(p, d, g, s);
  }
  if (d->pool) {            // stem + max-pool: y is the pooled [N, Ho/2, Wo/2, Cout] map
    if (!g.rowpack || x_bytes >= (1ull << 31) || d->tail_cout > 0 || d->x2_cin > 0 || d->has_residual) return FT_ERR_UNSUPPORTED;
    p.x_bytes = (unsigned)x_bytes;
    p.x_planar = d->x_nchw_f32 != 0;
    if (p.x_planar) {       // the buffer descriptor then covers the fp32 planes
      const unsigned long long pb = (unsigned long long)d->N * d->Cin * d->Hi * d->Wi * 4;
      if (pb >= (1ull << 31)) return FT_ERR_UNSUPPORTED;
      p.x_bytes = (unsigned)pb;
    }
    return launch_stem_pool(p, d, g, s);
  }
  if (d->tail_cout > 0) {   // conv + fused tail 1x1 conv: 128 pixels x all Cout channels per workgroup
    if (!g.dma || g.rowpack || x_bytes >= (1ull << 31) || g.cout_pad != d->Cout) return FT_ERR_UNSUPPORTED;
    if (!residual) return FT_ERR_INVALID_ARG;
    p.x_bytes = (unsigned)x_bytes;
    p.tail_w = static_cast<const char*>(residual);
    p.tail_cout = d->tail_cout;
    p.epi_lds = 1;
    // the 128-pixel tile (two workgroups per CU) unless the hint asks for the 8-phase 256 x 256 tile; a 256-pixel wide-K dma tile
    // was tried and was slower: profiles/HISTORY.md
    const ft_conv_tile t8 = tile(256, 256, 1, kWide8);
    const bool want8 = tile_decode(d->tile_hint).wide == kWide8 && d->Cout == 256 && tile_valid(d, g, t8);
    return launch_tile(p, d, g, want8 ? t8 : tile(128, d->Cout), nullptr, s);
  }

  // ---- channel-aligned layers: one tile of the dma / 8-phase / LDS-patch kernels ----
  if (g.dma) {
    if (x_bytes >= (1ull << 31)) return FT_ERR_UNSUPPORTED;   // packed for the dma layout but the activation buffer is >= 2 GiB
    p.x_bytes = (unsigned)x_bytes;
    return launch_tile(p, d, g, choose_tile(d, g, p.M, workspace, workspace_bytes), workspace, s);
  }

  // ---- generic layout: the few-output forms, else the generic GEMM kernel ----
  bool taken;
  st = launch_fewout_forms(p, d, g, x_bytes, s, &taken);
  if (taken) return st;
  const int bc = g.cout_pad % 128 == 0 && d->Cout > 64 ? 128 : (d->Cout <= 32 ? 32 : 64);
  p.npt = ceil_div(p.M, kBP);
  p.nct = g.cout_pad / bc;
  if ((long long)p.npt * p.nct * p.nph > 0x7fffffffLL) return FT_ERR_UNSUPPORTED;
  return launch_generic(p, d->dtype, bc, dim3(p.npt * p.nct * p.nph), s);
}

}  // namespace ft

using namespace ft;

extern "C" int ft_conv_tile_decode(int hint, ft_conv_tile* out) {
  if (!out || hint < 0) return FT_ERR_INVALID_ARG;
  *out = tile_decode(hint);
  return FT_OK;
}

extern "C" int ft_conv_tile_encode(const ft_conv_tile* t) { return t ? tile_encode(*t) : -FT_ERR_INVALID_ARG; }

extern "C" int ft_conv_tile_candidates(const ft_conv_desc* d, int* hints, int max) {
  Geometry g;
  int st = geometry(d, &g);
  if (st != FT_OK) return -st;
  if (!hints || max <= 0) return -FT_ERR_INVALID_ARG;
  if (d->pool) return 0;            // one kernel
  const ft_conv_tile t8 = tile(256, 256, 1, kWide8);
  if (d->tail_cout > 0) {           // pixel tile x ALL channels: the 128-pixel 8-wave tile (the default) or the 8-phase 256 x 256 tile
    if (max < 2 || d->Cout != 256 || !tile_valid(d, g, t8)) return 0;
    hints[0] = tile_encode(tile(128, 256));
    hints[1] = tile_encode(t8);
    return 2;
  }
  int n = 0;
  auto offer = [&](const ft_conv_tile& t) {
    if (n < max && tile_valid(d, g, t)) hints[n++] = tile_encode(t);
  };
  // the dma tiles in table order: 64-byte K-steps (with their intra-workgroup split-K forms), wide-K, all-256-channel tiles
  for (int i = 0; const DmaTile* r = dma_tile_at(i); ++i)
    if (r->dtype == d->dtype) offer(tile(r->bp, r->bc, r->ks, r->wide));
  // the 8-phase 256 x 256 tile, and its cross-workgroup split-K forms where the layer has fewer such tiles than CUs
  if (n < max && tile_valid(d, g, t8)) {
    hints[n++] = tile_encode(t8);
    const int Hq8 = d->transposed ? d->Hi : d->Ho, Wq8 = d->transposed ? d->Wi : d->Wo;
    const long long nblk8 = (long long)ceil_div(d->N * Hq8 * Wq8, 256) * (g.cout_pad / 256) * g.nphases;
    for (int sk = 2; sk <= 8; sk <<= 1)
      if (nblk8 <= 160 && nblk8 * sk <= 640) offer(tile(256, 256, 1, kWide8, sk));
    // odd splits where they bring the workgroup count closer to one round of 256 CUs than the neighbouring powers of two
    // (deconv.0 of the pose head at batch 64: 48 tiles x 5 slices = 240 workgroups; x 4 = 192, x 8 = 384)
    for (int sk = 3; sk <= 7; ++sk) {
      if (sk == 4) continue;
      if (nblk8 <= 160 && nblk8 * sk > 160 && nblk8 * sk <= 272) offer(tile(256, 256, 1, kWide8, sk));
    }
  }
  // cross-workgroup split-K where the layer has less than ~one workgroup per CU even on 64-wide tiles (long K, few
  // pixels: layer4 / FlowNet conv5..6 / every deep layer at small batch).  Needs ft_conv2d_fwd_ws.
  {
    const int Hq = d->transposed ? d->Hi : d->Ho, Wq = d->transposed ? d->Wi : d->Wo;
    const long long M = (long long)d->N * Hq * Wq;
    static const int kSkTiles[3][2] = {{128, 128}, {64, 128}, {64, 64}};   // the tiles it is OFFERED on (tile_valid takes more)
    constexpr int sk_max_blocks = 256;
    for (const auto& t : kSkTiles) {
      if (g.cout_pad % t[1] != 0) continue;
      const long long nblk = (long long)ceil_div((int)M, t[0]) * (g.cout_pad / t[1]) * g.nphases;
      const int wide = tile_valid(d, g, tile(t[0], t[1], 1, 1)) ? 1 : 0;
      for (int sk = 2; sk <= 8; sk <<= 1)
        if (nblk <= sk_max_blocks && nblk * sk <= 4 * sk_max_blocks + 512) offer(tile(t[0], t[1], 1, wide, sk));
    }
  }
  for (int bc = 128; bc >= 64; bc >>= 1) offer(tile(128, bc, 1, 0, 1, 1));
  return n;
}

extern "C" int ft_conv_pack_geometry(const ft_conv_desc* d, ft_conv_geometry* out) {
  Geometry g;
  int st = geometry(d, &g);
  if (st != FT_OK) return st;
  if (!out) return FT_ERR_INVALID_ARG;
  out->nphases = g.nphases;
  out->ntaps = g.ntaps;
  out->cin_pad = g.cin_pad;
  out->cout_pad = g.cout_pad;
  out->kpad = g.kpad;
  out->run_taps = g.run_taps;
  out->run_cpad = g.run_cpad;
  out->cin2_pad = g.cin2_pad;
  return FT_OK;
}

extern "C" int ft_conv_tap_source(const ft_conv_desc* d, int phase, int tap, int sub, int* ky, int* kx) {
  Geometry g;
  int st = geometry(d, &g);
  if (st != FT_OK) return st;
  if (phase < 0 || phase >= g.nphases || tap < 0 || tap >= g.ntaps || sub < 0 || sub >= g.run_taps || !ky || !kx)
    return FT_ERR_INVALID_ARG;
  if (g.rowpack) {
    *ky = tap;
    *kx = sub;
  } else if (d->transposed) {
    // out[2q+p] takes in[q + p - t] * W[k],  k = (p == 0) ? 1 + 2t : 2t   
    const int py = phase >> 1, px = phase & 1, ty = tap >> 1, tx = tap & 1;
    *ky = py == 0 ? 1 + 2 * ty : 2 * ty;
    *kx = px == 0 ? 1 + 2 * tx : 2 * tx;
  } else {
    *ky = tap / d->kw;
    *kx = tap % d->kw;
  }
  return FT_OK;
}

extern "C" double ft_conv_flops(const ft_conv_desc* d) {
  if (validate(d) != FT_OK) return 0.0;
  const double taps = d->transposed ? 4.0 : (double)d->kh * d->kw;  // per output pixel
  return 2.0 * d->N * (double)d->Ho * d->Wo * d->Cout * ((double)d->Cin * taps + (double)d->x2_cin + (double)d->tail_cout);
}

extern "C" size_t ft_conv_workspace_bytes(const ft_conv_desc* d) {
  int hints[64];     // every form the enumeration can produce (15 + 5 + 6 + 4 + 9 + 2 = 41): nothing truncated, max_sk is the true maximum
  const int n = ft_conv_tile_candidates(d, hints, 64);
  int max_sk = 1;
  for (int i = 0; i < n; ++i) {
    const int sk = tile_decode(hints[i]).sk;
    if (sk > max_sk) max_sk = sk;
  }
  if (max_sk == 1) return 0;                 // no split-K variant is offered for this layer
  Geometry g;
  if (geometry(d, &g) != FT_OK) return 0;
  const int Hq = d->transposed ? d->Hi : d->Ho, Wq = d->transposed ? d->Wi : d->Wo;
  return (size_t)max_sk * g.nphases * d->N * Hq * Wq * g.cout_pad * sizeof(float);
}

extern "C" int ft_conv_shift_nstride_supported(const ft_conv_desc* d) {
  Geometry g;
  const int st = geometry(d, &g);
  if (st != FT_OK) return st;
  return shift_n_ok(d, g) ? FT_OK : FT_ERR_UNSUPPORTED;
}

extern "C" int ft_conv2d_fwd(const ft_conv_desc* d, const void* x, const void* w_packed,
                             const float* scale, const float* shift, const void* residual, void* y,
                             ft_stream_t stream) {
  return conv2d_fwd_impl(d, x, w_packed, scale, shift, residual, y, nullptr, 0, stream);
}

extern "C" int ft_conv2d_fwd_ws(const ft_conv_desc* d, const void* x, const void* w_packed,
                                const float* scale, const float* shift, const void* residual, void* y,
                                void* workspace, size_t workspace_bytes, ft_stream_t stream) {
  if (workspace && (reinterpret_cast<uintptr_t>(workspace) & 15)) return FT_ERR_INVALID_ARG;
  return conv2d_fwd_impl(d, x, w_packed, scale, shift, residual, y, workspace, workspace_bytes, stream);
}
