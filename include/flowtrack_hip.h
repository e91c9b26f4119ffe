/*
 * flowtrack_hip.h — C ABI of libflowtrack_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the two dense-CNN hot paths of FlowTrack
 * (pose: ResNet + 3x deconv head; flow: FlowNet2-family).  It replaces the
 * reference's operator FFI — the cffi/THC entry points that the reference
 * binds through torch.utils.ffi — and the stock torch.nn layers the reference
 * runs through cuDNN.  Conventions (differences from the reference FFI are
 * deliberate):
 *
 *   - plain device pointers + explicit sizes + a hipStream_t (as void*); no
 *     torch / THC types, no global THCState;
 *   - the caller owns every buffer, including outputs and workspaces; nothing
 *     is resized, zero-filled or freed behind the caller's back
 *     (reference: correlation_cuda.c:36-42,83-84 resizes + frees scratch);
 *   - every entry point returns an int status (FT_OK == 0) and never aborts
 *     (reference: THError("aborting") correlation_cuda.c:87-89; exit(-1)
 *     roi_pooling_kernel.cu:94-98);
 *   - all work is enqueued asynchronously on the given stream; entry points
 *     are re-entrant and hold no global state (one process per GPU).
 *
 * Reference paths are relative to /root/reference.
 */
#ifndef FLOWTRACK_HIP_H_
#define FLOWTRACK_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------- */
enum {
  FT_OK = 0,
  FT_ERR_INVALID_ARG = 1,   /* bad size / alignment / enum */
  FT_ERR_UNSUPPORTED = 2,   /* valid but not implemented for this combination */
  FT_ERR_HIP = 3,           /* a HIP runtime call failed; see ft_last_hip_error */
  FT_ERR_NO_DEVICE = 4
};

/* ---- element types / layouts --------------------------------------------- */
enum { FT_F16 = 0, FT_F32 = 1 };
enum { FT_ACT_NONE = 0, FT_ACT_RELU = 1, FT_ACT_LEAKY = 2 };
enum { FT_LAYOUT_NHWC = 0, FT_LAYOUT_NCHW_F32 = 1 };

typedef void* ft_stream_t; /* hipStream_t */

/* ---- runtime ------------------------------------------------------------- */
int ft_version(void);
const char* ft_status_string(int status);
/* text of the last HIP error seen by the calling thread ("" if none) */
const char* ft_last_hip_error(void);
/* name (<= name_len bytes incl. NUL), CU count, HBM bytes of `device` */
int ft_device_info(int device, char* name, int name_len, int* cu_count,
                   uint64_t* hbm_bytes);

/* HIP-graph capture of a launch sequence issued on `stream` through this ABI
 * (replaces per-layer host launches in the hot loop). */
int ft_graph_begin_capture(ft_stream_t stream);
int ft_graph_end_capture(ft_stream_t stream, void** graph_exec_out);
int ft_graph_launch(void* graph_exec, ft_stream_t stream);
int ft_graph_destroy(void* graph_exec);

/* hipEvent helpers so a host in any language can time work on `stream`
 * (torch.cuda.Event only sees torch's current stream). */
int ft_event_create(void** event_out);
int ft_event_record(void* event, ft_stream_t stream);
/* later work on `stream` waits for `event` (fork / join of two streams; inside a stream capture this makes the second
 * stream a parallel branch of the graph) */
int ft_stream_wait_event(ft_stream_t stream, void* event);
int ft_event_synchronize(void* event);
int ft_event_elapsed_ms(void* start, void* stop, float* ms_out);
int ft_event_destroy(void* event);
int ft_stream_synchronize(ft_stream_t stream);
/* hipMemcpyAsync(hipMemcpyDefault) on `stream`: a host loop that drives launches through this ABI (the per-frame pose runner of
 * the tracking glue, lib/tracking/net_utils.py:36-71) brings its few kB of results back without a framework call in between;
 * a pinned host buffer makes the copy asynchronous. */
int ft_memcpy_async(void* dst, const void* src, size_t bytes, ft_stream_t stream);

/* ---- P1-P7 / F1-F3: fused conv / transposed-conv (implicit GEMM on MFMA) ---
 *
 * Replaces, on the reference path, the stock layers it runs via torch/cuDNN:
 *   nn.Conv2d (+BatchNorm2d eval, +ReLU/LeakyReLU, +residual add)
 *     lib/pose/models/resnet.py:19-23, blocks.py:89-119,
 *     lib/flownet/networks/submodules.py:7-32
 *   nn.ConvTranspose2d(k=4, s=2, p=1) (+BN, +ReLU / +bias, +LeakyReLU)
 *     lib/pose/models/pose_deconv.py:19-28, submodules.py:34-38,
 *     FlowNetS.py:42-45
 *
 *   y[n, oy, ox, co] = act( scale[co] * sum_{tap,ci} x[n, iy, ix, ci] * w[co,tap,ci]
 *                           + shift[co] (+ residual[n, oy, ox, co]) )
 *
 * Activations are NHWC with an explicit channel stride/offset so producers can
 * write straight into a channel slice of a concat buffer (torch.cat in
 * FlowNetS.py:73-88 disappears).  Cin is rounded up when reading: channels
 * [Cin, cin_pad) of every pixel of x (cin_pad from ft_conv_pack_geometry, at
 * least roundup8(Cin)) must exist inside x_cstride and be zero.
 */
typedef struct ft_conv_desc {
  int dtype;       /* FT_F16 (fp16 storage, fp32 accumulate) or FT_F32 */
  int N, Hi, Wi;   /* input batch / spatial size */
  int Cin;         /* logical input channels */
  int x_cstride;   /* elements between consecutive input pixels */
  int x_coff;      /* first channel inside the pixel (multiple of 8) */
  int Cout;        /* logical output channels */
  int kh, kw;      /* kernel (transposed: must be 4,4) */
  int stride, pad; /* conv: any; transposed: must be 2,1 */
  int transposed;  /* 0 = Conv2d, 1 = ConvTranspose2d(4,2,1) */
  int Ho, Wo;      /* output spatial size (validated against the formula) */
  int y_cstride;   /* NHWC: elements between output pixels; NCHW: ignored */
  int y_coff;      /* NHWC: first output channel inside the pixel (mult of 4) */
  int out_layout;  /* FT_LAYOUT_NHWC (dtype) or FT_LAYOUT_NCHW_F32 */
  int has_residual;
  int res_cstride, res_coff; /* residual is NHWC, output geometry */
  int act;         /* FT_ACT_* */
  float slope;     /* LeakyReLU negative slope */
  /* Row-packed input (small-Cin stem layers, e.g. the 7x7/s2 convs on 3/6/12 channels): when
   * x_wpitch > 0 the input buffer is [N, Hi, x_wpitch, x_cstride] with x_lpad >= pad zero columns
   * physically present left of pixel 0 and zero columns on the right up to x_wpitch.  A whole kernel
   * ROW (kw taps x x_cstride channels, contiguous in memory) then is one K-run, so the direct-to-LDS
   * kernel applies although Cin is tiny.  0 = plain NHWC. */
  int x_lpad, x_wpitch;
  /* 0 = let the library choose the workgroup tile; else one of the values ft_conv_tile_candidates()
   * returned for this descriptor (the pick of a plan-build-time benchmark, the counterpart of the
   * reference's `cudnn.benchmark = True`, tools/pose/main.py:59).  Only the speed depends on it, never
   * the packed-weight layout; an inapplicable value falls back to the heuristic.
   * Bit layout (ft_conv_tile_decode / ft_conv_tile_encode below are the codec; a field left 0 is the heuristic's):
   *   bits  0-11  bp    pixels per workgroup tile
   *   bits 12-20  bc    output channels per workgroup tile
   *   bits 21-23  sk    cross-workgroup K split (needs ft_conv2d_fwd_ws), as a code: 0..3 = 1, 2, 4, 8 slices,
   *                     4..7 = 3, 5, 6, 7 slices (8-phase kernel only)
   *   bits 24-27  ks    intra-workgroup K split (K-groups of waves, each with its own LDS ring): 1, 2 or 4
   *   bits 28-29  wide  0 = 64 bytes of K per tile row and step, 1 = 128 ("wide-K", fp16), 3 = the 256 x 256 tile on the
   *                     8-phase schedule
   *   bit  30     halo  the LDS-resident input patch kernels (3x3 / stride 1, transposed phases, row-packed stems)
   *   bit  31     0 */
  int tile_hint;
  /* Optional SECOND input summed into the same accumulator ("K-concat"):
   *   y = act(scale .* (W1 . x + W2 . x2[n, q*x2_stride]) + shift),   W = [W1 | W2] packed along K (K-run 1 = Cin
   * channels of x, K-run 2 = x2_cin channels of x2, each padded as ft_conv_pack_geometry reports).
   * It fuses the projection shortcut of a bottleneck block (`downsample` conv + bn, lib/pose/models/blocks.py:
   * 104-119) into its conv3: the caller folds both BatchNorms into the weights (scale = NULL) and sums the shifts.
   * Requirements: 1x1 / stride 1 / pad 0 main conv, has_residual = 0 — x2 is passed in ft_conv2d_fwd's `residual`
   * argument — x2 is NHWC `dtype` [N, x2_hi, x2_wi, x2_cstride] with Ho = (x2_hi - 1) / x2_stride + 1 (same for Wo).
   * Behind a TRANSPOSED main conv (transposed = 1, the 4x4 / stride 2 / pad 1 form) the same field gives one top-down step of
   * the lateral-deconv pose head (lib/pose/models/pose_net.py:63-65) in one launch:
   *   y[n, oy, ox, :] = act(scale .* (ConvT(x)[n, oy, ox, :] + W2 . x2[n, oy, ox, :]) + shift)
   * x2 is given at the OUTPUT geometry: x2_hi = Ho, x2_wi = Wo, x2_stride = 1 (anything else: FT_ERR_INVALID_ARG).  Each of the four
   * output-parity phases is one GEMM over K = [4 taps of x | x2], kpad = 4 * cin_pad + cin2_pad per phase, and every phase's
   * packed matrix carries the same W2 block behind its four taps; phase (py, px) reads x2 at its own pixels (2 qy + py, 2 qx + px).
   * Here scale / shift are usually a BatchNorm that FOLLOWS the sum, so the caller keeps them out of the weights.
   * has_residual and tail_cout stay excluded (FT_ERR_UNSUPPORTED): all three use the `residual` argument.
   * Both forms run on the channel-aligned kernel only: x_cstride >= x_coff + Cin padded to a K-step (32 fp16 / 16 fp32 channels) of
   * at least two steps, the same for x2, Cout > 32 — FT_ERR_UNSUPPORTED otherwise.  No split-K tile is offered with a second input
   * (ft_conv_tile_candidates lists none, ft_conv_workspace_bytes is 0); a hint for a form that does not take x2 (the 8-phase
   * kernel, the LDS-patch forms, split-K) falls back to the heuristic tile.
   * x2_cin = 0: no second input. */
  int x2_cin, x2_hi, x2_wi, x2_cstride, x2_coff, x2_stride;
  /* Optional fused TAIL 1x1 conv: y = Wt . act(scale .* conv(x) + shift) + bt with tail_cout <= 32 outputs.  The
   * intermediate (all Cout channels of a pixel tile) stays in LDS and is never written: it fuses the pose head's
   * last layers, `heatmap(deconv(...))` (lib/pose/models/pose_deconv.py:43-45), and saves the round trip of the
   * largest tensor of the head.  Requirements: FT_F16, Cout in {64, 128, 256}, has_residual = 0, x2_cin = 0; the
   * tail pack — fp16 [32][Cout] weights `hi` (rows >= tail_cout zero), fp32 [32] bias, fp16 [32][Cout] `lo` with
   * w = hi + lo (the tail weights keep ~22 bits: the heatmap conv decides the arg-max), and, REQUIRED when Cout = 256
   * and `tile_hint` selects the 8-phase tile (bits 28-29 == 3; never chosen without a hint): the same weights once more in
   * that kernel's operand order, fp16 [2][8][2][64][8] = [channel half wc][step st][hi, lo][lane = lhi * 32 + tail output][e]
   * holding channel wc * 128 + st * 16 + 4 * lhi + e % 4 + 8 * (e / 4) (32 KiB; total pack 64 KiB + 128 B) — is passed in
   * ft_conv2d_fwd's `residual` argument; `y` / out_layout / y_cstride / y_coff describe the TAIL output
   * (Ho x Wo x tail_cout).  tail_cout = 0: none. */
  int tail_cout;
  /* 1: fuse the 3x3 / stride 2 / pad 1 max-pool of the ResNet stem behind the activation (resnet.py:19-23: conv1 -> bn1
   * -> relu -> maxpool).  Ho / Wo stay the CONV's output size (even); `y` is the pooled NHWC map [N, Ho/2, Wo/2, y_cstride].
   * Supported for the row-packed 7x7 / stride 2 fp16 stem with relu, 64 outputs and x_lpad >= pad + 2 (the pooled patch
   * starts one stem column further left); FT_ERR_UNSUPPORTED otherwise.  Bit-identical to conv + ft_maxpool3x3s2_fwd. */
  int pool;
  /* 0: `shift` is one vector [Cout] shared by the batch.  > 0: `shift` is [N][shift_nstride] floats, sample n takes
   * shift + n * shift_nstride — the fold of FlowNet2*'s per-sample rgb mean into conv1 (ft_flow_mean_fold below).
   * Supported by the persistent row-packed 7x7 / stride 2 fp16 stem only; FT_ERR_UNSUPPORTED elsewhere. */
  int shift_nstride;
  /* 1: `x` is the reference's NCHW fp32 network input [N, Cin, Hi, Wi] itself (Cin <= 4), not a packed copy: the stem kernel
   * gathers its input patch from the planes, casts to fp16 and lays it out in LDS exactly as ft_pack_nchw_to_nhwc would have
   * written it, so the pack launch and its [N, Hi, x_wpitch, 4] buffer disappear and the result is bit-identical.  x_cstride (4),
   * x_lpad and x_wpitch then describe that VIRTUAL row-packed view.  Supported with pool = 1 (the fp16 ResNet stem,
   * lib/pose/models/resnet.py:19-23) only; FT_ERR_UNSUPPORTED elsewhere. */
  int x_nchw_f32;
} ft_conv_desc;

/* Packed-weight geometry (ft_conv_pack_geometry): w_packed is [nphases][cout_pad][kpad] of d->dtype,
 * zeros in all padding, and the element for (tap, sub, ci) sits at k = tap*cin_pad + sub*run_cpad + ci.
 * Plain layers: run_taps = 1 (sub = 0), tap = kernel element.  Row-packed layers: tap = kernel row,
 * sub = kernel column (run_taps = kw, run_cpad = x_cstride). ft_conv_tap_source maps (phase,tap,sub)
 * to the reference kernel element (ky,kx). */
typedef struct ft_conv_geometry {
  int nphases;   /* 1 conv, 4 transposed conv (one 2x2 conv per output parity) */
  int ntaps;     /* K-runs per phase */
  int cin_pad;   /* elements per K-run (channels padded; row-packed: roundup(kw * x_cstride)) */
  int cout_pad, kpad;
  int run_taps, run_cpad;
  int cin2_pad;  /* elements of the second input's K-run (x2_cin padded), 0 without one; kpad = ntaps * cin_pad + cin2_pad */
} ft_conv_geometry;

/* The layout depends only on (dtype, Cin, Cout, kernel, transposed, x_cstride - x_coff, row-packing):
 * when the input view has room for roundup(Cin, 32 fp16 / 16 fp32) channels per pixel (padding
 * channels zero) - or is row-packed - the direct-to-LDS kernel is used and every K-run is padded to
 * that multiple; otherwise cin_pad = roundup(Cin, 8) and the generic kernel runs. */
int ft_conv_pack_geometry(const ft_conv_desc* d, ft_conv_geometry* out);
/* Which original kernel element (ky, kx) element `sub` of K-run `tap` of phase `phase` reads. */
int ft_conv_tap_source(const ft_conv_desc* d, int phase, int tap, int sub, int* ky, int* kx);
/* scale/shift: float[Cout_pad] or NULL (=> 1 / 0). residual may be NULL. */
int ft_conv2d_fwd(const ft_conv_desc* d, const void* x, const void* w_packed,
                  const float* scale, const float* shift, const void* residual,
                  void* y, ft_stream_t stream);
/* Same as ft_conv2d_fwd with a scratch buffer (>= ft_conv_workspace_bytes(d), 16-byte aligned, contents don't care):
 * unlocks the tile variants that split K across workgroups (fp32 partial tiles in the workspace + a reduce launch) for
 * layers with few pixels and a long K (layer4, FlowNet conv5..6, every deep layer at small batch).  Without a
 * workspace those hints fall back to the unsplit variant of the same tile. */
int ft_conv2d_fwd_ws(const ft_conv_desc* d, const void* x, const void* w_packed,
                     const float* scale, const float* shift, const void* residual,
                     void* y, void* workspace, size_t workspace_bytes, ft_stream_t stream);
size_t ft_conv_workspace_bytes(const ft_conv_desc* d);
/* Writes up to `max` valid `tile_hint` values for `d` (pixel tile x channel tile x split-K variants of
 * the implicit-GEMM kernel) into hints[] and returns their count (0: the layer runs on a kernel without
 * tile variants); negative = error status. */
int ft_conv_tile_candidates(const ft_conv_desc* d, int* hints, int max);
/* The fields of a `tile_hint` (layout: ft_conv_desc.tile_hint).  `sk` is the slice count 1..8, not its code. */
typedef struct ft_conv_tile { int bp, bc, ks, sk, wide, halo; } ft_conv_tile;
/* FT_OK, or FT_ERR_INVALID_ARG for out == NULL or a negative hint. */
int ft_conv_tile_decode(int hint, ft_conv_tile* out);
/* The hint, or -FT_ERR_INVALID_ARG for a field that does not fit its bits (bp > 4095, bc > 511, ks > 15, sk outside 1..8,
 * wide > 3, halo > 1, anything negative).  Whether the tile applies to a layer is ft_conv_tile_candidates' business. */
int ft_conv_tile_encode(const ft_conv_tile* t);
/* algorithmic FLOPs (2*MACs, unpadded) of one ft_conv2d_fwd call */
double ft_conv_flops(const ft_conv_desc* d);

/* ---- 1x1 convolutions of the deep, small-map stages: weight-streaming GEMM, weights straight to registers ----------
 * Same math as ft_conv2d_fwd for a 1x1 / stride 1 / pad 0 fp16 NHWC layer (optionally with the K-concat second input
 * x2_* or an identity residual), for layers with few pixels and long K (ResNet layer3/4 at batch 64, blocks.py:89,95,
 * 98-103): a workgroup owns 96 pixels, the pixel operand streams through an LDS ring, each wave loads its weight
 * fragments from a fragment-ordered stream directly into registers (csrc/conv_direct.hip).
 * The same five entry points also carry the other weight-streaming / weight-stationary forms (each with its own stream layout,
 * told apart by ft_conv_direct_stream_id): 3x3 / stride 1 and 2 on whole small maps or row strips (512 / 1024 channels: ResNet
 * layer4's conv2, blocks.py:92-95; FlowNet conv5 .. conv6_1, FlowNetS.py:27-32), the 3x3 gather form, the persistent K = 256
 * form, and — round 4 — the REGISTER-STATIONARY 5x5 / stride 2 / pad 2 form on 64 input channels with Cout % 64 == 0 (FlowNet's
 * conv2, FlowNetS.py:21: csrc/conv_wstat.hip; plain NHWC fp16 input and output, no residual / second input).
 *   ft_conv_direct_supported     FT_OK when the shape qualifies (1x1: Cin, x2_cin multiples of 64, Cout multiple of 256 — or
 *                                Cin, x2_cin multiples of 256 and Cout of 64 for the K-split form)
 *   ft_conv_direct_weight_bytes  size of the weight stream
 *   ft_conv_direct_pack          builds it from the ft_conv_pack_geometry layout w_packed [cout_pad][kpad] (once per weight set)
 *   ft_conv_direct_fwd           arguments as ft_conv2d_fwd (residual = identity residual or the second input x2)
 *   ft_conv_direct_stream_id     identifies the stream LAYOUT `d` needs (>= 0; -1 when unsupported).  The kernel form — and
 *                                with it the fragment order of the stream — depends on the pixel count N * Ho * Wo, not only on
 *                                the weights: a stream packed for one descriptor may be passed to ft_conv_direct_fwd with
 *                                another descriptor only when both report the same id (all layouts of a layer have the same
 *                                byte count, so the size does not tell them apart). */
int ft_conv_direct_supported(const ft_conv_desc* d);
int ft_conv_direct_stream_id(const ft_conv_desc* d);
long long ft_conv_direct_weight_bytes(const ft_conv_desc* d);
int ft_conv_direct_pack(const ft_conv_desc* d, const void* w_packed, int kpad, int cout_pad, void* wstream, ft_stream_t stream);
int ft_conv_direct_fwd(const ft_conv_desc* d, const void* x, const void* wstream, const float* scale, const float* shift,
                       const void* residual, void* y, ft_stream_t stream);

/* ---- whole-bottleneck fusion (fp16) --------------------------------------------------------------
 * One launch for an identity-shortcut Bottleneck (reference: Bottleneck.forward, lib/pose/models/blocks.py:105-120,
 * the blocks whose `downsample` is empty, resnet.py:29-36):
 *   y = relu(bn3(conv3_1x1(relu(bn2(conv2_3x3(relu(bn1(conv1_1x1(x)))))))) + x)
 * t1 / t2 live in LDS only; x is read once (+ halo / residual re-reads from L2), y written once.
 * Supported: dtype FT_F16, C = 256, P = 64, stride 1 (ResNet layer1.1+); y must not alias x.
 * w1 / w2 / w3 are the ft_conv_pack_geometry layouts of the three convs on channel-aligned views
 * ([64][256], [64][9*64] with k = (ky*3+kx)*64 + ci, [256][64]); scale_shift = the three folded BatchNorms as one
 * float[2P + 2P + 2C] table: scale1[P] shift1[P] scale2[P] shift2[P] scale3[C] shift3[C]. */
typedef struct ft_bottleneck_desc {
  int dtype;
  int N, H, W;            /* block input = output size */
  int C, P;               /* block width (in = out channels) and planes */
  int x_cstride, x_coff;  /* NHWC views, element units, multiples of 8 */
  int y_cstride, y_coff;
  int head_only;          /* 1: conv1 + conv2 only, y = t2 [N,H,W,P] (C = 64: the stage's entry block, whose conv3 is
                             K-concatenated with its projection shortcut by ft_conv2d_fwd); w3 = NULL,
                             scale_shift = float[4P] */
  int projection;         /* 1: the stage's entry block WHOLE (blocks.py:104-119 with `downsample`): C = 64 input channels,
                             y = relu(bn3(conv3(t2)) + bn_d(conv_d(x))) [N,H,W,4P]; w3 = [4P][P | C] fp16, the two 1x1
                             convs K-concatenated with their BatchNorm scales folded in (the layout ft_conv2d_fwd's x2_*
                             path takes), scale_shift = float[4P + 8P]: {s1 b1 s2 b2} then scale3 = 1, shift3 = b3 + b_d */
  int stride;             /* stride of conv2 (0 / 1 = 1).  2 only with head_only in the streamed-weights form
                             (ft_bottleneck_stream_*: P = 256, C = 512, even H and W: layer3.0 of the ResNets, resnet.py:44-49):
                             y = t2 [N, H/2, W/2, P]; weight stream = w1 [P][C] then w2 [P][9P]; tables = float[6][2P] of
                             which {scale1, shift1} {scale2, shift2} are read.  (Appended in round 3: zero-initialised
                             descriptors of older callers keep their meaning.) */
  int folded;             /* ft_bottleneck_stream_fwd only (round 6; see ft_bottleneck_stream_folds).  1: the weight stream was packed
                             from weights with the BatchNorm SCALE already folded in (fp16(w * scale[co]), one rounding from the fp32
                             weights) and `tables` is NOT float[6][2P] but uint32 [P + P + C]: shift1, shift2, shift3 as (hi, lo) fp16
                             pairs, hi = fp16(shift) in bits 0-15, lo = fp16(shift - hi) in bits 16-31.  The kernels add the shift and
                             the identity residual as extra MFMA k-steps and their epilogues are fp16(relu(acc)).  0 = the scale /
                             shift tables of round 2. */
  int wfrag;              /* ft_bottleneck_fwd / ft_bottleneck_exit_fwd only (appended: zero-initialised descriptors of older callers keep
                             their meaning).  0: w1 / w2 / w3 are the three ft_conv_pack_geometry layouts.  1: w1 is the ONE
                             fragment-ordered stream ft_bottleneck_frag_pack built from them and w2 = w3 = NULL; the launch then takes
                             its weights from L2 straight to registers.  Same fp16 values, same accumulation order: bit-identical
                             outputs.  Not with head_only (FT_ERR_UNSUPPORTED). */
} ft_bottleneck_desc;
int ft_bottleneck_supported(const ft_bottleneck_desc* d);   /* FT_OK or FT_ERR_UNSUPPORTED / FT_ERR_INVALID_ARG */
int ft_bottleneck_fwd(const ft_bottleneck_desc* d, const void* x,
                      const void* w1, const void* w2, const void* w3,
                      const float* scale_shift, void* y, ft_stream_t stream);
/* algorithmic FLOPs of the three convs (2*MACs, no halo recompute) */
double ft_bottleneck_flops(const ft_bottleneck_desc* d);
/* The weight stream of ft_bottleneck_desc.wfrag = 1, built once per weight set.  It is a sequence of 1-KiB fragments in the order a
 * wave reads them; a fragment is the A operand of one mfma_f32_32x32x16_f16: 64 lanes x 16 bytes, lane l holds row 32 * tile + l % 32
 * of a weight block, the eight k from 16 * slice + 8 * (l / 32).  With nch = C / 64:
 *   W1  [chunk nch][tile 2][slice 4]    rows = output channels of conv1, k = 64 * chunk + ...
 *   W2  [tap 9][tile 2][slice 4]        rows = output channels of conv2, k = 64 * tap + ...
 *   W3  [quarter 4][tile 2][slice 4]    rows = 64 * quarter + 32 * tile + ... of conv3; projection = 1: [quarter 4][tile 2][8], the
 *                                       four slices of W3' (k 0..63 of the K-concatenated rows), then the four of Wd' (k 64..127)
 * ft_bottleneck_frag_bytes = 1024 * (8 nch + 72 + 32) = 139 264 for C = 256, 1024 * (8 + 72 + 64) = 147 456 with projection = 1;
 * 0 when the descriptor has no stream form (unsupported, or head_only).  ft_bottleneck_frag_pack takes w1 / w2 / w3 exactly as
 * ft_bottleneck_fwd with wfrag = 0 does and copies the fp16 values unchanged. */
long long ft_bottleneck_frag_bytes(const ft_bottleneck_desc* d);
int ft_bottleneck_frag_pack(const ft_bottleneck_desc* d, const void* w1, const void* w2, const void* w3, void* out, ft_stream_t stream);

/* Exit form of ft_bottleneck_fwd for a stage's LAST identity block (fp16, C = 256, P = 64, even H and W): the same block plus the
 * 1x1 conv + bn + relu that opens the next stage (layer2.0.conv1 of the ResNets, 256 -> tail_cout = 128, resnet.py:37-43) in one
 * launch.  Every 64-channel quarter of y is multiplied by its K-slice of the tail weights while it sits in LDS; t1 [N,H,W,128]
 * (view t1_cstride / t1_coff, element units, multiples of 8) holds the same roundings as ft_bottleneck_fwd followed by the conv on y:
 * only the fp32 summation order differs.  y_mode says what is written of y itself:
 *   FT_BNK_Y_FULL  [N,H,W,C] as ft_bottleneck_fwd
 *   FT_BNK_Y_EVEN  the even-row, even-column pixels only, compact: y = [N, H/2, W/2, C] with d->y_cstride / y_coff (what a
 *                  stride-2 1x1 shortcut reads)
 *   FT_BNK_Y_NONE  nothing (y may be NULL)
 *   ft_bottleneck_exit_weight_bytes  size of the packed tail stream (0 when unsupported)
 *   ft_bottleneck_exit_pack          builds it from the tail conv's ft_conv_pack_geometry layout ([cout_pad][kpad] fp16); once per
 *                                    weight set
 *   ft_bottleneck_exit_fwd           w1 / w2 / w3 / scale_shift as ft_bottleneck_fwd; tail_scale / tail_shift = the tail's folded
 *                                    BatchNorm, float[tail_cout] each; t1 must alias neither x nor y. */
enum { FT_BNK_Y_FULL = 0, FT_BNK_Y_EVEN = 1, FT_BNK_Y_NONE = 2 };
int ft_bottleneck_exit_supported(const ft_bottleneck_desc* d, int tail_cout, int t1_cstride, int t1_coff, int y_mode);
long long ft_bottleneck_exit_weight_bytes(const ft_bottleneck_desc* d, int tail_cout);
int ft_bottleneck_exit_pack(const ft_bottleneck_desc* d, int tail_cout, const void* wt_packed, int kpad, int cout_pad, void* wstream,
                            ft_stream_t stream);
int ft_bottleneck_exit_fwd(const ft_bottleneck_desc* d, const void* x, const void* w1, const void* w2, const void* w3,
                           const float* scale_shift, void* y, int y_mode, int tail_cout, const void* tail_wstream,
                           const float* tail_scale, const float* tail_shift, void* t1, int t1_cstride, int t1_coff,
                           ft_stream_t stream);

/* Streamed-weights form of the same fusion for the 128- and 256-plane stages (fp16, C = 4P, P = 128 or 256, stride 1,
 * head_only = 0; ResNet layer2.1+ / layer3.1+): a workgroup owns a full-width strip of output rows of one image, keeps
 * t1 / t2 in LDS and streams the block's weights once through an LDS ring (csrc/bottleneck_stream.hip).
 *   ft_bottleneck_stream_weight_bytes  size of the packed weight stream (0 when unsupported)
 *   ft_bottleneck_stream_pack          builds it from the three convs' ft_conv_pack_geometry layouts
 *                                      (w1 [P][C], w2 [P][9P] with k = (ky*3+kx)*P + ci, w3 [C][P]); once per weight set
 *   ft_bottleneck_stream_fwd           tables = float[6][2P]: {scale1, shift1} {scale2, shift2} then {scale3, shift3} of
 *                                      output channels [qP, qP+P) for q = 0..3 (d->folded = 0), or the shift pairs described at
 *                                      ft_bottleneck_desc.folded; y must not alias x. */
int ft_bottleneck_stream_supported(const ft_bottleneck_desc* d);
/* 1 when ft_bottleneck_stream_fwd takes the FOLDED operands for this block (d->folded = 1; every stride-1 identity block), 0 when only
 * the table form exists (the stride-2 head); the value of d->folded itself is ignored. */
int ft_bottleneck_stream_folds(const ft_bottleneck_desc* d);
/* Fragment order of the weight stream that ft_bottleneck_stream_pack writes and ft_bottleneck_stream_fwd reads for this descriptor
 * (d->folded counts) under the current developer switches: 0 = 32-channel tiles in K16 slices (every 32-pixel kernel), 1 = 16-channel
 * tiles in K32 slices (the 256-plane kernel on 16-pixel MFMA tiles), -1 = unsupported.  Same byte count either way.  A stream packed
 * for one order must not be fed to a launch that plans the other: callers that cache streams key them by this value. */
int ft_bottleneck_stream_layout(const ft_bottleneck_desc* d);
/* Kernel form that ft_bottleneck_stream_fwd launches for this descriptor (d->folded counts) under the current developer switches, -1 =
 * unsupported: 0 / 5 = the 128-plane ring kernel on large (<= 192 output pixels) / small (<= 128) strips, 7 / 8 = the 128-plane kernel
 * with the weights straight to registers on the same strips (folded operands only; reads the same stream as 0 / 5), 1 / 2 / 3 = the
 * 256-plane 32-pixel kernels (96- / 64-pixel strips, column split), 6 = the 256-plane kernel on 16-pixel tiles, 4 = the stride-2 head.
 * For tests and tools: ft_bottleneck_stream_layout cannot tell forms apart that share a stream. */
int ft_bottleneck_stream_variant(const ft_bottleneck_desc* d);
long long ft_bottleneck_stream_weight_bytes(const ft_bottleneck_desc* d);
int ft_bottleneck_stream_pack(const ft_bottleneck_desc* d, const void* w1, const void* w2, const void* w3, void* wstream,
                              ft_stream_t stream);
int ft_bottleneck_stream_fwd(const ft_bottleneck_desc* d, const void* x, const void* wstream, const float* tables, void* y,
                             ft_stream_t stream);

/* ---- layout / pooling helpers -------------------------------------------- */
/* NCHW fp32 [N,C,H,W] -> NHWC `dtype` [N,H,wpitch,cpad]: pixel x lands in column lpad + x, channels
 * >= C and all other columns are zeroed (wpitch = W, lpad = 0: plain NHWC; cpad multiple of 4).
 * First step of DeconvResnet.forward (pose_deconv.py:32-33). */
int ft_pack_nchw_to_nhwc(const float* x, void* y, int N, int C, int H, int W,
                         int cpad, int lpad, int wpitch, int dtype,
                         ft_stream_t stream);
/* NHWC `dtype` (channel stride/offset) -> NCHW fp32 */
int ft_unpack_nhwc_to_nchw(const void* x, float* y, int N, int C, int H, int W,
                           int x_cstride, int x_coff, int dtype,
                           ft_stream_t stream);
/* nn.MaxPool2d(3, 2, 1) on NHWC (resnet.py:23); C multiple of 8; padding is -inf, a NaN in the window gives NaN */
int ft_maxpool3x3s2_fwd(const void* x, void* y, int N, int Hi, int Wi, int C,
                        int dtype, ft_stream_t stream);

/* ---- P4: BatchNorm2d batch statistics -----------------------------------------
 * Per-channel mean and BIASED variance over N*H*W of an NHWC view (C and x_cstride multiples of 8) — the
 * reduction nn.BatchNorm2d performs in training mode (tools/pose/main.py:207,342; running-stat
 * recalibration).  The inference path does not need it (eval-mode BN is folded into ft_conv2d_fwd).
 * workspace: float[2*C] scratch (zeroed by the call); mean, var: float[C]. */
int ft_bn_batch_stats(const void* x, int N, int H, int W, int C, int x_cstride, int dtype,
                      float* workspace, float* mean, float* var, ft_stream_t stream);

/* ---- P8/P9: heatmap -> keypoints ------------------------------------------
 * max_preds + the adjust_coords nudge of final_preds
 * (lib/pose/utils/evaluation.py:11-35): per (n,k) map the arg-max over H*W
 * (first occurrence on ties), x = idx % W, y = idx / W (integer floor, torch
 * 0.4 semantics), coords zeroed where score <= 0, optional +/-0.25 px nudge.
 * heatmaps: NCHW fp32 [N,K,H,W]; idx int32 [N*K]; score fp32 [N*K];
 * coords fp32 [N*K*2] (x,y in heatmap pixels, before transform_preds).
 * NaN is outside what the reference defines; the kernel promises only this: a NaN
 * is never the arg-max, and a map of nothing but NaN gives idx 0 and coords (0, 0). */
int ft_heatmap_max_preds(const float* heatmaps, int N, int K, int H, int W,
                         int adjust_coords, int32_t* idx, float* score,
                         float* coords, ft_stream_t stream);
/* The same launch with the key points written as rows (x, y, score): rows fp32
 * [N*K*3] — the layout the tracking glue and the multi-GPU gather consume
 * (lib/tracking/net_utils.py: `preds` and `maxvals` concatenated), so no
 * concat launch follows the network. */
int ft_heatmap_keypoint_rows(const float* heatmaps, int N, int K, int H, int W,
                             int adjust_coords, int32_t* idx, float* rows,
                             ft_stream_t stream);

/* ---- flip test (reference tools/pose/main.py:289-299): the mirrored input, and the merge of the two passes ----
 * y[n,c,h,w] = x[n,c,h,W-1-w]; NCHW fp32; x and y must not overlap.  The mirrored input of the flip test
 * (tools/pose/main.py:289-291 of the reference).  16-byte loads and reversed 16-byte stores when W % 4 == 0 and both
 * pointers are 16-byte aligned, scalar otherwise. */
int ft_hflip_nchw_f32(const float* x, float* y, int N, int C, int H, int W, ft_stream_t stream);

/* Flip-test merge + max_preds in one launch (reference tools/pose/main.py:289-299, evaluation.py:11-35).
 *   merged[n,k,y,x] = (hm[n,k,y,x] + hm_flip[n,perm[k],y,W-1-x]) * 0.5f     -- exactly these two fp32 roundings
 * hm, hm_flip: NCHW fp32 [N,K,H,W] (plain pass / pass on the mirrored input).
 * perm: DEVICE int32[K], NULL = identity; an entry outside [0,K) is read as k itself (never an out-of-range read).
 * merged (fp32 [N,K,H,W]), idx (int32 [N*K]) and rows (fp32 [N*K*3] = x, y, score) may each be NULL, but not all
 * three, and idx and rows only together.  idx / rows are ft_heatmap_keypoint_rows of `merged`, including
 * adjust_coords and the NaN promise.  merged must not alias hm or hm_flip. */
int ft_heatmap_flip_merge(const float* hm, const float* hm_flip, const int32_t* perm, int N, int K, int H, int W,
                          int adjust_coords, float* merged, int32_t* idx, float* rows, ft_stream_t stream);

/* Arg-max margin screen of the fast (fp16) mode: min_margin[n] = min over the K maps of crop n of (largest - second largest
 * value, at different pixels; 0 for a tie).  A crop whose min_margin exceeds twice the heat-map error bound of the fp16
 * arithmetic has the same arg-max in every map as the fp32 parity mode (max_preds, evaluation.py:11-20); the others are the
 * ones a caller re-runs in fp32 (DeconvResnet.forward_keypoint_rows_exact).  heatmaps NCHW fp32 [N,K,H,W], min_margin fp32 [N]. */
int ft_heatmap_min_margin(const float* heatmaps, int N, int K, int H, int W, float* min_margin, ft_stream_t stream);

/* The same screen with a RELATIVE bound and the two cases the margin alone misses.  Per crop n: R = largest - smallest value
 * over its K maps, E = rel_bound * R (the fp16 mode's heat-map error scales with the maps' range); flags[n] = 1 when some map
 * has (top1 - top2) < 2 E (two values an error of E per element can reorder), or |top1| < E (max_preds zeroes the coordinates
 * where score <= 0, lib/pose/utils/evaluation.py:17-19: that mask can flip), or any non-finite value (NaN compares false: the
 * tests are written negated).  stats fp32 [N,4] = (smallest margin, R, smallest |top1|, E); flags int32 [N]; K <= 256. */
int ft_heatmap_argmax_screen(const float* heatmaps, int N, int K, int H, int W, float rel_bound, int32_t* flags, float* stats,
                             ft_stream_t stream);

/* The re-run set of that screen, built ON THE DEVICE (round 5; DeconvResnet.exact_submit / exact_finish): header[0] = number
 * of set flags, header[1 + j] = index of the j-th flagged row, and row idx[j] of `src` ([N] rows of row_bytes, a multiple of
 * 16) is copied to row j of `dst`.  No host read sits between the screen and the gather: the host looks at `header` one step
 * later, behind an event, and only then decides whether a re-run is needed.  N <= 1024; header: int32 [1 + N]. */
int ft_gather_flagged_rows(const int32_t* flags, int N, const void* src, long long row_bytes, void* dst, int32_t* header,
                           ft_stream_t stream);

/* ---- F1: FlowNet2* input normalisation ------------------------------------
 * rgb_mean over (pair,H,W) per (b,colour) then (x - mean) / rgb_max
 * (lib/flownet/model/models.py:255-257).  inputs: fp32 [B,3,2,H,W].
 * partial: float workspace [B*3*FT_RGB_MEAN_SPLITS]; mean: float [B*3]. */
#define FT_RGB_MEAN_SPLITS 64
int ft_flow_rgb_mean(const float* inputs, int B, int H, int W, float* partial,
                     float* mean, ft_stream_t stream);
/* mode 0: y = NHWC [B,H,wpitch,8]   channels (r0,g0,b0,r1,g1,b1,0,0)   (FlowNet2S)
 * mode 1: y = NHWC [2B,H,wpitch,4]  images 0..B-1 = frame0, B..2B-1 = frame1,
 *         channels (r,g,b,0)                           (FlowNetC siamese trunk)
 * pixel x lands in column lpad + x; the other columns are zeroed (wpitch = W, lpad = 0: plain). */
int ft_flow_pack_pair(const float* inputs, const float* mean, float rgb_max,
                      void* y, int B, int H, int W, int mode, int lpad,
                      int wpitch, int dtype, ft_stream_t stream);

/* The two calls above as ONE launch, writing the 6-channel (mode 0) view y [B,H,wpitch,8] and / or the siamese (mode 1) view y3
 * [2B,H,wpitch3,4] (either may be NULL): every workgroup keeps its rows of the sample in registers
 * across the mean reduction (partial sums exchanged as tagged 8-byte words in `state`), so the frame pair is read once
 * (lib/flownet/model/models.py:255-257).  `state`: ft_flow_mean_pack_pair_state_words(B, H, W) 8-byte words (0 = the shape is not
 * covered: W % 4 != 0, more than 42 x 6144 pixels per frame, or more than 512 workgroups = B x ceil(H x W / 6144) so that not
 * all of them would be resident while they wait for each other -> use the two calls), zeroed ONCE by the caller at allocation and
 * private to this (B, H, W) from then on; its last word becomes non-zero if a workgroup ever timed out waiting for its sample's
 * sums (means are NaN then).  mean fp32 [B*3] is written as well.  Same arithmetic per element as ft_flow_pack_pair; the mean's
 * summation order differs from ft_flow_rgb_mean's (last-bit differences). */
/* The mean folded into conv1 (FlowNet2S; lib/flownet/model/models.py:255-257 + FlowNetS.py:20 as ONE pass over the frames):
 * conv_zero-padded((x - mean) / rgb_max) = conv_mean-padded(x / rgb_max) - (mean / rgb_max) . sum of the kernel, so
 *  (1) ft_flow_pack_pair_sums writes the UN-centred pair y = fp16 [B, H + 2 pad, wpitch, 8] (pixel (yy, xx) at row pad + yy,
 *      column pad + xx, channels (r0,g0,b0,r1,g1,b1,0,0) = x / rgb_max; padding pixels untouched) and per-chunk colour sums
 *      partial fp32 [B*3][ft_flow_pack_pair_sums_chunks(H)] in the same pass (no dependency on the mean: the mean launch and
 *      its second read of the frames disappear);
 *  (2) ft_flow_mean_fold finishes the mean (fixed summation order), fills y's padding pixels with m16 = fp16(mean / rgb_max)
 *      per colour (the reference's zero padding of the centred input) and writes the per-sample shift
 *      shift_n[b][co] = shift[co] - scale[co] * sum_c m16[c % 3] * wsum[co][c]   (scale NULL = 1)
 *      with wsum fp32 [Cout][8] = the fp16-rounded conv1 weights summed over the kernel window per input channel;
 *  (3) conv1 runs as a pad-0 conv on the (H + 2 pad) x (W + 2 pad) row-packed view with ft_conv_desc.shift_nstride = Cout.
 * Differences from the two-launch path: the input is rounded to fp16 before the mean is removed (|x / rgb_max| <= 1 instead
 * of <= 0.5: one more bit of input rounding), and mean / rgb_max enters as its fp16 value.  W % 4 == 0, FT_F16 only. */
#define FT_PACK_SUMS_ROWS 4
int ft_conv_shift_nstride_supported(const ft_conv_desc* d);   /* FT_OK when ft_conv2d_fwd takes `d` with its shift_nstride */
long long ft_flow_pack_pair_sums_chunks(int H);
int ft_flow_pack_pair_sums(const float* inputs, float rgb_max, void* y, int B, int H, int W, int pad, int wpitch, int dtype,
                           float* partial, ft_stream_t stream);
int ft_flow_mean_fold(const float* partial, float rgb_max, void* y, int B, int H, int W, int pad, int wpitch, int dtype,
                      const float* wsum, const float* scale, const float* shift, int Cout, float* shift_n, float* mean,
                      ft_stream_t stream);

long long ft_flow_mean_pack_pair_state_words(int B, int H, int W);
int ft_flow_mean_pack_pair(const float* inputs, float rgb_max, void* y, int lpad, int wpitch, void* y3, int lpad3, int wpitch3,
                           int B, int H, int W, int dtype, unsigned long long* state, float* mean, ft_stream_t stream);

/* ---- F7: nn.Upsample(scale_factor=4, mode='bilinear') * mul ----------------
 * (FlowNetS.py:58, models.py:292; align_corners=False).  NCHW fp32 in/out. */
int ft_upsample_bilinear4x(const float* x, float* y, int N, int C, int h, int w,
                           float mul, ft_stream_t stream);

/* ---- FPN head: F.upsample(x, size=(ho, wo), mode='bilinear', align_corners=True) * scale ----
 * (lib/pose/models/pose_fpn.py:9-26, the resize inside _upsample_add).  NHWC `dtype` in, NHWC `dtype` out:
 *   y[n, oy, ox, c] = scale[c] * bilerp_ac(x[n, :, :, c], oy, ox)      c in [0, C); scale fp32 [C], NULL = 1
 * with torch's coordinate rule for float inputs, restated exactly (all of it in fp32):
 *   rh  = ho > 1 ? (float)(hi - 1) / (ho - 1) : 0        src = rh * oy
 *   i0  = (int)src          i1 = i0 + (i0 < hi - 1)      l1 = src - i0      l0 = 1 - l1
 * the same along x, and with a, b = row i0 at columns j0, j1 and c, d = row i1 at columns j0, j1
 *   bilerp_ac = l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d)
 * Arithmetic is fp32 (a product and the sum behind it may be one fused multiply-add); the result is rounded once, on store.
 * x_cstride / x_coff and y_cstride / y_coff as in ft_conv_desc: channel c of a pixel sits at element pixel * cstride + coff + c.
 * Channels [C, y_cstride - y_coff) of an output pixel, and everything in front of y_coff, stay untouched.
 * One thread per (output pixel, 16-byte channel group: 8 fp16 / 4 fp32 channels), so both offsets and both strides must be
 * multiples of that group and x, y 16-byte aligned (FT_ERR_INVALID_ARG otherwise, as for sizes <= 0); C itself may be any
 * positive number (a last partial group goes element by element).  x and y must not overlap.  No cap on N: the grid strides.
 * FT_ERR_UNSUPPORTED for a side above 2^24, where fp32 source coordinates stop being exact at the far end, and for an output
 * row of 2^31 or more channel groups (wo x ceil(C / group)). */
int ft_upsample_bilinear_ac_fwd(const void* x, void* y, int dtype, int N, int C, int hi, int wi, int ho, int wo,
                                int x_cstride, int x_coff, int y_cstride, int y_coff, const float* scale,
                                ft_stream_t stream);

/* Per-channel affine + activation on an NHWC view: the pre-activation `BatchNorm -> ReLU` in front of the first deconv of the
 * lateral-deconv pose head (lib/pose/models/pose_net.py:9-14), which reads layer4's already activated output and so folds into
 * no conv epilogue.  `dtype` in, `dtype` out, npix = N * H * W pixels:
 *   y[pix, c] = act(scale[c] * x[pix, c] + shift[c])      c in [0, C); scale, shift fp32 [C]
 * The arithmetic is the conv epilogue's: scale * x + shift in fp32 as ONE fused multiply-add (a single rounding), then the
 * activation (FT_ACT_*, `slope` for FT_ACT_LEAKY) with the epilogue's values for non-finite inputs (NaN stays NaN, ReLU(-inf) = 0),
 * then one rounding to the output type on store.
 * x_cstride / x_coff and y_cstride / y_coff as in ft_conv_desc: channel c of a pixel sits at element pixel * cstride + coff + c.
 * Channels outside [coff, coff + C) of an output pixel stay untouched.  y may be the same view as x (in place); any other overlap
 * is undefined.  Accesses are 16 bytes wide (8 fp16 / 4 fp32 channels per thread) where C, both offsets and both strides are
 * multiples of that group and x, y, scale, shift are 16-byte aligned; any other view goes element by element.  The grid is capped
 * and strides over the rest.
 * FT_ERR_INVALID_ARG: a NULL pointer, npix or C <= 0, a stride smaller than offset + C, a negative offset, an unknown dtype or
 * activation, a pointer that is not aligned to its element type.  FT_ERR_UNSUPPORTED: 2^31 or more (pixel, group) items. */
int ft_scale_shift_act_nhwc_fwd(const void* x, void* y, int dtype, long long npix, int C, int x_cstride, int x_coff,
                                int y_cstride, int y_coff, const float* scale, const float* shift, int act, float slope,
                                ft_stream_t stream);

/* ---- DenseNet trunks of the FPN pose model: the pre-activation 1x1 conv ----
 * Replaces `norm1 -> relu1 -> conv1 (-> norm2 -> relu2)` of a dense layer and `norm -> relu -> conv -> AvgPool2d(2, 2)` of a
 * transition (lib/pose/models/densenet.py:19-36, 47-54).  norm1 belongs to the layer that READS the concatenated input, so it folds
 * into no producer's epilogue; here it is applied to the GEMM's input operand on its way from memory.
 *   x [N, H, W, x_cstride] NHWC, FT_F16 or FT_F32; channels [x_coff, x_coff + Cin) of a pixel are read, NO other channel is (a
 *     channel at or above Cin may hold anything, a NaN included: it reaches no operand)
 *   pool = 0:  a[p][c] = dtype(relu(fma(pre_scale[c], float(x[p][c]), pre_shift[c])))      ft_scale_shift_act_nhwc_fwd's bits
 *   pool = 1:  a[p][c] = dtype(0.25f * ((r00 + r01) + (r10 + r11)))   r_ij = the four fp32 values relu(fma(...)) of the 2x2 window
 *              of output pixel p, unrounded; fp32 adds in this order, one rounding to dtype.  The output map is [N, H/2, W/2]
 *              (floor: an odd last row or column takes no part), which equals avg_pool(conv(.)) because the conv is linear
 *   acc[p][n] = sum_c a[p][c] * w[n][c]      fp32 accumulation (fp16: MFMA, exact products; fp32: one fma per product, ascending c)
 *   y[p][y_coff + n] = dtype(act(fma(post_scale[n], acc, post_shift[n])))      post_scale = post_shift = NULL: act(acc)
 * act is FT_ACT_NONE or FT_ACT_RELU.  Channels outside [y_coff, y_coff + Cout) of an output pixel stay untouched.  x and y must not
 * share bytes a launch both reads and writes (disjoint channel windows of one buffer are fine).
 * w: the packed [Cout, Cin] weights.  FT_F32: fp32 [Cout][Cin] row-major.  FT_F16: fp16 [Cout/32][ceil(Cin/64)][4][64][8] —
 * element (g, c, s, lane, e) = W[32 g + (lane & 31)][64 c + 32 (lane >> 5) + 8 s + e], zero where that channel is >= Cin (the
 * order in which mfma_f32_32x32x16_f16 takes its operand).  pre_scale, pre_shift: fp32 [Cin]; post_scale, post_shift: fp32 [Cout].
 * FT_ERR_UNSUPPORTED: Cout % 32 != 0; Cin, an offset or a stride that is no multiple of the 16-byte channel group (8 fp16 / 4 fp32
 * channels); pool = 1 with H < 2 or W < 2 (an empty output); 2^31 or more pixels.  FT_ERR_INVALID_ARG: a NULL pointer (only the
 * post_* pair may be NULL, together), a size <= 0, a negative offset, a stride smaller than offset + C, an unknown dtype, act or
 * pool, a pointer that is not 16-byte aligned.  A refused call launches nothing. */
int ft_preact_conv1x1_fwd(const void* x, const void* w, const float* pre_scale, const float* pre_shift,
                          const float* post_scale, const float* post_shift, void* y, int dtype, int N, int H, int W, int Cin,
                          int x_cstride, int x_coff, int Cout, int y_cstride, int y_coff, int pool, int act,
                          ft_stream_t stream);

/* ---- Stacked hourglass (lib/pose/models/hourglass.py:110-121): the two seams of a level that are not convs ----
 * Every block of the hourglass is pre-activation: it reads its raw input (the shortcut) and relu(bn(input)).  At the two
 * memory-bound seams of a level the activated copies are written while the map is in registers.  Both kernels: NHWC, FT_F16 or
 * FT_F32 in and out, `*_cstride` / `*_coff` channel views as above (channel c of a pixel at element pixel * cstride + coff + c;
 * channels outside [coff, coff + C) of an output stay untouched), one thread per 16-byte channel group (8 fp16 / 4 fp32 channels):
 * offsets and strides must be multiples of the group and every buffer 16-byte aligned; C is any positive number (a last partial
 * group goes element by element).  No cap on N or on the map: the grid is capped and strides over the rest.  scale_*, shift_*:
 * fp32 [C].  The affine + ReLU is ft_scale_shift_act_nhwc_fwd's with FT_ACT_RELU — one fma in fp32, the activation with the same
 * values for non-finite inputs, one rounding on store — so each activated output carries the bits that kernel would write.
 *
 * ft_hourglass_down_fwd reads x [N, H, W, C] once and writes up to three outputs; each is optional (NULL), at least one is given:
 *   pool  [N, H/2, W/2, C] = max over the 2x2 window (nn.MaxPool2d(2, stride=2): sizes round down, an odd last row or column
 *                            takes no part); the stored value is one of the four inputs, a NaN in the window is kept
 *   a_pool[N, H/2, W/2, C] = relu(fma(scale_pool[c], pool, shift_pool[c]))
 *   a_full[N, H,   W,   C] = relu(fma(scale_full[c], x, shift_full[c])) for ALL pixels, an odd last row or column included
 * FT_ERR_INVALID_ARG: x NULL, no output, a size <= 0, pool or a_pool with H < 2 or W < 2, an activated output without its scale
 * and shift, a misaligned view, an unknown dtype, an output that shares bytes with x or with another output (disjoint channel
 * windows of one buffer — same pointer and stride — do not).  FT_ERR_UNSUPPORTED: 2^31 or more channel groups in a row.
 *
 * ft_hourglass_up_fwd: skip [N, H, W, C], low [N, hl, wl, C]:
 *   sum   = dtype(skip + bilerp_ac(low))      F.upsample(low, size=(H, W), mode='bilinear', align_corners=True) + skip, the
 *                                             coordinate rule and the fp32 arithmetic of ft_upsample_bilinear_ac_fwd, one rounding
 *   a_sum = relu(fma(scale[c], sum AS STORED, shift[c]))      optional (NULL): from the rounded value, so that it equals
 *                                             ft_scale_shift_act_nhwc_fwd run on `sum`, bit for bit
 * sum is required; it may be the very view `skip` (same pointer, stride and offset: in place), shares no bytes with it otherwise,
 * and never any with `low`; a_sum shares none with any other view.  FT_ERR_INVALID_ARG as above; FT_ERR_UNSUPPORTED for a side
 * above 2^24 and for 2^31 or more channel groups in an output row, as for ft_upsample_bilinear_ac_fwd. */
int ft_hourglass_down_fwd(const void* x, int dtype, int N, int H, int W, int C, int x_cstride, int x_coff, void* pool,
                          int pool_cstride, int pool_coff, void* a_pool, int apool_cstride, int apool_coff,
                          const float* scale_pool, const float* shift_pool, void* a_full, int afull_cstride, int afull_coff,
                          const float* scale_full, const float* shift_full, ft_stream_t stream);
int ft_hourglass_up_fwd(const void* skip, const void* low, int dtype, int N, int C, int H, int W, int hl, int wl,
                        int skip_cstride, int skip_coff, int low_cstride, int low_coff, void* sum, int sum_cstride, int sum_coff,
                        void* a_sum, int asum_cstride, int asum_coff, const float* scale, const float* shift, ft_stream_t stream);

/* ---- F4-F6 parity: the entry points below (forward, the NHWC forms, the fused warp stage and the backward calls)
 * are held to numbers the REFERENCE'S OWN kernels computed: tests/golden/flowops_golden.npz, written by its .cu
 * files compiled for the CPU (oracle/cuda_on_cpu/, tests/test_flowops_pinned_gpu.py).  Not pinned that way: nvcc's
 * FMA contraction, the order of Resample2d's backward atomics, coordinates with |x + dx| >= 2^31 (CUDA's
 * saturating float-to-int conversion, restated). */
/* ---- F4: Correlation forward ---------------------------------------------
 * Replaces Correlation_forward_cuda (correlation_package/src/correlation_cuda.c:11-93,
 * kernels correlation_cuda_kernel.cu:10-106).  Same parameters and output
 * geometry; no rInput scratch tensors (padding is implicit), NCHW fp32 in/out:
 *   out[n, tj*D+ti, y, x] = 1/(k*k*C) * sum_{j,i,c} in1[n,c,y1+j,x1+i] * in2[n,c,y2+j,x2+i]
 * corr_type_multiply must be 1 (the only mode the reference implements). */
int ft_correlation_out_shape(int C, int H, int W, int pad_size, int kernel_size,
                             int max_displacement, int stride1, int stride2,
                             int* out_c, int* out_h, int* out_w);
int ft_correlation_fwd(const float* in1, const float* in2, float* out, int B,
                       int C, int H, int W, int pad_size, int kernel_size,
                       int max_displacement, int stride1, int stride2,
                       int corr_type_multiply, ft_stream_t stream);
/* Fused in-network form (FlowNetC.py:86-92): NHWC `dtype` features in, the
 * LeakyReLU'd cost volume written into channels [y_coff, y_coff+D*D) of an
 * NHWC concat buffer.  kernel_size=1, stride1=1, pad=max_displacement.
 *   y[pix, y_coff + (dy+r)*D + (dx+r)] = act(1/C * sum_c f1[pix, c] * f2[pix + stride2*(dy, dx), c]),
 *   act(v) = v > 0 ? v : k * v with k = 0 (FT_ACT_RELU), slope (FT_ACT_LEAKY, any finite slope) or 1 (FT_ACT_NONE), and
 *   torch's value for a NaN / +inf / -inf sum (NaN, +inf, the IEEE product k * -inf — NaN at slope 0; ReLU(-inf) = 0).
 * One of four kernels runs (csrc/flow_ops.hip); ft_correlation_nhwc_form tells which without touching a device:
 *
 *   id                    kernel                                  chosen when
 *   FT_CORR_FORM_ROWS64   correlation_mfma_rows64_kernel<16,3,10> fp16, C = 256, stride2 = 2, max_displacement = 20, features and
 *                         (3 rows per workgroup, W <= 64)         output below 2 GiB, act none or leaky with slope in (0, 1],
 *                                                                 W <= 64, y_coff % 8 == 0 and y_cstride % 8 == 0
 *   FT_CORR_FORM_ROWS     correlation_mfma_rows_kernel<16,3,10>   as above with W > 64, or y_coff % 8, or y_cstride % 8
 *                         (3 rows, 104-column window)
 *   FT_CORR_FORM_MFMA     correlation_mfma_kernel<16>             fp16, C = 256, stride2 = 2, even max_displacement <= 32, features
 *                         (one row per workgroup)                 below 2 GiB, and not a rows form: max_displacement != 20, or
 *                                                                 ReLU, or a leaky slope outside (0, 1], or an output >= 2 GiB
 *   FT_CORR_FORM_VALU     correlation_nhwc_kernel<half,32,..>     everything else: fp32 always; fp16 when C != 256, stride2 != 2,
 *                         / <float,16,..>                         an odd or > 32 max_displacement, or features >= 2 GiB
 *
 * ft_correlation_nhwc_form returns the id, or -1 where ft_correlation_nhwc_fwd refuses the call: FT_ERR_INVALID_ARG (sizes
 * <= 0, C % 8, f_cstride % 8, f_cstride < C, a slice [y_coff, y_coff + D*D) outside y_cstride, an unknown dtype) and the
 * FT_ERR_UNSUPPORTED of the VALU form when (2*tile + 2*max_displacement) * (C * elem + 16) + tile * D*D * 4 bytes of LDS
 * (tile = 32 pixels fp16, 16 fp32) exceed 160 KiB. */
enum { FT_CORR_FORM_VALU = 0, FT_CORR_FORM_MFMA = 1, FT_CORR_FORM_ROWS = 2, FT_CORR_FORM_ROWS64 = 3 };
int ft_correlation_nhwc_form(int B, int C, int H, int W, int max_displacement,
                             int stride2, int f_cstride, int y_cstride,
                             int y_coff, int act, float slope, int dtype);
int ft_correlation_nhwc_fwd(const void* f1, const void* f2, void* y, int B,
                            int C, int H, int W, int max_displacement,
                            int stride2, int f_cstride, int y_cstride,
                            int y_coff, int act, float slope, int dtype,
                            ft_stream_t stream);

/* ---- F5: Resample2d forward (flow warp) ------------------------------------
 * Replaces Resample2d_cuda_forward (resample2d_package/src/Resample2d_cuda.c,
 * kernel Resample2d_kernel.cu:20-66); kernel_size is fixed at 1 as in
 * modules/resample2d.py:8.  in1 [B,C,H,W], flow [B,2,H,W], out [B,C,H,W]. */
int ft_resample2d_fwd(const float* in1, const float* flow, float* out, int B,
                      int C, int H, int W, ft_stream_t stream);

/* ---- F6: ChannelNorm forward ------------------------------------------------
 * Replaces ChannelNorm_cuda_forward (channelnorm_package/src/ChannelNorm_cuda.c,
 * kernel ChannelNorm_kernel.cu:19-51): out[b,0,y,x] = sqrt(sum_c in^2). */
int ft_channelnorm_fwd(const float* in1, float* out, int B, int C, int H, int W,
                       ft_stream_t stream);

/* ---- F4-F6 backward (training: flownet/ops.py autograd Functions) ----------
 * Replace Correlation_backward_cuda, Resample2d_cuda_backward and
 * ChannelNorm_cuda_backward.  Contiguous NCHW fp32, same sizes as the forward
 * entry points (grad_out has the forward output's shape).  Either gradient
 * pointer may be NULL (not computed), not both.  Every requested gradient is
 * fully written: the calls zero-fill what they need themselves, so the caller
 * passes uninitialised buffers.  No host synchronisation, no allocation: the
 * calls can be captured into a graph.
 *   ft_correlation_bwd: the exact adjoint of ft_correlation_fwd (equals the
 *     reference's kernels for kernel_size 1 / stride1 1; see INTEGRATION.md §1
 *     for kernel_size > 1 and stride1 > 1).  Bit-reproducible.  Fast path:
 *     kernel_size 1, stride1 1, stride2 in {1, 2, 4} and
 *     1 <= max_displacement / stride2 <= 10 (every FlowNet of the reference);
 *     any other valid parameters take a slow gather kernel (correctness only).
 *   ft_resample2d_bwd: grad_in1 = adjoint of the forward, summed with float
 *     atomics (may differ in the last bits between runs, as the reference's);
 *     grad_flow = Resample2d_kernel.cu:118-186, bit-reproducible.
 *   ft_channelnorm_bwd: grad_in1 = grad_out * in1 / (out + 1e-9)
 *     (ChannelNorm_kernel.cu:54-81), out = the forward's output. */
int ft_correlation_bwd(const float* in1, const float* in2, const float* grad_out,
                       float* grad_in1, float* grad_in2, int B, int C, int H, int W,
                       int pad_size, int kernel_size, int max_displacement,
                       int stride1, int stride2, int corr_type_multiply,
                       ft_stream_t stream);
int ft_resample2d_bwd(const float* in1, const float* flow, const float* grad_out,
                      float* grad_in1, float* grad_flow, int B, int C, int H, int W,
                      ft_stream_t stream);
int ft_channelnorm_bwd(const float* in1, const float* out, const float* grad_out,
                       float* grad_in1, int B, int C, int H, int W,
                       ft_stream_t stream);

/* ---- F5+F6 fused stage between stacked FlowNets (models.py:396-403) -------
 * From x6 = NHWC `dtype` [B,H,x_wpitch,8] (normalised img0|img1, pixel x in column x_lpad + x) and
 * flow NCHW fp32 [B,2,H,W] (already multiplied by div_flow) builds the 12-channel input of the
 * next FlowNetS: (img0, img1, warp(img1,flow), flow/div_flow, |img0-warp|)
 * as NHWC `dtype` [B,H,y_wpitch,16] (channels 12..15 and the padding columns zero). */
int ft_flow_warp_concat(const void* x6, const float* flow, float div_flow,
                        void* y, int B, int H, int W, int x_lpad, int x_wpitch,
                        int y_lpad, int y_wpitch, int dtype, ft_stream_t stream);

/* ---- N4: full FlowNet2 stack helpers -------------------------------------------
 * nn.Upsample(scale_factor=4, mode='nearest') of (x * mul) (lib/flownet/model/models.py:59-60,448). */
int ft_upsample_nearest4x(const float* x, float* y, int N, int C, int h, int w, float mul,
                          ft_stream_t stream);
/* Input of FlowNetFusion (models.py:140-168) in one pass: from x6 (as ft_flow_warp_concat) and two flow fields
 * NCHW fp32 [B,2,H,W] builds NHWC `dtype` [B,H,y_wpitch,16] (pixel x at column y_lpad + x; padding columns untouched) = (img0(3), flow_sd(2), flow_s2(2), |flow_sd|, |flow_s2|,
 * |img0 - warp(img1, flow_sd)|, |img0 - warp(img1, flow_s2)|, 0...) — two Resample2d + four ChannelNorm + cat. */
int ft_flow_fusion_concat(const void* x6, const float* flow_sd, const float* flow_s2, void* y, int B, int H,
                          int W, int x_lpad, int x_wpitch, int y_lpad, int y_wpitch, int dtype,
                          ft_stream_t stream);

/* ---- N2: person crops for the pose net --------------------------------------
 * Replaces the per-box host loop `transform_image` = cv2.warpAffine(img, t[:2], (res_w, res_h))
 * (lib/pose/utils/transforms.py:231-240, geometry :173-184; caller lib/tracking/net_utils.py:49-57).
 * img: HWC uint8 frame on the device (C <= 4); boxes: float[nb*3] = (center_x, center_y, scale) per crop;
 * out: NCHW fp32 [nb, C, rh, rw] = (bilinear(img) * pre_scale - mean[c]) * inv_std[c] (mean / inv_std may be
 * NULL), constant-0 border, fp32 interpolation weights (cv2's 1/32-px weight quantisation is not reproduced). */
int ft_crop_affine_fwd(const uint8_t* img, int H, int W, int C, const float* boxes, int nb, int rh, int rw,
                       const float* mean, const float* inv_std, float pre_scale, float* out,
                       ft_stream_t stream);

/* The same crop in the fixed-point arithmetic of cv2.warpAffine for a uint8 frame (round 5) — bit-exact to the RESTATED classic OpenCV
 * path (oracle/tracking_ref.py::warp_affine_cv2_ref; no cv2 in this image, so parity with a real cv2 build is UNPINNED; OpenCV >= 4.11,
 * IPP and HAL builds may differ in the last bit): OpenCV's fixed-point INTER_LINEAR
 * (imgwarp.cpp cv::warpAffine / WarpAffineInvoker / remapBilinear<FixedPtCast<int, uchar, 15>>; the third-party
 * dependency behind lib/pose/utils/transforms.py:238).  minv: double[nb*6], per box the dst -> src 2x3 map that
 * cv::warpAffine derives from the matrix it is handed (the caller inverts in double, cv2's operation order:
 * tracking.net_utils.cv2_crop_matrices).  out_u8: NHWC uint8 [nb, rh, rw, C] = cv2's return value (may be NULL);
 * out: NCHW fp32 [nb, C, rh, rw] = (float(u8) * pre_scale - mean[c]) * inv_std[c] (may be NULL; not both). */
int ft_crop_affine_cv2_fwd(const uint8_t* img, int H, int W, int C, const double* minv, int nb, int rh, int rw,
                           const float* mean, const float* inv_std, float pre_scale, uint8_t* out_u8, float* out,
                           ft_stream_t stream);

/* ---- N3: the clip's sequential tracking pass on the device ------------------------------------------------------
 * What tools/tracking/demo.py: tracking_pass_steps does per frame on the host between two pose replays, as three
 * single-workgroup launches whose counts live in device int32 words: no entry reads a count from the host, so a whole clip is
 * enqueued without a host wait (tracking/device_pass.py).  Bit-exact to the host functions they restate for finite inputs
 * with coordinates below 2^31 in magnitude (float64 geometry, float32 NMS, every operation rounded separately; NaN scores
 * are outside the contract).  Refused arguments launch nothing.
 *
 * ft_track_propagate — tracking/tracker.py:21 propagate_keypoints + tracking/flow_utils.py:15 box_propagation
 * (lib/tracking/flow_utils.py:7-35).  kps_prev: float[P*K*3] (x, y, score); flow: float[2*H*W] (u, v);
 * older_in: double[n_old*P*K*2] (NULL with n_old = 0).  moved_out: double[(1+n_old)*P*K*2]: [0] = kps_prev's (x, y) moved by
 * the flow at the truncated, clipped pixel, [1+a] = older_in[a] advanced by the same rule; boxes_out: float[P*4] = the
 * propagated boxes (joints with score > 0, grown by 15 %, clipped to the image).  All P rows are processed. */
int ft_track_propagate(const float* kps_prev, const float* flow, int H, int W, const double* older_in, int n_old, int P,
                       int K, double* moved_out, float* boxes_out, ft_stream_t stream);

/* ft_track_select — tools/tracking/demo.py:118-133: union of the detector boxes dets float[n*5] with the propagated boxes
 * prop_boxes float[P*4] (scores: column 4 of prev_boxes float[P*5]; the first *count_prev of them, a NULL count_prev or a
 * count of 0 = no previous poses: the detector boxes pass through, no NMS, no cap), tracking/flow_utils.py:35 nms
 * (lib/detection/nms/src/nms.c:36-63: score-descending, stable on ties, IoU >= thresh suppresses, +1 widths), the first
 * max_keep survivors kept.  Out: boxes float[cap*5], src int32[cap] (index into the union, -1 past the count), *count,
 * kps float[cap*K*3] (kp_det float[n*K*3] rows of the boxes that come from the detector, zero elsewhere), *nprop and
 * prop_slot int32[bucket] (the slots of the kept propagated boxes, in kept order, -1 past nprop), params float[bucket*3] =
 * (center_x, center_y, scale) of those boxes for ft_crop_affine_fwd (tracking/net_utils.py:36 boxes_to_center_scale in
 * float64, cast to float32; rows past nprop repeat row 0, (0, 0, 1) when nprop = 0).  rh, rw: the pose input resolution.
 * FT_ERR_INVALID_ARG: n > cap, max_keep > cap, sizes <= 0; FT_ERR_UNSUPPORTED: n + P > 512, K > 32, bucket < min(cap, P). */
int ft_track_select(const float* dets, const float* kp_det, int n, const float* prop_boxes, const float* prev_boxes, int P,
                    const int32_t* count_prev, int K, float thresh, int max_keep, int cap, int rh, int rw, int bucket,
                    float* boxes, int32_t* src, int32_t* count, float* kps, int32_t* nprop, int32_t* prop_slot,
                    float* params, ft_stream_t stream);

/* ft_track_place_rows — tracking/net_utils.py:143 heatmap_rows_to_image (the inverse crop affine of
 * lib/pose/utils/transforms.py:173-184): rows float[bucket*K*3] (x, y, score) in pixels of the h x w heat map ->
 * kps[prop_slot[j]] for j < *nprop in image pixels; centre and scale recomputed in float64 from boxes float[cap*5]
 * (params is not read), result cast to float32, score copied.  K <= 32. */
int ft_track_place_rows(const float* rows, const float* boxes, const int32_t* prop_slot, const int32_t* nprop, int bucket,
                        int cap, int K, int h, int w, int rh, int rw, float* kps, ft_stream_t stream);

/* ---- the detector's region stage (csrc/detect_ops.hip) --------------------------------------------------------
 * What lies between the RPN's two output maps and the tensor layer4 consumes (reference lib/detection: nms/,
 * layer_utils/roi_pooling, layer_utils/roi_align, model/bbox_transform.py, nets/network.py:93-121).  Every entry is
 * asynchronous on `stream`, launches nothing on refused arguments, and returns FT_OK without a launch for zero boxes /
 * RoIs.  FT_ERR_UNSUPPORTED when an element count (input, output or workspace) reaches 2^31.  All float arithmetic is
 * fp32 with every operation rounded separately (no FMA contraction), IEEE division.  Indices read from device data (a
 * RoI's batch index, box_ind, a stored arg-max) are range-checked in the kernels before they address anything. */

/* ft_box_nms — greedy box NMS of dets float[n*5] = (x1, y1, x2, y2, score), ALREADY in score-descending order
 * (nms/pth_nms.py:33-36 sorts first).  Step 1: the pairwise bit mask in 64 x 64 tiles on or above the diagonal, IoU as
 * devIoU of nms/src/cuda/nms_kernel.cu:16-24 (+1 widths, Sa + Sb - inter in that order).  Step 2: the sweep of
 * nms/src/nms_cuda.c:47-58 as one single-workgroup launch on the device (the reference copies the mask to the host):
 * box i is kept iff no earlier kept box marked it; it stops after max_keep survivors (max_keep <= 0: no cap).
 * inclusive = 0 suppresses on IoU > thresh (the CUDA path the reference's detector runs), 1 on IoU >= thresh
 * (nms/src/nms.c:59; the same float expressions).  keep int32[n]: indices into dets in kept order, -1 past *count.
 * workspace: ft_box_nms_workspace_bytes(n) bytes (0 for n outside [1, 16384]), contents undefined before and after.
 * n = 0: FT_OK, nothing is written.  n > 16384: FT_ERR_UNSUPPORTED. */
long long ft_box_nms_workspace_bytes(int n);
int ft_box_nms(const float* dets, int n, float thresh, int inclusive, int max_keep, void* workspace, int32_t* keep,
               int32_t* count, ft_stream_t stream);

/* ft_roi_pool_fwd / _bwd — layer_utils/roi_pooling/src/cuda/roi_pooling_kernel.cu:15-75: features float[B,C,H,W],
 * rois float[R*5] = (batch, x1, y1, x2, y2) in image pixels -> out float[R,C,ph,pw], argmax int32 of the same shape (may
 * be NULL in fwd).  Corners are round(v * spatial_scale), half away from zero; a malformed RoI is 1 x 1; bins are clipped
 * to the map; an empty bin gives 0 with arg-max -1; the max is a strict >, so the first occurrence in (h, w) row-major
 * order wins; the arg-max is the index inside the image, (c*H + h)*W + w.  Two deliberate departures from the reference:
 *   - a RoI whose batch index is outside [0, B) yields zeros / -1 (the reference reads out of bounds);
 *   - backward routes each grad_out element to the arg-max element of the RoI's OWN image (the reference's `== index`
 *     at :170 compares an in-image index with a global one and is right for image 0 only).
 * Backward zero-fills grad_in float[B,C,H,W] and scatters with float atomics, one per pooled element (an arg-max outside
 * [0, C*H*W) is skipped): sums of several RoIs on one element can differ in the last bits from run to run; it is
 * bit-reproducible where every such sum is exact (one contribution, or integer-valued gradients). */
int ft_roi_pool_fwd(const float* features, const float* rois, int B, int C, int H, int W, int R, float spatial_scale,
                    int pooled_h, int pooled_w, float* out, int32_t* argmax, ft_stream_t stream);
int ft_roi_pool_bwd(const float* grad_out, const float* rois, const int32_t* argmax, int B, int C, int H, int W, int R,
                    int pooled_h, int pooled_w, float* grad_in, ft_stream_t stream);

/* ft_crop_and_resize_fwd / _bwd — layer_utils/roi_align/src/cuda/crop_and_resize_kernel.cu:10-82, :84-165: image
 * float[B,C,H,W], boxes float[R*4] = normalised (y1, x1, y2, x2), box_ind int32[R] -> out float[R,C,crop_h,crop_w].
 * A crop dimension > 1 samples at y1*(H-1) + y*((y2-y1)*(H-1)/(crop_h-1)), a dimension of 1 at the centre
 * 0.5*(y1+y2)*(H-1); extrapolation_value where a sample leaves [0, H-1] / [0, W-1]; floor / ceil neighbours;
 * top + (bottom - top)*y_lerp with the x-lerps formed first; flipped boxes are allowed; a box whose box_ind is outside
 * [0, B) yields an all-zero crop.  Backward is the image gradient only: the entry zero-fills grad_image float[B,C,H,W]
 * and adds with float atomics, as the reference does: NOT bit-reproducible in general. */
int ft_crop_and_resize_fwd(const float* image, const float* boxes, const int32_t* box_ind, int B, int C, int H, int W, int R,
                           int crop_h, int crop_w, float extrapolation_value, float* out, ft_stream_t stream);
int ft_crop_and_resize_bwd(const float* grad_out, const float* boxes, const int32_t* box_ind, int B, int C, int H, int W, int R,
                           int crop_h, int crop_w, float* grad_image, ft_stream_t stream);

/* ft_roi_crop_nhwc_fwd — the inference form of Network._crop_pool_layer (nets/network.py:93-121) on dense NHWC features
 * [B,H,W,C], dtype FT_F16 or FT_F32, 16-byte aligned, C % 8 == 0 and H, W >= 2 (FT_ERR_INVALID_ARG otherwise):
 * rois float[R*5] in image pixels, (int)rois[.][0] the image; x / feat_stride, then / (W-1) and / (H-1), then the
 * crop arithmetic above at `pooled` (max_pool = 0; ResNet) or at 2*pooled followed by a 2 x 2 max (max_pool = 1; VGG),
 * extrapolation value 0.  Interpolation and the max run in fp32, rounded once on the store.  out [R,pooled,pooled,C] in
 * the input dtype: the N = R, Hi = Wi = pooled input of ft_conv2d_fwd.  An image index outside [0, B) yields zeros. */
int ft_roi_crop_nhwc_fwd(int dtype, const void* features, const float* rois, int B, int H, int W, int C, int R,
                         float feat_stride, int pooled, int max_pool, void* out, ft_stream_t stream);

/* ft_rpn_decode_boxes — bbox_transform_inv + clip_boxes (model/bbox_transform.py:35-80) in one pass: anchors float[A*4],
 * deltas float[A*4] (dx, dy, dw, dh) -> boxes float[A*4] clipped to [0, im_w - 1] x [0, im_h - 1]; expf, no fast-math
 * form.  The three arrays are 16-byte aligned. */
int ft_rpn_decode_boxes(const float* anchors, const float* deltas, int A, float im_h, float im_w, float* boxes,
                        ft_stream_t stream);

/* ---- the detector network's glue (reference lib/detection/model/test.py, nets/network.py, nets/resnet_v1.py) -----
 * csrc/detect_net_ops.hip.  fp32 arithmetic with every operation rounded separately, expf, IEEE division.  A call with zero
 * rows returns FT_OK without a launch; a refused call launches nothing. */

/* ft_detect_blob_fwd — model/test.py:37-58 (_get_image_blob) + nets/network.py:378: frame u8[H,W,3] (BGR, on the device)
 * -> blob float[1,3,Hb,Wb], the trunk's staged input.  means double[3] is read on the HOST at call time.  Per pixel and
 * channel: (float)((double)u8 - mean) (the reference subtracts float64 means into a float32 image), then OpenCV's INTER_LINEAR rule for float images: per axis the source coordinate
 * (d + 0.5) * scale - 0.5 (double, rounded to float; scale = 1 / f), floor, fraction; weight zeroed and index clamped at
 * both borders; s0 * (1 - f) + s1 * f along x for the two rows, then along y.  scale 1 is the identity minus the means. */
int ft_detect_blob_fwd(const uint8_t* frame, int H, int W, const double* means, int Hb, int Wb, double scale_y, double scale_x,
                       float* blob, ft_stream_t stream);

/* ft_rpn_softmax_fwd — nets/network.py:234-238: scores [rows, x_cstride] (FT_F16 or FT_F32; the 2A score channels start at
 * x_coff) -> prob float[rows, 2A]: exp(x - max) / sum over each pair (a, a + A). */
int ft_rpn_softmax_fwd(int dtype, const void* scores, long long rows, int A, int x_cstride, int x_coff, float* prob,
                       ft_stream_t stream);

/* ft_rcnn_mean_pool_fwd — nets/resnet_v1.py:113 (`.mean(3).mean(2)`): x [R,P,P,C] NHWC (FT_F16 or FT_F32, dense, 16-byte
 * aligned, C % 8 == 0) -> out [R,C] in the same dtype: per row the sum over x in order divided by P, those means summed over
 * y in order and divided by P, all in fp32, rounded once on the store. */
int ft_rcnn_mean_pool_fwd(int dtype, const void* x, int R, int P, int C, void* out, ft_stream_t stream);

/* ft_rcnn_detections_fwd — nets/network.py:270, :386-389 and model/test.py:97-104: cls_score float[R,K], bbox_pred
 * float[R,4K], rois float[R,5] in blob pixels; stds / means float[4] are read on the HOST at call time.
 *   cls_prob   float[R,K]   exp(x - max) / sum over the K classes
 *   deltas     float[R,4K]  bbox_pred * stds + means (per class)
 *   pred_boxes float[R,4K]  bbox_transform_inv of the deltas against rois[:,1:5] / im_scale, then _clip_boxes to the
 *                           im_h x im_w frame: x1, y1 are only raised to 0, x2, y2 only lowered to im_w - 1 / im_h - 1
 * Any K >= 1.  An output pointer may be NULL: that output is skipped (and the inputs only it reads may be NULL too).
 * bbox_pred, deltas and pred_boxes are 16-byte aligned. */
int ft_rcnn_detections_fwd(const float* cls_score, const float* bbox_pred, const float* rois, int R, int K, const float* stds,
                           const float* means, float im_scale, float im_h, float im_w, float* cls_prob, float* deltas,
                           float* pred_boxes, ft_stream_t stream);

/* ---- the VGG16 detector trunk (reference lib/detection/nets/vgg16.py; csrc/vgg_ops.hip) -------------------------
 * A refused call launches nothing.  (The unit's FC entry points, ft_fc_*, are declared under FT_EXPERIMENTAL below.) */

/* ft_maxpool2x2s2_fwd — nn.MaxPool2d(2, 2) (floor mode) on a dense NHWC map [N,Hi,Wi,C] -> [N,Hi/2,Wi/2,C], FT_F16 or FT_F32,
 * C % 8 == 0, both buffers 16-byte aligned; the last row / column of an odd map is never read.  The max is over the four values
 * themselves (an all-negative window gives its negative max; a NaN stays): the output is one of the inputs, bit for bit.
 * Hi < 2, Wi < 2 and bad arguments: FT_ERR_INVALID_ARG; N*Hi*Wi*C >= 2^31: FT_ERR_UNSUPPORTED. */
int ft_maxpool2x2s2_fwd(const void* x, void* y, int N, int Hi, int Wi, int C, int dtype, ft_stream_t stream);

/* ---- the detector's frame step without a host wait (csrc/detect_pass_ops.hip) ----------------------------------
 * What detection.proposal.proposal_layer and detection.test.detect_persons do in torch around a device -> host read, with
 * every count in a device int32 word, so that the frames of a clip are enqueued back to back (detection/test.py:
 * detect_persons_clip).  The conventions of the region stage above hold: asynchronous on `stream`, a refused call launches
 * nothing, fp32 with every operation rounded separately, indices and counts read from device data are clamped or
 * range-checked before they address anything. */

/* ft_topk_desc_f32 — the first k entries of torch.sort(scores, descending=True, stable=True) of scores float[n]: sorted
 * float[k] (the scores themselves, bit for bit scores[order[i]]) and order int32[k] (indices into scores).  The order is
 * that of the unique key (order key of the score, index): larger scores first, equal scores by ascending index, -0.0 ties
 * with +0.0, every NaN sorts in front of +inf (NaNs among themselves by index).  One launch of one 1024-thread workgroup:
 * the scores read once into registers, radix select of the k-th key in 8-bit digits, the k winners compacted into LDS,
 * merge sort there; no assumption on the spread of the scores.  Entries past k of order / sorted are not
 * written.  n = 0 or k = 0: FT_OK, no launch.  FT_ERR_UNSUPPORTED outside 1 <= k <= min(n, 16384), n <= 65536.
 * workspace: ft_topk_desc_f32_workspace_bytes(n, k) bytes; this form needs none (the query returns 0 and NULL is accepted):
 * the argument is there so that a form for larger n keeps the signature. */
long long ft_topk_desc_f32_workspace_bytes(int n, int k);
int ft_topk_desc_f32(const float* scores, int n, int k, int32_t* order, float* sorted, void* workspace, ft_stream_t stream);

/* ft_proposal_rois_fwd — the blob of layer_utils/proposal_layer.py:52-55 from ft_box_nms's output: boxes float[m,4] (the
 * boxes that went into the NMS, in its order), keep int32[m], *count.  With c = min(*count, rows, m) clamped at 0:
 * rois[j] = (0, boxes[keep[j]]) for j < c (a keep entry outside [0, m) gives a zero row), every row from c to rows is zeroed
 * (the buffer is reused from frame to frame), *n_rois = c.  rows = 0: FT_OK, nothing is written. */
int ft_proposal_rois_fwd(const float* boxes, const int32_t* keep, const int32_t* count, int m, int rows, float* rois,
                         int32_t* n_rois, ft_stream_t stream);

/* ft_detect_select_fwd — lib/tracking/net_utils.py:14-34 (`detect`) behind im_detect, one workgroup.  Candidates: the rows
 * r < *n_rois (clamped to [0, R]) of cls_prob float[R,K] / pred_boxes float[R,4K] as (pred_boxes[r, 4p:4p+4], cls_prob[r, p])
 * with p = person_id, followed by the first *extra_count rows (all M when extra_count is NULL) of extra float[M,5]
 * (extra = NULL: none).  Candidates with score < min_score are dropped (0 keeps every probability: the reference).  Stable
 * descending sort by score in the order of ft_topk_desc_f32 (detector rows before extras on ties), greedy NMS with the float
 * expressions of ft_box_nms at inclusive = 0 (IoU > thresh suppresses), stopping after max_keep survivors (<= 0: cap).
 * dets float[cap,5]: the survivors (x1, y1, x2, y2, score) in kept order, zeros past *count.
 * FT_ERR_INVALID_ARG: person_id outside [0, K), cap < 1, NaN thresh / min_score, a missing pointer;
 * FT_ERR_UNSUPPORTED: R + M > 1024. */
int ft_detect_select_fwd(const float* cls_prob, const float* pred_boxes, int R, const int32_t* n_rois, int K, int person_id,
                         const float* extra, int M, const int32_t* extra_count, float min_score, float thresh, int max_keep,
                         int cap, float* dets, int32_t* count, ft_stream_t stream);

/* ---- experimental entry points (NOT part of the drop-in boundary) -------------------------------------------
 * Measured alternatives (of the fused-block kernels, and of the VGG16 detector's FC layers) that the default plans do not
 * record or record second (profiles/README.md has their numbers).  They are exported by the library so that the tests and tools/dev can reach them, but they are declared only
 * when the includer defines FT_EXPERIMENTAL; signatures may change between rounds. */
#ifdef FT_EXPERIMENTAL
/* Register-stationary strip form of the same identity block (csrc/bottleneck_rstat.hip; fp16, C = 256, P = 64, stride 1,
 * 3 <= W <= 62): one persistent 8-wave workgroup per strip of full-width rows keeps all weights in registers.  The folded
 * BatchNorms travel INSIDE the weight buffer, which the caller builds once per weight set (fp16, from the fp32 weights):
 *   [64][272]  w1[co][ci] * scale1[co], then 16 columns {hi(shift1[co]), lo(shift1[co]), 0 x 14}
 *   [64][592]  w2[co][(ky*3+kx)*64 + ci] * scale2[co], then the 16 shift columns
 *   [256][80]  w3[co][ci] * scale3[co], then the 16 shift columns          (hi = fp16(shift), lo = fp16(shift - hi))
 * (the shift is added by one extra MFMA k-step against a vector of ones, the residual by two k-steps against an identity).
 * _supported also applies the cost rule (at least eight 64-pixel steps per strip) unless FT_BNK_RSTAT=2; FT_BNK_RSTAT=0 -> unsupported. */
int ft_bottleneck_rstat_supported(const ft_bottleneck_desc* d);
long long ft_bottleneck_rstat_weight_bytes(void);
int ft_bottleneck_rstat_fwd(const ft_bottleneck_desc* d, const void* x, const void* wpack, void* y, ft_stream_t stream);

/* CLUSTER form of the same block for the 256-plane stage on maps of <= 192 pixels (fp16, P = 256, C = 1024, stride 1;
 * layer3.1+ of the ResNets at 256 x 192; csrc/bottleneck_cluster.hip, round 5): the work of one image is shared by four
 * workgroups that exchange t1 / t2 through `workspace` INSIDE the launch (agent-scope hand-off, bounded spins), so a CU
 * streams about half the weight bytes of the strip form and no MFMA tile is padded.  Same wstream / tables as
 * ft_bottleneck_stream_fwd.  workspace: ft_bottleneck_cluster_workspace_bytes(d) bytes, ZEROED ONCE by the caller and
 * then left alone (it holds monotonic per-cluster arrival counters across calls); one workspace must not be used by two
 * launches that may run concurrently.  The 32-bit word at ft_bottleneck_cluster_status_offset(d) becomes non-zero if a
 * hand-off ever timed out (a member was not resident in time: the output of that call is wrong). */
int ft_bottleneck_cluster_supported(const ft_bottleneck_desc* d);
long long ft_bottleneck_cluster_workspace_bytes(const ft_bottleneck_desc* d);
long long ft_bottleneck_cluster_status_offset(const ft_bottleneck_desc* d);
int ft_bottleneck_cluster_fwd(const ft_bottleneck_desc* d, const void* x, const void* wstream, const float* tables, void* y,
                              void* workspace, ft_stream_t stream);

/* ft_fc_fwd (csrc/vgg_ops.hip) — nn.Linear (+ ReLU) on a few hundred rows as a weight-streaming split-K GEMM (vgg.classifier.0 / .3
 * of the VGG16 detector's region head).  Measured at 300 rows it does not beat ft_conv2d_fwd on the [rows,1,1,K] view (138 vs 115 us
 * at K = 25088, 38 vs 33 us at K = 4096; profiles/README.md), so detection.nets.vgg16 records it second, as the "fc" option.
 * y[R,N] = act(x[R,K] . W[N,K]^T + bias[N]); fp16 x, W and y, fp32 accumulation on MFMA, bias float[N] (NULL: none), act
 * FT_ACT_NONE or FT_ACT_RELU.  x and y are row-strided (x_stride >= K, y_stride >= N, in elements, multiples of
 * 8), so an NHWC [R,7,7,512] buffer is the [R,25088] input as it stands.
 *   constraints   K % 64 == 0, N % 64 == 0, any R >= 0; N*K, R*x_stride, R*y_stride and 64*R*N below 2^31; x, wpack, y, bias and
 *                 workspace 16-byte aligned.  FT_F32 and every other shape: FT_ERR_UNSUPPORTED (ft_fc_supported returns the code
 *                 ft_fc_fwd would, without pointers); negative sizes, short or odd strides, NULL / misaligned pointers, another
 *                 act, a workspace below ft_fc_workspace_bytes(R, K, N): FT_ERR_INVALID_ARG.
 *   ft_fc_pack    W fp16 [N,K] row-major -> wpack, N*K fp16, once per weight set: per 32 outputs g and 64-wide K-step t one 4 KB
 *                 block, lane l of a wave holding W[32 g + (l & 31)][64 t + 32 (l >> 5) + 0..31].
 *   two launches  K is split over workgroups (the grid fills 256 CUs at R <= 320, N = 4096); every slice writes an fp32 slab
 *                 [slice][R][N] into `workspace`, the second launch sums the slabs in slice order, adds the bias, applies act and
 *                 rounds once.  No atomics, no workgroup waits on another: the same call gives the same bits every time. */
int ft_fc_supported(int dtype, int R, int K, int N, int x_stride, int y_stride);
long long ft_fc_workspace_bytes(int R, int K, int N);
int ft_fc_pack(const void* w, int N, int K, void* wpack, ft_stream_t stream);
int ft_fc_fwd(int dtype, const void* x, int x_stride, const void* wpack, const float* bias, void* y, int y_stride, int R, int K,
              int N, int act, void* workspace, size_t workspace_bytes, ft_stream_t stream);
#endif /* FT_EXPERIMENTAL */

#ifdef __cplusplus
}
#endif
#endif /* FLOWTRACK_HIP_H_ */
