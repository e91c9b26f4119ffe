/*
 * ORACLE — TEST INFRASTRUCTURE ONLY.  Never imported, linked or executed by the product path
 * (flowtrack/pytorch_amd); only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg
 * may use it, and only as the checker.
 *
 * Plain-C CPU restatement of FlowNet2's three CUDA-only operators (the reference has no CPU
 * implementation: correlation_package/src/correlation.c:3-33 are empty stubs), following the
 * reference kernels step by step, including the explicit zero-padded NHWC staging buffers:
 *   correlation_fwd   <- correlation_cuda_kernel.cu:10-32 (channels_first), :34-106 (Correlation_forward),
 *                        output geometry correlation_cuda.c:25-38
 *   resample2d_fwd    <- Resample2d_kernel.cu:20-66
 *   channelnorm_fwd   <- ChannelNorm_kernel.cu:19-51
 *   upsample4x_fwd    <- nn.Upsample(scale_factor=4, mode='bilinear') as used at FlowNetS.py:58
 *                        (align_corners=False semantics; checked against torch in tests)
 * Parity status: PINNED for the three operators' forwards.  The reference's own .cu kernels, compiled for the CPU by
 * oracle/cuda_on_cpu/build_ref.py (one thread at a time, warp lockstep order, no FMA contraction), wrote
 * tests/golden/flowops_golden.npz; correlation_fwd, resample2d_fwd and channelnorm_fwd below reproduce it BIT FOR BIT
 * (tests/test_flowops_pinned_cpu.py, which also compares against the live library on a wider sweep where it is built).
 * Not pinned: nvcc's default FMA contraction (bounded by a test), coordinates with |x + dx| >= 2^31 (the clamp before the
 * int conversion in resample2d_fwd restates CUDA's saturating conversion, which a host compile cannot run).  Further checks:
 * an independent numpy formulation in oracle/ops_ref.py and closed-form cases in tests/ (shifts, identities).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define THREADS_PER_BLOCK 32 /* the reference's partial-sum width; reproduced to keep its summation order */

/* in: [B,C,H,W] -> out: zero-initialised [B,H+2p,W+2p,C] (correlation_cuda_kernel.cu:10-32) */
static void channels_first(const float* in, float* rin, int B, int C, int H, int W, int pad) {
  const int pW = W + 2 * pad, pH = H + 2 * pad;
  for (int n = 0; n < B; ++n)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        for (int c = 0; c < C; ++c)
          rin[(((size_t)n * pH + (y + pad)) * pW + (x + pad)) * C + c] = in[(((size_t)n * C + c) * H + y) * W + x];
}

int correlation_out_shape(int C, int H, int W, int pad, int ksize, int max_disp, int s1, int s2, int* oc, int* oh,
                          int* ow) {
  const int krad = (ksize - 1) / 2, border = krad + max_disp;
  const int pH = H + 2 * pad, pW = W + 2 * pad;
  const int D = (max_disp / s2) * 2 + 1;
  *oc = D * D;
  *oh = (int)ceilf((float)(pH - 2 * border) / (float)s1);
  *ow = (int)ceilf((float)(pW - 2 * border) / (float)s1);
  return (*oh > 0 && *ow > 0) ? 0 : 1;
}

/* out: [B, D*D, oh, ow]; returns 0 on success */
int correlation_fwd(const float* in1, const float* in2, float* out, int B, int C, int H, int W, int pad, int ksize,
                    int max_disp, int s1, int s2) {
  int oc, oh, ow;
  if (correlation_out_shape(C, H, W, pad, ksize, max_disp, s1, s2, &oc, &oh, &ow)) return 1;
  const int pH = H + 2 * pad, pW = W + 2 * pad;
  const size_t psz = (size_t)B * pH * pW * C;
  float* r1 = (float*)calloc(psz, sizeof(float));
  float* r2 = (float*)calloc(psz, sizeof(float));
  if (!r1 || !r2) { free(r1); free(r2); return 2; }
  channels_first(in1, r1, B, C, H, W, pad);
  channels_first(in2, r2, B, C, H, W, pad);
  const int krad = (ksize - 1) / 2, drad = max_disp / s2, D = 2 * drad + 1;
  const float nelems = (float)(ksize * ksize * C);
  for (int n = 0; n < B; ++n)
    for (int by = 0; by < oh; ++by)
      for (int bx = 0; bx < ow; ++bx) {
        const int y1 = by * s1 + max_disp + krad, x1 = bx * s1 + max_disp + krad;
        for (int tj = -drad; tj <= drad; ++tj)
          for (int ti = -drad; ti <= drad; ++ti) {
            float prod_sum[THREADS_PER_BLOCK];
            const int x2 = x1 + ti * s2, y2 = y1 + tj * s2;
            for (int c = 0; c < THREADS_PER_BLOCK; ++c) prod_sum[c] = 0.f;
            for (int j = -krad; j <= krad; ++j)
              for (int i = -krad; i <= krad; ++i)
                for (int c = 0; c < THREADS_PER_BLOCK; ++c)
                  for (int ch = c; ch < C; ch += THREADS_PER_BLOCK) {
                    const size_t i1 = (((size_t)n * pH + (y1 + j)) * pW + (x1 + i)) * C + ch;
                    const size_t i2 = (((size_t)n * pH + (y2 + j)) * pW + (x2 + i)) * C + ch;
                    prod_sum[c] += r1[i1] * r2[i2];
                  }
            float reduce_sum = 0.f;
            for (int c = 0; c < THREADS_PER_BLOCK; ++c) reduce_sum += prod_sum[c];
            const int tc = (tj + drad) * D + (ti + drad);
            out[(((size_t)n * oc + tc) * oh + by) * ow + bx] = reduce_sum / nelems;
          }
      }
  free(r1);
  free(r2);
  return 0;
}

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* in1 [B,C,H,W], flow [B,2,H,W] -> out [B,C,H,W]; kernel_size = 1 (modules/resample2d.py:8) */
void resample2d_fwd(const float* in1, const float* flow, float* out, int B, int C, int H, int W) {
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c)
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const float dx = flow[(((size_t)b * 2 + 0) * H + y) * W + x];
          const float dy = flow[(((size_t)b * 2 + 1) * H + y) * W + x];
          const float xf = (float)x + dx, yf = (float)y + dy;
          const float alpha = xf - floorf(xf), beta = yf - floorf(yf);
          /* clamp before the int conversion so absurd flows stay defined; identical for finite in-range values */
          const float fxl = fminf(fmaxf(floorf(xf), -1.0f), (float)W), fyl = fminf(fmaxf(floorf(yf), -1.0f), (float)H);
          const int xL = clampi((int)fxl, 0, W - 1), xR = clampi((int)fxl + 1, 0, W - 1);
          const int yT = clampi((int)fyl, 0, H - 1), yB = clampi((int)fyl + 1, 0, H - 1);
          const float* p = in1 + ((size_t)b * C + c) * H * W;
          /* the reference mixes double weights into a float accumulator (val += double*float) */
          float val = 0.0f;
          val += (1. - alpha) * (1. - beta) * p[(size_t)yT * W + xL];
          val += (alpha) * (1. - beta) * p[(size_t)yT * W + xR];
          val += (1. - alpha) * (beta) * p[(size_t)yB * W + xL];
          val += (alpha) * (beta) * p[(size_t)yB * W + xR];
          out[(((size_t)b * C + c) * H + y) * W + x] = val;
        }
}

/* in [B,C,H,W] -> out [B,1,H,W] */
void channelnorm_fwd(const float* in, float* out, int B, int C, int H, int W) {
  const size_t HW = (size_t)H * W;
  for (int b = 0; b < B; ++b)
    for (size_t p = 0; p < HW; ++p) {
      float result = 0.0f;
      for (int c = 0; c < C; ++c) {
        const float v = in[((size_t)b * C + c) * HW + p];
        result += v * v;
      }
      out[(size_t)b * HW + p] = sqrtf(result);
    }
}

/* x [N,C,h,w] -> y [N,C,4h,4w], y = bilinear(x * mul), half-pixel centres, edge clamp */
void upsample4x_fwd(const float* x, float* y, int N, int C, int h, int w, float mul) {
  const int H = 4 * h, W = 4 * w;
  for (int nc = 0; nc < N * C; ++nc) {
    const float* p = x + (size_t)nc * h * w;
    float* q = y + (size_t)nc * H * W;
    for (int oy = 0; oy < H; ++oy) {
      float sy = ((float)oy + 0.5f) * 0.25f - 0.5f;
      if (sy < 0.f) sy = 0.f;
      const int y0 = (int)sy, y1 = y0 + (y0 < h - 1 ? 1 : 0);
      const float ly = sy - (float)y0, hy = 1.f - ly;
      for (int ox = 0; ox < W; ++ox) {
        float sx = ((float)ox + 0.5f) * 0.25f - 0.5f;
        if (sx < 0.f) sx = 0.f;
        const int x0 = (int)sx, x1 = x0 + (x0 < w - 1 ? 1 : 0);
        const float lx = sx - (float)x0, hx = 1.f - lx;
        q[(size_t)oy * W + ox] = hy * (hx * (p[y0 * w + x0] * mul) + lx * (p[y0 * w + x1] * mul)) +
                                 ly * (hx * (p[y1 * w + x0] * mul) + lx * (p[y1 * w + x1] * mul));
      }
    }
  }
}

/* Direct NCHW conv / transposed conv in double accumulation: an arithmetic cross-check of the torch
 * functional oracle on small shapes (definition of Conv2d / ConvTranspose2d, no im2col, no BLAS).
 * x [N,Cin,H,W]; conv: w [Cout,Cin,k,k]; transposed: w [Cin,Cout,k,k]; bias may be NULL. */
void conv2d_direct(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int H, int W, int Cout,
                   int k, int stride, int pad) {
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  for (int n = 0; n < N; ++n)
    for (int co = 0; co < Cout; ++co)
      for (int oy = 0; oy < Ho; ++oy)
        for (int ox = 0; ox < Wo; ++ox) {
          double acc = bias ? bias[co] : 0.0;
          for (int ci = 0; ci < Cin; ++ci)
            for (int ky = 0; ky < k; ++ky) {
              const int iy = oy * stride - pad + ky;
              if (iy < 0 || iy >= H) continue;
              for (int kx = 0; kx < k; ++kx) {
                const int ix = ox * stride - pad + kx;
                if (ix < 0 || ix >= W) continue;
                acc += (double)x[(((size_t)n * Cin + ci) * H + iy) * W + ix] *
                       (double)w[(((size_t)co * Cin + ci) * k + ky) * k + kx];
              }
            }
          y[(((size_t)n * Cout + co) * Ho + oy) * Wo + ox] = (float)acc;
        }
}

void conv_transpose2d_direct(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int H, int W,
                             int Cout, int k, int stride, int pad) {
  const int Ho = (H - 1) * stride - 2 * pad + k, Wo = (W - 1) * stride - 2 * pad + k;
  double* acc = (double*)calloc((size_t)Ho * Wo, sizeof(double));
  for (int n = 0; n < N; ++n)
    for (int co = 0; co < Cout; ++co) {
      for (int i = 0; i < Ho * Wo; ++i) acc[i] = bias ? bias[co] : 0.0;
      for (int ci = 0; ci < Cin; ++ci)
        for (int iy = 0; iy < H; ++iy)
          for (int ix = 0; ix < W; ++ix) {
            const double v = x[(((size_t)n * Cin + ci) * H + iy) * W + ix];
            for (int ky = 0; ky < k; ++ky) {
              const int oy = iy * stride - pad + ky;
              if (oy < 0 || oy >= Ho) continue;
              for (int kx = 0; kx < k; ++kx) {
                const int ox = ix * stride - pad + kx;
                if (ox < 0 || ox >= Wo) continue;
                acc[(size_t)oy * Wo + ox] += v * (double)w[(((size_t)ci * Cout + co) * k + ky) * k + kx];
              }
            }
          }
      for (int i = 0; i < Ho * Wo; ++i) y[((size_t)n * Cout + co) * Ho * Wo + i] = (float)acc[i];
    }
  free(acc);
}
