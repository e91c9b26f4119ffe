// The two seams of an hourglass level (models.hg; lib/pose/models/hourglass.py:110-121) that are not convs.  Every block of the
// hourglass is pre-activation: it reads its raw input (the shortcut) AND relu(bn(input)), and that BatchNorm + ReLU folds into no
// conv epilogue.  At the two memory-bound seams the map passes through registers anyway, so the activated copies ride along:
//   ft_hourglass_down_fwd  x -> MaxPool2d(2, 2)(x), relu(bn_b(pool)), relu(bn_a(x)): one read of x, up to three outputs
//   ft_hourglass_up_fwd    skip + bilinear_ac(low) -> sum, relu(bn(sum as stored))
// Both are pure streaming kernels, bound by HBM: one thread per 16-byte channel group, fp32 arithmetic, one rounding on store; the
// affine + ReLU is ft_scale_shift_act_nhwc_fwd's (one fma in fp32, act_mul with k = 0), so a fused output carries the bits a
// separate launch of that kernel would write.
#include "bilerp_ac.h"

namespace ft {

// relu(fma(s, x, b)): posenet_ops.hip's ssa_one at k = 0
__device__ __forceinline__ float hg_bn_relu(float x, float s, float b) { return act_mul(__builtin_fmaf(s, x, b), 0.f); }

// max that keeps a NaN (torch's max_pool2d, numpy's max) and returns one of its arguments unchanged
template <typename T>
__device__ __forceinline__ T hg_max(T a, T b) {
  return ((float)b > (float)a || b != b) ? b : a;
}

// G consecutive entries of a per-channel fp32 table from channel c0 (a multiple of G): 16-byte loads where the table's base is
// 16-byte aligned (`vec`, uniform over the launch), else one entry at a time; a NULL table gives zeros that nobody reads
template <int G>
__device__ __forceinline__ void hg_table(const float* __restrict__ t, int c0, bool vec, float (&out)[G]) {
  if (!t) {
#pragma unroll
    for (int e = 0; e < G; ++e) out[e] = 0.f;
  } else if (vec) {
#pragma unroll
    for (int q = 0; q < G / 4; ++q) {
      const float4_t v = *reinterpret_cast<const float4_t*>(t + c0 + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) out[4 * q + e] = v[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < G; ++e) out[e] = t[c0 + e];
  }
}

static bool hg_tables_vec(const float* a, const float* b, const float* c = nullptr, const float* d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

// images in flight (the grid's y extent): one per workgroup while that keeps the launch under ~16 workgroups per CU, else fewer,
// each workgroup striding over several images with its channel tables in registers
static unsigned hg_grid_images(int N, long long rows, long long pieces) {
  const long long per = rows * pieces, want = (4096 + per - 1) / per;
  const long long cap = N < 65535 ? N : 65535;
  return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
}

struct HgView {      // channel window of an NHWC buffer: channel c of pixel p at element p * cstride + coff + c
  int cstride, coff;
};

// grid = (cell rows, images in flight, pieces of one cell row): a cell is the 2x2 input window of one pooled pixel; an odd last
// row / column makes a last row / column of partial cells, which take part in a_full only.  blockIdx.x is the cell row; a thread
// takes the (cell column, channel group) items j, j + 256 gridDim.z, .. of that row and, per item, the images blockIdx.y,
// blockIdx.y + gridDim.y, ..  Lanes run along the channels, then along x.
template <typename T>
__global__ __launch_bounds__(256) void hourglass_down_kernel(const T* __restrict__ x, T* __restrict__ pool, T* __restrict__ a_pool,
                                                             T* __restrict__ a_full, const float* __restrict__ scale_pool,
                                                             const float* __restrict__ shift_pool, const float* __restrict__ scale_full,
                                                             const float* __restrict__ shift_full, int N, int H, int W, int C, HgView xv,
                                                             HgView pv, HgView apv, HgView afv, unsigned groups, unsigned row_items,
                                                             bool tab_vec) {
  constexpr int G = Group<T>::G;
  typedef typename Group<T>::vec vec;
  const int Ho = H / 2, Wo = W / 2;
  const int cy = blockIdx.x, y0 = 2 * cy;
  const bool row1 = y0 + 1 < H;
  const size_t x_image = (size_t)H * W * xv.cstride, p_image = (size_t)Ho * Wo * pv.cstride, ap_image = (size_t)Ho * Wo * apv.cstride,
               af_image = (size_t)H * W * afv.cstride;
  for (unsigned j = blockIdx.z * 256u + threadIdx.x; j < row_items; j += 256u * gridDim.z) {
    const unsigned cx = j / groups;
    const int c0 = (int)(j - cx * groups) * G;
    const int x0 = 2 * (int)cx;
    const bool col1 = x0 + 1 < W, whole = row1 && col1;
    const size_t pix00 = (size_t)y0 * W + x0;          // pixel index of the cell's corner; its right / lower neighbours: + 1, + W
    const size_t opix = (size_t)cy * Wo + cx;           // the pooled pixel (whole cells only)
    const bool do_pool = whole && (pool || a_pool);
    if (c0 + G <= C) {
      float sf[G], bf[G], sp[G], bp[G];
      hg_table<G>(a_full ? scale_full : nullptr, c0, tab_vec, sf);
      hg_table<G>(a_full ? shift_full : nullptr, c0, tab_vec, bf);
      hg_table<G>(a_pool ? scale_pool : nullptr, c0, tab_vec, sp);
      hg_table<G>(a_pool ? shift_pool : nullptr, c0, tab_vec, bp);
      for (size_t n = blockIdx.y; n < (size_t)N; n += gridDim.y) {
        const T* xn = x + n * x_image + xv.coff + c0;
        vec v[4];
        v[0] = *reinterpret_cast<const vec*>(xn + pix00 * xv.cstride);
        v[1] = col1 ? *reinterpret_cast<const vec*>(xn + (pix00 + 1) * xv.cstride) : v[0];
        v[2] = row1 ? *reinterpret_cast<const vec*>(xn + (pix00 + W) * xv.cstride) : v[0];
        v[3] = whole ? *reinterpret_cast<const vec*>(xn + (pix00 + W + 1) * xv.cstride) : v[0];
        if (a_full) {
          T* an = a_full + n * af_image + afv.coff + c0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if ((q & 1) && !col1) continue;
            if ((q & 2) && !row1) continue;
            vec o;
#pragma unroll
            for (int e = 0; e < G; ++e) o[e] = (T)hg_bn_relu((float)v[q][e], sf[e], bf[e]);
            *reinterpret_cast<vec*>(an + (pix00 + (q & 1) + (q & 2 ? W : 0)) * afv.cstride) = o;
          }
        }
        if (do_pool) {
          vec m;
#pragma unroll
          for (int e = 0; e < G; ++e) m[e] = hg_max(hg_max(v[0][e], v[1][e]), hg_max(v[2][e], v[3][e]));
          if (pool) *reinterpret_cast<vec*>(pool + n * p_image + opix * pv.cstride + pv.coff + c0) = m;
          if (a_pool) {
            vec o;
#pragma unroll
            for (int e = 0; e < G; ++e) o[e] = (T)hg_bn_relu((float)m[e], sp[e], bp[e]);
            *reinterpret_cast<vec*>(a_pool + n * ap_image + opix * apv.cstride + apv.coff + c0) = o;
          }
        }
      }
    } else {
      // the last group of a C that is no multiple of G: element by element, channels >= C are neither read nor written
      for (size_t n = blockIdx.y; n < (size_t)N; n += gridDim.y) {
        const T* xn = x + n * x_image + xv.coff + c0;
        for (int e = 0; c0 + e < C; ++e) {
          const T v0 = xn[pix00 * xv.cstride + e];
          const T v1 = col1 ? xn[(pix00 + 1) * xv.cstride + e] : v0;
          const T v2 = row1 ? xn[(pix00 + W) * xv.cstride + e] : v0;
          const T v3 = whole ? xn[(pix00 + W + 1) * xv.cstride + e] : v0;
          if (a_full) {
            T* an = a_full + n * af_image + afv.coff + c0 + e;
            const float s = scale_full[c0 + e], b = shift_full[c0 + e];
            an[pix00 * afv.cstride] = (T)hg_bn_relu((float)v0, s, b);
            if (col1) an[(pix00 + 1) * afv.cstride] = (T)hg_bn_relu((float)v1, s, b);
            if (row1) an[(pix00 + W) * afv.cstride] = (T)hg_bn_relu((float)v2, s, b);
            if (whole) an[(pix00 + W + 1) * afv.cstride] = (T)hg_bn_relu((float)v3, s, b);
          }
          if (do_pool) {
            const T m = hg_max(hg_max(v0, v1), hg_max(v2, v3));
            if (pool) pool[n * p_image + opix * pv.cstride + pv.coff + c0 + e] = m;
            if (a_pool) a_pool[n * ap_image + opix * apv.cstride + apv.coff + c0 + e] = (T)hg_bn_relu((float)m, scale_pool[c0 + e], shift_pool[c0 + e]);
          }
        }
      }
    }
  }
}

// grid as in upsample_bilinear_ac_kernel (fpn_ops.hip): blockIdx.x is the output row, so its source rows and weights are uniform over
// the workgroup.  skip and sum are not __restrict__: they may be the same view (a thread reads its skip group before it writes it).
template <typename T>
__global__ __launch_bounds__(256) void hourglass_up_kernel(const T* skip, const T* __restrict__ low, T* sum, T* __restrict__ a_sum,
                                                           const float* __restrict__ scale, const float* __restrict__ shift, int N, int C,
                                                           int H, int W, int hl, int wl, HgView kv, HgView lv, HgView sv, HgView av, float rh,
                                                           float rw, unsigned groups, unsigned row_items, bool tab_vec) {
  constexpr int G = Group<T>::G;
  typedef typename Group<T>::vec vec;
  const int oy = blockIdx.x;
  int y0, y1;
  float l0h, l1h;
  ac_source(rh, oy, hl, y0, y1, l0h, l1h);
  const size_t k_image = (size_t)H * W * kv.cstride, l_image = (size_t)hl * wl * lv.cstride, s_image = (size_t)H * W * sv.cstride,
               a_image = (size_t)H * W * av.cstride;
  for (unsigned j = blockIdx.z * 256u + threadIdx.x; j < row_items; j += 256u * gridDim.z) {
    const unsigned ox = j / groups;
    const int c0 = (int)(j - ox * groups) * G;
    int x0, x1;
    float l0w, l1w;
    ac_source(rw, (int)ox, wl, x0, x1, l0w, l1w);
    const size_t oa = ((size_t)y0 * wl + x0) * lv.cstride + lv.coff + c0, ob = ((size_t)y0 * wl + x1) * lv.cstride + lv.coff + c0;
    const size_t oc = ((size_t)y1 * wl + x0) * lv.cstride + lv.coff + c0, od = ((size_t)y1 * wl + x1) * lv.cstride + lv.coff + c0;
    const size_t opix = (size_t)oy * W + ox;
    const size_t ok = opix * kv.cstride + kv.coff + c0, os = opix * sv.cstride + sv.coff + c0, oav = opix * av.cstride + av.coff + c0;
    if (c0 + G <= C) {
      float s[G], b[G];
      hg_table<G>(a_sum ? scale : nullptr, c0, tab_vec, s);
      hg_table<G>(a_sum ? shift : nullptr, c0, tab_vec, b);
      for (size_t n = blockIdx.y; n < (size_t)N; n += gridDim.y) {
        const T* ln = low + n * l_image;
        const vec va = *reinterpret_cast<const vec*>(ln + oa), vb = *reinterpret_cast<const vec*>(ln + ob);
        const vec vc = *reinterpret_cast<const vec*>(ln + oc), vd = *reinterpret_cast<const vec*>(ln + od);
        const vec k = *reinterpret_cast<const vec*>(skip + n * k_image + ok);
        vec o;
#pragma unroll
        for (int e = 0; e < G; ++e)
          o[e] = (T)((float)k[e] + (l0h * (l0w * (float)va[e] + l1w * (float)vb[e]) + l1h * (l0w * (float)vc[e] + l1w * (float)vd[e])));
        *reinterpret_cast<vec*>(sum + n * s_image + os) = o;
        if (a_sum) {
          vec a;
#pragma unroll
          for (int e = 0; e < G; ++e) a[e] = (T)hg_bn_relu((float)o[e], s[e], b[e]);      // from the sum AS STORED
          *reinterpret_cast<vec*>(a_sum + n * a_image + oav) = a;
        }
      }
    } else {
      // the last group of a C that is no multiple of G: element by element, channels >= C are neither read nor written
      for (size_t n = blockIdx.y; n < (size_t)N; n += gridDim.y) {
        const T* ln = low + n * l_image;
        for (int e = 0; c0 + e < C; ++e) {
          const float v = l0h * (l0w * (float)ln[oa + e] + l1w * (float)ln[ob + e]) + l1h * (l0w * (float)ln[oc + e] + l1w * (float)ln[od + e]);
          const T o = (T)((float)skip[n * k_image + ok + e] + v);
          sum[n * s_image + os + e] = o;
          if (a_sum) a_sum[n * a_image + oav + e] = (T)hg_bn_relu((float)o, scale[c0 + e], shift[c0 + e]);
        }
      }
    }
  }
}

// a view as the host checks it: where its first and one-past-last bytes lie, and its channel window
struct HgSpan {
  uintptr_t base, lo, hi;
  int cstride, coff, C;
};

static HgSpan hg_span(const void* p, long long npix, int cstride, int coff, int C, size_t esz) {
  const uintptr_t b = reinterpret_cast<uintptr_t>(p);
  return {b, b + (uintptr_t)coff * esz, b + (uintptr_t)(((unsigned long long)(npix - 1) * cstride + coff + C) * esz), cstride, coff, C};
}

// two views share bytes — unless they are disjoint channel windows of one buffer (same base and stride)
static bool hg_overlap(const HgSpan& a, const HgSpan& b) {
  if (a.hi <= b.lo || b.hi <= a.lo) return false;
  if (a.base == b.base && a.cstride == b.cstride && (a.coff + a.C <= b.coff || b.coff + b.C <= a.coff)) return false;
  return true;
}

static bool hg_view_ok(const void* p, int cstride, int coff, int C, int G) {
  return coff >= 0 && cstride >= coff + C && coff % G == 0 && cstride % G == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

}  // namespace ft

using namespace ft;

extern "C" int ft_hourglass_down_fwd(const void* x, int dtype, int N, int H, int W, int C, int x_cstride, int x_coff, void* pool,
                                     int pool_cstride, int pool_coff, void* a_pool, int apool_cstride, int apool_coff,
                                     const float* scale_pool, const float* shift_pool, void* a_full, int afull_cstride, int afull_coff,
                                     const float* scale_full, const float* shift_full, ft_stream_t stream) {
  if (!x || N <= 0 || H <= 0 || W <= 0 || C <= 0) return FT_ERR_INVALID_ARG;
  if (dtype != FT_F16 && dtype != FT_F32) return FT_ERR_INVALID_ARG;
  if (!pool && !a_pool && !a_full) return FT_ERR_INVALID_ARG;
  if ((pool || a_pool) && (H < 2 || W < 2)) return FT_ERR_INVALID_ARG;
  if (a_pool && (!scale_pool || !shift_pool)) return FT_ERR_INVALID_ARG;
  if (a_full && (!scale_full || !shift_full)) return FT_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(scale_pool) | reinterpret_cast<uintptr_t>(shift_pool) | reinterpret_cast<uintptr_t>(scale_full) |
       reinterpret_cast<uintptr_t>(shift_full)) & 3)
    return FT_ERR_INVALID_ARG;
  const int G = dtype == FT_F16 ? 8 : 4;
  const size_t esz = dtype_size(dtype);
  // every 16-byte access must be aligned: offsets and strides in whole groups, base pointers on 16 bytes
  if (!hg_view_ok(x, x_cstride, x_coff, C, G)) return FT_ERR_INVALID_ARG;
  if (pool && !hg_view_ok(pool, pool_cstride, pool_coff, C, G)) return FT_ERR_INVALID_ARG;
  if (a_pool && !hg_view_ok(a_pool, apool_cstride, apool_coff, C, G)) return FT_ERR_INVALID_ARG;
  if (a_full && !hg_view_ok(a_full, afull_cstride, afull_coff, C, G)) return FT_ERR_INVALID_ARG;
  const int Ho = H / 2, Wo = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const long long npix = (long long)N * H * W, opix = (long long)N * Ho * Wo;
  HgSpan spans[4];
  int ns = 0;
  spans[ns++] = hg_span(x, npix, x_cstride, x_coff, C, esz);
  if (pool) spans[ns++] = hg_span(pool, opix, pool_cstride, pool_coff, C, esz);
  if (a_pool) spans[ns++] = hg_span(a_pool, opix, apool_cstride, apool_coff, C, esz);
  if (a_full) spans[ns++] = hg_span(a_full, npix, afull_cstride, afull_coff, C, esz);
  for (int i = 0; i < ns; ++i)
    for (int j = i + 1; j < ns; ++j)
      if (hg_overlap(spans[i], spans[j])) return FT_ERR_INVALID_ARG;      // no output may share bytes with x or another output
  const int groups = (C + G - 1) / G;
  const long long row_items = (long long)Wc * groups;       // (cell column, channel group) items of one cell row: a 32-bit index
  if (row_items > 0x7fffffffLL) return FT_ERR_UNSUPPORTED;
  const long long pieces = (row_items + 255) / 256;
  // no cap on N: a workgroup strides over the images the grid's y extent does not cover
  const long long zp = pieces < 64 ? pieces : 64;
  const dim3 grid((unsigned)Hc, hg_grid_images(N, Hc, zp), (unsigned)zp);
  const bool tab_vec = hg_tables_vec(scale_pool, shift_pool, scale_full, shift_full);
  const HgView xv{x_cstride, x_coff}, pv{pool_cstride, pool_coff}, apv{apool_cstride, apool_coff}, afv{afull_cstride, afull_coff};
  if (dtype == FT_F16)
    hipLaunchKernelGGL(hourglass_down_kernel<half_t>, grid, dim3(256), 0, as_stream(stream), static_cast<const half_t*>(x),
                       static_cast<half_t*>(pool), static_cast<half_t*>(a_pool), static_cast<half_t*>(a_full), scale_pool, shift_pool,
                       scale_full, shift_full, N, H, W, C, xv, pv, apv, afv, (unsigned)groups, (unsigned)row_items, tab_vec);
  else
    hipLaunchKernelGGL(hourglass_down_kernel<float>, grid, dim3(256), 0, as_stream(stream), static_cast<const float*>(x),
                       static_cast<float*>(pool), static_cast<float*>(a_pool), static_cast<float*>(a_full), scale_pool, shift_pool,
                       scale_full, shift_full, N, H, W, C, xv, pv, apv, afv, (unsigned)groups, (unsigned)row_items, tab_vec);
  FT_LAUNCH_CHECK("hourglass_down_kernel");
  return FT_OK;
}

extern "C" int ft_hourglass_up_fwd(const void* skip, const void* low, int dtype, int N, int C, int H, int W, int hl, int wl, int skip_cstride,
                                   int skip_coff, int low_cstride, int low_coff, void* sum, int sum_cstride, int sum_coff, void* a_sum,
                                   int asum_cstride, int asum_coff, const float* scale, const float* shift, ft_stream_t stream) {
  if (!skip || !low || !sum || N <= 0 || C <= 0 || H <= 0 || W <= 0 || hl <= 0 || wl <= 0) return FT_ERR_INVALID_ARG;
  if (dtype != FT_F16 && dtype != FT_F32) return FT_ERR_INVALID_ARG;
  if (a_sum && (!scale || !shift)) return FT_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(shift)) & 3) return FT_ERR_INVALID_ARG;
  const int G = dtype == FT_F16 ? 8 : 4;
  const size_t esz = dtype_size(dtype);
  if (!hg_view_ok(skip, skip_cstride, skip_coff, C, G) || !hg_view_ok(low, low_cstride, low_coff, C, G) ||
      !hg_view_ok(sum, sum_cstride, sum_coff, C, G))
    return FT_ERR_INVALID_ARG;
  if (a_sum && !hg_view_ok(a_sum, asum_cstride, asum_coff, C, G)) return FT_ERR_INVALID_ARG;
  const long long npix = (long long)N * H * W;
  const HgSpan ks = hg_span(skip, npix, skip_cstride, skip_coff, C, esz), ls = hg_span(low, (long long)N * hl * wl, low_cstride, low_coff, C, esz);
  const HgSpan ss = hg_span(sum, npix, sum_cstride, sum_coff, C, esz);
  // sum is the very view skip (in place) or shares nothing with it; it never shares bytes with low
  const bool in_place = sum == skip && sum_cstride == skip_cstride && sum_coff == skip_coff;
  if ((!in_place && hg_overlap(ss, ks)) || hg_overlap(ss, ls)) return FT_ERR_INVALID_ARG;
  if (a_sum) {
    const HgSpan as = hg_span(a_sum, npix, asum_cstride, asum_coff, C, esz);
    if (hg_overlap(as, ks) || hg_overlap(as, ls) || hg_overlap(as, ss)) return FT_ERR_INVALID_ARG;
  }
  // source coordinates are fp32 (torch's rule): above 2^24 rows or columns they stop being exact integers at the far end
  if (hl > (1 << 24) || wl > (1 << 24) || H > (1 << 24) || W > (1 << 24)) return FT_ERR_UNSUPPORTED;
  const int groups = (C + G - 1) / G;
  const long long row_items = (long long)W * groups;
  if (row_items > 0x7fffffffLL) return FT_ERR_UNSUPPORTED;
  const float rh = ac_ratio(hl, H), rw = ac_ratio(wl, W);
  const long long pieces = (row_items + 255) / 256;
  const long long zp = pieces < 64 ? pieces : 64;
  const dim3 grid((unsigned)H, hg_grid_images(N, H, zp), (unsigned)zp);
  const bool tab_vec = hg_tables_vec(scale, shift);
  const HgView kv{skip_cstride, skip_coff}, lv{low_cstride, low_coff}, sv{sum_cstride, sum_coff}, av{asum_cstride, asum_coff};
  if (dtype == FT_F16)
    hipLaunchKernelGGL(hourglass_up_kernel<half_t>, grid, dim3(256), 0, as_stream(stream), static_cast<const half_t*>(skip),
                       static_cast<const half_t*>(low), static_cast<half_t*>(sum), static_cast<half_t*>(a_sum), scale, shift, N, C, H, W, hl, wl,
                       kv, lv, sv, av, rh, rw, (unsigned)groups, (unsigned)row_items, tab_vec);
  else
    hipLaunchKernelGGL(hourglass_up_kernel<float>, grid, dim3(256), 0, as_stream(stream), static_cast<const float*>(skip),
                       static_cast<const float*>(low), static_cast<float*>(sum), static_cast<float*>(a_sum), scale, shift, N, C, H, W, hl, wl, kv,
                       lv, sv, av, rh, rw, (unsigned)groups, (unsigned)row_items, tab_vec);
  FT_LAUNCH_CHECK("hourglass_up_kernel");
  return FT_OK;
}
