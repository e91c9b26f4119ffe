// The detector's frame step without a host wait (detection/proposal.py: proposal_layer_device, detection/nets.py: detect_enqueue,
// detection/test.py: detect_persons_clip): the three steps that the per-frame path runs in torch with a device -> host read.
//   ft_topk_desc_f32       the first k entries of torch.sort(scores, descending=True, stable=True) as ONE single-workgroup launch:
//                          the scores read once into registers, radix-select of the k-th largest (score, index) key, the k winners
//                          compacted into LDS, merge sort there
//   ft_proposal_rois_fwd   the [rows,5] RoI blob of proposal_layer.py:52-55 from ft_box_nms's keep list and device count
//   ft_detect_select_fwd   detect_persons behind im_detect (lib/tracking/net_utils.py:14-34): person column (+ extra boxes), score
//                          screen, stable descending sort, greedy NMS with ft_box_nms's float expressions, one workgroup
// Every count is a device word; nothing here is read by the host.  Float arithmetic is fp32 with every operation rounded separately
// (the pragma; no fast-math flag, so `/` is the correctly rounded division).
// Device safety: every index that comes from device data (a count, a keep entry, the index bits of a sorted key) is clamped or
// range-checked before it becomes an address; every loop bound is a kernel argument or a value clipped against one; no kernel waits
// on another workgroup.
#include "ft_common.h"

#pragma clang fp contract(off)

namespace ft {

constexpr int TOPK_THREADS = 1024;
constexpr int TOPK_MAX_N = 65536;                    // the index takes the low 16 bits of the 48-bit key
constexpr int TOPK_MAX_K = 16384;                    // (16384 + 1024 of padding) x 8 B of LDS; the limit of ft_box_nms, which consumes the result
constexpr int TOPK_PASSES = 6;                       // 48 key bits in 8-bit digits

// The order key of a score: a larger key sorts earlier.  torch.sort(descending=True) puts NaN in front (every NaN equal), and
// -0.0 ties with +0.0; both hold here.  No float maps to a key below 0x007FFFFF (-inf), so 0 is free as "no entry".
__device__ __forceinline__ uint32_t order_key(float f) {
  if (f != f) return 0xFFFFFFFFu;
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The unique key of a score is (order key << 16) | (65535 - index): descending order of it is the stable descending sort (equal
// scores by ascending index).  ROUNDS: scores per thread (n <= ROUNDS * 1024), held as order keys in registers from one pass over global memory; E: keys per
// thread of the sort (P = E * the sorting threads).
template <int ROUNDS, int E>
__global__ __launch_bounds__(TOPK_THREADS) void topk_desc_kernel(const float* __restrict__ scores, int n, int k, int P,
                                                                 int32_t* __restrict__ order, float* __restrict__ sorted) {
  extern __shared__ unsigned long long s_keys[];     // P entries (P = the power of two >= k), one slot of padding behind every E
  // the sort's threads walk runs that start E keys apart: without the padding 32 lanes would meet in 64 / E banks
  auto at = [](int idx) { return E > 1 ? idx + idx / E : idx; };
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_digit, s_kk, s_all, s_fill;
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid == 0) s_fill = 0;
  uint32_t key[ROUNDS];                              // of score r * 1024 + tid; 0 (below every key) past n
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int i = r * TOPK_THREADS + tid;
    key[r] = i < n ? order_key(scores[i]) : 0u;
  }
  auto full_key = [&](int r) { return ((unsigned long long)key[r] << 16) | (unsigned long long)(TOPK_MAX_N - 1 - (r * TOPK_THREADS + tid)); };

  // ---- radix select: `prefix` grows by one digit per pass towards the k-th largest key; kk = its rank among the keys that
  // share the prefix.  Equal digits are the rule, not the exception (synthetic RPN scores all lie within a few ulps of 0.5; the
  // index digits are equal across a wave), so a wave first merges up to four groups of equal digits into one LDS add each;
  // whatever is left adds singly.
  unsigned long long prefix = 0;
  unsigned kk = (unsigned)k;
  int shift = 0;
  for (int pass = 0; pass < TOPK_PASSES; ++pass) {
    shift = 40 - 8 * pass;
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      if (r * TOPK_THREADS >= n) break;              // uniform
      const unsigned long long c = full_key(r);
      bool live = r * TOPK_THREADS + tid < n && (pass == 0 || (c >> (shift + 8)) == prefix);
      const unsigned digit = (unsigned)(c >> shift) & 255u;
      for (int it = 0; it < 4; ++it) {
        const unsigned long long m = __ballot(live);
        if (!m) break;                               // wave-uniform
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
        const unsigned d = (unsigned)__builtin_amdgcn_readlane((int)digit, leader);
        const bool mine = live && digit == d;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(&s_hist[d], (unsigned)__popcll(same));
        if (mine) live = false;
      }
      if (live) atomicAdd(&s_hist[digit], 1u);
    }
    __syncthreads();
    if (tid < 64) {                                  // lane l: bins 255 - 4l .. 252 - 4l, so the wave walks the digits downwards
      unsigned h[4], s = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        h[e] = s_hist[255 - (4 * lane + e)];
        s += h[e];
      }
      unsigned incl = s;
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
      }
      unsigned above = incl - s;                     // keys with this prefix and a larger digit
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (above < kk && kk <= above + h[e]) {      // exactly one (lane, e): the bins hold at least kk keys in all
          s_digit = 255u - (unsigned)(4 * lane + e);
          s_kk = kk - above;
          s_all = (kk - above == h[e]) ? 1u : 0u;
        }
        above += h[e];
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | s_digit;
    kk = s_kk;
    if (s_all) break;                                // every key with this prefix is a winner: the lower digits need no pass
  }
  const unsigned long long cut = prefix << shift;    // winners: key >= cut, exactly k of them

  // ---- compact the winners into LDS (any order: the sort follows), pad to P with 0 (below every key)
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    if (r * TOPK_THREADS >= n) break;
    const unsigned long long c = full_key(r);
    const bool win = r * TOPK_THREADS + tid < n && c >= cut;
    const unsigned long long m = __ballot(win);
    if (m) {
      const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
      unsigned base = 0;
      if (lane == leader) base = atomicAdd(&s_fill, (unsigned)__popcll(m));
      base = (unsigned)__builtin_amdgcn_readlane((int)base, leader);
      const unsigned pos = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
      if (win && pos < (unsigned)P) s_keys[at((int)pos)] = c;
    }
  }
  __syncthreads();
  const unsigned filled = s_fill < (unsigned)P ? s_fill : (unsigned)P;
  for (int i = (int)filled + tid; i < P; i += TOPK_THREADS) s_keys[at(i)] = 0ull;
  __syncthreads();

  // ---- merge sort, descending: P / E threads sort E keys each in registers (odd-even transposition), then the runs are merged
  // pairwise, log2(P / E) rounds; a thread finds the start of its E outputs on the merge path by binary search (the keys are
  // unique; the pads tie only with each other, behind every key) and merges them into registers, which go back behind a barrier.
  const int NT = P / E;
  const bool sorter = tid < NT;
  unsigned long long v[E];
  if (sorter) {
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = s_keys[at(tid * E + e)];
#pragma unroll
    for (int round = 0; round < E; ++round) {
#pragma unroll
      for (int e = round & 1; e + 1 < E; e += 2) {
        const unsigned long long hi = v[e] > v[e + 1] ? v[e] : v[e + 1], lo = v[e] > v[e + 1] ? v[e + 1] : v[e];
        v[e] = hi;
        v[e + 1] = lo;
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) s_keys[at(tid * E + e)] = v[e];
  }
  __syncthreads();
  for (int L = E; L < P; L <<= 1) {
    if (sorter) {
      const int o = tid * E, pb = o & ~(2 * L - 1), d = o - pb;
      auto A = [&](int x) { return s_keys[at(pb + x)]; };
      auto B = [&](int x) { return s_keys[at(pb + L + x)]; };
      int lo = d > L ? d - L : 0, hi = d < L ? d : L;
      while (lo < hi) {                              // lo = the keys of A among the first d of the merged run
        const int mid = (lo + hi) >> 1;
        if (A(mid) > B(d - 1 - mid)) lo = mid + 1; else hi = mid;
      }
      int i = lo, j = d - lo;
      unsigned long long a = i < L ? A(i) : 0ull, b = j < L ? B(j) : 0ull;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const bool take_a = j >= L || (i < L && a > b);
        v[e] = take_a ? a : b;
        if (take_a) {
          ++i;
          a = i < L ? A(i) : 0ull;
        } else {
          ++j;
          b = j < L ? B(j) : 0ull;
        }
      }
    }
    __syncthreads();
    if (sorter) {
#pragma unroll
      for (int e = 0; e < E; ++e) s_keys[at(tid * E + e)] = v[e];
    }
    __syncthreads();
  }

  for (int i = tid; i < k; i += TOPK_THREADS) {
    const int idx = TOPK_MAX_N - 1 - (int)(s_keys[at(i)] & 0xFFFFull);
    if (idx < n) {                                   // holds for every winner; a pad (never among the first k) would fail it
      order[i] = idx;
      sorted[i] = scores[idx];                       // the score itself: -0.0 and a NaN's payload come out as they went in
    }
  }
}

// ---- the RoI blob ---------------------------------------------------------------------------------------------------------
constexpr int DPS_THREADS = 256;

__global__ __launch_bounds__(DPS_THREADS) void proposal_rois_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ keep,
                                                                    const int32_t* __restrict__ count, int m, int rows,
                                                                    float* __restrict__ rois, int32_t* __restrict__ n_rois) {
  int c = *count;
  const int lim = rows < m ? rows : m;
  c = c < 0 ? 0 : (c > lim ? lim : c);
  const int j = blockIdx.x * DPS_THREADS + threadIdx.x;
  if (j == 0) *n_rois = c;
  if (j >= rows) return;
  float* o = rois + (size_t)j * 5;
  const int b = j < c ? keep[j] : -1;
  o[0] = 0.f;
  if (b >= 0 && b < m) {
    const float* s = boxes + (size_t)b * 4;
    o[1] = s[0]; o[2] = s[1]; o[3] = s[2]; o[4] = s[3];
  } else {
    o[1] = o[2] = o[3] = o[4] = 0.f;
  }
}

// ---- the person select ----------------------------------------------------------------------------------------------------
constexpr int SEL_THREADS = 1024;
constexpr int SEL_MAX = 1024;                        // candidates: one per thread
constexpr int SEL_WORDS = SEL_MAX / 64;
constexpr int SEL_MASK_WORDS = 64 * (SEL_WORDS * (SEL_WORDS + 1) / 2);   // the hit mask on or above the diagonal, by 64-row block
constexpr size_t SEL_LDS = (size_t)SEL_MAX * 4 * 7 + (size_t)SEL_MASK_WORDS * 8;

// word `w` (>= i / 64) of row i of the triangular hit mask: block b = i / 64 holds 64 rows of SEL_WORDS - b words
__device__ __forceinline__ int sel_mask_at(int i, int w) {
  const int b = i >> 6;
  return 64 * (b * SEL_WORDS - b * (b - 1) / 2) + (i & 63) * (SEL_WORDS - b) + (w - b);
}

__global__ __launch_bounds__(SEL_THREADS) void detect_select_kernel(const float* __restrict__ cls_prob, const float* __restrict__ pred_boxes,
                                                                    int R, const int32_t* __restrict__ n_rois, int K, int person,
                                                                    const float* __restrict__ extra, int M,
                                                                    const int32_t* __restrict__ extra_count, float min_score, float thresh,
                                                                    int limit, int cap, float* __restrict__ dets, int32_t* __restrict__ count) {
  extern __shared__ unsigned long long s_dyn[];
  unsigned long long* s_hit = s_dyn;                                     // SEL_MASK_WORDS
  uint32_t* s_key = reinterpret_cast<uint32_t*>(s_dyn + SEL_MASK_WORDS);  // by candidate slot; 0 = no candidate
  float* s_x1 = reinterpret_cast<float*>(s_key + SEL_MAX);               // by rank from here on
  float* s_y1 = s_x1 + SEL_MAX;
  float* s_x2 = s_y1 + SEL_MAX;
  float* s_y2 = s_x2 + SEL_MAX;
  float* s_sc = s_y2 + SEL_MAX;
  int* s_keep = reinterpret_cast<int*>(s_sc + SEL_MAX);                  // kept list: ranks, in kept order
  __shared__ int s_n, s_cnt;
  const int tid = threadIdx.x;
  const int U = R + M;                               // slots: the detector rows, then the extras (<= SEL_MAX)
  int nr = R > 0 ? *n_rois : 0;
  nr = nr < 0 ? 0 : (nr > R ? R : nr);
  int ne = M > 0 ? (extra_count ? *extra_count : M) : 0;
  ne = ne < 0 ? 0 : (ne > M ? M : ne);
  if (tid == 0) s_n = 0;

  float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, sc = 0.f;
  bool ok = false;
  if (tid < U) {
    if (tid < R) {
      ok = tid < nr;
      if (ok) {
        const float* b = pred_boxes + (size_t)tid * 4 * K + 4 * person;
        x1 = b[0]; y1 = b[1]; x2 = b[2]; y2 = b[3];
        sc = cls_prob[(size_t)tid * K + person];
      }
    } else {
      ok = tid - R < ne;
      if (ok) {
        const float* b = extra + (size_t)(tid - R) * 5;
        x1 = b[0]; y1 = b[1]; x2 = b[2]; y2 = b[3]; sc = b[4];
      }
    }
    if (ok && sc < min_score) ok = false;
  }
  s_key[tid] = ok ? order_key(sc) : 0u;
  __syncthreads();
  // rank by counting = the stable descending argsort: candidates with a larger key, plus equal ones in an earlier slot
  if (ok) {
    const uint32_t key = s_key[tid];
    int r = 0;
    for (int v = 0; v < U; ++v) {
      const uint32_t kv = s_key[v];
      r += (kv > key || (kv == key && v < tid)) ? 1 : 0;
    }
    s_x1[r] = x1; s_y1[r] = y1; s_x2[r] = x2; s_y2[r] = y2; s_sc[r] = sc;
    atomicAdd(&s_n, 1);
  }
  __syncthreads();
  const int N = s_n, NW = (N + 63) >> 6;
  // the pairwise hit mask in rank order, 64 columns per task, words on or above the diagonal only
  for (int task = tid; task < NW * N; task += SEL_THREADS) {
    const int w = task / N, i = task - w * N;
    if ((i >> 6) > w) continue;
    const int j0 = (w << 6) > i + 1 ? (w << 6) : i + 1, j1 = ((w + 1) << 6) < N ? ((w + 1) << 6) : N;
    const float ax1 = s_x1[i], ay1 = s_y1[i], ax2 = s_x2[i], ay2 = s_y2[i];
    const float sa = (ax2 - ax1 + 1.f) * (ay2 - ay1 + 1.f);
    unsigned long long bits = 0;
    for (int j = j0; j < j1; ++j) {                  // the expressions of nms_mask_kernel (detect_ops.hip)
      const float left = fmaxf(ax1, s_x1[j]), right = fminf(ax2, s_x2[j]);
      const float top = fmaxf(ay1, s_y1[j]), bottom = fminf(ay2, s_y2[j]);
      const float ww = fmaxf(right - left + 1.f, 0.f), hh = fmaxf(bottom - top + 1.f, 0.f);
      const float inter = ww * hh;
      const float sb = (s_x2[j] - s_x1[j] + 1.f) * (s_y2[j] - s_y1[j] + 1.f);
      const float iou = inter / (sa + sb - inter);
      if (iou > thresh) bits |= 1ull << (j & 63);
    }
    s_hit[sel_mask_at(i, w)] = bits;
  }
  __syncthreads();
  // greedy walk by one wave: lane l < NW owns word l of the suppressed set; the walk jumps from kept box to kept box
  if (tid < 64) {
    unsigned long long removed = 0;
    int cnt = 0;
    for (int w = 0; w < NW && cnt < limit; ++w) {
      const int left = N - (w << 6);
      unsigned long long open = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
      while (cnt < limit) {
        const unsigned long long avail = open & ~__shfl(removed, w, 64);
        if (!avail) break;
        const int b = __ffsll((long long)avail) - 1;
        const int i = (w << 6) + b;
        if (tid == 0) s_keep[cnt] = i;
        ++cnt;
        if (tid >= w && tid < NW) removed |= s_hit[sel_mask_at(i, tid)];
        open &= b == 63 ? 0ull : ~((2ull << b) - 1ull);
      }
    }
    if (tid == 0) s_cnt = cnt;
  }
  __syncthreads();
  const int cnt = s_cnt;                             // <= min(limit, N) <= cap
  for (int s = tid; s < cap; s += SEL_THREADS) {
    float* o = dets + (size_t)s * 5;
    if (s < cnt) {
      const int r = s_keep[s];
      o[0] = s_x1[r]; o[1] = s_y1[r]; o[2] = s_x2[r]; o[3] = s_y2[r]; o[4] = s_sc[r];
    } else {
      o[0] = o[1] = o[2] = o[3] = o[4] = 0.f;
    }
  }
  if (tid == 0) *count = cnt;
}

}  // namespace ft

using namespace ft;

extern "C" long long ft_topk_desc_f32_workspace_bytes(int n, int k) {
  (void)n;
  (void)k;
  return 0;                                          // the single-workgroup form keeps its candidates in LDS
}

extern "C" int ft_topk_desc_f32(const float* scores, int n, int k, int32_t* order, float* sorted, void* workspace, ft_stream_t stream) {
  (void)workspace;
  if (n < 0 || k < 0) return FT_ERR_INVALID_ARG;
  if (n == 0 || k == 0) return FT_OK;
  if (n > TOPK_MAX_N || k > TOPK_MAX_K || k > n) return FT_ERR_UNSUPPORTED;
  if (!scores || !order || !sorted) return FT_ERR_INVALID_ARG;
  int P = 1;
  while (P < k) P <<= 1;
  const int E = P <= TOPK_THREADS ? 1 : P / TOPK_THREADS;
  const int rounds = n <= 8 * TOPK_THREADS ? 8 : (n <= 24 * TOPK_THREADS ? 24 : (n <= 40 * TOPK_THREADS ? 40 : 64));   // 21 546 and 35 721 anchors: 24, 40
#define FT_TOPK_LAUNCH(ROUNDS, EE)                                                                                              \
  do {                                                                                                                          \
    FT_RAISE_LDS((topk_desc_kernel<ROUNDS, EE>), (size_t)(TOPK_MAX_K + TOPK_THREADS) * sizeof(unsigned long long));             \
    hipLaunchKernelGGL((topk_desc_kernel<ROUNDS, EE>), dim3(1), dim3(TOPK_THREADS),                                              \
                       (size_t)(P + (EE > 1 ? P / EE : 0)) * sizeof(unsigned long long), as_stream(stream), scores, n, k, P, order,  \
                       sorted);                                                                                                 \
  } while (0)
#define FT_TOPK_BY_E(ROUNDS)                                                                                                    \
  do {                                                                                                                          \
    if (E == 1) FT_TOPK_LAUNCH(ROUNDS, 1);                                                                                      \
    else if (E == 2) FT_TOPK_LAUNCH(ROUNDS, 2);                                                                                 \
    else if (E == 4) FT_TOPK_LAUNCH(ROUNDS, 4);                                                                                 \
    else if (E == 8) FT_TOPK_LAUNCH(ROUNDS, 8);                                                                                 \
    else FT_TOPK_LAUNCH(ROUNDS, 16);                                                                                            \
  } while (0)
  if (rounds == 8) FT_TOPK_BY_E(8);
  else if (rounds == 24) FT_TOPK_BY_E(24);
  else if (rounds == 40) FT_TOPK_BY_E(40);
  else FT_TOPK_BY_E(64);
#undef FT_TOPK_BY_E
#undef FT_TOPK_LAUNCH
  FT_LAUNCH_CHECK("topk_desc_kernel");
  return FT_OK;
}

extern "C" int ft_proposal_rois_fwd(const float* boxes, const int32_t* keep, const int32_t* count, int m, int rows, float* rois,
                                    int32_t* n_rois, ft_stream_t stream) {
  if (m < 0 || rows < 0) return FT_ERR_INVALID_ARG;
  if (rows == 0) return FT_OK;
  if (!count || !rois || !n_rois || (m > 0 && (!boxes || !keep))) return FT_ERR_INVALID_ARG;
  if (5ll * rows >= (1ll << 31) || 4ll * m >= (1ll << 31)) return FT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(proposal_rois_kernel, dim3((unsigned)((rows + DPS_THREADS - 1) / DPS_THREADS)), dim3(DPS_THREADS), 0, as_stream(stream),
                     boxes, keep, count, m, rows, rois, n_rois);
  FT_LAUNCH_CHECK("proposal_rois_kernel");
  return FT_OK;
}

extern "C" int ft_detect_select_fwd(const float* cls_prob, const float* pred_boxes, int R, const int32_t* n_rois, int K, int person_id,
                                    const float* extra, int M, const int32_t* extra_count, float min_score, float thresh, int max_keep,
                                    int cap, float* dets, int32_t* count, ft_stream_t stream) {
  if (R < 0 || M < 0 || K < 1 || person_id < 0 || person_id >= K || cap < 1 || !dets || !count || !(thresh == thresh) ||
      !(min_score == min_score))
    return FT_ERR_INVALID_ARG;
  if (R > 0 && (!cls_prob || !pred_boxes || !n_rois)) return FT_ERR_INVALID_ARG;
  if (!extra) M = 0;                                 // no extras: M and extra_count are not looked at
  if ((long long)R + M > SEL_MAX) return FT_ERR_UNSUPPORTED;
  if (4ll * R * K >= (1ll << 31) || 5ll * cap >= (1ll << 31)) return FT_ERR_UNSUPPORTED;
  const int limit = max_keep <= 0 || max_keep > cap ? cap : max_keep;
  FT_RAISE_LDS(detect_select_kernel, SEL_LDS);
  hipLaunchKernelGGL(detect_select_kernel, dim3(1), dim3(SEL_THREADS), SEL_LDS, as_stream(stream), cls_prob, pred_boxes, R, n_rois, K,
                     person_id, extra, M, extra_count, min_score, thresh, limit, cap, dets, count);
  FT_LAUNCH_CHECK("detect_select_kernel");
  return FT_OK;
}
