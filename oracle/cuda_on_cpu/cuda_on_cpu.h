/*
 * ORACLE — TEST INFRASTRUCTURE ONLY.  A CUDA-on-CPU execution shim: just enough of the CUDA language surface to compile the
 * reference's three FlowNet2 .cu files with g++ and run their own kernels and host launchers on the CPU.  build_ref.py
 * rewrites `k<<<grid, block, shmem, stream>>>(args)` into `coc::launch(k, grid, block, shmem, stream)(args)`; everything else
 * in those files is compiled as written.
 *
 * Execution model (deliberately the narrowest one the kernels are correct under):
 *   - blocks run one after another, blockIdx.x fastest;
 *   - inside a block exactly ONE thread runs at a time, each on a ucontext fiber; a thread runs until it returns or reaches
 *     __syncthreads(), then the next higher thread index runs; when every live thread has arrived, the round starts again at
 *     the lowest live index.  A thread that has returned no longer takes part in barriers.
 *   This is warp lockstep seen from outside for a 32-thread block, and it is needed: Correlation_forward re-zeroes
 *   prod_sum[c] for the next displacement while thread 0 may still be reducing the previous one, with no second barrier.
 *   On one 32-lane warp the reduction is over before any lane moves on; with free-running host threads it is a data race.
 *   Here thread 0 finishes its reduction (it runs first after the barrier, up to the next barrier) before thread 1 resumes.
 *   - atomicAdd is a plain read-modify-write (one thread at a time), so "atomic order" is ascending global thread index.
 *     A GPU's order is arbitrary; only sums whose terms are exact can be compared bit for bit.
 *   - __shared__ is `static`: one copy, reused by the blocks as they run in turn.
 *
 * Arithmetic: CUDA's overload set, not C's.  floor(float) and sqrt(float) stay in float (checked below), max / min are the
 * int overloads, literals such as 1. and 1e-9 stay double.  Compile with -ffp-contract=off (nvcc would contract to FMA; that
 * difference is bounded by a test, not reproduced).  int(float) outside the int range is undefined here and saturates on
 * CUDA: callers keep coordinates inside (-2^31, 2^31).
 */
#ifndef FLOWTRACK_CUDA_ON_CPU_H
#define FLOWTRACK_CUDA_ON_CPU_H

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <ucontext.h>

#include <type_traits>

#define __global__
#define __device__
#define __host__
#define __shared__ static

struct uint3 {
  unsigned x, y, z;
};
struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct long4 {
  long x, y, z, w;
};
static inline long4 make_long4(long x, long y, long z, long w) {
  long4 v = {x, y, z, w};
  return v;
}

typedef void* cudaStream_t;
typedef int cudaError_t;
enum { cudaSuccess = 0 };
static inline cudaError_t cudaGetLastError() { return cudaSuccess; }
static inline const char* cudaGetErrorString(cudaError_t) { return "no error"; }

static inline int max(int a, int b) { return a > b ? a : b; }
static inline int min(int a, int b) { return a < b ? a : b; }
static_assert(std::is_same<decltype(floor(1.0f)), float>::value, "floor(float) must stay in float, as in CUDA");
static_assert(std::is_same<decltype(sqrt(1.0f)), float>::value, "sqrt(float) must stay in float, as in CUDA");

static inline float atomicAdd(float* p, float v) {
  const float old = *p;
  *p = old + v;
  return old;
}

static uint3 threadIdx, blockIdx;
static dim3 blockDim, gridDim;

namespace coc {

enum { kStackBytes = 64 * 1024 };

struct Fiber {
  ucontext_t ctx;
  uint3 tid;
  bool done;
};

static ucontext_t g_sched;
static Fiber* g_fibers = nullptr;
static char* g_stacks = nullptr;
static unsigned g_capacity = 0, g_cur = 0;
static void (*g_body)(void*) = nullptr;
static void* g_arg = nullptr;

static void trampoline() {
  g_body(g_arg);
  g_fibers[g_cur].done = true;   // uc_link returns to the scheduler
}

static inline void barrier() { swapcontext(&g_fibers[g_cur].ctx, &g_sched); }

static void run_block(dim3 b, void (*body)(void*), void* arg) {
  const unsigned n = b.x * b.y * b.z;
  if (n > g_capacity) {
    free(g_fibers);
    free(g_stacks);
    g_fibers = (Fiber*)malloc(sizeof(Fiber) * n);
    g_stacks = (char*)malloc((size_t)kStackBytes * n);
    if (!g_fibers || !g_stacks) abort();
    g_capacity = n;
  }
  g_body = body;
  g_arg = arg;
  for (unsigned t = 0; t < n; ++t) {
    Fiber& f = g_fibers[t];
    f.tid.x = t % b.x;
    f.tid.y = (t / b.x) % b.y;
    f.tid.z = t / (b.x * b.y);
    f.done = false;
    getcontext(&f.ctx);
    f.ctx.uc_stack.ss_sp = g_stacks + (size_t)kStackBytes * t;
    f.ctx.uc_stack.ss_size = kStackBytes;
    f.ctx.uc_link = &g_sched;
    makecontext(&f.ctx, trampoline, 0);
  }
  unsigned live = n;
  while (live) {                       // one pass = one barrier phase, ascending thread index
    for (unsigned t = 0; t < n; ++t) {
      if (g_fibers[t].done) continue;
      g_cur = t;
      threadIdx = g_fibers[t].tid;
      swapcontext(&g_sched, &g_fibers[t].ctx);
      if (g_fibers[t].done) --live;
    }
  }
}

template <class F>
static void thunk(void* p) {
  (*static_cast<F*>(p))();
}

template <class F>
static void run_grid(dim3 g, dim3 b, F& body) {
  gridDim = g;
  blockDim = b;
  for (unsigned z = 0; z < g.z; ++z)
    for (unsigned y = 0; y < g.y; ++y)
      for (unsigned x = 0; x < g.x; ++x) {
        blockIdx.x = x;
        blockIdx.y = y;
        blockIdx.z = z;
        run_block(b, &thunk<F>, &body);
      }
}

template <class... P>
struct Launch {
  void (*kernel)(P...);
  dim3 grid, block;
  template <class... A>
  void operator()(A... args) const {   // by value, as a kernel launch copies its arguments
    auto body = [&]() { kernel(args...); };
    run_grid(grid, block, body);
  }
};

template <class... P>
static Launch<P...> launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t /*shmem*/, cudaStream_t /*stream*/) {
  Launch<P...> l = {kernel, grid, block};
  return l;
}

}  // namespace coc

static inline void __syncthreads() { coc::barrier(); }

#endif
