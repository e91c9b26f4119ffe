/* ORACLE — TEST INFRASTRUCTURE ONLY.  Stand-in for the THC tensor API, as far as the reference's Resample2d / ChannelNorm
 * launchers use it: a contiguous fp32 tensor of four dimensions in host memory.  oracle/ref_ops.py fills the same struct. */
#ifndef FLOWTRACK_THC_STANDIN_H
#define FLOWTRACK_THC_STANDIN_H

#include "cuda_on_cpu.h"

struct THCState;
struct THCudaTensor {
  long size[4];
  long stride[4];
  float* data;
};

static inline long THCudaTensor_nElement(THCState*, const THCudaTensor* t) {
  return t->size[0] * t->size[1] * t->size[2] * t->size[3];
}
static inline float* THCudaTensor_data(THCState*, const THCudaTensor* t) { return t->data; }
static inline cudaStream_t THCState_getCurrentStream(THCState*) { return nullptr; }
#define THCudaCheck(err) \
  do {                   \
    if ((err) != cudaSuccess) abort(); \
  } while (0)

#endif
