/* ORACLE — TEST INFRASTRUCTURE ONLY.  Stand-in for the header the reference's correlation kernels include: it brings in the
 * CUDA-on-CPU shim.  The two launchers are defined extern "C" by the kernel file itself; oracle/ref_ops.py binds them. */
#include "cuda_on_cpu.h"
