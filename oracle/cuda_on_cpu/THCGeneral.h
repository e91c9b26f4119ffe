/* ORACLE — TEST INFRASTRUCTURE ONLY.  Stand-in: everything the reference's kernels need is in THC.h. */
#include "THC.h"
