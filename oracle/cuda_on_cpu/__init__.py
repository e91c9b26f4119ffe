"""ORACLE — TEST INFRASTRUCTURE ONLY.  CUDA-on-CPU shim, THC stand-ins and the recipe (build_ref.py) that compiles the
reference's FlowNet2 operator kernels into oracle/_ref/.  See cuda_on_cpu.h for the execution model."""
