"""ORACLE — TEST INFRASTRUCTURE ONLY.

CPU restatement of the reference's algorithms for the FlowTrack pose / flow hot paths.  Only
tests/, __graft_entry__.smoke() and bench.py's `cpu_baseline` leg may import this package, and only
as the checker — the product path (flowtrack/pytorch_amd) never routes through it.

Contents
  ops_ref.py        ctypes binding of flow_ops_ref.c (plain C, follows the reference .cu kernels) and
                    independent numpy formulations of the same operators
  cuda_on_cpu/      a CUDA-on-CPU execution shim, THC stand-in headers and the recipe (build_ref.py) that compiles the
                    reference's own correlation / Resample2d / ChannelNorm .cu files into oracle/_ref/ (never committed;
                    built by ops_ref.build() where the reference checkout is present, skipped silently elsewhere)
  ref_ops.py        ctypes binding of the reference's six host launchers in oracle/_ref/libflowtrack_ref_ops.so
  pose_ref.py       functional torch-CPU fp32 graph of DeconvResnet (the reference's own arithmetic
                    for the stock layers is torch CPU: SURVEY §8(c) "third-party arithmetic")
  flow_ref.py       functional torch-CPU fp32 graphs of FlowNet2S / FlowNet2C / FlowNet2CS
  keypoints_ref.py  numpy restatement of max_preds / final_preds / OKS with torch-0.4 semantics

Pinning: pose_ref / flow_ref(FlowNet2S) / keypoints_ref are checked against the imported reference
classes by tests/golden/make_golden.py (run in the build container only; the vectors it wrote are
committed under tests/golden/).  The three CUDA-only ops are pinned by tests/golden/flowops_golden.npz, which the
reference's own kernels wrote through cuda_on_cpu/ (tests/golden/make_flowops_golden.py): flow_ops_ref.c reproduces their
forward bit for bit.  Not pinned: nvcc's FMA contraction (bounded by a test), the order of Resample2d's backward atomics,
anything that relies on more than warp lockstep, coordinates outside the int range.
"""
