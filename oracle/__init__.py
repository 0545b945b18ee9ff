# The CPU floating-point environment the golden train vectors (tests/golden/make_golden.py) are generated and compared in:
# MKL's conditional-numerical-reproducibility path, ATen's scalar kernels and one thread give the same fp32 rounding on any
# x86-64 CPU.  Without it the reduction order follows the host's instruction set and core count, and the receiver's y2.bias
# (exact gradient 0: RMSprop turns its rounding noise into +-lr steps) and near-threshold ReLU units differ from host to host.
# Takes effect only in a process that sets it before torch is imported (which also calls torch.set_num_threads(1)).
PORTABLE_FP_ENV = {"MKL_CBWR": "COMPATIBLE", "MKL_NUM_THREADS": "1", "OMP_NUM_THREADS": "1", "ATEN_CPU_CAPABILITY": "default"}
