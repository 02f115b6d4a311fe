# oracle/_ref: the reference's OWN kernel file, compiled as it lies for gfx950 and linked with our launch driver:
#   /root/reference/src/pb_kernels.cu   every __global__ of the filterbank path (K1-K5, K7-K11, the FRB injection).  It
#                                       takes from CUDA only cufftReal / cufftComplex, the thread and block built-ins,
#                                       __shared__, __syncthreads, atomicAdd and libm, so behind the stand-in
#                                       ref_shim/cufft.h (a HIP include and two typedefs) hipcc reads it unchanged.
#   ref_kernels_driver.hip              ours: extern "C" refk_<kernel>() entry points that restate the launch sites of
#                                       src/process_baseband.cu (which cannot be compiled: cuFFT, psrdada, vdifio).
# Two libraries, the same sources:
#   _ref/libref_kernels.so        -ffp-contract=off: the compiler's strict reading; tests/test_gpu_ref_kernels.py holds
#                                 pb_oracle.c to it kernel by kernel, bit for bit
#   _ref/libref_kernels_fmad.so   -ffp-contract=fast: a real compiler's choice of which a*b+c to fuse, in place of the
#                                 guess behind liboracle_fmad.so; used to count the codes that choice moves
# -fvisibility=hidden: only refk_* is exported -- the reference's kernel names (kurtosis, pscrunch, ...) stay out of a
# process that also holds libpb_hip.so; hipcc gives each kernel's host-side handle default visibility all the same, so
# the linker's version script ref_kernels.map makes everything but refk_* local.  Division and sqrt correctly rounded
# (written out), no fast-math, no xnack+.
# Built in the build container only (/root/reference does not exist on the GPU box); the output stays out of git
# history (.gitignore) but travels with the snapshot.  Test infrastructure: nothing in the product links or loads it.
REF ?= /root/reference/src
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
REFK_FLAGS = -x hip --offload-arch=$(ARCH) -O2 -fPIC -shared -fvisibility=hidden -fno-fast-math \
             -fhip-fp32-correctly-rounded-divide-sqrt -Wl,--version-script=ref_kernels.map -Iref_shim -I$(REF)
REFK_SRC = ref_kernels_driver.hip $(REF)/pb_kernels.cu
REFK_DEP = $(REFK_SRC) $(REF)/process_baseband.h ref_shim/cufft.h ref_kernels.mk ref_kernels.map

all: _ref/libref_kernels.so _ref/libref_kernels_fmad.so

_ref/libref_kernels.so: $(REFK_DEP)
	mkdir -p _ref
	$(HIPCC) $(REFK_FLAGS) -ffp-contract=off -o $@ $(REFK_SRC)

_ref/libref_kernels_fmad.so: $(REFK_DEP)
	mkdir -p _ref
	$(HIPCC) $(REFK_FLAGS) -ffp-contract=fast -o $@ $(REFK_SRC)
