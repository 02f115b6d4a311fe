#include <hip/hip_runtime.h>
typedef float cufftReal;
typedef float2 cufftComplex;
