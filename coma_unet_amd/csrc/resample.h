// The nearest-neighbour index map and the nan_to_num of the input pipeline, shared by resample_nn_k (metrics.hip) and the
// fused-source staging of gauss_smooth_k (smooth.hip): both must pick the same source voxel and the same value, bit for bit.
#pragma once
#include "common.h"

// output index -> source index along one axis: continuous index o * new_spacing / old_spacing (in double, like ITK's
// physical-point round trip), rounded half up; -1 outside [-0.5, size - 0.5)
__device__ __forceinline__ int nn_index(int o, double ratio, int size) {
  const double c = (double)o * ratio;                 // continuous input index
  if (!(c >= -0.5 && c < (double)size - 0.5)) return -1;
  return (int)floor(c + 0.5);                         // itk::Math::RoundHalfIntegerUp
}

// torch.nan_to_num defaults: nan -> 0, +-inf -> +-FLT_MAX
__device__ __forceinline__ float nan_to_num_f(float v) {
  if (v != v) return 0.f;
  if (v == INFINITY) return 3.402823466e+38f;
  if (v == -INFINITY) return -3.402823466e+38f;
  return v;
}
