// sample_pdf_sample.h -- ONE SAMPLE of sample_pdf, shared by the kernels and the host loop of implicit.hip (as box3d_geom.h is shared by
// box3d.hip's): the contract of the reference's compiled CPU operator with its binary search (implicit_abi.h: p3di_sample_pdf).
// Plain float32 expressions, no FMA (the build has -ffp-contract=off), an IEEE division; every index stays inside [0, n_bins).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define P3D_HD __host__ __device__ __forceinline__
#else
#define P3D_HD inline
#endif

namespace p3d {

// std::lower_bound over partial[0 .. n_bins - 1): the first i with !(partial[i] < v), n_bins - 1 if there is none.  Written out as the
// standard's halving loop so that unordered data (a NaN among the sums) takes the same steps on the host and on the device.
P3D_HD int64_t sample_pdf_lower_bound(const float* partial, int64_t n_bins, float v) {
  int64_t first = 0, len = n_bins - 1;
  while (len > 0) {
    const int64_t half = len >> 1, mid = first + half;
    if (partial[mid] < v) {
      first = mid + 1;
      len = len - half - 1;
    } else {
      len = half;
    }
  }
  return first;
}

// partial: the row's running sums (n_bins); weights (n_bins) and bins (n_bins + 1): the row's; total = partial[n_bins - 1] + eps.
P3D_HD float sample_pdf_one(const float* partial, const float* weights, const float* bins, int64_t n_bins, float total, float eps,
                            float u) {
  float uniform = total * u;
  const int64_t i = sample_pdf_lower_bound(partial, n_bins, uniform);
  if (i > 0) uniform = uniform - partial[i - 1];
  const float bin_start = bins[i], bin_end = bins[i + 1], w = weights[i];
  if (uniform > w) return bin_end;
  if (w > eps) return bin_start + (uniform / w) * (bin_end - bin_start);
  return bin_start;
}

}  // namespace p3d
