// Typed voxel loads and the slope / inter scaling of the scan ingest, shared by every kernel that reads a scan or a mask in its on-disk
// type (csrc/ingest.hip, csrc/radiomics.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

namespace mmnn {

struct IgScale {
  double slope, inter;
  int on;                                   // 0: the raw value is the value
};

#if defined(__HIPCC__)
template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) IgVec { T e[VEC]; };

template <typename T, int VEC>
__device__ __forceinline__ void ig_load_t(const void* base, long idx, double (&out)[VEC]) {
  const IgVec<T, VEC> v = *reinterpret_cast<const IgVec<T, VEC>*>(static_cast<const T*>(base) + idx);
#pragma unroll
  for (int k = 0; k < VEC; ++k) out[k] = (double)v.e[k];
}

// VEC consecutive voxels starting at element `idx` (a multiple of VEC when VEC > 1), widened to fp64 (exact for every supported type).
// The type code is the same in every lane: a uniform branch.
template <int VEC>
__device__ __forceinline__ void ig_load(const void* base, int code, long idx, double (&out)[VEC]) {
  switch (code) {
    case 2:   ig_load_t<uint8_t, VEC>(base, idx, out); break;
    case 4:   ig_load_t<int16_t, VEC>(base, idx, out); break;
    case 8:   ig_load_t<int32_t, VEC>(base, idx, out); break;
    case 16:  ig_load_t<float, VEC>(base, idx, out); break;
    case 64:  ig_load_t<double, VEC>(base, idx, out); break;
    case 256: ig_load_t<int8_t, VEC>(base, idx, out); break;
    case 512: ig_load_t<uint16_t, VEC>(base, idx, out); break;
    default:  ig_load_t<uint32_t, VEC>(base, idx, out); break;   // 768 (the host admits no other code)
  }
}

// raw * slope + inter as numpy evaluates it: two roundings
__device__ __forceinline__ double ig_scaled(double raw, const IgScale& s) {
  return s.on ? __dadd_rn(__dmul_rn(raw, s.slope), s.inter) : raw;
}
#endif  // __HIPCC__

inline int ig_type_size(int code) {
  switch (code) {
    case 2: case 256: return 1;
    case 4: case 512: return 2;
    case 8: case 16: case 768: return 4;
    case 64: return 8;
    default: return 0;
  }
}

// nibabel's reading of scl_slope / scl_inter: a slope of 0, NaN or +-inf switches scaling off; a non-finite inter is 0.  The header's
// float32 values are widened to fp64 before they meet a voxel.
inline IgScale ig_scale(float slope, float inter) {
  IgScale s{1.0, 0.0, 0};
  if (slope == 0.f || !std::isfinite(slope)) return s;
  s.slope = (double)slope;
  s.inter = std::isfinite(inter) ? (double)inter : 0.0;
  s.on = !(s.slope == 1.0 && s.inter == 0.0);
  return s;
}

}  // namespace mmnn
