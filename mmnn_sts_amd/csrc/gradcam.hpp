// Shared piece of the two Grad-CAM paths (gradcam.hip, gradcam_unimodal.hip).
#pragma once
#include "../../include/mmnn_sts.h"
#include "common.hpp"
#include "reduce.hpp"

namespace mmnn {

// Trilinear up-sampling (F.interpolate, align_corners=False) of `maps` low-resolution maps heat [maps][d*h*w] to
// out [maps][D][H][W]: gradcam_upsample_kernel, one grid row (blockIdx.y) per map.
int launch_gradcam_upsample(int d, int h, int w, int D, int H, int W, int maps, const float* heat, float* out, hipStream_t st);

}  // namespace mmnn
