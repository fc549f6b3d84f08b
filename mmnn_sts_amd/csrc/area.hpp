// The window rule of an area resize (torch.nn.functional.interpolate(mode="area") = adaptive average pooling), shared by the
// transforms (csrc/transforms.hip: Resize, RandZoom) and the scan ingest (csrc/ingest.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace mmnn {

// window of intermediate index j (extent m) over a source axis of extent n: adaptive_avg_pool's [floor(j n / m), ceil((j + 1) n / m))
__device__ __forceinline__ void area_window(int o, int n, int m, int off, int& b, int& e) {
  const int j = min(max(o + off, 0), m - 1);
  b = (j * n) / m;
  e = ((j + 1) * n + m - 1) / m;
}

}  // namespace mmnn
