// 3x3x3 weight-gradient kernels: instantiations + launches (its own translation unit: the kernels are heavily unrolled and this
// file and wgrad_k1.hip are the two longest compiles of the build).  Host-side validation and split selection: wgrad.hip.
#include <algorithm>

#include "wgrad.hpp"

namespace mmnn {

template <int PRO_X, int TD, int TH, int TW>
static int launch3_batched(const WgradArgs* host, const WgradArgs* dev, int count, uint64_t seed, hipStream_t stream) {
  using C = Wg3Cfg<TD, TH, TW>;
  constexpr auto kern = wgrad3_batched_kernel<PRO_X, TD, TH, TW>;
  const size_t smem = C::smem_bytes();
  if (int rc = allow_dynamic_lds<kern>(smem)) return rc;
  int gx = 1, gy = 1;
  bool uniform = true;
  for (int i = 0; i < count; ++i) {
    gx = std::max(gx, host[i].nsplit); gy = std::max(gy, cdiv(host[i].Cin, 32));
    uniform = uniform && host[i].nsplit == host[0].nsplit && cdiv(host[i].Cin, 32) == cdiv(host[0].Cin, 32);
  }
  if (uniform && gy > 1) {
    const long ngroups = (long)count * gx;                       // (layer, split) pairs; each owns gy blocks on one XCD
    const long blocks = 8l * gy * ((ngroups + 7) / 8);
    MMNN_REQUIRE(blocks < (1l << 31), "wgrad batch: grid out of range");
    MMNN_LAUNCH(kern, dim3((unsigned)blocks), dim3(C::NTHREADS), smem, stream, dev, seed, gx, gy, (int)ngroups);
  } else {
    MMNN_LAUNCH(kern, dim3(gx, gy, count), dim3(C::NTHREADS), smem, stream, dev, seed, gx, gy, 0);
  }
  MMNN_HIP(hipGetLastError());
  return 0;
}

int wgrad3_launch_batched(const WgradArgs* host, const WgradArgs* dev, int count, uint64_t seed, hipStream_t stream) {
  const WgradArgs& f = host[0];
  if (f.W > 16) return launch3_batched<PRO_BNRELU, 1, 2, 32>(host, dev, count, seed, stream);
  if (f.W > 8) return launch3_batched<PRO_BNRELU, 1, 4, 16>(host, dev, count, seed, stream);
  if (f.W > 4) return launch3_batched<PRO_BNRELU, 2, 4, 8>(host, dev, count, seed, stream);
  return launch3_batched<PRO_BNRELU, 4, 4, 4>(host, dev, count, seed, stream);
}

}  // namespace mmnn
