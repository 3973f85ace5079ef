// C ABI of the compact feature feed (include/n2nmn.h section 11): argument checks and the choice between the
// 16-byte and the one-element path.  Host code only; kernels: kernels_feed.hip.  No handle: both entries run on the
// current device and keep nothing.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/n2nmn.h"
#include "feed_kernels.h"

#include "ctx.h"

using namespace n2nmn;

extern "C" {

int n2nmn_features_expand(const void* src, int src_dtype, int64_t src_rows, const int32_t* index, int64_t N,
                          int64_t pixels, int64_t D, int64_t dst_pixel_stride, float* dst, n2nmn_stream stream) {
  N2_REQUIRE(src_dtype == N2NMN_FEAT_F32 || src_dtype == N2NMN_FEAT_F16, N2NMN_EINVAL,
             "features_expand: unknown src_dtype " + std::to_string(src_dtype) + " (N2NMN_FEAT_F32, N2NMN_FEAT_F16)");
  N2_REQUIRE(src_rows >= 0 && N >= 0 && pixels >= 0 && D >= 0, N2NMN_EINVAL, "features_expand: negative size");
  N2_REQUIRE(dst_pixel_stride >= D, N2NMN_EINVAL, "features_expand: dst_pixel_stride < D");
  if (N == 0 || pixels == 0 || D == 0) return N2NMN_OK;
  N2_REQUIRE(dst, N2NMN_EINVAL, "features_expand: null dst");
  N2_REQUIRE(src || src_rows == 0, N2NMN_EINVAL, "features_expand: null src with src_rows > 0");
  N2_REQUIRE(index || N <= src_rows, N2NMN_EINVAL, "features_expand: without an index N must not exceed src_rows");
  // positions inside a row are 32-bit in the kernel; rows are addressed in 64 bits
  N2_REQUIRE(pixels <= INT32_MAX / dst_pixel_stride, N2NMN_ECAPACITY,
             "features_expand: a row (pixels * dst_pixel_stride) must stay below 2^31 elements");
  (void)launch_features_expand(src, src_dtype == N2NMN_FEAT_F16, src_rows, index, N, pixels, D, dst_pixel_stride, dst,
                               S(stream));
  return check_launch("features_expand");
}

int n2nmn_features_narrow(const float* src, int64_t n, void* dst_f16, n2nmn_stream stream) {
  N2_REQUIRE(n >= 0, N2NMN_EINVAL, "features_narrow: negative size");
  if (n == 0) return N2NMN_OK;
  N2_REQUIRE(src && dst_f16, N2NMN_EINVAL, "features_narrow: null argument");
  (void)launch_features_narrow(src, n, dst_f16, S(stream));
  return check_launch("features_narrow");
}

}  // extern "C"
