// Launchers of the compact feature feed (kernels_feed.hip; include/n2nmn.h section 11): image features cross the
// link as fp16 and / or one row per image and are widened / gathered into the fp32 slot the kernels read.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace n2nmn {

// dst[n][p][0:D] = (float) src[index ? index[n] : n][p][0:D]; elements D .. stride-1 of a destination pixel are
// not written.  src_f16 != 0: src holds IEEE halves, else fp32.  A row whose index is outside [0, src_rows) is
// written as zeros and reads nothing.  pixels * D and pixels * stride < 2^31, N > 0 (the caller checks).  Picks the
// 16-byte path when D, stride and both pointers allow it, else one element per lane; returns which (1 / 0).
int launch_features_expand(const void* src, int src_f16, int64_t src_rows, const int32_t* index, int64_t N,
                           int64_t pixels, int64_t D, int64_t stride, float* dst, hipStream_t s);

// dst[i] = half(src[i]), round to nearest even; n > 0.  16-byte path when both pointers are 16-byte aligned.
int launch_features_narrow(const float* src, int64_t n, void* dst_f16, hipStream_t s);

}  // namespace n2nmn
