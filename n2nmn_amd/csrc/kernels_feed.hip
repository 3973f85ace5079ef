// The compact feature feed (include/n2nmn.h section 11): image features are the outputs of a frozen extractor, so
// they may be stored and shipped as IEEE halves, and one row per IMAGE serves every question about it.  Both reduce
// to   slot[n] = widen(src[index[n]])   behind a smaller H2D copy; every kernel of both phases keeps reading the
// fp32 [N][H][W][D] slot (or the [N][H][W][Dp] slab of models_vqa, whose coordinate channels are not touched).
//
//   * features_expand_kernel<T, V>: a streaming gather.  A unit of work is 4 x 256 lane-pieces of V elements of one
//     destination row; a workgroup reads the row's source index once per unit (wave-uniform) and strides over the
//     units behind a grid capped at 2048 workgroups.  V = 8 halves (one 16-byte load, two 16-byte stores) or 4
//     floats (one of each) when D, the pixel stride and both pointers allow it, else V = 1.  A unit's loads are all
//     issued before its first store.  Plain stores: the slot's lines stay in the XCD's L2 for the conv_image GEMM
//     that reads them next; a repeated index reads its row from L2.
//   * features_narrow_kernel: fp32 -> half, round to nearest even (v_cvt_f16_f32 in the default rounding and
//     denormal modes: overflow to infinity, subnormal results kept), 8 elements per lane when aligned.
// Widening is v_cvt_f32_f16: exact for every half, subnormals included; a NaN stays a NaN.
#include <algorithm>

#include "feed_kernels.h"

namespace n2nmn {

namespace {

constexpr int FEED_THREADS = 256;
constexpr int FEED_UNROLL = 4;                     // lane-pieces per lane and unit
constexpr int FEED_MAX_GRID = 2048;                // 256 CUs x 8 workgroups; the rest is strided over

template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
  T v[V];
};

// row_pieces = pixels * D / V pieces per row, dpieces = D / V per pixel; dense: stride == D.
template <typename T, int V>
__global__ __launch_bounds__(FEED_THREADS) void features_expand_kernel(
    const T* __restrict__ src, int64_t src_rows, const int32_t* __restrict__ index, int64_t N, uint32_t row_pieces,
    uint32_t dpieces, uint32_t stride, int64_t src_row_elems, int64_t dst_row_elems, int dense, uint32_t chunks,
    float* __restrict__ dst) {
  constexpr int W = V < 4 ? V : 4;                 // floats per store
  const int64_t units = N * chunks;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t n = u / chunks;
    const uint32_t c = (uint32_t)(u - n * chunks);
    const int64_t r = index ? (int64_t)index[n] : n;
    const bool ok = r >= 0 && r < src_rows;        // outside: the row is zeros and nothing is read
    const T* s = src + (ok ? r : 0) * src_row_elems;
    float* d = dst + n * dst_row_elems;
    const uint32_t p0 = c * (FEED_UNROLL * FEED_THREADS) + threadIdx.x;
    Pack<T, V> in[FEED_UNROLL];
#pragma unroll
    for (int k = 0; k < FEED_UNROLL; ++k) {
      const uint32_t p = p0 + k * FEED_THREADS;
      if (ok && p < row_pieces) {
        in[k] = *reinterpret_cast<const Pack<T, V>*>(s + (size_t)p * V);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) in[k].v[j] = (T)0;
      }
    }
#pragma unroll
    for (int k = 0; k < FEED_UNROLL; ++k) {
      const uint32_t p = p0 + k * FEED_THREADS;
      if (p >= row_pieces) continue;
      size_t off = (size_t)p * V;
      if (!dense) {
        const uint32_t px = p / dpieces;
        off = (size_t)px * stride + (size_t)(p - px * dpieces) * V;
      }
#pragma unroll
      for (int h = 0; h < V / W; ++h) {
        Pack<float, W> o;
#pragma unroll
        for (int j = 0; j < W; ++j) o.v[j] = (float)in[k].v[h * W + j];
        *reinterpret_cast<Pack<float, W>*>(d + off + h * W) = o;
      }
    }
  }
}

// groups of 8 behind a grid-stride loop; the n % 8 tail (and everything, when vec == 0) one element per lane
__global__ __launch_bounds__(FEED_THREADS) void features_narrow_kernel(const float* __restrict__ src, int64_t n,
                                                                        _Float16* __restrict__ dst, int vec) {
  const int64_t tid = (int64_t)blockIdx.x * FEED_THREADS + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * FEED_THREADS;
  int64_t done = 0;
  if (vec) {
    const int64_t groups = n / 8;
    for (int64_t g = tid; g < groups; g += step) {
      const Pack<float, 4> a = *reinterpret_cast<const Pack<float, 4>*>(src + g * 8);
      const Pack<float, 4> b = *reinterpret_cast<const Pack<float, 4>*>(src + g * 8 + 4);
      Pack<_Float16, 8> o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o.v[j] = (_Float16)a.v[j];
        o.v[4 + j] = (_Float16)b.v[j];
      }
      *reinterpret_cast<Pack<_Float16, 8>*>(dst + g * 8) = o;
    }
    done = groups * 8;
  }
  for (int64_t i = done + tid; i < n; i += step) dst[i] = (_Float16)src[i];
}

template <typename T, int V>
void expand_launch(const T* src, int64_t src_rows, const int32_t* index, int64_t N, int64_t pixels, int64_t D,
                   int64_t stride, float* dst, hipStream_t s) {
  const uint32_t row_pieces = (uint32_t)(pixels * D / V);
  const uint32_t per_unit = FEED_UNROLL * FEED_THREADS;
  const uint32_t chunks = (row_pieces + per_unit - 1) / per_unit;
  const int64_t units = N * chunks;
  const int grid = (int)std::min<int64_t>(units, FEED_MAX_GRID);
  hipLaunchKernelGGL((features_expand_kernel<T, V>), dim3(grid), dim3(FEED_THREADS), 0, s, src, src_rows, index, N,
                     row_pieces, (uint32_t)(D / V), (uint32_t)stride, pixels * D, pixels * stride,
                     stride == D ? 1 : 0, chunks, dst);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int launch_features_expand(const void* src, int src_f16, int64_t src_rows, const int32_t* index, int64_t N,
                           int64_t pixels, int64_t D, int64_t stride, float* dst, hipStream_t s) {
  const bool vec = D % (src_f16 ? 8 : 4) == 0 && stride % 4 == 0 && aligned16(src) && aligned16(dst);
  if (src_f16) {
    const _Float16* p = static_cast<const _Float16*>(src);
    if (vec) expand_launch<_Float16, 8>(p, src_rows, index, N, pixels, D, stride, dst, s);
    else expand_launch<_Float16, 1>(p, src_rows, index, N, pixels, D, stride, dst, s);
  } else {
    const float* p = static_cast<const float*>(src);
    if (vec) expand_launch<float, 4>(p, src_rows, index, N, pixels, D, stride, dst, s);
    else expand_launch<float, 1>(p, src_rows, index, N, pixels, D, stride, dst, s);
  }
  return vec ? 1 : 0;
}

int launch_features_narrow(const float* src, int64_t n, void* dst_f16, hipStream_t s) {
  const int vec = aligned16(src) && aligned16(dst_f16) ? 1 : 0;
  const int64_t lanes = vec ? (n + 7) / 8 : n;
  const int grid = (int)std::min<int64_t>((lanes + FEED_THREADS - 1) / FEED_THREADS, FEED_MAX_GRID);
  hipLaunchKernelGGL(features_narrow_kernel, dim3(grid), dim3(FEED_THREADS), 0, s, src, n,
                     static_cast<_Float16*>(dst_f16), vec);
  return vec;
}

}  // namespace n2nmn
