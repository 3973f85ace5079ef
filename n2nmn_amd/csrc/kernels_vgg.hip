// VGG-16 up to pool5 (models_clevr/vgg_net.py:16-56 <- exp_clevr/data/extract_visual_features_vgg_pool5.py):
// 13 SAME 3x3 convolutions with bias + ReLU (util/cnn.py conv_relu_layer) and five 2x2 stride-2 SAME max-pools
// (util/cnn.py pooling_layer), exact fp32.
//
// Every activation is NHWC with a one-pixel zero halo ([N][H + 2][W + 2][C], vgg_kernels.h).  A SAME 3x3
// convolution over it reads no pixel outside its buffer and needs no bounds test: an out-of-image tap reads a
// halo zero, which is the zero TF pads the ACTIVATION with.  Kernels write interiors only, so a halo zeroed once
// stays zero for as long as the geometry stays.
//
//   * vgg_conv3_kernel: implicit GEMM on gemm_dma_kernel's 128 x 128 x 32 LDS-DMA tile (gemm_dma_tile.h).
//     Rows = output pixels (n, h, w) in raster order, columns = Cout, k = (dy, dx, c): the reference's HWIO
//     weights [3][3][Cin][Cout] ARE the row-major [9 Cin][Cout] B matrix (PK-packed once, at commit).  With
//     NHWC input and Cin % 32 == 0 a 32-wide k stage lies inside one tap, and for one dy the three taps
//     dx = 0, 1, 2 are 3 Cin CONTIGUOUS floats of the input (pixels (h + dy, w .. w + 2) of the haloed buffer):
//     the A operand of an output pixel is three contiguous runs, and a stage's A rows are the same 128-byte
//     row pieces the dense GEMM stages -- only the per-row base (the pixel) and a wave-uniform k offset
//     differ.  No im2col matrix exists anywhere.
//   * vgg_conv1_kernel: conv1_1 (Cin = 3, K = 27) is 0.5 GFLOP and 39 MB of output per 320 x 480 image: write
//     bound, so plain FMAs, one thread per (pixel, 4 output channels), 16 lanes cover a pixel's 256 contiguous
//     output bytes.  It reads the RAW image (uint8 or fp32) and subtracts channel_mean itself; TF subtracts
//     before it pads, so an out-of-image tap contributes 0, not -mean * w: the tap is skipped.
//   * vgg_pool_kernel: a kernel of its own (DESIGN.md section 15 says why), one thread per (output pixel,
//     4 channels), the window clipped to the image.
#include <algorithm>
#include <atomic>

#include "device_utils.h"
#include "gemm_dma_tile.h"
#include "vgg_kernels.h"

namespace n2nmn {

namespace {

using namespace dma_tile;

__global__ __launch_bounds__(DMA_THREADS) void vgg_conv3_kernel(VggConvArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  __shared__ uint32_t opix[DM];                  // haloed output pixel of every tile row (~0u: no such row)
  // consecutive workgroup ids go round-robin over the 8 XCDs (as gemm_dma_kernel): runs of 8 consecutive
  // tiles -- neighbouring row tiles, which share their halo rows, or the column tiles of a row tile -- stay
  // on one XCD
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int t = (((slot >> 3) << 3) + xcd) * 8 + (slot & 7);
  const int HW = a.H * a.W, M = a.N * HW;
  const int gx = (a.Cout + DN - 1) / DN;
  if (t >= gx * ((M + DM - 1) / DM)) return;
  const int bx = t % gx, by = t / gx;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int m0 = by * DM, n0 = bx * DN;
  const int Wh = a.W + 2;

  if (tid < DM) {                                // (visible after the first stage's barrier)
    const int gm = m0 + tid;
    const int n = gm / HW, rem = gm - n * HW, h = rem / a.W, x = rem - h * a.W;
    opix[tid] = gm < M ? (uint32_t)((n * (a.H + 2) + h + 1) * Wh + x + 1) : ~0u;
  }

  // A rows: tile row -> output pixel (n, h, w) -> byte offset of haloed input pixel (n, h, w), the tap
  // (dy, dx) = (0, 0); rows past M re-read the last pixel (never stored)
  uint32_t a_off[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = a_row(w, u, lane);
    const int gm = min(m0 + row, M - 1);
    const int n = gm / HW, rem = gm - n * HW, h = rem / a.W, x = rem - h * a.W;
    a_off[u] = ((uint32_t)((n * (a.H + 2) + h) * Wh + x) * (uint32_t)a.Cin + 4u * a_chunk(row, lane)) * 4u;
  }
  // k offset of stage s (bytes, wave-uniform): the stages of one dy walk 3 Cin contiguous floats, then the
  // run of the next dy starts one haloed row further.  accumulate() issues the stages in order.
  const int per_dy = 3 * a.Cin / DK;
  const uint32_t dy_jump = (uint32_t)(a.W - 1) * (uint32_t)a.Cin * 4u;
  uint32_t koff = 0;
  int left = per_dy;
  const float* const Ap = a.in;
  const uint32_t b_off = ((uint32_t)w * (uint32_t)a.Np + (uint32_t)n0 + (uint32_t)lane) * 16u;
  const uint32_t b_slab = 8u * (uint32_t)a.Np * 16u;
  f32x16 acc[2];
  accumulate(smem, 9 * a.Cin / DK, a.Bp, b_off, b_slab, [&](int, uint32_t st) {
#pragma unroll
    for (int u = 0; u < 2; ++u) glds16(Ap, a_off[u] + koff, st + a_piece_lds(w, u));
    koff += DK * 4u;
    if (--left == 0) { left = per_dy; koff += dy_jump; }
  }, acc);

  // ---- epilogue: bias + ReLU into the interior of the haloed output ------------------------------------
  const int li = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
    const int col = n0 + wn * 64 + 32 * t2 + li;
    if (col >= a.Cout) continue;
    const float bias = a.bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t pix = opix[wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh];
      if (pix != ~0u) a.out[(size_t)pix * a.Cout + col] = fmaxf(acc[t2][r] + bias, 0.f);
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void vgg_conv1_kernel(const T* __restrict__ img, int N, int H, int W,
                                                       const float* __restrict__ Wt, const float* __restrict__ bias,
                                                       float* __restrict__ out) {
  const int cg = threadIdx.x & 15;               // output channels 4 cg .. 4 cg + 3
  float4 wt[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) wt[k] = *reinterpret_cast<const float4*>(Wt + k * 64 + 4 * cg);
  const float4 b = *reinterpret_cast<const float4*>(bias + 4 * cg);
  const float mean[3] = {123.68f, 116.779f, 103.939f};        // vgg_net.py:14 channel_mean
  const long long total = (long long)N * H * W;
  for (long long p = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); p < total; p += (long long)gridDim.x * 16) {
    const int n = (int)(p / ((long long)H * W));
    const int rem = (int)(p - (long long)n * H * W);
    const int h = rem / W, x = rem - h * W;
    float4 acc = b;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int hh = h + dy - 1;
      if (hh < 0 || hh >= H) continue;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int ww = x + dx - 1;
        if (ww < 0 || ww >= W) continue;
        const T* px = img + (((size_t)n * H + hh) * W + ww) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float v = (float)px[c] - mean[c];
          const float4 q = wt[(dy * 3 + dx) * 3 + c];
          acc.x = fmaf(v, q.x, acc.x); acc.y = fmaf(v, q.y, acc.y);
          acc.z = fmaf(v, q.z, acc.z); acc.w = fmaf(v, q.w, acc.w);
        }
      }
    }
    acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f);
    *reinterpret_cast<float4*>(out + (((size_t)n * (H + 2) + h + 1) * (W + 2) + x + 1) * 64 + 4 * cg) = acc;
  }
}

__global__ __launch_bounds__(256) void vgg_pool_kernel(const float* __restrict__ in, int N, int H, int W, int C,
                                                      float* __restrict__ out, int out_halo) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, C4 = C / 4;
  const size_t total = (size_t)N * Ho * Wo * C4;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c4 = (int)(i % C4);
  size_t p = i / C4;
  const int x = (int)(p % Wo); p /= Wo;
  const int y = (int)(p % Ho);
  const int n = (int)(p / Ho);
  const float* src = in + (((size_t)n * (H + 2) + 2 * y + 1) * (W + 2) + 2 * x + 1) * C + 4 * c4;
  float4 m = *reinterpret_cast<const float4*>(src);
  auto take = [&](const float* q) {
    const float4 v = *reinterpret_cast<const float4*>(q);
    m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
  };
  const bool right = 2 * x + 1 < W, below = 2 * y + 1 < H;
  if (right) take(src + C);
  if (below) take(src + (size_t)(W + 2) * C);
  if (right && below) take(src + (size_t)(W + 3) * C);
  float* dst = out_halo ? out + (((size_t)n * (Ho + 2) + y + 1) * (Wo + 2) + x + 1) * C + 4 * c4
                        : out + (((size_t)n * Ho + y) * Wo + x) * C + 4 * c4;
  *reinterpret_cast<float4*>(dst) = m;
}

template <bool TO_HALO>
__global__ __launch_bounds__(256) void vgg_repad_kernel(const float* __restrict__ src, int N, int H, int W, int C,
                                                       float* __restrict__ dst) {
  const int C4 = C / 4;
  const size_t total = (size_t)N * H * W * C4;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c4 = (int)(i % C4);
  size_t p = i / C4;
  const int x = (int)(p % W); p /= W;
  const int y = (int)(p % H);
  const int n = (int)(p / H);
  const size_t dense = (((size_t)n * H + y) * W + x) * C + 4 * c4;
  const size_t halo = (((size_t)n * (H + 2) + y + 1) * (W + 2) + x + 1) * C + 4 * c4;
  if (TO_HALO) *reinterpret_cast<float4*>(dst + halo) = *reinterpret_cast<const float4*>(src + dense);
  else *reinterpret_cast<float4*>(dst + dense) = *reinterpret_cast<const float4*>(src + halo);
}

inline unsigned blocks256(size_t total) { return (unsigned)((total + 255) / 256); }

}  // namespace

bool vgg_conv3_supported(const VggConvArgs& a) {
  // A and B are addressed with 32-bit byte offsets from their bases; a k stage must lie inside one tap
  return a.N > 0 && a.H > 0 && a.W > 0 && a.Cin > 0 && a.Cin % DK == 0 && a.Cout > 0 && a.Np % DN == 0 &&
         a.Np >= a.Cout && vgg_halo_floats(a.N, a.H, a.W, a.Cin) * 4 < ((size_t)1 << 32) &&
         (size_t)9 * a.Cin * a.Np * 4 < ((size_t)1 << 32) &&
         vgg_halo_floats(a.N, a.H, a.W, 1) < ((size_t)1 << 31);
}

void launch_vgg_conv3(const VggConvArgs& a, hipStream_t s) {
  const int M = a.N * a.H * a.W;
  const int tiles = ((a.Cout + DN - 1) / DN) * ((M + DM - 1) / DM);
  static std::atomic<uint64_t> attr{0};
  ensure_dynamic_lds(reinterpret_cast<const void*>(vgg_conv3_kernel), 2 * DSTAGE, attr);
  hipLaunchKernelGGL(vgg_conv3_kernel, dim3((tiles + 63) / 64 * 64), dim3(DMA_THREADS), 2 * DSTAGE, s, a);
}

void launch_vgg_conv1(const void* img, int is_uint8, int N, int H, int W, const float* Wt, const float* bias,
                      float* out, hipStream_t s) {
  const long long total = (long long)N * H * W;
  const unsigned grid = (unsigned)std::min<long long>((total + 15) / 16, 16384);
  if (is_uint8)
    hipLaunchKernelGGL(vgg_conv1_kernel<uint8_t>, dim3(grid), dim3(256), 0, s, static_cast<const uint8_t*>(img), N, H,
                       W, Wt, bias, out);
  else
    hipLaunchKernelGGL(vgg_conv1_kernel<float>, dim3(grid), dim3(256), 0, s, static_cast<const float*>(img), N, H, W,
                       Wt, bias, out);
}

void launch_vgg_pool(const float* in, int N, int H, int W, int C, float* out, int out_halo, hipStream_t s) {
  const size_t total = (size_t)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4);
  hipLaunchKernelGGL(vgg_pool_kernel, dim3(blocks256(total)), dim3(256), 0, s, in, N, H, W, C, out, out_halo);
}

void launch_vgg_pad(const float* dense, int N, int H, int W, int C, float* haloed, hipStream_t s) {
  const size_t total = (size_t)N * H * W * (C / 4);
  hipLaunchKernelGGL(vgg_repad_kernel<true>, dim3(blocks256(total)), dim3(256), 0, s, dense, N, H, W, C, haloed);
}

void launch_vgg_unpad(const float* haloed, int N, int H, int W, int C, float* dense, hipStream_t s) {
  const size_t total = (size_t)N * H * W * (C / 4);
  hipLaunchKernelGGL(vgg_repad_kernel<false>, dim3(blocks256(total)), dim3(256), 0, s, haloed, N, H, W, C, dense);
}

}  // namespace n2nmn
