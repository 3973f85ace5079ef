// ResNet-152 up to res5c (He et al., as deployed in Caffe), exact fp32, on the haloed NHWC
// activations of kernels_vgg.hip.  Batch-norm and scale are folded into the convolutions on the host, so a
// layer is convolution + bias (+ residual) (+ ReLU).  The 3x3 convolutions of the bottlenecks are
// launch_vgg_conv3, unchanged; what ResNet adds is here:
//
//   * resnet_stem_kernel: conv1, 7x7 stride 2 pad 3, Cin = 3 (K = 147): 0.94 GFLOP and 12.8 MB of output per
//     448 x 448 image -- as conv1_1 of VGG, too thin a K for the MFMA tile and close to write bound, so plain
//     FMAs, one thread per (output pixel, 4 output channels); the Cout / 4 lanes of a pixel write its
//     contiguous output bytes and read the same image bytes (a broadcast), the weights come from L1/L2.  It
//     reads the RAW image and subtracts the mean itself, before the padding: a tap outside the image is
//     skipped, not -mean * w.
//   * resnet_pool_kernel: pool1, 3x3 stride 2 pad 0 in Caffe's ceil mode.  The last window of an extent may
//     overhang the image by one row / column; it is clipped, so the halo zero never wins over negative values.
//   * resnet_conv1x1_kernel: a GEMM on the 128 x 128 x 32 LDS-DMA tile (gemm_dma_tile.h).  Rows = OUTPUT pixels
//     in raster order, k = the Cin contiguous floats of input pixel (n, stride h, stride w): an A row is one
//     run, addressed straight in the haloed input -- stride 2 only changes the per-row base, nothing is
//     gathered.  The [1][1][Cin][Cout] HWIO weights are the row-major [Cin][Cout] B matrix (PK-packed at
//     commit).  Epilogue: + bias, + residual (a second haloed buffer at the output's coordinates), ReLU.
#include <algorithm>
#include <atomic>

#include "device_utils.h"
#include "gemm_dma_tile.h"
#include "resnet_kernels.h"

namespace n2nmn {

namespace {

using namespace dma_tile;

__global__ __launch_bounds__(DMA_THREADS) void resnet_conv1x1_kernel(ResConv1Args a) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  __shared__ uint32_t opix[DM];                  // haloed output pixel of every tile row (~0u: no such row)
  // workgroup -> tile as vgg_conv3_kernel: runs of 8 consecutive tiles stay on one XCD
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

  if (tid < DM) {                                // (visible after the first stage's barrier)
    const int gm = m0 + tid;
    const int n = gm / HW, rem = gm - n * HW, h = rem / a.W, x = rem - h * a.W;
    opix[tid] = gm < M ? (uint32_t)((n * (a.H + 2) + h + 1) * (a.W + 2) + x + 1) : ~0u;
  }

  // A rows: tile row -> output pixel (n, h, w) -> byte offset of haloed input pixel (n, stride h, stride w);
  // rows past M re-read the last pixel (never stored)
  uint32_t a_off[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = a_row(w, u, lane);
    const int gm = min(m0 + row, M - 1);
    const int n = gm / HW, rem = gm - n * HW, h = rem / a.W, x = rem - h * a.W;
    a_off[u] = ((uint32_t)((n * (a.Hin + 2) + a.stride * h + 1) * (a.Win + 2) + a.stride * x + 1) * (uint32_t)a.Cin +
                4u * a_chunk(row, lane)) * 4u;
  }
  const float* const Ap = a.in;
  const uint32_t b_off = ((uint32_t)w * (uint32_t)a.Np + (uint32_t)n0 + (uint32_t)lane) * 16u;
  const uint32_t b_slab = 8u * (uint32_t)a.Np * 16u;
  f32x16 acc[2];
  accumulate(smem, a.Cin / DK, a.Bp, b_off, b_slab, [&](int s, uint32_t st) {
#pragma unroll
    for (int u = 0; u < 2; ++u) glds16(Ap, a_off[u] + (uint32_t)s * (DK * 4u), st + a_piece_lds(w, u));
  }, acc);

  // ---- epilogue: bias (+ residual) (+ ReLU) into the interior of the haloed output ----------------------
  const int li = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
    const int col = n0 + wn * 64 + 32 * t2 + li;
    if (col >= a.Cout) continue;
    const float bias = a.bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t pix = opix[wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh];
      if (pix == ~0u) continue;
      const size_t at = (size_t)pix * a.Cout + col;
      float v = acc[t2][r] + bias;
      if (a.res) v += a.res[at];
      a.out[at] = a.relu ? fmaxf(v, 0.f) : v;
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void resnet_stem_kernel(const T* __restrict__ img, int N, int H, int W,
                                                         const float* __restrict__ Wt, const float* __restrict__ bias,
                                                         float mean0, float mean1, float mean2, int Cout,
                                                         float* __restrict__ out) {
  const int Ho = resnet_half(H), Wo = resnet_half(W), C4 = Cout / 4;
  const size_t total = (size_t)N * Ho * Wo * C4;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c4 = (int)(i % C4);
  size_t p = i / C4;
  const int x = (int)(p % Wo); p /= Wo;
  const int y = (int)(p % Ho);
  const int n = (int)(p / Ho);
  const float mean[3] = {mean0, mean1, mean2};
  float4 acc = *reinterpret_cast<const float4*>(bias + 4 * c4);
  for (int dy = 0; dy < 7; ++dy) {
    const int hh = 2 * y + dy - 3;
    if (hh < 0 || hh >= H) continue;
#pragma unroll
    for (int dx = 0; dx < 7; ++dx) {
      const int ww = 2 * x + dx - 3;
      if (ww < 0 || ww >= W) continue;
      const T* px = img + (((size_t)n * H + hh) * W + ww) * 3;
      const float* wt = Wt + (size_t)((dy * 7 + dx) * 3) * Cout + 4 * c4;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = (float)px[c] - mean[c];
        const float4 q = *reinterpret_cast<const float4*>(wt + (size_t)c * Cout);
        acc.x = fmaf(v, q.x, acc.x); acc.y = fmaf(v, q.y, acc.y);
        acc.z = fmaf(v, q.z, acc.z); acc.w = fmaf(v, q.w, acc.w);
      }
    }
  }
  acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f);
  *reinterpret_cast<float4*>(out + (((size_t)n * (Ho + 2) + y + 1) * (Wo + 2) + x + 1) * Cout + 4 * c4) = acc;
}

__global__ __launch_bounds__(256) void resnet_pool_kernel(const float* __restrict__ in, int N, int H, int W, int C,
                                                         float* __restrict__ out) {
  const int Ho = resnet_pool_out(H), Wo = resnet_pool_out(W), C4 = C / 4;
  const size_t total = (size_t)N * Ho * Wo * C4;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c4 = (int)(i % C4);
  size_t p = i / C4;
  const int x = (int)(p % Wo); p /= Wo;
  const int y = (int)(p % Ho);
  const int n = (int)(p / Ho);
  // window rows 2y .. 2y + 2 and columns 2x .. 2x + 2, clipped to the image (its first pixel always exists)
  const int ny = min(3, H - 2 * y), nx = min(3, W - 2 * x);
  const float* src = in + (((size_t)n * (H + 2) + 2 * y + 1) * (W + 2) + 2 * x + 1) * C + 4 * c4;
  float4 m = *reinterpret_cast<const float4*>(src);
  for (int dy = 0; dy < ny; ++dy)
    for (int dx = 0; dx < nx; ++dx) {
      const float4 v = *reinterpret_cast<const float4*>(src + ((size_t)dy * (W + 2) + dx) * C);
      m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
  *reinterpret_cast<float4*>(out + (((size_t)n * (Ho + 2) + y + 1) * (Wo + 2) + x + 1) * C + 4 * c4) = m;
}

inline unsigned blocks256(size_t total) { return (unsigned)((total + 255) / 256); }

}  // namespace

bool resnet_conv1x1_supported(const ResConv1Args& a) {
  // A and B are addressed with 32-bit byte offsets from their bases; output pixels with 32-bit indices
  const bool geom = a.stride == 1 ? (a.H == a.Hin && a.W == a.Win)
                                  : (a.stride == 2 && a.H == resnet_half(a.Hin) && a.W == resnet_half(a.Win));
  return a.N > 0 && a.Hin > 0 && a.Win > 0 && geom && a.Cin > 0 && a.Cin % DK == 0 && a.Cout > 0 &&
         a.Np % DN == 0 && a.Np >= a.Cout && vgg_halo_floats(a.N, a.Hin, a.Win, a.Cin) * 4 < ((size_t)1 << 32) &&
         (size_t)a.Cin * a.Np * 4 < ((size_t)1 << 32) && vgg_halo_floats(a.N, a.H, a.W, 1) < ((size_t)1 << 31);
}

void launch_resnet_conv1x1(const ResConv1Args& a, hipStream_t s) {
  const int M = a.N * a.H * a.W;
  const int tiles = ((a.Cout + DN - 1) / DN) * ((M + DM - 1) / DM);
  static std::atomic<uint64_t> attr{0};
  ensure_dynamic_lds(reinterpret_cast<const void*>(resnet_conv1x1_kernel), 2 * DSTAGE, attr);
  hipLaunchKernelGGL(resnet_conv1x1_kernel, dim3((tiles + 63) / 64 * 64), dim3(DMA_THREADS), 2 * DSTAGE, s, a);
}

void launch_resnet_stem(const void* img, int is_uint8, int N, int H, int W, const float* Wt, const float* bias,
                        const float mean[3], int Cout, float* out, hipStream_t s) {
  const size_t total = (size_t)N * resnet_half(H) * resnet_half(W) * (Cout / 4);
  if (is_uint8)
    hipLaunchKernelGGL(resnet_stem_kernel<uint8_t>, dim3(blocks256(total)), dim3(256), 0, s,
                       static_cast<const uint8_t*>(img), N, H, W, Wt, bias, mean[0], mean[1], mean[2], Cout, out);
  else
    hipLaunchKernelGGL(resnet_stem_kernel<float>, dim3(blocks256(total)), dim3(256), 0, s,
                       static_cast<const float*>(img), N, H, W, Wt, bias, mean[0], mean[1], mean[2], Cout, out);
}

void launch_resnet_pool(const float* in, int N, int H, int W, int C, float* out, hipStream_t s) {
  const size_t total = (size_t)N * resnet_pool_out(H) * resnet_pool_out(W) * (C / 4);
  hipLaunchKernelGGL(resnet_pool_kernel, dim3(blocks256(total)), dim3(256), 0, s, in, N, H, W, C, out);
}

}  // namespace n2nmn
