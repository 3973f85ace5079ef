// Launchers of the VGG-16 pool5 feature extractor (kernels_vgg.hip; models_clevr/vgg_net.py:16-56).
// Activations are NHWC with a one-pixel zero halo: pixel (n, h, w) of an [N][H][W][C] activation lives at
// [n][h + 1][w + 1][:] of an [N][H + 2][W + 2][C] buffer whose border pixels are zero.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace n2nmn {

inline size_t vgg_halo_floats(int N, int H, int W, int C) { return (size_t)N * (H + 2) * (W + 2) * C; }

// conv1_1: out = relu(conv3x3_SAME(img - channel_mean) + bias), Cin = 3, Cout = 64.  img [N][H][W][3] uint8
// or fp32 (no halo); Wt [27][64] = the reference's [3][3][3][64]; out haloed.
void launch_vgg_conv1(const void* img, int is_uint8, int N, int H, int W, const float* Wt, const float* bias,
                      float* out, hipStream_t s);

// out = relu(conv3x3_SAME(in) + bias) as an implicit GEMM on the 128 x 128 LDS-DMA tile: M = N H W output
// pixels, N = Cout, K = 9 Cin.  in / out haloed; Bp = PK pack [9 Cin / 4][Np][4] of the reference's
// [3][3][Cin][Cout], Np = round_up(Cout, 128).
struct VggConvArgs {
  const float* in; float* out; const float* Bp; const float* bias;
  int N, H, W, Cin, Cout, Np;
};
bool vgg_conv3_supported(const VggConvArgs& a);
void launch_vgg_conv3(const VggConvArgs& a, hipStream_t s);

// 2x2 stride-2 max-pool, TF SAME: out extent ceil(n / 2), the last window of an odd extent has one row /
// column (the pad never takes part).  in haloed [N][H + 2][W + 2][C]; out haloed, or dense [N][Ho][Wo][C]
// when out_halo == 0.  C % 4 == 0.
void launch_vgg_pool(const float* in, int N, int H, int W, int C, float* out, int out_halo, hipStream_t s);

// dense [N][H][W][C] <-> the interior of a haloed buffer (the pad does not touch the halo).  C % 4 == 0.
void launch_vgg_pad(const float* dense, int N, int H, int W, int C, float* haloed, hipStream_t s);
void launch_vgg_unpad(const float* haloed, int N, int H, int W, int C, float* dense, hipStream_t s);

}  // namespace n2nmn
