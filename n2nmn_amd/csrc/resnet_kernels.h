// Launchers of the ResNet-152 res5c feature extractor (kernels_resnet.hip).  Activations
// are haloed NHWC exactly as the VGG ones (vgg_kernels.h): the 3x3 convolutions of the bottlenecks ARE
// launch_vgg_conv3, and a dense copy of a haloed activation is launch_vgg_unpad.  Batch-norm and scale are
// folded into weights and biases before they get here, so every layer is convolution + bias (+ residual)
// (+ ReLU).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "vgg_kernels.h"

namespace n2nmn {

// output extents: 7x7 stride-2 pad-3 stem and the stride-2 1x1 convolutions: floor((n - 1) / 2) + 1;
// 3x3 stride-2 pad-0 max-pool in Caffe's ceil mode: ceil((n - 3) / 2) + 1 (n / 2 for n >= 2)
__host__ __device__ inline int resnet_half(int n) { return (n - 1) / 2 + 1; }
__host__ __device__ inline int resnet_pool_out(int n) { return n / 2 > 1 ? n / 2 : 1; }

// conv1: out = relu(conv7x7_s2_p3(img - mean) + bias), Cin = 3, Cout % 4 == 0.  img [N][H][W][3] uint8 or
// fp32 (dense); Wt [147][Cout] = HWIO [7][7][3][Cout]; out haloed at resnet_half(H) x resnet_half(W).  The mean
// is subtracted before the padding: a tap outside the image contributes 0.
void launch_resnet_stem(const void* img, int is_uint8, int N, int H, int W, const float* Wt, const float* bias,
                        const float mean[3], int Cout, float* out, hipStream_t s);

// pool1: in haloed [N][H + 2][W + 2][C] -> out haloed at resnet_pool_out(H) x resnet_pool_out(W); windows are
// clipped to the image, the halo never takes part.  C % 4 == 0.
void launch_resnet_pool(const float* in, int N, int H, int W, int C, float* out, hipStream_t s);

// out = act(conv1x1_stride(in) + bias (+ res)) as a GEMM on the 128 x 128 LDS-DMA tile: M = N H W OUTPUT pixels,
// K = Cin, columns = Cout.  in haloed at Hin x Win, out and res haloed at H x W = resnet_half (stride 2) or
// Hin x Win (stride 1); res == nullptr: no residual; relu != 0: act = max(0, .).  Bp = PK pack [Cin / 4][Np][4]
// of the HWIO [1][1][Cin][Cout], Np = round_up(Cout, 128).
struct ResConv1Args {
  const float* in; float* out; const float* res; const float* Bp; const float* bias;
  int N, Hin, Win, H, W, Cin, Cout, Np, stride, relu;
};
bool resnet_conv1x1_supported(const ResConv1Args& a);
void launch_resnet_conv1x1(const ResConv1Args& a, hipStream_t s);

}  // namespace n2nmn
