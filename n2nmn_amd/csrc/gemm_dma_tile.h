// The 128 x 128 x 32 LDS-DMA tile of gemm_dma_kernel (kernels_gemm_dma.hip, whose header describes it),
// as a main loop that two kernels share: the dense GEMM, whose A rows are rows of a matrix, and the 3x3
// convolution (kernels_vgg.hip), whose A rows are pixels of a zero-haloed NHWC image and whose 32-wide
// k stage lies inside one filter tap.  Only the per-row SOURCE address of A differs, so the caller
// supplies the instructions that fetch A (issue_a); the B (PK pack) DMA, the stage ring, the swizzled
// fragment reads and the MFMA order live here once.
#pragma once
#include "device_utils.h"

namespace n2nmn {
namespace dma_tile {

constexpr int DM = 128, DN = 128, DK = 32;
constexpr int DMA_THREADS = 512;
constexpr int DSTAGE = (DM * DK + DK * DN) * 4;          // 32 KiB: A image 16 KiB, then B image
constexpr int DB_IMAGE = DM * DK * 4;

struct Frag { float4 a; float4 b[2]; };

// A-side DMA roles: wave w moves A rows [16w, 16w + 16) of the tile as two pieces (u = 0, 1) of 8 rows x
// 128 B; lane `lane` of piece u fetches 16 B of row a_row(w, u, lane), namely the chunk a_chunk(row, lane)
// of the stage's 8 (the source-side swizzle: LDS position c of a row holds chunk c ^ ((row >> 1) & 7)),
// and the piece lands at LDS byte a_piece_lds(w, u) of the stage.
__device__ __forceinline__ int a_row(int w, int u, int lane) { return 16 * w + 8 * u + (lane >> 3); }
__device__ __forceinline__ uint32_t a_chunk(int row, int lane) { return (uint32_t)((lane & 7) ^ ((row >> 1) & 7)); }
__device__ __forceinline__ uint32_t a_piece_lds(int w, int u) { return (uint32_t)(16 * w + 8 * u) * 128u; }

// acc[t] (t = 0, 1: columns wn * 64 + 32 t ..) += A tile . B tile over nst stages of 32 k.
//   issue_a(s, st): issue this wave's two A pieces of stage s into the stage image at LDS address st
//   Bp + b_off: this lane's 16 B of k4 slab w, column n0 + lane, of stage 0; b_slab: bytes per stage
// C/D layout of the result: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the wave's
// 32 rows wm * 32 ..
template <class IssueA>
__device__ __forceinline__ void accumulate(char* smem, const int nst, const float* const Bp, const uint32_t b_off,
                                           const uint32_t b_slab, IssueA&& issue_a, f32x16 (&acc)[2]) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  auto issue = [&](int s) {
    const uint32_t st = lds0 + (uint32_t)(s & 1) * DSTAGE;
    issue_a(s, st);
#pragma unroll
    for (int u = 0; u < 2; ++u)
      glds16(Bp, b_off + (uint32_t)s * b_slab + (uint32_t)u * 1024u,
             st + DB_IMAGE + (uint32_t)(w * DN + 64 * u) * 16u);
  };

  // ---- fragment addressing -------------------------------------------------------------------------
  const int li = lane & 31, kh = lane >> 5;
  const int arow = wm * 32 + li;
  const uint32_t a_base = (uint32_t)arow * 128u;
  const uint32_t a_x = (uint32_t)((arow >> 1) & 7);
  const uint32_t b_base = (uint32_t)DB_IMAGE + (uint32_t)(wn * 64 + li) * 16u;
  auto read_frag = [&](int s, int g) {
    const char* st = smem + (size_t)(s & 1) * DSTAGE;
    const uint32_t chunk = (uint32_t)(2 * g + kh);
    Frag f;
    f.a = *reinterpret_cast<const float4*>(st + a_base + ((chunk ^ a_x) << 4));
    f.b[0] = *reinterpret_cast<const float4*>(st + b_base + chunk * (DN * 16u));
    f.b[1] = *reinterpret_cast<const float4*>(st + b_base + chunk * (DN * 16u) + 32u * 16u);
    return f;
  };
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  auto mma = [&](const Frag& f) {
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a.x, f.b[t].x, acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a.y, f.b[t].y, acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a.z, f.b[t].z, acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a.w, f.b[t].w, acc[t], 0, 0, 0);
  };

  issue(0);
  for (int s = 0; s < nst; ++s) {
    // this wave's pieces of stage s have landed; after the barrier everyone's have, and everyone is
    // done reading stage s - 1, whose buffer the DMA of stage s + 1 refills under this stage's MFMAs
    wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    if (s + 1 < nst) issue(s + 1);
    Frag P = read_frag(s, 0);
    Frag Q = read_frag(s, 1);
    __builtin_amdgcn_sched_barrier(0);       // (left alone, hipcc sinks the reads below the MFMAs)
    mma(P);
    P = read_frag(s, 2);
    __builtin_amdgcn_sched_barrier(0);
    mma(Q);
    Q = read_frag(s, 3);
    __builtin_amdgcn_sched_barrier(0);
    mma(P);
    mma(Q);
  }
}

}  // namespace dma_tile
}  // namespace n2nmn
