// Beam search over the sequential decoder (include/n2nmn.h section 2b): what runs per step besides the
// ordinary decoder launches.  Decoder rows are beam-major, row = beam * N + question, so a beam is a block of N
// rows and the recurrent-step / attention kernels run on K N rows (DecStepArgs::beam_Nq maps a row to its
// question's encoder tensors).  Per step:
//   beam_select_kernel   one workgroup per question ranks its K * 16 candidates (beam, token) by the total order
//                        of the header -- score descending, then beam ascending, then token ascending -- and
//                        writes the K new beams: parent, token, score, automaton state, next input, <eos> flag
//   beam_gather_kernel   h / c of both LSTM layers from parent row to child row, into the alternate buffers
// and once per call:
//   beam_init_kernel     scores (0, -inf, ...), automaton state (0, 0, T_dec), flags
//   beam_backtrack_kernel  follows the parent pointers from the final order to the outputs of the greedy call
// No atomics anywhere: a rank is a count, and every output element has exactly one writer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.h"

namespace n2nmn {
namespace {

struct BeamGatherArgs {
  const float* src[4]; float* dst[4];
  const int32_t* src_row;
  int mod, rows, L, Rs, Rd;
};
// rows across lanes, 4 k-slices per workgroup (the access pattern of gather_state_kernel): a lane moves the
// 16-byte k-quad of its row, so a wave writes 1 KB contiguous and reads 64 quads of one k-plane
__global__ __launch_bounds__(256) void beam_gather_kernel(BeamGatherArgs g) {
  const int r = blockIdx.x * 64 + (threadIdx.x & 63);
  const int sub = threadIdx.x >> 6;
  if (r >= g.rows) return;
  int pr = g.src_row ? g.src_row[r] : r % g.mod;
  pr = min(max(pr, 0), g.Rs - 1);                  // (a parent row is < rows by construction; never read outside)
  const int k4n = g.L / 4;
  for (int k4 = blockIdx.y * 4 + sub; k4 < k4n; k4 += gridDim.y * 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = *reinterpret_cast<const float4*>(g.src[i] + ((size_t)k4 * g.Rs + pr) * 4);
      *reinterpret_cast<float4*>(g.dst[i] + ((size_t)k4 * g.Rd + r) * 4) = v;
    }
  }
}

__global__ void beam_init_kernel(float* __restrict__ score, int32_t* __restrict__ state,
                                 int32_t* __restrict__ seen, int K, int N, int T_dec) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= K * N) return;
  score[r] = r < N ? 0.f : -INFINITY;              // step 0: one live beam per question
  state[r * 3 + 0] = 0; state[r * 3 + 1] = 0; state[r * 3 + 2] = T_dec;
  seen[r] = 0;
}

// One workgroup of 256 threads per question; thread c = 16 * beam + token owns one candidate.  Its key is
// score[beam] + log p_beam(token) where the token is valid (and the key is a number), -inf otherwise; its rank
// is the number of candidates in front of it in the total order (key descending, then c ascending -- which is
// beam ascending, then token ascending).  Ranks are a permutation of 0 .. 255, so new beam j < K has exactly one
// writer.  -inf candidates take part like any other (they tie and fall back to c): a question with fewer than K
// finite candidates fills up with dead beams (score -inf) that no finite candidate ever loses to.
__global__ __launch_bounds__(256) void beam_select_kernel(BeamSelectArgs a) {
  __shared__ float keys[BEAM_MAX_K * BEAM_MAX_V];
  const int n = blockIdx.x, c = threadIdx.x;
  const int b = c / BEAM_MAX_V, s = c % BEAM_MAX_V;
  const int K = a.K, N = a.N;
  const bool exists = b < K && s < a.V;            // (slots of tokens >= V hold NaN: they compare false both ways)
  float key = NAN, p = 0.f;
  const int row = b * N + n;
  if (exists) {
    const float sc = a.score_in[row];
    p = a.p[(size_t)row * BEAM_MAX_V + s];
    key = -INFINITY;
    if (((a.valid[row] >> s) & 1) && sc > -INFINITY) key = sc + logf(p);
    if (!(key == key)) key = -INFINITY;            // never rank a NaN
  }
  keys[c] = key;
  __syncthreads();
  if (!exists) return;
  int rank = 0;
  const int nc = K * BEAM_MAX_V;
#pragma unroll 8
  for (int o = 0; o < nc; ++o) {
    const float ko = keys[o];                       // (same address across the wave: an LDS broadcast)
    rank += (ko > key || (ko == key && o < c)) ? 1 : 0;
  }
  if (rank >= K) return;
  const int j = rank, out = j * N + n;
  a.parent[out] = b;
  a.token[out] = s;
  a.tprob[out] = p;
  a.ent_out[out] = a.ent[row];
  a.score_out[out] = key;
  const int sv = min(s, a.V - 1);
#pragma unroll
  for (int i = 0; i < 3; ++i) a.state_out[out * 3 + i] = a.state_in[row * 3 + i] + a.P[sv * 3 + i];
  a.seen_out[out] = ((a.seen_in ? a.seen_in[row] : 0) != 0 || s == a.eos) ? 1 : 0;
  a.next_idx[out] = sv;
  a.src_row[out] = row;
}

// One workgroup per (question, output beam); blockIdx.y == 0 is the best beam, whose chain also fills the
// outputs of the greedy call.  The question's parent pointers (T_dec * K ints) are staged in LDS first, so the
// chain is walked without dependent global loads.
constexpr int BEAM_MAX_TD = 64;
__global__ __launch_bounds__(256) void beam_backtrack_kernel(BeamBacktrackArgs a) {
  __shared__ int par[BEAM_MAX_TD * BEAM_MAX_K];
  __shared__ int at[BEAM_MAX_TD];                  // beam index (after step t's selection) of the chain at step t
  const int n = blockIdx.x, jb = blockIdx.y, tid = threadIdx.x;
  const int K = a.K, N = a.N, Td = a.Td, T = a.T;
  for (int i = tid; i < Td * K; i += 256) par[i] = a.parent[(size_t)i * N + n];
  __syncthreads();
  if (tid == 0) {
    int cur = jb;
    for (int t = Td - 1; t >= 0; --t) {
      at[t] = cur;
      cur = min(max(par[t * K + cur], 0), K - 1);
    }
  }
  __syncthreads();
  for (int t = tid; t < Td; t += 256) {
    const size_t e = ((size_t)t * K + at[t]) * N + n;
    const int tok = a.token[e];
    if (a.beam_tokens) a.beam_tokens[((size_t)jb * Td + t) * N + n] = tok;
    if (jb == 0) {
      a.tokens[(size_t)t * N + n] = tok;
      a.tprobs[(size_t)t * N + n] = a.tprob[e];
      a.ent_t[(size_t)t * N + n] = a.ent[e];
    }
  }
  if (jb != 0) return;
  const int R = K * N;
  for (int i = tid; i < Td * T; i += 256) {
    const int t = i / T, tau = i - t * T;
    // the row that computed step t of this chain is the PARENT of the beam chosen at step t
    const int prow = min(max(par[t * K + at[t]], 0), K - 1) * N + n;
    a.atts[((size_t)t * T + tau) * N + n] = a.atts_rows[((size_t)t * T + tau) * R + prow];
  }
}

}  // namespace

void launch_beam_gather(const float* const src[4], float* const dst[4], const int32_t* src_row, int mod,
                        int rows, int L, int Rs, int Rd, hipStream_t s) {
  BeamGatherArgs g{};
  for (int i = 0; i < 4; ++i) { g.src[i] = src[i]; g.dst[i] = dst[i]; }
  g.src_row = src_row; g.mod = mod > 0 ? mod : 1; g.rows = rows; g.L = L; g.Rs = Rs; g.Rd = Rd;
  hipLaunchKernelGGL(beam_gather_kernel, dim3((rows + 63) / 64, std::min(32, std::max(1, L / 16))), dim3(256), 0,
                     s, g);
}

void launch_beam_init(float* score, int32_t* state, int32_t* seen, int K, int N, int T_dec, hipStream_t s) {
  hipLaunchKernelGGL(beam_init_kernel, dim3((K * N + 255) / 256), dim3(256), 0, s, score, state, seen, K, N,
                     T_dec);
}

void launch_beam_select(const BeamSelectArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(beam_select_kernel, dim3(a.N), dim3(256), 0, s, a);
}

void launch_beam_backtrack(const BeamBacktrackArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(beam_backtrack_kernel, dim3(a.N, a.beam_tokens ? a.K : 1), dim3(256), 0, s, a);
}

}  // namespace n2nmn
