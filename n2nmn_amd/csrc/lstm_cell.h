// What the four recurrent step kernels share (lstm_step_kernel / lstm_step_wide_kernel in
// kernels_seq2seq.hip, lstm_tile_kernel, lstm_tile3_kernel): the kernel argument, everything after the
// last MFMA -- the cell update
//   c' = c * sig(f + 1) + sig(i) * tanh(j) ;  h' = tanh(c') * sig(o)
// (TF 1.0.0 BasicLSTMCell / dynamic_rnn semantics per SURVEY.md Appendix A.1-A.2) with every optional
// output of a LstmJob -- and the block id -> work mapping of the two tile kernels.  The kernels differ
// only in how [x, h] . W reaches the matrix cores.
//
// A thread owns W consecutive hidden units of one row: W = 1 in the K-split kernels (thread = (row,
// unit)), W = 4 in the tile kernels (lane = (row, float4 element of the k-interleaved state)).
#pragma once
#include "device_utils.h"
#include "kernels.h"

namespace n2nmn {

struct LstmJobs {
  LstmJob j[2];
};
// the kernel argument of a launch of `njobs` (1 or 2) jobs: the slots behind them are inactive
inline LstmJobs lstm_jobs(const LstmJob* jobs, int njobs) {
  LstmJobs js;
  for (int i = 0; i < 2; ++i) {
    if (i < njobs) js.j[i] = jobs[i];
    else { js.j[i] = LstmJob{}; js.j[i].active = 0; }
  }
  return js;
}

// ---- where a thread's W units live --------------------------------------------------------------------
struct LstmCellAt {
  int row;     // state row (length-sorted order), < N
  int orow;    // its original row: perm[row]
  int grp;     // 4-unit group of its units (the K-split kernels': their column tile, a scalar -- kept apart
  int ul;      // from the unit within the group, a multiple of W, so that grp * R, 16 * grp stay scalar)
  __device__ __forceinline__ int unit() const { return 4 * grp + ul; }   // first of the W hidden units
};

// ---- W floats at once (W = 4: one 16-byte access) ------------------------------------------------------
template <int W>
__device__ __forceinline__ void ldw(float (&v)[W], const float* p) {
  if constexpr (W == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = *p;
  }
}
template <int W>
__device__ __forceinline__ void stw(float* p, const float (&v)[W]) {
  if constexpr (W == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}
// the bf16 planes [3][L/8][R][8] of W units of state row `row` (LstmJob::h_new_b ...)
template <int W>
__device__ __forceinline__ void store_planes_w(uint16_t* planes, int L, int R, const LstmCellAt& at, int row,
                                               const float (&v)[W]) {
  if constexpr (W == 4) {
    // a 4-unit group = half of a k8 group
    store_planes(planes, (size_t)(L / 8) * R * 8, ((size_t)(at.grp >> 1) * R + row) * 8 + (size_t)(at.grp & 1) * 4,
                 make_float4(v[0], v[1], v[2], v[3]));
  } else {
    store_plane1(planes, L, R, at.unit(), row, v[0]);
  }
}

__device__ __forceinline__ int lstm_orow(const LstmJob& jb, int row) { return jb.perm ? jb.perm[row] : row; }
// element (row, unit 4 grp + ul) of a k-interleaved buffer [L/4][R][4]: a tile's 64 rows x 4 units are one
// contiguous KB instead of 64 sixteen-byte pieces of 64 different lines
__device__ __forceinline__ size_t lstm_packed_index(int R, int row, int grp, int ul) {
  return ((size_t)grp * R + row) * 4 + ul;
}
// element of a state buffer (c, h, h_drop): k-interleaved with R = hp_R rows when hp_R > 0, else
// row-major [N][L].  The float4 a W = 4 thread owns is an ELEMENT of the k-interleaved layout: the tile
// kernels run on it only (lstm_tile_supported).
template <int W>
__device__ __forceinline__ size_t lstm_state_index(const LstmJob& jb, int L, int row, const LstmCellAt& at) {
  return (W == 4 || jb.hp_R > 0) ? lstm_packed_index(jb.hp_R, row, at.grp, at.ul) : (size_t)row * L + at.unit();
}
// dynamic_rnn's zero output row (Appendix A.2): all that is left of the step where every row of a
// block is past its length.  Such rows are never read again: the recurrence only contracts over rows of
// blocks that are still active, c is updated in place, and a row's final state was captured at its last
// valid step (fin_c / fin_h).
template <int W>
__device__ __forceinline__ void lstm_zero_output(const LstmJob& jb, int L, int orow, const LstmCellAt& at) {
  const float zero[W] = {};
  if (jb.out_seq) stw<W>(jb.out_seq + (size_t)orow * L + at.unit(), zero);
}

// ---- epilogue operands: issued BEFORE the MFMA phase, used after it -------------------------------------
template <int W>
struct LstmCellIn {
  float add[4][W];                    // what z lacks: the x-table row (layer 0) or the bias, per gate
  float c_old[W] = {}, h_prev[W] = {};
  bool masked = false;                // dynamic_rnn past the row's length (A.2): the state is copied
};
template <int W>
__device__ __forceinline__ void lstm_cell_prefetch(const LstmJob& jb, int L, const LstmCellAt& at,
                                                   LstmCellIn<W>& in) {
  // tile column order of xtab / bias: [4-unit group][gate][unit], 16 values = one 64-byte line
  const float* ar = jb.bias;
  if (jb.xtab) {
    const int xi = jb.xidx ? jb.xidx[at.orow] : jb.xidx_const;
    ar = jb.xtab + (size_t)xi * 4 * L;
  }
  ar += 16 * at.grp + at.ul;
#pragma unroll
  for (int g = 0; g < 4; ++g) ldw<W>(in.add[g], ar + 4 * g);
  const size_t sidx = lstm_state_index<W>(jb, L, at.row, at);
  ldw<W>(in.c_old, jb.c_in + sidx);
  in.masked = jb.seq_len && jb.t >= jb.seq_len[at.orow];
  if (in.masked) ldw<W>(in.h_prev, jb.h_old + sidx);
}

// ---- the cell update and its stores ------------------------------------------------------------------------
// OUT: the optional stores a kernel compiles in (a property of the operand route, not of the caller: the
// recorded activations need the exact fp32 product, the planes exist in the split-operand mode only)
enum {
  LSTM_OUT_SAVE = 1,      // save_gates / save_c / save_h / save_hd: lstm_tile3_supported rejects them
  LSTM_OUT_PLANES = 2,    // h_new_b / h_drop_b / fin_h_b: no lstm_tile_kernel launch carries them (capi.cpp
                          // lstm_step_route sends a split-operand pass to lstm_tile3 or the K-split tiles)
};
// z[g][r]: pre-activation of gate g (i, j, f, o) of unit at.unit + r, in.add included (the K-split
// kernels start their sum over the 8 waves' partial tiles FROM in.add, the tile kernels add it last:
// the order is each route's own, so the sum stays with the caller)
template <int W>
__device__ __forceinline__ void lstm_add_last(float (&z)[4][W], const LstmCellIn<W>& in) {
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int r = 0; r < W; ++r) z[g][r] += in.add[g][r];
}
template <int W, int OUT>
__device__ __forceinline__ void lstm_cell_update(const LstmJob& jb, int L, const LstmCellAt& at,
                                                 const LstmCellIn<W>& in, const float (&z)[4][W]) {
  float gi[W], gj[W], gf[W], go[W], c[W], h[W], o[W];
#pragma unroll
  for (int r = 0; r < W; ++r) {
    gi[r] = fast_sigmoid(z[0][r]); gj[r] = fast_tanh(z[1][r]); gf[r] = fast_sigmoid(z[2][r] + 1.0f);
    go[r] = fast_sigmoid(z[3][r]);
    c[r] = in.c_old[r] * gf[r] + gi[r] * gj[r];
    h[r] = fast_tanh(c[r]) * go[r];
    o[r] = h[r];
  }
  if (in.masked) {
#pragma unroll
    for (int r = 0; r < W; ++r) { c[r] = in.c_old[r]; h[r] = in.h_prev[r]; o[r] = 0.f; }
  }
  const bool planes = (OUT & LSTM_OUT_PLANES) && (W == 4 || jb.hp_R > 0);
  const size_t sidx = lstm_state_index<W>(jb, L, at.row, at);
  stw<W>(jb.c_out + sidx, c);
  stw<W>(jb.h_new + sidx, h);
  // split-operand bf16 mode: the planes the next step's MFMAs read.  The tail steps of a pass run on the
  // K-split kernels (exact fp32), but later steps / the decoder read the planes of what they write
  if (planes && jb.h_new_b) store_planes_w<W>(jb.h_new_b, L, jb.hp_R, at, at.row, h);
  const size_t oidx = (size_t)at.orow * L + at.unit();
  // training: what the cell backward needs (ORIGINAL row order; masked rows keep finite values, their dz
  // is zero)
  if ((OUT & LSTM_OUT_SAVE) && jb.save_gates) {
#pragma unroll
    for (int r = 0; r < W; ++r) jb.save_gates[oidx + r] = make_float4(gi[r], gj[r], gf[r], go[r]);
    stw<W>(jb.save_c + oidx, c);
    stw<W>(jb.save_h + oidx, h);
  }
  if (jb.out_seq) stw<W>(jb.out_seq + oidx, o);
  if (jb.h_drop) {                // dropped copy of the OUTPUT for the layer above (models_vqa)
    float hd[W];
    ldw<W>(hd, jb.drop + oidx);
#pragma unroll
    for (int r = 0; r < W; ++r) hd[r] = h[r] * hd[r];
    stw<W>(jb.h_drop + sidx, hd);
    if (planes && jb.h_drop_b) store_planes_w<W>(jb.h_drop_b, L, jb.hp_R, at, at.row, hd);
    if ((OUT & LSTM_OUT_SAVE) && jb.save_hd) stw<W>(jb.save_hd + oidx, hd);
  }
  if (jb.fin_c && jb.seq_len && jb.t == jb.seq_len[at.orow] - 1) {   // the row's last valid step
    const size_t fidx = lstm_packed_index(jb.hp_R, at.orow, at.grp, at.ul);   // (fin_*: always k-interleaved)
    stw<W>(jb.fin_c + fidx, c);
    stw<W>(jb.fin_h + fidx, h);
    if (planes && jb.fin_h_b) store_planes_w<W>(jb.fin_h_b, L, jb.hp_R, at, at.orow, h);
  }
}

// ---- tile kernels: flat block id -> (job, row block, column tile) ------------------------------------------
// rows [nact, N) of a job are past their length (length-sorted encoder, retired decoder rows); a
// recorded (training) step keeps every row
__device__ __forceinline__ int lstm_tile_nact(const LstmJob& jb, int N) {
  return (jb.n_active && !jb.save_gates) ? *jb.n_active : N;
}
struct LstmTileId {
  int job;           // < 0: nothing left for this workgroup
  int rb, ct;        // block of ROWS rows, tile of 16 hidden units
  bool zero_fill;    // every row of the block is past its length: only lstm_zero_output is left
};
// Only row blocks with an active row do the step.  Their workgroups take the ids
// [0, (nab1 + nab0) * ntile), the K = 2L job first -- with two workgroups per CU every CU gets one
// K = 2L and one K = L tile -- so the dispatcher spreads THEM over all CUs (with the blocks numbered in
// place, a half-active step ran two workgroups on half of the CUs).  The column tile runs fastest, so
// that tile % 8 is the XCD of the workgroup: an XCD's L2 keeps ITS eighth of the weights across the
// steps of a pass and only h (new every step) comes over the fabric.  The ids behind write
// dynamic_rnn's zero output rows of the inactive blocks or leave.
template <int ROWS>
__device__ __forceinline__ LstmTileId lstm_tile_id(const LstmJobs& jobs, int njobs, int N, int ntile,
                                                   int nrb) {
  int nab[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const LstmJob& jq = jobs.j[j];
    int n = 0;
    if (j < njobs && jq.active) n = (min(max(lstm_tile_nact(jq, N), 0), N) + ROWS - 1) / ROWS;
    nab[j] = n;
  }
  int rem = blockIdx.x / ntile;
  LstmTileId id;
  id.ct = blockIdx.x - rem * ntile;
  id.job = -1; id.rb = 0; id.zero_fill = false;
#pragma unroll
  for (int j = 1; j >= 0; --j)
    if (id.job < 0) { if (rem < nab[j]) { id.job = j; id.rb = rem; } else rem -= nab[j]; }
#pragma unroll
  for (int j = 1; j >= 0; --j)
    if (id.job < 0 && j < njobs && jobs.j[j].active && jobs.j[j].out_seq) {
      if (rem < nrb - nab[j]) { id.job = j; id.rb = nab[j] + rem; id.zero_fill = true; } else rem -= nrb - nab[j];
    }
  return id;
}

}  // namespace n2nmn
