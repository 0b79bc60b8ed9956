// dsea_block_lanczos.hip -- the basis-free block Lanczos recurrence (docs/design/27-finite-temperature.md): k_sblock_norm<R>,
// k_sblock_update<R>, k_sblock_finish<R>, their driver block_lanczos_drive and its scratch size.  Nothing here knows the
// operator: the driver runs the kernels around a caller's mat-vec step, the LZ kernel of dsea_sector_block.hip or of
// dsea_hubbard_block.hip.
//
// The recurrence (per column j, all columns in the same launches, nothing read back by the host during a run):
//   start:   norm2_j = |Q_j|^2, beta_0 = sqrt(norm2_j), Q_j /= beta_0
//   step i:  W = H Q_i - Q_{i-1} diag(beta_i)   (W overwrites Q_{i-1}; i = 0: W = H Q_0),  partials of alpha_j = Q_i[:, j] . W[:, j]
//            W -= Q_i diag(alpha),  partials of |W_j|^2
//            alphas[i, j] = alpha_j, betas[i, j] = beta_{i+1} = |W_j|, Q_{i+1} = W / beta_{i+1}
// Column j breaks at the first s = i + 1 with !(beta_s > 1e-13 max(earlier |alpha_j|, |beta_j|)) (the rule of
// dsea_lanczos_status; a start column of norm 0 breaks at s = 0): steps[j] = s, the column is zeroed in both blocks, its later
// alphas and betas (and the breaking beta) are written as 0, and nothing divides by its beta.  The other columns go on.
// Every reduction is wave, block, then the per-block partials summed in index order by every block alike: no atomics, two
// identical calls give identical bits.  The per-column state (beta, scale, alive) lives in the caller's scratch in two copies
// that alternate by step, so that no launch reads a word that another block of the same launch writes.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsea_block.h"

namespace dsea {

// per-block partials of |q_j|^2 of the start block
template <int R>
__global__ __launch_bounds__(256) void k_sblock_norm(const double* __restrict__ q, int64_t n, double* __restrict__ P) {
  __shared__ double sm[R][4];
  double acc[R];
#pragma unroll
  for (int j = 0; j < R; ++j) acc[j] = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    double v[R];
    block_load<R>(v, q, r);
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = fma(v[j], v[j], acc[j]);
  }
  block_partials<R>(acc, sm, P);
}

// alpha_j = the sum of the mat-vec's partials PA (every block sums them alike; block 0 stores alphas_row[j]);
// w -= q diag(alpha); per-block partials PB of |w_j|^2
template <int R>
__global__ __launch_bounds__(256) void k_sblock_update(const double* __restrict__ q, double* __restrict__ w, int64_t n,
                                                       const double* __restrict__ PA, int count, double* __restrict__ alphas_row,
                                                       double* __restrict__ PB) {
  __shared__ double sm5[5];
  __shared__ double sm[R][4];
  double alpha[R], acc[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    alpha[j] = sum_partials_block(PA + (int64_t)j * count, count, sm5);
    acc[j] = 0.0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < R; ++j) alphas_row[j] = alpha[j];
  }
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    double qv[R], wv[R];
    block_load<R>(qv, q, r);
    block_load<R>(wv, w, r);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      wv[j] = __dsub_rn(wv[j], __dmul_rn(alpha[j], qv[j]));
      acc[j] = fma(wv[j], wv[j], acc[j]);
    }
    block_store<R>(w, r, wv);
  }
  block_partials<R>(acc, sm, PB);
}

// beta_j = sqrt of the sum of the partials PB; the break decision (the same in every block); w = w / beta for a live column,
// 0 for a broken one -- a column that breaks now is also zeroed in `other` (Q_i; null at the start).  Block 0 stores
// out_row[j] (betas[i, j]; norm2[j] at the start, step = 0), steps[j] and the next copy of the state.  step = i + 1.
template <int R>
__global__ __launch_bounds__(256) void k_sblock_finish(double* __restrict__ w, double* __restrict__ other, int64_t n,
                                                       const double* __restrict__ PB, int count,
                                                       const double* __restrict__ alphas_row, double* __restrict__ out_row,
                                                       const double* __restrict__ st_in, double* __restrict__ st_out,
                                                       int32_t* __restrict__ steps, int step, int k) {
  __shared__ double sm5[5];
  const bool start = step == 0;
  double beta[R];
  bool live[R], now[R];
  bool any_now = false;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const double sumsq = sum_partials_block(PB + (int64_t)j * count, count, sm5);
    const bool alive = start ? true : st_in[2 * R + j] != 0.0;
    double scale = start ? 0.0 : st_in[R + j];
    beta[j] = 0.0;
    now[j] = false;
    if (alive) {
      if (!start) scale = fmax(scale, fabs(alphas_row[j]));
      const double b = sqrt(sumsq);
      if (!(b > DSEA_BREAK_TOL * scale)) {          // (also catches NaN; at the start the scale is 0: a zero column)
        now[j] = true;
      } else {
        beta[j] = b;
        scale = fmax(scale, b);
      }
    }
    live[j] = alive && !now[j];
    any_now |= now[j];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      out_row[j] = start ? sumsq : beta[j];
      st_out[j] = beta[j];
      st_out[R + j] = scale;
      st_out[2 * R + j] = live[j] ? 1.0 : 0.0;
      if (now[j]) steps[j] = step;
      else if (start) steps[j] = k;
    }
  }
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    double v[R];
    block_load<R>(v, w, r);
#pragma unroll
    for (int j = 0; j < R; ++j) v[j] = live[j] ? v[j] / beta[j] : 0.0;
    block_store<R>(w, r, v);
    if (any_now && other) {
#pragma unroll
      for (int j = 0; j < R; ++j)
        if (now[j]) other[r * R + j] = 0.0;
    }
  }
}

// doubles of scratch a block Lanczos run may touch at any grid cap: two copies of the state, then the two partial arrays
int64_t block_lanczos_scratch_doubles(int64_t n, int R) {
  int64_t nblk = (n + 255) / 256;
  if (nblk > DSEA_MAX_TFIM_BLOCKS) nblk = DSEA_MAX_TFIM_BLOCKS;
  return 2 * DSEA_SBLOCK_STATE + 2 * (int64_t)R * nblk;
}

// The recurrence for any operator: start (norm, finish) and k steps of three launches each -- the caller's mat-vec step, update,
// finish; nothing is read back.  Q and W change roles from step to step.  step(q, w, state, first, PA) launches, on st and with
// nblk blocks, W = H q - w diag(state[0 .. R)) over w (first: W = H q, w not read) and the partials PA[j * nblk + block] of
// q_j . W_j.
int block_lanczos_drive(int64_t n, int nblk, int R, int k, double* Q, double* W, double* norm2, double* alphas, double* betas,
                        int32_t* steps, double* scratch, hipStream_t st, const BlockLanczosStep& step) {
  double* state[2] = {scratch, scratch + DSEA_SBLOCK_STATE};
  double* PA = scratch + 2 * DSEA_SBLOCK_STATE;
  double* PB = PA + (int64_t)R * nblk;
  dispatch_block_width(R, [&](auto r) {
    constexpr int RR = decltype(r)::value;
    klaunch(nullptr, k_sblock_norm<RR>, nblk, 256, 0, st, Q, n, PB);
    klaunch(nullptr, k_sblock_finish<RR>, nblk, 256, 0, st, Q, nullptr, n, PB, nblk, nullptr, norm2, nullptr, state[0], steps, 0, k);
    double* q = Q;
    double* w = W;
    for (int i = 0; i < k; ++i) {
      step(q, w, state[i & 1], i == 0 ? 1 : 0, PA);
      klaunch(nullptr, k_sblock_update<RR>, nblk, 256, 0, st, q, w, n, PA, nblk, alphas + (int64_t)i * RR, PB);
      klaunch(nullptr, k_sblock_finish<RR>, nblk, 256, 0, st, w, q, n, PB, nblk, alphas + (int64_t)i * RR, betas + (int64_t)i * RR,
              state[i & 1], state[(i + 1) & 1], steps, i + 1, k);
      double* t = q;
      q = w;
      w = t;
    }
  });
  return 0;
}

}  // namespace dsea
