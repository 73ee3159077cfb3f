// Batched in-place Cholesky factorization, log-determinant, and
// forward/backward substitution — the GP fit/predict linear algebra
// (replaces the LAPACK calls inside sklearn GaussianProcessRegressor,
// reference model.py:1246-1265). Exact fp32; non-PD pivots clamp and set
// info[b]. Three right-looking blocked factorizations (BS = 32), chosen by
// batch count and size in launch_cholesky_batched / launch_cholesky_multik:
//
// B > CHOL_MULTIK_MAX_B: cholesky_batched_kernel, ONE workgroup (1024
// threads) per matrix, batch parallelism fills the chip:
//   * diagonal block factored in LDS (stride-33 rows: conflict-free),
//   * panel solve with each ROW held in 32 VGPRs (float4 global loads),
//     back-substituted against the LDS diagonal block,
//   * trailing SYRK update C -= P P^T fed ENTIRELY from LDS: the panel is
//     staged in chunk pairs (CHUNK x 32 floats each) so every multiply
//     reads LDS, with 2x2 register tiles per thread.
//
// B <= CHOL_MULTIK_MAX_B, 32 < N <= 615 (both panel buffers inside one CU's
// LDS): chol_whole_kernel, ONE launch and one workgroup of 16 waves per
// matrix for the whole factorization — wave 0 runs the serial chain of
// diagonal factors, the other waves the MFMA trailing update beside it, every
// hand-off through LDS and block barriers; optionally carrying a fused
// forward solve and the NMLL reduction.
//
// B <= CHOL_MULTIK_MAX_B otherwise: the multi-launch path (a 384-thread
// panel block per matrix plus 256-thread MFMA SYRK tiles spread over the
// chip, one launch per panel step), with the same optional riders.

#include "common.h"
#include "launchers.h"
#include <math.h>
#include <stdlib.h>

#define CHOL_BS 32
#ifndef CHOL_TPB
#define CHOL_TPB 1024
#endif
#define CHOL_CHUNK 384  // panel rows staged per LDS buffer (384*32*4 = 48 KiB)

struct CholLds {
  // all row strides padded +1: an unpadded 32-float (128 B) stride puts
  // every row on the same b32 bank group -> 32-way conflicts in the SYRK
  float S[CHOL_BS][CHOL_BS + 1];
  float Pi[CHOL_CHUNK][CHOL_BS + 1];  // i-side panel chunk
  float Pj[CHOL_CHUNK][CHOL_BS + 1];  // j-side panel chunk
  float ld_accum;
};

// ~100 KiB of LDS: above the 64 KiB static default, so allocated
// dynamically (gfx950 has 160 KiB per CU).
__global__ __launch_bounds__(CHOL_TPB) void cholesky_batched_kernel(
    float* __restrict__ A,       // (B, N, N)
    float* __restrict__ logdet,  // (B,)
    int* __restrict__ info,      // (B,)
    int N) {
  extern __shared__ char smem[];
  CholLds& L = *reinterpret_cast<CholLds*>(smem);
  const int b = blockIdx.x;
  float* M = A + (long long)b * N * N;
  const int tid = threadIdx.x;
  if (tid == 0) L.ld_accum = 0.f;
  __syncthreads();

  for (int k0 = 0; k0 < N; k0 += CHOL_BS) {
    const int bs = min(CHOL_BS, N - k0);

    // --- diagonal block: staged into LDS and factored there column by
    // column with workgroup barriers
    for (int idx = tid; idx < bs * bs; idx += CHOL_TPB)
      L.S[idx / bs][idx % bs] =
          M[(long long)(k0 + idx / bs) * N + k0 + idx % bs];
    __syncthreads();
    for (int j = 0; j < bs; ++j) {
      if (tid == 0) {
        float djj = L.S[j][j];
        if (djj <= 0.f) {
          info[b] = 1;
          djj = 1e-30f;
        }
        L.S[j][j] = sqrtf(djj);
        L.ld_accum += __logf(L.S[j][j]);
      }
      __syncthreads();
      for (int i = j + 1 + tid; i < bs; i += CHOL_TPB) L.S[i][j] /= L.S[j][j];
      __syncthreads();
      const int rem_d = bs - j - 1;
      for (int idx = tid; idx < rem_d * rem_d; idx += CHOL_TPB) {
        const int rr = j + 1 + idx / rem_d;
        const int cc = j + 1 + idx % rem_d;
        if (cc <= rr) L.S[rr][cc] -= L.S[rr][j] * L.S[cc][j];
      }
      __syncthreads();
    }
    for (int idx = tid; idx < bs * bs; idx += CHOL_TPB) {
      const int rr = idx / bs, cc = idx % bs;
      M[(long long)(k0 + rr) * N + k0 + cc] = (cc <= rr) ? L.S[rr][cc] : 0.f;
    }
    __syncthreads();

    const int rem = N - k0 - bs;
    if (rem <= 0) continue;

    // --- panel solve: row_i <- row_i * L11^-T with the row in registers.
    // float4 loads need 16-B alignment: row offset i*N + k0 is 16-B aligned
    // for all i iff N % 4 == 0 (k0 is a multiple of 32).
    const bool aligned4 = (N & 3) == 0;
    for (int i = k0 + bs + tid; i < N; i += CHOL_TPB) {
      float* grow = M + (long long)i * N + k0;
      float row[CHOL_BS];
      if (aligned4) {
#pragma unroll
        for (int t = 0; t < CHOL_BS; t += 4) {
          const float4 v = *(const float4*)(grow + t);
          row[t] = v.x; row[t + 1] = v.y; row[t + 2] = v.z; row[t + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int t = 0; t < CHOL_BS; ++t) row[t] = grow[t];
      }
      for (int j = 0; j < bs; ++j) {
        float v = row[j];
        for (int t = 0; t < j; ++t) v = fmaf(-row[t], L.S[j][t], v);
        row[j] = v / L.S[j][j];
      }
      if (aligned4) {
#pragma unroll
        for (int t = 0; t < CHOL_BS; t += 4) {
          float4 v;
          v.x = row[t]; v.y = row[t + 1]; v.z = row[t + 2]; v.w = row[t + 3];
          *(float4*)(grow + t) = v;
        }
      } else {
#pragma unroll
        for (int t = 0; t < CHOL_BS; ++t) grow[t] = row[t];
      }
    }
    __syncthreads();

    // --- trailing SYRK: A22 -= P P^T, LDS-fed chunk pairs, lower triangle
    for (int jc = 0; jc < rem; jc += CHOL_CHUNK) {
      const int jrows = min(CHOL_CHUNK, rem - jc);
      for (int idx = tid; idx < jrows * CHOL_BS; idx += CHOL_TPB) {
        const int r = idx / CHOL_BS, c = idx % CHOL_BS;
        L.Pj[r][c] = M[(long long)(k0 + bs + jc + r) * N + k0 + c];
      }
      __syncthreads();
      for (int ic = jc; ic < rem; ic += CHOL_CHUNK) {
        const int irows = min(CHOL_CHUNK, rem - ic);
        const bool same = (ic == jc);
        if (!same) {
          for (int idx = tid; idx < irows * CHOL_BS; idx += CHOL_TPB) {
            const int r = idx / CHOL_BS, c = idx % CHOL_BS;
            L.Pi[r][c] = M[(long long)(k0 + bs + ic + r) * N + k0 + c];
          }
        }
        __syncthreads();
        const float(*PI)[CHOL_BS + 1] = same ? L.Pj : L.Pi;
        // 2x2 register tiles over (irows x jrows)
        const int ti = (irows + 1) / 2, tj = (jrows + 1) / 2;
        for (int t = tid; t < ti * tj; t += CHOL_TPB) {
          const int tir = t / tj, tjr = t % tj;
          const int i0 = tir * 2, j0 = tjr * 2;
          const int gi0 = k0 + bs + ic + i0;
          const int gj0 = k0 + bs + jc + j0;
          if (same && gj0 > gi0 + 1) continue;  // fully-upper tile
          float acc00 = 0.f, acc01 = 0.f, acc10 = 0.f, acc11 = 0.f;
          const int i1 = min(i0 + 1, irows - 1);
          const int j1 = min(j0 + 1, jrows - 1);
#pragma unroll 8
          for (int s = 0; s < CHOL_BS; ++s) {
            const float a0 = PI[i0][s], a1 = PI[i1][s];
            const float b0 = L.Pj[j0][s], b1 = L.Pj[j1][s];
            acc00 = fmaf(a0, b0, acc00);
            acc01 = fmaf(a0, b1, acc01);
            acc10 = fmaf(a1, b0, acc10);
            acc11 = fmaf(a1, b1, acc11);
          }
          const int gi1 = k0 + bs + ic + i1;
          const int gj1 = k0 + bs + jc + j1;
          if (gj0 <= gi0) M[(long long)gi0 * N + gj0] -= acc00;
          if (j1 != j0 && gj1 <= gi0) M[(long long)gi0 * N + gj1] -= acc01;
          if (i1 != i0 && gj0 <= gi1) M[(long long)gi1 * N + gj0] -= acc10;
          if (i1 != i0 && j1 != j0 && gj1 <= gi1) M[(long long)gi1 * N + gj1] -= acc11;
        }
        __syncthreads();
      }
    }
  }
  if (tid == 0) logdet[b] = L.ld_accum;
}

// ---------------------------------------------------------------------------
// Multi-launch right-looking factorization for SMALL batch counts.
//
// The single-block kernel above runs one block per matrix: at the headline
// shape (B ~ 12 systems of N=300 from the speculative SCE-UA stages) that
// leaves 244 of 256 CUs idle. Here the trailing update, which is ~90% of the
// FLOPs, runs as 64x64 tiles spread across B * O((N/64)^2) workgroups. Two
// schedules with bit-identical results (chol_multik_classic /
// chol_multik_lookahead below): a panel launch (grid B) followed by a SYRK
// launch (grid B x tile-pairs) per 32-column step, or one combined
// chol_step_kernel launch per step.

// Panel / step workgroup width: 384 threads solve the whole N=300 trailing
// panel in ONE LDS chunk (256 needs two sequential chunk rounds: stage +
// solve + writeback + 3 barriers each); static LDS caps the width at 384
// (P[384][33] + S + colbuf = 55 KB < 64 KB).
#define CHOL_PANEL_TPB 384
// Columns factored per round of the "lds" diagonal factor (chol_panel_body).
#define CHOL_GROUP_COLS 2
// Rows of the diagonal-block buffer S: the block plus, as row 32, the rhs
// segment that rides the "reg" factor.
#define CHOL_S_ROWS (CHOL_BS + 1)
// Multipliers fetched per batch of the "reg" factor's rank-1 update.
#define CHOL_REG_BATCH 8

// v_readlane_b32 at a compile-time lane: one lane's value into a scalar
// register, no LDS round trip (unlike __shfl = ds_bpermute). Ignores EXEC.
__device__ __forceinline__ float chol_readlane(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}
#define CHOL_SYRK_TPB 256  // SYRK tile workgroup: 4 waves x 4 sub-tiles
#define SYRK_TS 64         // trailing-update tile edge

// Shared arithmetic of the rank-32 trailing update. EVERY path that applies
// a panel's update — the SYRK tile kernel and both roles of the look-ahead
// step kernel — goes through these two inlines,
// so an output element's value cannot depend on which block, tile origin or
// schedule computed it (NOTES.md -ffp-contract rule: one inline per chain).
typedef __attribute__((ext_vector_type(4))) float f32x4;

// One 16x16 sub-tile: acc = 0, then v_mfma_f32_16x16x4_f32 over k = 0..28.
// arow / brow point at this lane's operand rows (A[i][.] and B[.][j] =
// P[j][.]) in LDS; aswz / bswz are the rows' XOR swizzles (0 = unswizzled).
// The caller subtracts acc from the element it owns (operand map in
// chol_syrk_kernel's comment).
__device__ __forceinline__ f32x4 chol_subtile_acc(const float* arow, int aswz,
                                                  const float* brow, int bswz,
                                                  int lk) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < CHOL_BS; k += 4) {
    const float a = arow[(k + lk) ^ aswz];
    const float b = brow[(k + lk) ^ bswz];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// One rhs entry of the fused forward solve: the 32-step fmaf chain in t
// order against the panel's solved segment z.
__device__ __forceinline__ float chol_rhs_row_update(const float* prow,
                                                     int swz,
                                                     const float* z,
                                                     float acc) {
#pragma unroll
  for (int t = 0; t < CHOL_BS; ++t) acc = fmaf(-prow[t ^ swz], z[t], acc);
  return acc;
}

// Look-ahead role A, strip part: rows [c0, c0+rows) of the 32-column strip
// at k0 receive the PREVIOUS panel's update in place in the TRSM staging
// buffer: on exit P[r][0..31] holds the updated strip row
// A[c0+r][k0..k0+31] - acc, ready for the TRSM. Lj holds the previous
// panel's rows k0..k0+31 (swizzled, published by a block barrier before the
// call). Wave w of nw takes the 16-row groups w, w+nw, ...; it stages the
// previous panel's rows of a group into P itself (coalesced, zero beyond
// `rows`), multiplies, and overwrites them with the result. A group's rows
// are touched by that one wave only, so there is no block barrier inside
// and wave 0 never waits for this staging. P keeps its +1-padded layout
// instead of the SYRK tiles' swizzle so the update can land in place (a
// separate swizzled copy of up to TPB rows would push the static LDS past
// 64 KB); the operand read is 2-way bank-conflicted at worst.
__device__ __forceinline__ void chol_strip_rows(
    const float* __restrict__ Ab, int N, int k0, int c0, int rows,
    float (*P)[CHOL_BS + 1], float (*Lj)[CHOL_BS], int w, int nw) {
  const int lane = threadIdx.x & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const int ngroups = (rows + 15) / 16;
  const int kp = k0 - CHOL_BS;
  for (int g = w; g < ngroups; g += nw) {
    const int r16 = g * 16;
#pragma unroll
    for (int q = 0; q < 8; ++q) {  // 16 rows x 32 columns, 2 rows per pass
      const int rr = r16 + q * 2 + (lane >> 5), c = lane & 31;
      P[rr][c] = (rr < rows) ? Ab[(long long)(c0 + rr) * N + kp + c] : 0.0f;
    }
    __threadfence_block();  // staged rows cross lanes inside the wave
    float a0[4], a1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = r16 + lk * 4 + r;
      const bool ok = rr < rows;
      const float* src = Ab + (long long)(c0 + rr) * N + k0 + lr;
      a0[r] = ok ? src[0] : 0.0f;
      a1[r] = ok ? src[16] : 0.0f;
    }
    const int rb1 = 16 + lr;
    const f32x4 acc0 =
        chol_subtile_acc(P[r16 + lr], 0, Lj[lr], (lr & 7) << 2, lk);
    const f32x4 acc1 =
        chol_subtile_acc(P[r16 + lr], 0, Lj[rb1], (rb1 & 7) << 2, lk);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = r16 + lk * 4 + r;
      if (rr < rows) {
        P[rr][lr] = a0[r] - acc0[r];
        P[rr][16 + lr] = a1[r] - acc1[r];
      }
    }
  }
}

// The "reg" diagonal factor of chol_panel_body, run by the whole first wave:
// lane i holds row i of the block in r[], lane 32 (optionally) the rhs
// segment, every other lane zeros. Right-looking, one column per round, no
// LDS and no fence on the chain: column j's pivot and multipliers leave the
// owning lane's register through v_readlane at constant lanes. Per element
// the fmaf sequence is that of the lds factor (updates in ascending column
// order, then the true divide), so the factor, and z in row 32, keep every
// bit. Division and update are UNMASKED: rows above the diagonal collect
// junk that no lane reads back (multipliers come from lanes t > j only) and
// that is never written out. The pivot is wave-uniform, so bad (first
// failing column, 1-based) is tracked as a uniform. Returns the lane's
// logdet term: lane j ends up holding d_j, so it is one logf per lane after
// the loop, off the column chain — the same term per lane as the lds factor.
__device__ __forceinline__ float chol_factor_reg(float (&r)[CHOL_BS], int lane,
                                                 int bs, int k0, int& bad) {
  float dj = 1.0f;
  // Always 32 columns, straight-line: a partial block (bs < 32) arrives
  // padded with identity rows and columns, whose rounds divide by 1 and
  // update with zero multipliers. A `j < bs` branch per column instead
  // turns every r[t] into a phi, and the SLP vectorizer then packs the
  // update into v_pk_fma_f32 at three v_mov per pair (read the .s).
#pragma unroll
  for (int j = 0; j < CHOL_BS; ++j) {
    float d = chol_readlane(r[j], j);
    if (d <= 0.0f || !isfinite(d)) {
      bad = (bad || j >= bs) ? bad : (k0 + j + 1);
      d = 1e-30f;
    }
    d = sqrtf(d);
    const float q = r[j] / d;
    r[j] = (lane == j) ? d : q;
    dj = (lane == j) ? d : dj;
    // multipliers in batches: back-to-back readlane/fma pairs would each
    // pay the scalar-write-to-VALU-read wait states
#pragma unroll
    for (int t0 = j + 1; t0 < CHOL_BS; t0 += CHOL_REG_BATCH) {
      float m[CHOL_REG_BATCH];
#pragma unroll
      for (int u = 0; u < CHOL_REG_BATCH; ++u)
        if (t0 + u < CHOL_BS) m[u] = chol_readlane(r[j], t0 + u);
#pragma unroll
      for (int u = 0; u < CHOL_REG_BATCH; ++u)
        if (t0 + u < CHOL_BS) r[t0 + u] = fmaf(-r[j], m[u], r[t0 + u]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return (lane < bs) ? logf(dj) : 0.0f;
}

// TRSM of ONE strip row against the factored diagonal block S, in place in
// LDS: prow <- prow * L11^-T. The row is promoted to registers, so the
// 512-fmaf chain reads only registers and broadcast S rows. ONE source
// expression for the panel body and the one-launch kernel (fmaf in ascending
// t, then the true divide).
__device__ __forceinline__ void chol_trsm_row(float* prow,
                                              float (*S)[CHOL_BS + 1]) {
  float row[CHOL_BS];
#pragma unroll
  for (int t = 0; t < CHOL_BS; ++t) row[t] = prow[t];
#pragma unroll
  for (int j = 0; j < CHOL_BS; ++j) {
    float v = row[j];
#pragma unroll
    for (int t = 0; t < j; ++t) v = fmaf(-row[t], S[j][t], v);
    row[j] = v / S[j][j];
  }
#pragma unroll
  for (int t = 0; t < CHOL_BS; ++t) prow[t] = row[t];
}

// Factor the 32x32 diagonal block at (k0,k0) and panel-solve the rows below
// it. One block per matrix; also accumulates the step's logdet contribution
// deterministically (no atomics: k-steps are stream-ordered).
// Device body of chol_panel_kernel (PRE = false) and of chol_step_kernel's
// role A (PRE = true), run by CHOL_PANEL_TPB threads.
//
// PRE = true is the look-ahead schedule's role A (chol_step_kernel): the
// previous panel's rank-32 update has been applied everywhere EXCEPT this
// panel's own strip (rows >= k0, columns k0..k0+bs-1) and rhs segment, so
// the body first applies it there — through the shared inlines above, so
// each element sees the arithmetic the SYRK tile would have given it — and
// then proceeds exactly as the plain panel. Lj ([33][32]) stages the
// previous panel's rows k0..k0+31 (swizzled) and, in row 32, its solved rhs
// segment; unused (nullptr) when PRE is false.
//
// REG selects the diagonal factor (DMOSOPT_CHOL_FACTOR, bitwise-identical
// results, A/B in profiles/README.md):
//   false ("lds") — 2-column rounds broadcast through colbuf, then a
//     separate 32-step shuffle solve of the rhs segment after the barrier;
//   true  ("reg") — column j's pivot and multipliers leave the owning
//     lane's register through v_readlane at constant lanes, the logdet term
//     is one logf per lane after the loop, and the rhs segment rides the
//     factor as row 32 of the bordered block (lane 32, S row 32): dividing
//     that row by the pivot and giving it the other rows' rank-1 update IS
//     the forward solve, fmaf for fmaf. colbuf is unused.
template <bool PRE, bool REG>
__device__ __forceinline__ void chol_panel_body(
    float* __restrict__ Ab, float* __restrict__ logdet_b,
    int* __restrict__ info_b, int N, int k0, float* __restrict__ rhs_b,
    float (*S)[CHOL_BS + 1], float (*colbuf)[CHOL_BS],
    float (*P)[CHOL_BS + 1], float (*Lj)[CHOL_BS] = nullptr) {
  // rhs != nullptr: FUSED FORWARD SOLVE (bordered-matrix scheme). rhs (B, N)
  // starts as y and finishes as z = L^-1 y without a separate TRSV kernel:
  // this panel solves entries [k0, k0+bs) against the factored diagonal
  // block (the rhs is one extra TRSM row), and the trailing SYRK's diagonal
  // tiles apply the rank-32 update to the remaining entries. Saves the
  // ~61 us serial forward_solve_batched launch per NMLL (same serial-chain
  // structure as the factorization it now rides on).
  const int tid = threadIdx.x;
  const int bs = min(CHOL_BS, N - k0);

  // Wave-parallel diagonal factor: lane i of the first wave owns row i of
  // the 32x32 block in registers; column j's pivot and multipliers move by
  // __shfl broadcast. Zero block barriers in the serial dependency chain
  // (the barrier version spent ~96 barriers here and dominated the whole
  // multi-launch path at 54 us per panel).
  // coalesced stage of the block into LDS by the whole workgroup first —
  // a single wave doing the 32x32 global load directly issues ~1000
  // uncoalesced (1200 B stride) loads and stalls on memory latency
  if (!PRE) {
    for (int idx = tid; idx < bs * bs; idx += blockDim.x)
      S[idx / bs][idx % bs] =
          Ab[(long long)(k0 + idx / bs) * N + k0 + idx % bs];
    if (REG && rhs_b != nullptr && tid >= CHOL_PANEL_TPB - CHOL_BS) {
      const int t = tid - (CHOL_PANEL_TPB - CHOL_BS);
      if (t < bs) S[CHOL_BS][t] = rhs_b[k0 + t];
    }
    __syncthreads();
  }
  // TRSM staging buffer, declared up front: waves 1+ stage the FIRST chunk
  // of trailing panel rows into LDS concurrently with wave 0's serial
  // diagonal factor (the staging reads last step's SYRK output — global
  // memory untouched by the factor — so the ~34 KB coalesced load hides
  // entirely under the factor's shuffle chain instead of serializing after
  // it; disjoint LDS regions).
  const int c0_first = k0 + CHOL_BS;
  const int rows_first = min(CHOL_PANEL_TPB, N - c0_first);
  if (PRE) {
    // whole workgroup: coalesced stage of the previous panel's rows of the
    // diagonal block into Lj (3 loads per thread) and of its solved rhs
    // segment into Lj's extra row. This is all wave 0 waits for: the strip
    // rows are staged wave-locally by waves 1+ (chol_strip_rows). Wave 0
    // issues the loads of its own diagonal-block elements and rhs entry
    // BEFORE the barrier, so their latency overlaps the staging.
    const int kp = k0 - CHOL_BS;
    const int lr = tid & 15, lk = (tid >> 4) & 3;
    float adiag[4][4];
    float yv = 0.0f;
    if (tid < 64) {
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        const int r16 = (sub >> 1) * 16, c16 = (sub & 1) * 16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = r16 + lk * 4 + r, j = c16 + lr;
          adiag[sub][r] = (i < bs && j < bs)
                              ? Ab[(long long)(k0 + i) * N + k0 + j]
                              : 0.0f;
        }
      }
      if (rhs_b != nullptr && tid < bs) yv = rhs_b[k0 + tid];
    }
    for (int idx = tid; idx < CHOL_BS * CHOL_BS; idx += CHOL_PANEL_TPB) {
      const int r = idx / CHOL_BS, c = idx % CHOL_BS;
      Lj[r][c ^ ((r & 7) << 2)] =
          (k0 + r < N) ? Ab[(long long)(k0 + r) * N + kp + c] : 0.0f;
    }
    if (rhs_b != nullptr && tid >= CHOL_PANEL_TPB - CHOL_BS)
      Lj[CHOL_BS][tid - (CHOL_PANEL_TPB - CHOL_BS)] =
          rhs_b[kp + tid - (CHOL_PANEL_TPB - CHOL_BS)];
    __syncthreads();
    if (tid < 64) {
      // wave 0: updated diagonal block straight into S (only its lower
      // triangle is updated, as in the SYRK tiles, and only that is read),
      // then the rhs segment's update; the factor below waits for this
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        const int r16 = (sub >> 1) * 16, c16 = (sub & 1) * 16;
        const int ra = r16 + lr, rb = c16 + lr;
        const f32x4 acc = chol_subtile_acc(Lj[ra], (ra & 7) << 2, Lj[rb],
                                           (rb & 7) << 2, lk);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = r16 + lk * 4 + r, j = c16 + lr;
          if (i < bs && j < bs)
            S[i][j] = (j <= i) ? adiag[sub][r] - acc[r] : adiag[sub][r];
        }
      }
      if (rhs_b != nullptr && tid < bs) {
        const float yu = chol_rhs_row_update(Lj[tid], (tid & 7) << 2,
                                             Lj[CHOL_BS], yv);
        if (REG) S[CHOL_BS][tid] = yu;  // row 32 of the bordered block
        else rhs_b[k0 + tid] = yu;
      }
      __threadfence_block();  // S rows cross lanes inside wave 0
    }
  }
  if (tid >= 64) {
    if (PRE) {
      // waves 1+: the first chunk's strip update, concurrent with wave 0
      chol_strip_rows(Ab, N, k0, c0_first, rows_first, P, Lj, (tid >> 6) - 1,
                      CHOL_PANEL_TPB / 64 - 1);
    } else {
      for (int idx = tid - 64; idx < rows_first * CHOL_BS;
           idx += CHOL_PANEL_TPB - 64) {
        const int r = idx / CHOL_BS, c = idx % CHOL_BS;
        P[r][c] = Ab[(long long)(c0_first + r) * N + k0 + c];
      }
    }
  } else {
    const int lane = tid;
    // reg: lane 32 is the rhs row whatever bs is; a partial block is padded
    // to 32 x 32 with the identity and every lane beyond holds zeros
    // (v_readlane ignores EXEC: nothing it can reach may be uninitialized)
    const int rhs_lane = (REG && rhs_b != nullptr) ? CHOL_BS : -1;
    const bool own = lane < bs || lane == rhs_lane;
    float r[CHOL_BS];
#pragma unroll
    for (int t = 0; t < CHOL_BS; ++t)
      r[t] = (own && t < bs) ? S[lane][t]
                             : ((REG && lane == t) ? 1.0f : 0.0f);
    float mylog = 0.0f;
    int bad = 0;
    if (REG) mylog = chol_factor_reg(r, lane, bs, k0, bad);
    // CHOL_GROUP_COLS columns per round: within the group each column first
    // receives the updates of its in-group predecessors, is factored
    // (shfl pivot + sqrt + div), and broadcast through LDS with ONE
    // workgroup fence; then ONE fused rank-GROUP pass updates the
    // remaining columns. Halves the update-loop rounds on the serial
    // pivot chain (the dominant latency of this kernel) while keeping the
    // fmaf sequence PER ELEMENT that of sequential rank-1 passes — the
    // factor does not depend on the group size (SCE-UA accept decisions
    // are bit-stable). Groups of 4 and a pure-shuffle factor measured
    // slower: profiles/README.md.
#pragma unroll
    for (int g = 0; g < (REG ? 0 : CHOL_BS); g += CHOL_GROUP_COLS) {
      if (g >= bs) continue;
#pragma unroll
      for (int q = 0; q < CHOL_GROUP_COLS; ++q) {
        const int j = g + q;
        if (j >= bs) break;
        // in-group predecessor updates for column j (same order as the
        // sequential rank-1 passes)
#pragma unroll
        for (int p = 0; p < CHOL_GROUP_COLS; ++p) {
          if (p >= q) break;
          if (lane >= j) r[j] = fmaf(-r[g + p], colbuf[p][j], r[j]);
        }
        float d = __shfl(r[j], j);
        if (d <= 0.0f || !isfinite(d)) {
          bad = bad ? bad : (k0 + j + 1);
          d = 1e-30f;
        }
        d = sqrtf(d);
        if (lane == j) {
          r[j] = d;
          mylog += logf(d);
        } else if (lane > j) {
          r[j] /= d;
        }
        // broadcast column j through LDS with ONE workgroup fence: the
        // reads then pipeline freely, unlike a per-t __shfl chain
        // (ds_bpermute each) or a volatile pointer (per-access ordering)
        if (lane < bs) colbuf[q][lane] = r[j];
        __threadfence_block();
      }
      // fused rank-GROUP update of the columns beyond the group
      const int gend = min(g + CHOL_GROUP_COLS, bs);
#pragma unroll
      for (int t = 0; t < CHOL_BS; ++t) {
        if (t < g + CHOL_GROUP_COLS || t >= bs) continue;
        if (lane >= t) {
#pragma unroll
          for (int q = 0; q < CHOL_GROUP_COLS; ++q) {
            if (g + q >= gend) break;
            r[t] = fmaf(-r[g + q], colbuf[q][t], r[t]);
          }
        }
      }
    }
    // stage the factored block back to LDS (global writeback below is
    // done coalesced by the whole workgroup); reg: row 32 is the solved z
    if (own) {
#pragma unroll
      for (int t = 0; t < CHOL_BS; ++t) {
        if (t >= bs) continue;
        S[lane][t] = r[t];
      }
    }
    // wave-reduce the logdet contribution and error flag
    for (int off = 32; off > 0; off >>= 1) {
      mylog += __shfl_down(mylog, off);
      const int ob = __shfl_down(bad, off);
      bad = bad ? bad : ob;
    }
    if (lane == 0) {
      *logdet_b += mylog;
      if (bad && *info_b == 0) *info_b = bad;
    }
  }
  __syncthreads();
  // fused-solve panel step: wave 0 solves the rhs segment against the
  // factored diagonal block (wave-synchronous, lane j owns entry j; same
  // shuffle scheme as forward_solve_batched_kernel's diagonal solve). The
  // segment already carries the trailing updates of all previous steps.
  if (!REG && rhs_b != nullptr && tid < 64) {
    float* yb = rhs_b + k0;
    const int j = tid;
    float v = (j < bs) ? yb[j] : 0.0f;
    for (int t = 0; t < bs; ++t) {
      const float zt = __shfl(v, t) / S[t][t];
      if (j == t) v = zt;
      else if (j > t && j < bs) v = fmaf(-S[j][t], zt, v);
    }
    if (j < bs) yb[j] = v;
  }
  // reg: z left the factor in S row 32; wave 1 writes it out
  if (REG && rhs_b != nullptr && tid >= 64 && tid < 64 + bs)
    rhs_b[k0 + tid - 64] = S[CHOL_BS][tid - 64];
  // factored-block writeback by waves 1+ (concurrent with wave 0's rhs
  // solve above; both only READ S)
  for (int idx = tid - 64; idx >= 0 && idx < bs * bs;
       idx += CHOL_PANEL_TPB - 64) {
    const int i = idx / bs, t = idx % bs;
    if (t <= i) Ab[(long long)(k0 + i) * N + k0 + t] = S[i][t];
  }
  // no barrier: the first chunk's P and the factored S were published by
  // the post-factor barrier; the writes above touch disjoint addresses
  // panel solve, chunked through LDS: per-thread direct row loads are
  // uncoalesced (64 lanes touch 64 cache lines per load instruction, a
  // constant ~27 us regardless of row count), so each chunk is
  // staged with a COALESCED copy, solved entirely in LDS (one row per
  // thread; the +1-padded stride keeps lanes on distinct banks), and
  // written back coalesced. The FIRST chunk was pre-staged during the
  // factor. Trailing rows exist only under a FULL panel
  // (k0 + bs < N implies bs == CHOL_BS): constant trip counts throughout.
  for (int c0 = c0_first; c0 < N; c0 += CHOL_PANEL_TPB) {
    const int rows = min(CHOL_PANEL_TPB, N - c0);
    if (c0 != c0_first) {
      if (PRE) {
        // later chunks: every wave stages and updates its own row groups
        chol_strip_rows(Ab, N, k0, c0, rows, P, Lj, tid >> 6,
                        CHOL_PANEL_TPB / 64);
      } else {
        for (int idx = tid; idx < rows * CHOL_BS; idx += CHOL_PANEL_TPB) {
          const int r = idx / CHOL_BS, c = idx % CHOL_BS;
          P[r][c] = Ab[(long long)(c0 + r) * N + k0 + c];
        }
      }
      __syncthreads();
    }
    if (tid < rows) {
      // own row promoted to registers: the j-loop's 512-FMA dependency
      // chain then reads only registers and broadcast S rows (the LDS
      // version serializes a ds_read into every fmaf of the chain);
      // identical fmaf order — the solve is bitwise unchanged
      chol_trsm_row(P[tid], S);
    }
    __syncthreads();
    for (int idx = tid; idx < rows * CHOL_BS; idx += CHOL_PANEL_TPB) {
      const int r = idx / CHOL_BS, c = idx % CHOL_BS;
      Ab[(long long)(c0 + r) * N + k0 + c] = P[r][c];
    }
    __syncthreads();
  }
}

template <bool REG>
__global__ __launch_bounds__(CHOL_PANEL_TPB) void chol_panel_kernel(
    float* __restrict__ A, float* __restrict__ logdet, int* __restrict__ info,
    int N, int k0, float* __restrict__ rhs) {
  __shared__ float S[CHOL_S_ROWS][CHOL_BS + 1];
  __shared__ float colbuf[CHOL_GROUP_COLS][CHOL_BS];
  __shared__ float P[CHOL_PANEL_TPB][CHOL_BS + 1];
  const int b = blockIdx.x;
  chol_panel_body<false, REG>(A + (long long)b * N * N, logdet + b, info + b, N, k0,
                         rhs ? rhs + (long long)b * N : nullptr, S, colbuf, P);
}

// Trailing update A[ti,tj] -= P_i P_j^T for one 64x64 tile (ti, tj) of the
// submatrix below/right of the panel at k0: the block's first four waves
// each compute four 16x16 MFMA sub-tiles.
// r0 is the tile origin (first row and column the tiles cover): k0 + 32 for
// the classic full trailing update, k0 + 64 for the look-ahead schedule's
// role B, whose first 32 columns belong to role A's strip.
__device__ __forceinline__ void chol_syrk_tile_body(
    float* __restrict__ Ab, int N, int k0, int r0, int ti, int tj,
    float* __restrict__ rhs_b, float (*Pi)[CHOL_BS], float (*Pj)[CHOL_BS]) {
  const int i0 = r0 + ti * SYRK_TS, j0 = r0 + tj * SYRK_TS;
  const int tid = threadIdx.x;

  // Pi / Pj: stride 32 with an XOR swizzle on the k-column: the MFMA operand
  // read (lane -> [row + lr][k + lk]) hits banks (row+lk) mod 32 under a +1
  // pad, an up-to-8-way conflict (PMC: 2.2 extra cycles per LDS
  // instruction); c = k ^ ((row & 7) << 2) spreads (lr, lk) over all 32
  // banks.
  for (int idx = tid; idx < SYRK_TS * CHOL_BS; idx += blockDim.x) {
    const int r = idx / CHOL_BS, c = idx % CHOL_BS;
    const int cs = c ^ ((r & 7) << 2);  // swizzled physical column
    Pi[r][cs] = (i0 + r < N) ? Ab[(long long)(i0 + r) * N + k0 + c] : 0.0f;
    Pj[r][cs] = (j0 + r < N) ? Ab[(long long)(j0 + r) * N + k0 + c] : 0.0f;
  }
  __syncthreads();

  // MFMA tile core: C -= Pi * Pj^T on the matrix units.
  // v_mfma_f32_16x16x4_f32 is EXACT fp32 (identical to an fmaf chain) at
  // the f32 vector rate; operand map (cdna4_isa section 10):
  // A: lane l -> A[l&15][l>>4]; B: lane l -> B[l>>4][l&15];
  // C/D (f32x4): col = lane&15, row = (lane>>4)*4 + reg.
  const int wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int sIdx = 0; sIdx < 4; ++sIdx) {
    const int sub = wave * 4 + sIdx;        // 4x4 grid of 16x16 subtiles
    if (sub >= 16) break;  // blocks wider than 4 waves: extra waves idle
    const int r16 = (sub >> 2) * 16, c16 = (sub & 3) * 16;
    const int ra = r16 + lr, rb = c16 + lr;
    // A[i][k] = Pi[i][k], B[k][j] = Pj[j][k]
    const f32x4 acc =
        chol_subtile_acc(Pi[ra], (ra & 7) << 2, Pj[rb], (rb & 7) << 2, lk);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + r16 + lk * 4 + r;
      const int j = j0 + c16 + lr;
      if (i < N && j < N && j <= i) Ab[(long long)i * N + j] -= acc[r];
    }
  }
  // fused-solve trailing update: the diagonal tiles apply the panel's
  // rank-32 update to their 64 rhs entries (scheme in chol_panel_body)
  if (rhs_b != nullptr && ti == tj && tid < 64) {
    const int i = i0 + tid;
    if (i < N) {
      rhs_b[i] = chol_rhs_row_update(Pi[tid], (tid & 7) << 2, rhs_b + k0,
                                     rhs_b[i]);
    }
  }
}

// Full trailing update of the classic schedule: grid (B, tile pairs),
// blockIdx.y walks the lower triangle of 64x64 tiles from tile (0, 0) at
// origin k0 + 32.
__global__ __launch_bounds__(CHOL_SYRK_TPB) void chol_syrk_kernel(
    float* __restrict__ A, int N, int k0, float* __restrict__ rhs) {
  __shared__ float Pi[SYRK_TS][CHOL_BS];
  __shared__ float Pj[SYRK_TS][CHOL_BS];
  const int b = blockIdx.x;
  float* Ab = A + (long long)b * N * N;
  int ti, tj;
  tri_tile_decode(blockIdx.y, &ti, &tj);
  chol_syrk_tile_body(Ab, N, k0, k0 + CHOL_BS, ti, tj,
                      rhs ? rhs + (long long)b * N : nullptr, Pi, Pj);
}

// Final NMLL assembly: out = 0.5 * sum(z^2) + half_logdet + c, inf where the
// factorization failed or the value is non-finite — fuses the (z*z).sum +
// scalar-combine + masking chain (a handful of torch dispatches per SCE-UA
// stage). ONE body for nmll_reduce_kernel and for the epilogue of the last
// chol_step_kernel launch, with explicit fmaf, so both give the same bits:
// a strided partial per thread over the first NMLL_REDUCE_TPB threads, then
// the tree. Every thread of the block must call it (barriers); threads
// beyond NMLL_REDUCE_TPB only keep the barriers company. part: LDS,
// NMLL_REDUCE_TPB floats.
#define NMLL_REDUCE_TPB 256
__device__ __forceinline__ void nmll_reduce_body(
    const float* z, const float* half_logdet_b, const int* info_b,
    float* out_b, int N, float c, float* part) {
  const int tid = threadIdx.x;
  if (tid < NMLL_REDUCE_TPB) {
    float acc = 0.f;
    for (int i = tid; i < N; i += NMLL_REDUCE_TPB) acc = fmaf(z[i], z[i], acc);
    part[tid] = acc;
  }
  __syncthreads();
  for (int off = NMLL_REDUCE_TPB >> 1; off > 0; off >>= 1) {
    if (tid < off) part[tid] += part[tid + off];
    __syncthreads();
  }
  if (tid == 0) {
    float v = fmaf(0.5f, part[0], *half_logdet_b) + c;
    if (*info_b != 0 || !isfinite(v)) v = INFINITY;
    *out_b = v;
  }
}

// ------------------------------------------------------ look-ahead step
// One launch per panel step s >= 1 (k0 = 32 s), grid (B, 1 + tiles); the
// kernel boundary is the only synchronization (one stream, no events, no
// flags). Both roles consume panel s-1, written by the previous launch:
//   block y = 0  (role A): applies panel s-1's update to strip s only
//     (rows >= k0, columns k0..k0+31) and to the rhs segment, then factors
//     and solves panel s exactly like chol_panel_kernel;
//   blocks y >= 1 (role B): apply panel s-1's update to the REST of the
//     trailing matrix (rows and columns >= k0 + 32, rhs rows >= k0 + 32) as
//     64x64 tiles with origin k0 + 32.
// Written regions are disjoint (A: columns [k0, k0+32) and rhs [k0, k0+32);
// B: columns and rhs rows >= k0+32), and neither role reads what the other
// writes: both read only columns [k0-32, k0) and rhs [k0-32, k0). The
// full-matrix SYRK therefore runs BESIDE the panel instead of in front of
// it: ceil(N/32) launches instead of 2 ceil(N/32) - 1. Element values are
// those of the classic schedule bit for bit (shared inlines above).
// Role B's tile buffers alias the panel's TRSM buffer P (a block has one
// role), keeping the static LDS at the panel's ~55 KB + 4 KB for Lj.
template <bool REG>
__global__ __launch_bounds__(CHOL_PANEL_TPB) void chol_step_kernel(
    float* __restrict__ A, float* __restrict__ logdet, int* __restrict__ info,
    int N, int k0, float* __restrict__ rhs, float* __restrict__ nmll_out,
    float nmll_c) {
  __shared__ float S[CHOL_S_ROWS][CHOL_BS + 1];
  __shared__ float colbuf[CHOL_GROUP_COLS][CHOL_BS];
  __shared__ float P[CHOL_PANEL_TPB][CHOL_BS + 1];
  __shared__ float Lj[CHOL_BS + 1][CHOL_BS];  // + the solved rhs segment
  static_assert(CHOL_PANEL_TPB * (CHOL_BS + 1) >= 2 * SYRK_TS * CHOL_BS,
                "tile buffers must fit in the TRSM buffer");
  const int b = blockIdx.x;
  float* Ab = A + (long long)b * N * N;
  float* rhs_b = rhs ? rhs + (long long)b * N : nullptr;
  if (blockIdx.y == 0) {
    chol_panel_body<true, REG>(Ab, logdet + b, info + b, N, k0, rhs_b, S,
                               colbuf, P, Lj);
    if (nmll_out != nullptr) {
      // NMLL epilogue of the LAST step (no role-B blocks, no trailing rows):
      // the final rhs segment has just been solved and written (by wave 0,
      // or by wave 1 under the reg factor), so Z[b], logdet[b] and info[b]
      // are final and this block reduces them itself. The barrier and fence
      // publish those global writes to the other waves; the partials reuse
      // the (idle) TRSM buffer.
      __syncthreads();
      __threadfence_block();
      nmll_reduce_body(rhs_b, logdet + b, info + b, nmll_out + b, N, nmll_c,
                       &P[0][0]);
    }
  } else {
    float(*Pi)[CHOL_BS] = (float(*)[CHOL_BS]) & P[0][0];
    float(*Pj)[CHOL_BS] = Pi + SYRK_TS;
    int ti, tj;
    tri_tile_decode(blockIdx.y - 1, &ti, &tj);
    chol_syrk_tile_body(Ab, N, k0 - CHOL_BS, k0 + CHOL_BS, ti, tj, rhs_b, Pi,
                        Pj);
  }
}

// ------------------------------------------------------ one-launch kernel
// The WHOLE factorization of one matrix in one workgroup of 16 waves
// (CHOL_SCHED_ONELAUNCH): the look-ahead schedule's dependency structure
// with every hand-off inside the workgroup — LDS and two block barriers per
// panel step, no kernel boundary, no device-scope flag. Per step s
// (k0 = 32 s), between the two barriers:
//   wave 0: applies panel s-1's update to diagonal block s and rhs segment s
//     and factors them (chol_factor_reg, rhs as row 32), operands from LDS;
//   waves 1..15: write panel s-1 out to global (the output L), then apply
//     its update as 16x16 MFMA tiles to strip s (rows >= k0 + 32, columns
//     k0..k0+31; result lands in the TRSM buffer) and to the rest of the
//     trailing matrix (in place in global / L2) and the rhs rows >= k0 + 32;
// then, behind the first barrier, the one-row-per-thread TRSM of strip s
// (chol_trsm_row) while the idle waves write the factored block and z out
// and stage diagonal block s+1 and its rhs segment from global into LDS for
// wave 0. The solved strip stays in LDS as panel s: two panel buffers
// alternate.
// A 16x16 tile (I, J) of the lower triangle belongs to worker
// (I (I + 1) / 2 + J) mod 15 for the whole factorization, and so does a
// 64-row group of the rhs: successive updates of an element are ordered by
// its owner's program order, hand-offs to wave 0 and the TRSM by the
// barriers. Element values are those of the other schedules bit for bit:
// every update goes through chol_subtile_acc / chol_rhs_row_update, whose
// result does not depend on the tiling or on the operands' LDS layout.
#define CHOL_WHOLE_TPB 1024
#define CHOL_WHOLE_WORKERS (CHOL_WHOLE_TPB / 64 - 1)
// tiles a worker keeps in flight: their global loads are issued together
#define CHOL_WHOLE_TILE_BATCH 4
// LDS of one CU (gfx950)
#define CHOL_CU_LDS_BYTES (160 * 1024)

// S + previous z and next rhs segments + NMLL partials + the next diagonal
// block + two panel buffers of N - 32 rows
static inline size_t chol_whole_lds_bytes(int N) {
  return sizeof(float) *
         ((size_t)CHOL_S_ROWS * (CHOL_BS + 1) + 2 * CHOL_BS +
          NMLL_REDUCE_TPB + (size_t)CHOL_BS * (CHOL_BS + 1) +
          2 * (size_t)(N - CHOL_BS) * (CHOL_BS + 1));
}

__global__ __launch_bounds__(CHOL_WHOLE_TPB) void chol_whole_kernel(
    float* __restrict__ A, float* __restrict__ logdet, int* __restrict__ info,
    int N, float* __restrict__ rhs, float* __restrict__ nmll_out,
    float nmll_c) {
  extern __shared__ float whole_lds[];
  float(*S)[CHOL_BS + 1] = (float(*)[CHOL_BS + 1]) whole_lds;
  float* zprev = whole_lds + CHOL_S_ROWS * (CHOL_BS + 1);
  float* ynext = zprev + CHOL_BS;
  float* part = ynext + CHOL_BS;
  float(*D)[CHOL_BS + 1] = (float(*)[CHOL_BS + 1])(part + NMLL_REDUCE_TPB);
  float(*P0)[CHOL_BS + 1] = D + CHOL_BS;
  float(*P1)[CHOL_BS + 1] = P0 + (N - CHOL_BS);
  const int b = blockIdx.x;
  float* Ab = A + (long long)b * N * N;
  float* rhs_b = rhs ? rhs + (long long)b * N : nullptr;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  float ld = 0.0f;  // wave 0, lane 0: logdet, accumulated in step order
  int inf = 0;      // wave 0, lane 0: first failing column
  if (wave == 0) {
    // the serial chain is issue-bound: it goes first on its SIMD
    __builtin_amdgcn_s_setprio(3);
    inf = info[b];
  }
  // block 0 and its rhs segment, coalesced by the whole workgroup
  for (int idx = tid; idx < CHOL_BS * CHOL_BS; idx += CHOL_WHOLE_TPB)
    S[idx / CHOL_BS][idx % CHOL_BS] =
        Ab[(long long)(idx / CHOL_BS) * N + idx % CHOL_BS];
  if (rhs_b != nullptr && tid >= CHOL_WHOLE_TPB - CHOL_BS)
    S[CHOL_BS][tid - (CHOL_WHOLE_TPB - CHOL_BS)] =
        rhs_b[tid - (CHOL_WHOLE_TPB - CHOL_BS)];
  __syncthreads();

  for (int k0 = 0, s = 0; k0 < N; k0 += CHOL_BS, ++s) {
    const int bs = min(CHOL_BS, N - k0);
    const int rows = N - k0 - CHOL_BS;  // strip rows (<= 0: none)
    float(*Pcur)[CHOL_BS + 1] = (s & 1) ? P1 : P0;   // strip s -> panel s
    float(*Pprev)[CHOL_BS + 1] = (s & 1) ? P0 : P1;  // panel s-1: rows k0..N-1
    if (wave == 0) {
      if (s > 0) {
        // diagonal block and rhs segment: panel s-1's update, as in
        // chol_panel_body<true>; Pprev's first 32 rows are its Lj. Operand
        // rows past the matrix are clamped: they feed only discarded outputs.
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
          const int r16 = (sub >> 1) * 16, c16 = (sub & 1) * 16;
          const int ra = min(r16 + lr, bs - 1), rb = min(c16 + lr, bs - 1);
          const f32x4 acc = chol_subtile_acc(Pprev[ra], 0, Pprev[rb], 0, lk);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = r16 + lk * 4 + r, j = c16 + lr;
            const float a = D[i][j];
            if (i < bs && j < bs) S[i][j] = (j <= i) ? a - acc[r] : a;
          }
        }
        if (rhs_b != nullptr && lane < bs)
          S[CHOL_BS][lane] =
              chol_rhs_row_update(Pprev[lane], 0, zprev, ynext[lane]);
        __threadfence_block();  // S rows cross lanes inside wave 0
      }
      // lane 32 is the rhs row; a partial block is padded with the identity
      const int rhs_lane = (rhs_b != nullptr) ? CHOL_BS : -1;
      const bool own = lane < bs || lane == rhs_lane;
      float r[CHOL_BS];
#pragma unroll
      for (int t = 0; t < CHOL_BS; ++t)
        r[t] = (own && t < bs) ? S[lane][t] : ((lane == t) ? 1.0f : 0.0f);
      int bad = 0;
      float mylog = chol_factor_reg(r, lane, bs, k0, bad);
      if (own) {
#pragma unroll
        for (int t = 0; t < CHOL_BS; ++t) {
          if (t >= bs) continue;
          S[lane][t] = r[t];
        }
      }
      for (int off = 32; off > 0; off >>= 1) {
        mylog += __shfl_down(mylog, off);
        const int ob = __shfl_down(bad, off);
        bad = bad ? bad : ob;
      }
      ld += mylog;
      if (bad && inf == 0) inf = bad;
    } else if (s == 0) {
      // strip 0 as it stands
      for (int idx = tid - 64; idx < rows * CHOL_BS;
           idx += CHOL_WHOLE_TPB - 64) {
        const int r = idx / CHOL_BS, c = idx % CHOL_BS;
        Pcur[r][c] = Ab[(long long)(CHOL_BS + r) * N + c];
      }
    } else {
      const int w = wave - 1;
      // panel s-1 leaves for global, coalesced
      for (int idx = tid - 64; idx < (N - k0) * CHOL_BS;
           idx += CHOL_WHOLE_TPB - 64) {
        const int r = idx / CHOL_BS, c = idx % CHOL_BS;
        Ab[(long long)(k0 + r) * N + k0 - CHOL_BS + c] = Pprev[r][c];
      }
      // this worker's tiles (I, J), I >= imin, jmin <= J <= I, walked in
      // steps of 15 along the row-major index of the lower triangle
      const int jmin = k0 >> 4, imin = jmin + 2;
      const int ng = (N + 15) >> 4;
      int I = imin, J = jmin;
      {
        const int t0 = imin * (imin + 1) / 2 + jmin;
        J += (w + CHOL_WHOLE_WORKERS - t0 % CHOL_WHOLE_WORKERS) %
             CHOL_WHOLE_WORKERS;
        while (J > I) { J -= I + 1; ++I; }
      }
      while (I < ng) {
        int tI[CHOL_WHOLE_TILE_BATCH], tJ[CHOL_WHOLE_TILE_BATCH];
#pragma unroll
        for (int u = 0; u < CHOL_WHOLE_TILE_BATCH; ++u) {
          while (I < ng && J < jmin) {  // columns of finished panels
            J += CHOL_WHOLE_WORKERS;
            while (J > I) { J -= I + 1; ++I; }
          }
          tI[u] = I;
          tJ[u] = J;
          if (I < ng) {
            J += CHOL_WHOLE_WORKERS;
            while (J > I) { J -= I + 1; ++I; }
          }
        }
        float c[CHOL_WHOLE_TILE_BATCH][4];
#pragma unroll
        for (int u = 0; u < CHOL_WHOLE_TILE_BATCH; ++u) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = tI[u] * 16 + lk * 4 + r, j = tJ[u] * 16 + lr;
            c[u][r] = (tI[u] < ng && i < N && j < N && j <= i)
                          ? Ab[(long long)i * N + j]
                          : 0.0f;
          }
        }
#pragma unroll
        for (int u = 0; u < CHOL_WHOLE_TILE_BATCH; ++u) {
          if (tI[u] >= ng) continue;
          const int ra = min(tI[u] * 16 + lr, N - 1) - k0;
          const int rb = min(tJ[u] * 16 + lr, N - 1) - k0;
          const f32x4 acc = chol_subtile_acc(Pprev[ra], 0, Pprev[rb], 0, lk);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = tI[u] * 16 + lk * 4 + r, j = tJ[u] * 16 + lr;
            if (i < N && j < N && j <= i) {
              const float v = c[u][r] - acc[r];
              if (tJ[u] < imin) Pcur[i - k0 - CHOL_BS][j - k0] = v;  // strip s
              else Ab[(long long)i * N + j] = v;
            }
          }
        }
      }
      if (rhs_b != nullptr) {
        for (int g = w; g * 64 < N; g += CHOL_WHOLE_WORKERS) {
          const int i = g * 64 + lane;
          if (i >= k0 + CHOL_BS && i < N)
            rhs_b[i] = chol_rhs_row_update(Pprev[i - k0], 0, zprev, rhs_b[i]);
        }
      }
    }
    __syncthreads();
    // TRSM of strip s, one row per thread; the waves it leaves idle write
    // the factored block and z out and keep z for the next step's updates
    const int rows_up = rows > 0 ? (rows + 63) & ~63 : 0;
    if (tid < rows) {
      chol_trsm_row(Pcur[tid], S);
    } else if (tid >= rows_up) {
      const int u = tid - rows_up, nu = CHOL_WHOLE_TPB - rows_up;
      for (int idx = u; idx < bs * bs; idx += nu) {
        const int i = idx / bs, t = idx % bs;
        if (t <= i) Ab[(long long)(k0 + i) * N + k0 + t] = S[i][t];
      }
      if (rhs_b != nullptr && u < bs) {
        const float z = S[CHOL_BS][u];
        rhs_b[k0 + u] = z;
        zprev[u] = z;
      }
      if (rows > 0) {
        // the NEXT diagonal block and rhs segment as global holds them
        // (their last update is in front of the barrier above), staged
        // coalesced so that wave 0 finds them in LDS: no global latency in
        // front of the factor
        const int kn = k0 + CHOL_BS, bn = min(CHOL_BS, N - kn);
        for (int idx = u; idx < CHOL_BS * CHOL_BS; idx += nu) {
          const int i = idx / CHOL_BS, j = idx % CHOL_BS;
          D[i][j] = (i < bn && j < bn) ? Ab[(long long)(kn + i) * N + kn + j]
                                       : 0.0f;
        }
        if (rhs_b != nullptr && u < CHOL_BS)
          ynext[u] = (u < bn) ? rhs_b[kn + u] : 0.0f;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    logdet[b] = ld;
    info[b] = inf;
  }
  if (nmll_out != nullptr) {
    // z, logdet and info are final; the barrier publishes them
    __syncthreads();
    __threadfence_block();
    nmll_reduce_body(rhs_b, logdet + b, info + b, nmll_out + b, N, nmll_c,
                     part);
  }
}

// Blocked forward substitution: solve L z = y for R right-hand sides.
// One block per (batch, rhs). Per 32-column panel: wave 0 solves the
// 32x32 diagonal block wave-synchronously (lane j owns row j, solved
// entries broadcast by shuffle), then all threads apply the rank-32
// update in parallel — 2 barriers per panel instead of 2 per column (the
// former per-column loop spent ~600 barriers on N=300).
#define TRSV_BS 32

__global__ void forward_solve_batched_kernel(const float* __restrict__ L,
                                             float* __restrict__ Y,  // (B,N,R) inout
                                             int N, int R) {
  __shared__ float S[TRSV_BS][TRSV_BS + 1];
  __shared__ float z[TRSV_BS];
  __shared__ float yp[TRSV_BS];
  const int b = blockIdx.x;
  const int r = blockIdx.y;
  if (r >= R) return;
  const float* Lb = L + (long long)b * N * N;
  float* y = Y + (long long)b * N * R;
  const int tid = threadIdx.x;
  for (int k0 = 0; k0 < N; k0 += TRSV_BS) {
    const int bs = min(TRSV_BS, N - k0);
    // stage panel of L and the panel's rhs entries into LDS in parallel
    for (int idx = tid; idx < bs * bs; idx += blockDim.x)
      S[idx / bs][idx % bs] = Lb[(long long)(k0 + idx / bs) * N + k0 + idx % bs];
    if (tid < bs) yp[tid] = y[(k0 + tid) * R + r];
    __syncthreads();
    // wave-parallel diagonal solve: lane j owns panel row j; per column t
    // the solved z_t is broadcast with __shfl — no block barrier, no
    // global traffic inside the serial dependency chain.
    if (tid < 64) {
      const int j = tid;  // lanes >= bs just follow along
      float v = (j < bs) ? yp[j] : 0.0f;
      for (int t = 0; t < bs; ++t) {
        const float zt = __shfl(v, t) / S[t][t];
        if (j == t) {
          v = zt;
          z[t] = zt;
        } else if (j > t && j < bs) {
          v = fmaf(-S[j][t], zt, v);
        }
      }
      if (j < bs) y[(k0 + j) * R + r] = v;
    }
    __syncthreads();
    // rank-32 update of the remaining rows: rows below exist only under a
    // FULL panel, so the trip count is compile-time (unrolled loads)
    for (int i = k0 + TRSV_BS + tid; i < N; i += blockDim.x) {
      float acc = y[i * R + r];
      const float* row = Lb + (long long)i * N + k0;
#pragma unroll
      for (int t = 0; t < TRSV_BS; ++t) acc = fmaf(-row[t], z[t], acc);
      y[i * R + r] = acc;
    }
    __syncthreads();
  }
}

// Blocked backward substitution: solve L^T x = z (same structure, panels
// walked from the bottom; the update reads row segments of L, coalesced).
__global__ void backward_solve_batched_kernel(const float* __restrict__ L,
                                              float* __restrict__ Y,  // (B,N,R)
                                              int N, int R) {
  __shared__ float S[TRSV_BS][TRSV_BS + 1];
  __shared__ float z[TRSV_BS];
  __shared__ float yp[TRSV_BS];
  const int b = blockIdx.x;
  const int r = blockIdx.y;
  if (r >= R) return;
  const float* Lb = L + (long long)b * N * N;
  float* y = Y + (long long)b * N * R;
  const int tid = threadIdx.x;
  const int first = ((N - 1) / TRSV_BS) * TRSV_BS;
  for (int k0 = first; k0 >= 0; k0 -= TRSV_BS) {
    const int bs = min(TRSV_BS, N - k0);
    for (int idx = tid; idx < bs * bs; idx += blockDim.x)
      S[idx / bs][idx % bs] = Lb[(long long)(k0 + idx / bs) * N + k0 + idx % bs];
    if (tid < bs) yp[tid] = y[(k0 + tid) * R + r];
    __syncthreads();
    // wave-parallel diagonal solve against S^T, columns walked bottom-up
    if (tid < 64) {
      const int j = tid;
      float v = (j < bs) ? yp[j] : 0.0f;
      for (int t = bs - 1; t >= 0; --t) {
        const float zt = __shfl(v, t) / S[t][t];
        if (j == t) {
          v = zt;
          z[t] = zt;
        } else if (j < t) {
          v = fmaf(-S[t][j], zt, v);
        }
      }
      if (j < bs) y[(k0 + j) * R + r] = v;
    }
    __syncthreads();
    // update rows above the panel: x_i -= sum_t L[k0+t][i] * z[t]
    // (specialized full-panel path so the column loads unroll)
    if (bs == TRSV_BS) {
      for (int i = tid; i < k0; i += blockDim.x) {
        float acc = y[i * R + r];
#pragma unroll
        for (int t = 0; t < TRSV_BS; ++t)
          acc = fmaf(-Lb[(long long)(k0 + t) * N + i], z[t], acc);
        y[i * R + r] = acc;
      }
    } else {
      for (int i = tid; i < k0; i += blockDim.x) {
        float acc = y[i * R + r];
        for (int t = 0; t < bs; ++t)
          acc = fmaf(-Lb[(long long)(k0 + t) * N + i], z[t], acc);
        y[i * R + r] = acc;
      }
    }
    __syncthreads();
  }
}

__global__ void nmll_reduce_kernel(const float* __restrict__ Z,
                                   const float* __restrict__ half_logdet,
                                   const int* __restrict__ info,
                                   float* __restrict__ out, int N, float c) {
  __shared__ float part[NMLL_REDUCE_TPB];
  const int b = blockIdx.x;
  nmll_reduce_body(Z + (long long)b * N, half_logdet + b, info + b, out + b, N,
                   c, part);
}

extern "C" void launch_nmll_reduce(const float* Z, const float* half_logdet,
                                   const int* info, float* out, int B, int N,
                                   float c, hipStream_t stream) {
  hipLaunchKernelGGL(nmll_reduce_kernel, dim3(B), dim3(NMLL_REDUCE_TPB), 0,
                     stream, Z, half_logdet, info, out, N, c);
}

__global__ void zero_f32_kernel(float* __restrict__ p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0.0f;
}

// logdet accumulates across the panel launches, so every multik entry zeroes
// it first. An explicit zero KERNEL instead of hipMemsetAsync: under hipGraph
// stream capture (models/gp_core.py _NmllGraph) the captured memset node was
// observed to race with the first panel kernel's logdet accumulation on
// replay (bit-nondeterministic outputs with bit-identical inputs,
// scripts_det_debug6.py); a kernel node orders correctly.
static inline void launch_zero_logdet(float* logdet, int B,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(zero_f32_kernel, dim3((B + 255) / 256), dim3(256), 0,
                     stream, logdet, B);
}

// diagonal factor of the panel (chol_panel_body's REG):
//   lds — 2-column LDS broadcast rounds, separate shuffle solve of the rhs;
//   reg — register broadcast, deferred logdet, rhs as row 32.
// DMOSOPT_CHOL_FACTOR=lds/reg selects it, latched once per process; bitwise-
// identical results, measured A/B in profiles/README.md.
enum { CHOL_FACTOR_LDS = 0, CHOL_FACTOR_REG = 1 };
#define CHOL_FACTOR_DEFAULT CHOL_FACTOR_REG
static inline int chol_factor_default() {
  static int f = -1;
  if (f < 0) {
    const char* e = getenv("DMOSOPT_CHOL_FACTOR");
    f = e ? (e[0] == 'l' ? CHOL_FACTOR_LDS : CHOL_FACTOR_REG)
          : CHOL_FACTOR_DEFAULT;
  }
  return f;
}

// Plain panel launch, shared by the classic schedule, panel 0 of the
// look-ahead schedule and the bf16 path.
static inline void launch_chol_panel(float* A, float* logdet, int* info,
                                     float* rhs, int B, int N, int k0,
                                     int factor, hipStream_t stream) {
  if (factor == CHOL_FACTOR_REG)
    hipLaunchKernelGGL(chol_panel_kernel<true>, dim3(B), dim3(CHOL_PANEL_TPB),
                       0, stream, A, logdet, info, N, k0, rhs);
  else
    hipLaunchKernelGGL(chol_panel_kernel<false>, dim3(B),
                       dim3(CHOL_PANEL_TPB), 0, stream, A, logdet, info, N,
                       k0, rhs);
}

// 64x64 lower-triangle tile pairs of the trailing matrix that starts at r0
// (0 when nothing is left).
static inline int chol_tile_pairs(int N, int r0) {
  const int trailing = N - r0;
  if (trailing <= 0) return 0;
  const int nt = (trailing + SYRK_TS - 1) / SYRK_TS;
  return nt * (nt + 1) / 2;
}

// trailing-update schedule of the multik path:
//   classic    — panel launch, then a full-matrix SYRK launch, per step;
//   look-ahead — plain panel 0, then ONE chol_step_kernel launch per
//                remaining panel (bitwise-identical results).
// DMOSOPT_CHOL_LOOKAHEAD=1/0 selects it, latched once per process;
// measured A/B in profiles/README.md.
enum {
  CHOL_SCHED_CLASSIC = 0,
  CHOL_SCHED_LOOKAHEAD = 1,
  CHOL_SCHED_ONELAUNCH = 2  // further down
};
#define CHOL_LOOKAHEAD_DEFAULT 1
static inline int chol_lookahead_default() {
  static int la = -1;
  if (la < 0) {
    const char* e = getenv("DMOSOPT_CHOL_LOOKAHEAD");
    la = e ? (e[0] == '1' ? 1 : 0) : CHOL_LOOKAHEAD_DEFAULT;
  }
  return la;
}

static void chol_multik_classic(float* A, float* logdet, int* info,
                                float* rhs, int B, int N, int factor,
                                hipStream_t stream) {
  for (int k0 = 0; k0 < N; k0 += CHOL_BS) {
    launch_chol_panel(A, logdet, info, rhs, B, N, k0, factor, stream);
    const int pairs = chol_tile_pairs(N, k0 + CHOL_BS);
    if (pairs > 0)
      hipLaunchKernelGGL(chol_syrk_kernel, dim3(B, pairs),
                         dim3(CHOL_SYRK_TPB), 0, stream, A, N, k0, rhs);
  }
}

// nmll_out != nullptr (needs rhs and N > 32): the LAST step launch also
// reduces the NMLL into nmll_out (B,) — see chol_step_kernel.
static void chol_multik_lookahead(float* A, float* logdet, int* info,
                                  float* rhs, int B, int N, int factor,
                                  hipStream_t stream,
                                  float* nmll_out = nullptr,
                                  float nmll_c = 0.f) {
  launch_chol_panel(A, logdet, info, rhs, B, N, 0, factor, stream);
  for (int k0 = CHOL_BS; k0 < N; k0 += CHOL_BS) {
    // role B covers rows/columns >= k0 + 32; none left on the last steps
    const int pairs = chol_tile_pairs(N, k0 + CHOL_BS);
    const bool last = k0 + CHOL_BS >= N;
    float* out = last ? nmll_out : (float*)nullptr;
    if (factor == CHOL_FACTOR_REG)
      hipLaunchKernelGGL(chol_step_kernel<true>, dim3(B, 1 + pairs),
                         dim3(CHOL_PANEL_TPB), 0, stream, A, logdet, info, N,
                         k0, rhs, out, nmll_c);
    else
      hipLaunchKernelGGL(chol_step_kernel<false>, dim3(B, 1 + pairs),
                         dim3(CHOL_PANEL_TPB), 0, stream, A, logdet, info, N,
                         k0, rhs, out, nmll_c);
  }
}

// Up to this batch count the one-block-per-matrix kernel cannot fill the 256
// CUs, so the multi-launch path wins. DMOSOPT_CHOL_MODE=single|multik
// overrides the choice for A/B measurement.
#define CHOL_MULTIK_MAX_B 48

// one-launch schedule: chol_whole_kernel, ONE launch per factorization
// (grid B), logdet and info written by the kernel itself. It implements the
// reg factor only and needs more than one panel and both panel buffers
// inside one CU's LDS (N <= 615); any other request runs the look-ahead
// schedule. DMOSOPT_CHOL_ONELAUNCH=1/0 (latched once per process) says
// whether the default routes take it for B <= CHOL_MULTIK_MAX_B; measured
// A/B in profiles/README.md.
#define CHOL_ONELAUNCH_DEFAULT 1
static inline int chol_onelaunch_default() {
  static int ol = -1;
  if (ol < 0) {
    const char* e = getenv("DMOSOPT_CHOL_ONELAUNCH");
    ol = e ? (e[0] == '1' ? 1 : 0) : CHOL_ONELAUNCH_DEFAULT;
  }
  return ol;
}

static inline bool chol_onelaunch_fits(int N, int factor) {
  return factor == CHOL_FACTOR_REG && N > CHOL_BS &&
         chol_whole_lds_bytes(N) <= CHOL_CU_LDS_BYTES;
}

static void chol_onelaunch(float* A, float* logdet, int* info, float* rhs,
                           int B, int N, hipStream_t stream,
                           float* nmll_out = nullptr, float nmll_c = 0.f) {
  static bool lds_attr_set = false;
  if (!lds_attr_set) {
    hipFuncSetAttribute((const void*)chol_whole_kernel,
                        hipFuncAttributeMaxDynamicSharedMemorySize,
                        CHOL_CU_LDS_BYTES);
    lds_attr_set = true;
  }
  hipLaunchKernelGGL(chol_whole_kernel, dim3(B), dim3(CHOL_WHOLE_TPB),
                     chol_whole_lds_bytes(N), stream, A, logdet, info, N, rhs,
                     nmll_out, nmll_c);
}

// Explicit-schedule, explicit-factor entry (tests and isolated timing
// compare the schedules and the factors inside one process; the env switches
// are latched). factor < 0: the process default.
extern "C" void launch_cholesky_multik_sched(float* A, float* logdet,
                                             int* info, float* rhs, int B,
                                             int N, int sched, int factor,
                                             hipStream_t stream) {
  if (factor < 0) factor = chol_factor_default();
  if (sched == CHOL_SCHED_ONELAUNCH) {
    if (chol_onelaunch_fits(N, factor)) {
      chol_onelaunch(A, logdet, info, rhs, B, N, stream);
      return;
    }
    sched = CHOL_SCHED_LOOKAHEAD;
  }
  launch_zero_logdet(logdet, B, stream);
  if (sched == CHOL_SCHED_LOOKAHEAD)
    chol_multik_lookahead(A, logdet, info, rhs, B, N, factor, stream);
  else
    chol_multik_classic(A, logdet, info, rhs, B, N, factor, stream);
}

// 1 when the default routes factor (B, N) with the one-launch kernel.
static inline bool chol_onelaunch_applies(int B, int N) {
  return chol_onelaunch_default() && chol_lookahead_default() &&
         B <= CHOL_MULTIK_MAX_B &&
         chol_onelaunch_fits(N, chol_factor_default());
}

extern "C" void launch_cholesky_multik(float* A, float* logdet, int* info,
                                       float* rhs, int B, int N,
                                       hipStream_t stream) {
  launch_cholesky_multik_sched(
      A, logdet, info, rhs, B, N,
      chol_onelaunch_applies(B, N)
          ? CHOL_SCHED_ONELAUNCH
          : (chol_lookahead_default() ? CHOL_SCHED_LOOKAHEAD
                                      : CHOL_SCHED_CLASSIC),
      -1, stream);
}

// bf16-SYRK variant of the classic schedule (config-#2 precision route):
// panels factor in exact fp32 (chol_panel_kernel), only the trailing
// C -= P P^T runs on the bf16 matrix units (matern_bf16.hip).
extern "C" void launch_cholesky_multik_bf16(float* A, float* logdet,
                                            int* info, int B, int N,
                                            hipStream_t stream) {
  launch_zero_logdet(logdet, B, stream);
  for (int k0 = 0; k0 < N; k0 += CHOL_BS) {
    launch_chol_panel(A, logdet, info, nullptr, B, N, k0,
                      chol_factor_default(), stream);
    const int pairs = chol_tile_pairs(N, k0 + CHOL_BS);
    if (pairs > 0) launch_chol_syrk_bf16(A, N, k0, pairs, B, stream);
  }
}

// Factor with the forward solve of rhs (B, N) fused into the multik launch
// chain. Returns -1 without launching anything when the multik path does not
// apply (DMOSOPT_CHOL_MODE=single, DMOSOPT_CHOL_FUSED_SOLVE=0, a single
// panel, or a batch large enough for the one-block-per-matrix kernel); the
// caller then factors and solves separately.
static inline bool chol_fused_solve_applies(int B, int N) {
  static int ok = -1;
  if (ok < 0) {
    const char* m = getenv("DMOSOPT_CHOL_MODE");
    const char* f = getenv("DMOSOPT_CHOL_FUSED_SOLVE");
    ok = ((m && m[0] == 's') || (f && f[0] == '0')) ? 0 : 1;
  }
  return ok && N > CHOL_BS && B <= CHOL_MULTIK_MAX_B;
}

extern "C" int launch_cholesky_fused_solve(float* A, float* logdet,
                                           int* info, float* rhs, int B,
                                           int N, hipStream_t stream) {
  if (!chol_fused_solve_applies(B, N)) return -1;
  launch_cholesky_multik(A, logdet, info, rhs, B, N, stream);
  return 0;
}

// 1 when launch_cholesky_fused_solve would take the look-ahead multik route
// for this shape: the route whose launch chain can carry the NMLL prologue
// and epilogue (launch_cholesky_nmll_chain).
extern "C" int cholesky_nmll_chain_applies(int B, int N) {
  return chol_fused_solve_applies(B, N) && chol_lookahead_default();
}

// Factor + fused forward solve + NMLL and nothing else: one chol_whole_kernel
// launch where the one-launch schedule applies, else the look-ahead
// schedule's ceil(N/32) launches. The caller's assemble launch has already
// set rhs = y, logdet = 0 and info = 0 (matern.hip's prologue variant), and
// the last launch writes out (B,). Only where
// cholesky_nmll_chain_applies(B, N).
extern "C" void launch_cholesky_nmll_chain(float* A, float* logdet, int* info,
                                           float* rhs, float* out, int B,
                                           int N, float c,
                                           hipStream_t stream) {
  if (chol_onelaunch_applies(B, N))
    chol_onelaunch(A, logdet, info, rhs, B, N, stream, out, c);
  else
    chol_multik_lookahead(A, logdet, info, rhs, B, N, chol_factor_default(),
                          stream, out, c);
}

extern "C" void launch_cholesky_batched(float* A, float* logdet, int* info,
                                        int B, int N, hipStream_t stream) {
  static int multik_max_b = -2;
  if (multik_max_b == -2) {
    const char* env = getenv("DMOSOPT_CHOL_MODE");
    if (env && env[0] == 's') multik_max_b = 0;
    else if (env && env[0] == 'm') multik_max_b = 1 << 30;
    else multik_max_b = CHOL_MULTIK_MAX_B;
  }
  if (B <= multik_max_b && N > CHOL_BS) {
    launch_cholesky_multik(A, logdet, info, nullptr, B, N, stream);
    return;
  }
  static bool lds_attr_set = false;
  if (!lds_attr_set) {
    hipFuncSetAttribute((const void*)cholesky_batched_kernel,
                        hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)sizeof(CholLds));
    lds_attr_set = true;
  }
  hipLaunchKernelGGL(cholesky_batched_kernel, dim3(B), dim3(CHOL_TPB),
                     sizeof(CholLds), stream, A, logdet, info, N);
}

extern "C" void launch_forward_solve_batched(const float* L, float* Y, int B,
                                             int N, int R, hipStream_t stream) {
  dim3 block(256, 1);
  dim3 grid(B, R);
  hipLaunchKernelGGL(forward_solve_batched_kernel, grid, block, 0, stream, L,
                     Y, N, R);
}

extern "C" void launch_backward_solve_batched(const float* L, float* Y, int B,
                                              int N, int R, hipStream_t stream) {
  dim3 block(256, 1);
  dim3 grid(B, R);
  hipLaunchKernelGGL(backward_solve_batched_kernel, grid, block, 0, stream, L,
                     Y, N, R);
}
