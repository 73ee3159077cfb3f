// Device inlines shared by the per-generation MOEA kernels (pareto.hip,
// variation.hip, moea_ops.hip). A value that must be bitwise identical in two
// kernels is computed by ONE inline here: identical source expressions in two
// kernels may contract differently under -ffp-contract=fast (NOTES.md).
#pragma once

#include "common.h"
#include <math.h>

// SBX / mutation child arithmetic with a PINNED fmaf order: under the
// default -ffp-contract=fast the compiler may contract the blend
// differently in different kernels (observed: sbx_batch_kernel vs
// variation_events_kernel differed by ULPs for identical Philox draws),
// which breaks the cross-path bitwise-identity guarantee the tests assert.
__device__ __forceinline__ void sbx_children(float a, float b, float beta,
                                             float lo, float hi, float* c1,
                                             float* c2) {
  const float x1 = 0.5f * fmaf(-beta, a, fmaf(beta, b, a + b));
  const float x2 = 0.5f * fmaf(beta, a, fmaf(-beta, b, a + b));
  *c1 = fminf(fmaxf(x1, lo), hi);
  *c2 = fminf(fmaxf(x2, lo), hi);
}

__device__ __forceinline__ float mutated_child(float p, float delta, float lo,
                                               float hi) {
  const float v = fmaf(hi - lo, delta, p);
  return fminf(fmaxf(v, lo), hi);
}

// Gene g of event ev of the event-decoded variation: crossover event ev < C
// writes both children (one Philox draw) to rows ci[2 ev], ci[2 ev + 1] of out,
// mutation event ev - C to row mi[ev - C]. Parent row r of the pool is row
// pool_row[r] of src when pool_row is given (the pool was never gathered), row
// r of src without it. PoolIdx is int (LDS) or long long (global).
template <typename PoolIdx>
__device__ __forceinline__ void variation_event_gene(
    const float* __restrict__ src, const PoolIdx* pool_row,
    const long long* __restrict__ ci, const long long* __restrict__ mi,
    const long long* __restrict__ p1, const long long* __restrict__ p2,
    const long long* __restrict__ im, const float* __restrict__ di_c,
    const float* __restrict__ di_m, const float* __restrict__ lo,
    const float* __restrict__ hi, float* __restrict__ out, int ev, int g,
    int C, int d, float mutation_rate, unsigned long long seed_sbx,
    unsigned long long seed_mut) {
  if (ev < C) {
    long long r1 = p1[ev], r2 = p2[ev];
    if (pool_row) { r1 = (long long)pool_row[r1]; r2 = (long long)pool_row[r2]; }
    const float a = src[r1 * d + g];
    const float b = src[r2 * d + g];
    const Philox4 r = philox4x32(seed_sbx, (unsigned long long)ev * d + g);
    const float u = u01(r.c0);
    const float e = 1.f / (di_c[g] + 1.f);
    const float beta = (u <= 0.5f) ? __powf(2.f * u, e)
                                   : __powf(1.f / (2.f * (1.f - u)), e);
    float c1, c2;
    sbx_children(a, b, beta, lo[g], hi[g], &c1, &c2);
    out[ci[2 * ev] * d + g] = c1;
    out[ci[2 * ev + 1] * d + g] = c2;
  } else {
    const int m = ev - C;
    long long r0 = im[m];
    if (pool_row) r0 = (long long)pool_row[r0];
    const float p = src[r0 * d + g];
    const Philox4 ph =
        philox4x32(seed_mut ^ 0x5deece66dULL, (unsigned long long)m * d + g);
    const float u = u01(ph.c0);
    const float e = 1.f / (di_m[g] + 1.f);
    const float delta = (u < mutation_rate)
                            ? __powf(2.f * u, e) - 1.f
                            : 1.f - __powf(2.f * (1.f - u), e);
    out[mi[m] * d + g] = mutated_child(p, delta, lo[g], hi[g]);
  }
}

// Gaps of one ascending-sorted objective column: row idxs[i] gets boundary = 1,
// interior = (vals[i+1] - vals[i-1]) / span in out[idxs[i]]; the column min /
// max are vals[0] / vals[N-1]. No barrier.
__device__ __forceinline__ void crowding_gaps(const float* vals,
                                              const int* idxs, float* out,
                                              int N, int tid, int nthreads) {
  const float l = vals[0];
  const float h = vals[N - 1];
  float s = h - l;
  if (!(s > 0.f) || !isfinite(s)) s = 1.f;
  for (int i = tid; i < N; i += nthreads) {
    float d = (i == 0 || i == N - 1) ? 1.f : (vals[i + 1] - vals[i - 1]) / s;
    if (isnan(d)) d = 0.f;
    out[idxs[i]] = d;
  }
}

// Crowding of one objective column by a whole workgroup: vals / idxs (npow2
// each, LDS) hold the raw column padded with +inf and the row numbers; they
// are bitonic-sorted ascending, then crowding_gaps writes out. The value given to
// tied column entries depends on the network's tie order, which depends on
// npow2 alone (each pass's compare-exchange pairs are disjoint, so not on the
// number of threads): every caller that must agree passes the same npow2.
// tid / nthreads number the threads that share this column: a workgroup may
// sort several columns at once, each with its own group of threads and its
// own arrays. The barriers are the block's, so every thread of the block
// makes the call with the same npow2, a group without a column with active =
// false. Ends with a block barrier after the sort, none after the writes to
// out.
__device__ __forceinline__ void crowding_sort_gaps(float* vals, int* idxs,
                                                   float* out, int N,
                                                   int npow2, int tid,
                                                   int nthreads,
                                                   bool active = true) {
  // bitonic sort ascending (stable order not required: equal normalized
  // values produce zero gaps either way)
  for (int ksz = 2; ksz <= npow2; ksz <<= 1) {
    for (int jsz = ksz >> 1; jsz > 0; jsz >>= 1) {
      for (int i = tid; active && i < npow2; i += nthreads) {
        const int ixj = i ^ jsz;
        if (ixj > i) {
          const bool up = ((i & ksz) == 0);
          const bool swap = up ? (vals[i] > vals[ixj]) : (vals[i] < vals[ixj]);
          if (swap) {
            float tv = vals[i]; vals[i] = vals[ixj]; vals[ixj] = tv;
            int tixx = idxs[i]; idxs[i] = idxs[ixj]; idxs[ixj] = tixx;
          }
        }
      }
      __syncthreads();
    }
  }
  if (active) crowding_gaps(vals, idxs, out, N, tid, nthreads);
}

// (rank << 32) | ~monotone_bits(crowd): descending crowding within ascending
// rank (the key of ops.fused_rank_metric_perm)
__device__ __forceinline__ long long rank_crowd_key(long long rank, float d) {
  if (isnan(d)) d = 0.f;
  const unsigned int b = __float_as_uint(d);
  const unsigned int asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return (rank << 32) | (long long)(0xFFFFFFFFu - asc);
}

// (key asc, idx asc) bitonic sort of M = 2^k pairs in LDS by a whole
// workgroup: torch's stable argsort of the key. Ends with a block barrier.
__device__ __forceinline__ void key_idx_sort(long long* keys, int* idxs, int M,
                                             int tid, int nthreads) {
  for (int k = 2; k <= M; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < M; i += nthreads) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const bool up = ((i & k) == 0);
          const long long ka = keys[i], kb = keys[ixj];
          const int ia = idxs[i], ib = idxs[ixj];
          const bool gt = (ka > kb) || (ka == kb && ia > ib);
          if (gt == up) {
            keys[i] = kb; keys[ixj] = ka;
            idxs[i] = ib; idxs[ixj] = ia;
          }
        }
      }
      __syncthreads();
    }
  }
}
