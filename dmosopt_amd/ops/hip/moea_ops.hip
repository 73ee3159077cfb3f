// Small fused MOEA kernels for the per-generation loop.
//
// The generation loop is launch-count bound (~9-12 us of in-stream gap per
// kernel on this stack, measured from rocpd timelines), so these kernels
// exist to collapse chains of tiny torch ops into single launches:
//   tournament_kernel: stable rank sort + Gumbel top-k weighted sampling
//                      without replacement + pool gather  (~8 launches -> 1)
//   survivor_count_kernel: operator-success accounting against the
//                      survivor permutation                (~8 launches -> 1)

#include "common.h"
#include "launchers.h"
#include <math.h>

#define TOUR_TPB 256
#define TOUR_NMAX 2048  // npow2 cap; LDS fits the 64 KB default

// population (N, d) f32; rank (N,) int64. Writes pool (poolsize, d) and
// pool_idx (poolsize,) int64.
// Sampling: candidates sorted by (rank, index) ascending; candidate at
// sorted position i gets weight p*(1-p)^i (reference MOEA.py:385-395);
// weighted sampling WITHOUT replacement via Gumbel top-k on
// key_i = i*log(1-p) + Gumbel_i (constants cancel under top-k).
template <int TPB>
__global__ __launch_bounds__(TPB) void tournament_kernel(
    const float* __restrict__ population, const long long* __restrict__ rank,
    float* __restrict__ pool, long long* __restrict__ pool_idx, int N, int d,
    int poolsize, int npow2, float log1mp, unsigned long long seed) {
  extern __shared__ char sh_raw[];
  long long* key = (long long*)sh_raw;        // npow2 (composite sort key)
  int* idx = (int*)(key + npow2);             // npow2
  float* gkey = (float*)(idx + npow2);        // npow2 (gumbel keys)

  const int tid = threadIdx.x;
  __shared__ int unsorted;
  if (tid == 0) unsorted = 0;
  __syncthreads();
  // stage 1: stable sort by rank — composite integer key rank*N + index.
  // nsga2_select emits the population ALREADY rank-sorted, making this a
  // provable identity permutation (stable sort of a non-decreasing key):
  // detect and skip the whole bitonic pass in that (dominant) case.
  for (int i = tid; i < npow2; i += TPB) {
    key[i] = (i < N) ? (rank[i] * (long long)N + i) : 0x7FFFFFFFFFFFFFFFLL;
    idx[i] = i;
    if (i + 1 < N && rank[i] > rank[i + 1]) atomicOr(&unsorted, 1);
  }
  __syncthreads();
  if (unsorted)
  for (int ks = 2; ks <= npow2; ks <<= 1) {
    for (int js = ks >> 1; js > 0; js >>= 1) {
      for (int i = tid; i < npow2; i += TPB) {
        const int ixj = i ^ js;
        if (ixj > i) {
          const bool up = ((i & ks) == 0);
          if (up ? (key[i] > key[ixj]) : (key[i] < key[ixj])) {
            long long tk = key[i]; key[i] = key[ixj]; key[ixj] = tk;
            int ti = idx[i]; idx[i] = idx[ixj]; idx[ixj] = ti;
          }
        }
      }
      __syncthreads();
    }
  }
  // idx[i] now = candidate at sorted position i. Stage 2: Gumbel keys per
  // position, sort DESCENDING, take first poolsize.
  for (int i = tid; i < npow2; i += TPB) {
    if (i < N) {
      Philox4 r = philox4x32(seed, (unsigned long long)i);
      const float u = u01(r.c0);
      gkey[i] = (float)i * log1mp - logf(-logf(u));
    } else {
      gkey[i] = -INFINITY;
    }
  }
  __syncthreads();
  for (int ks = 2; ks <= npow2; ks <<= 1) {
    for (int js = ks >> 1; js > 0; js >>= 1) {
      for (int i = tid; i < npow2; i += TPB) {
        const int ixj = i ^ js;
        if (ixj > i) {
          const bool up = ((i & ks) == 0);
          // descending overall
          if (up ? (gkey[i] < gkey[ixj]) : (gkey[i] > gkey[ixj])) {
            float tg = gkey[i]; gkey[i] = gkey[ixj]; gkey[ixj] = tg;
            int ti = idx[i]; idx[i] = idx[ixj]; idx[ixj] = ti;
          }
        }
      }
      __syncthreads();
    }
  }
  // stage 3: gather the pool rows
  for (int j = tid; j < poolsize; j += TPB) pool_idx[j] = idx[j];
  __syncthreads();
  for (long long t = tid; t < (long long)poolsize * d; t += TPB) {
    const int r = (int)(t / d), c = (int)(t % d);
    pool[t] = population[(long long)idx[r] * d + c];
  }
}

// Multi-block route for the Gumbel tournament keys (same Philox counters
// and formula as tournament_kernel's stage 2): for N beyond the one-
// workgroup bitonic's sweet spot the caller sorts these with a radix
// argsort instead. Continuous keys -> tie order never matters, so both
// routes produce the same pool for the same seed.
__global__ void tournament_keys_kernel(float* __restrict__ gkey, int N,
                                       float log1mp,
                                       unsigned long long seed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  Philox4 r = philox4x32(seed, (unsigned long long)i);
  const float u = u01(r.c0);
  gkey[i] = (float)i * log1mp - logf(-logf(u));
}

extern "C" void launch_tournament_keys(float* gkey, int N, float log1mp,
                                       unsigned long long seed,
                                       hipStream_t stream) {
  hipLaunchKernelGGL(tournament_keys_kernel, dim3((N + 255) / 256), dim3(256),
                     0, stream, gkey, N, log1mp, seed);
}

extern "C" int launch_tournament(const float* population, const long long* rank,
                                 float* pool, long long* pool_idx, int N,
                                 int d, int poolsize, float log1mp,
                                 unsigned long long seed, hipStream_t stream) {
  int npow2 = 1;
  while (npow2 < N) npow2 <<= 1;
  if (npow2 > TOUR_NMAX) return -1;
  const size_t lds = (size_t)npow2 * (8 + 4 + 4);
  if (npow2 > 512)
    hipLaunchKernelGGL(tournament_kernel<1024>, dim3(1), dim3(1024), lds,
                       stream, population, rank, pool, pool_idx, N, d,
                       poolsize, npow2, log1mp, seed);
  else
    hipLaunchKernelGGL(tournament_kernel<TOUR_TPB>, dim3(1), dim3(TOUR_TPB),
                       lds, stream, population, rank, pool, pool_idx, N, d,
                       poolsize, npow2, log1mp, seed);
  return 0;
}

// Survivor accounting: children occupied rows [0, n_children) of the
// concatenated population; c_idx lists the crossover child slots. Adds
// (#surviving crossover children)/2 and #surviving mutation children to the
// int64 scalar counters.
__global__ void survivor_count_kernel(const long long* __restrict__ perm,
                                      const long long* __restrict__ c_idx,
                                      int n_perm, int n_cross, int n_children,
                                      long long* __restrict__ succ_cross,
                                      long long* __restrict__ succ_mut) {
  __shared__ unsigned int is_cross[(2048 + 31) / 32];
  __shared__ int cnt_c, cnt_m;
  const int tid = threadIdx.x;
  const int words = (n_children + 31) / 32;
  for (int w = tid; w < words; w += blockDim.x) is_cross[w] = 0u;
  if (tid == 0) { cnt_c = 0; cnt_m = 0; }
  __syncthreads();
  for (int i = tid; i < n_cross; i += blockDim.x) {
    const int s = (int)c_idx[i];
    atomicOr(&is_cross[s >> 5], 1u << (s & 31));
  }
  __syncthreads();
  int lc = 0, lm = 0;
  for (int i = tid; i < n_perm; i += blockDim.x) {
    const long long e = perm[i];
    if (e < n_children) {
      if (is_cross[(int)(e >> 5)] & (1u << ((int)e & 31))) ++lc;
      else ++lm;
    }
  }
  atomicAdd(&cnt_c, lc);
  atomicAdd(&cnt_m, lm);
  __syncthreads();
  if (tid == 0) {
    atomicAdd((unsigned long long*)succ_cross, (unsigned long long)(cnt_c / 2));
    atomicAdd((unsigned long long*)succ_mut, (unsigned long long)cnt_m);
  }
}

extern "C" int launch_survivor_count(const long long* perm,
                                     const long long* c_idx, int n_perm,
                                     int n_cross, int n_children,
                                     long long* succ_cross,
                                     long long* succ_mut,
                                     hipStream_t stream) {
  if (n_children > 2048) return -1;
  hipLaunchKernelGGL(survivor_count_kernel, dim3(1), dim3(256), 0, stream,
                     perm, c_idx, n_perm, n_cross, n_children, succ_cross,
                     succ_mut);
  return 0;
}

// key[i] = (rank[i] << 32) | (0x7FFFFFFF - float_bits(max(crowd,0)))
// (one launch instead of the 5-op torch packing chain in survivor select)
__global__ void pack_rank_crowd_kernel(const long long* __restrict__ rank,
                                       const float* __restrict__ crowd,
                                       long long* __restrict__ key, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float d = crowd[i];
  if (!(d >= 0.f)) d = 0.f;               // clamp + NaN
  if (isinf(d)) d = 3.4028235e38f;        // +inf -> fmax
  unsigned int bits = __float_as_uint(d);
  key[i] = (rank[i] << 32) | (long long)(0x7FFFFFFFu - bits);
}

extern "C" void launch_pack_rank_crowd(const long long* rank,
                                       const float* crowd, long long* key,
                                       int N, hipStream_t stream) {
  hipLaunchKernelGGL(pack_rank_crowd_kernel, dim3((N + 255) / 256), dim3(256),
                     0, stream, rank, crowd, key, N);
}

// One launch gathering the three survivor outputs.
__global__ void gather3_kernel(const float* __restrict__ parm,
                               const float* __restrict__ obj,
                               const long long* __restrict__ rank,
                               const long long* __restrict__ perm,
                               float* __restrict__ parm_o,
                               float* __restrict__ obj_o,
                               long long* __restrict__ rank_o, int pop, int d,
                               int m) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)pop * (d + m + 1);
  if (t >= total) return;
  const int r = (int)(t / (d + m + 1));
  const int c = (int)(t % (d + m + 1));
  const long long src = perm[r];
  if (c < d) parm_o[(long long)r * d + c] = parm[src * d + c];
  else if (c < d + m) obj_o[(long long)r * m + (c - d)] = obj[src * m + (c - d)];
  else rank_o[r] = rank[src];
}

extern "C" void launch_gather3(const float* parm, const float* obj,
                               const long long* rank, const long long* perm,
                               float* parm_o, float* obj_o, long long* rank_o,
                               int pop, int d, int m, hipStream_t stream) {
  const long long total = (long long)pop * (d + m + 1);
  hipLaunchKernelGGL(gather3_kernel, dim3((int)((total + 255) / 256)),
                     dim3(256), 0, stream, parm, obj, rank, perm, parm_o,
                     obj_o, rank_o, pop, d, m);
}

// ---------------------------------------------- fused rank/crowd argsort
// (key, idx) pairs bitonic-sorted in LDS by ONE workgroup: replaces
// pack_rank_crowd + torch's radix argsort (3-4 launches) with one. The
// comparator is (key asc, idx asc) — exactly torch's stable argsort of the
// packed key, so the selection permutation is bitwise unchanged.
#define RCS_TPB 1024

__global__ __launch_bounds__(RCS_TPB) void rank_crowd_sort_kernel(
    const long long* __restrict__ rank, const float* __restrict__ crowd,
    long long* __restrict__ perm, int N, int pop) {
  extern __shared__ char sh[];
  long long* keys = (long long*)sh;  // M
  int* idxs = (int*)(keys + 0);      // placed after keys below
  int M = 1;
  while (M < N) M <<= 1;
  idxs = (int*)(keys + M);
  const int tid = threadIdx.x;

  for (int i = tid; i < M; i += RCS_TPB) {
    if (i < N) {
      // (rank << 32) | ~monotone_bits(crowd): descending crowding within
      // ascending rank (same mapping as pack_rank_crowd_kernel /
      // ops.fused_rank_metric_perm)
      float d = crowd[i];
      if (isnan(d)) d = 0.f;
      unsigned int b = __float_as_uint(d);
      unsigned int asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
      keys[i] = ((long long)rank[i] << 32) |
                (long long)(0xFFFFFFFFu - asc);
      idxs[i] = i;
    } else {
      keys[i] = 0x7FFFFFFFFFFFFFFFLL;  // pads sort to the end
      idxs[i] = 0x7FFFFFFF;
    }
  }
  __syncthreads();
  for (int k = 2; k <= M; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < M; i += RCS_TPB) {
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
  for (int i = tid; i < pop && i < N; i += RCS_TPB)
    perm[i] = (long long)idxs[i];
}

extern "C" int launch_rank_crowd_sort(const long long* rank,
                                      const float* crowd, long long* perm,
                                      int N, int pop, hipStream_t stream) {
  int M = 1;
  while (M < N) M <<= 1;
  const size_t lds = (size_t)M * (sizeof(long long) + sizeof(int));
  if (lds > 144 * 1024) return -1;  // caller uses pack + torch argsort
  static bool attr_set = false;
  if (!attr_set) {
    hipFuncSetAttribute((const void*)rank_crowd_sort_kernel,
                        hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
    attr_set = true;
  }
  hipLaunchKernelGGL(rank_crowd_sort_kernel, dim3(1), dim3(RCS_TPB), lds,
                     stream, rank, crowd, perm, N, pop);
  return 0;
}

// ------------------------------------------------- SMPSO velocity update
// Constriction-factor velocity + clamp in one launch (reference
// SMPSO.py:316-348; replaces the ~6-op torch expression per swarm per
// generation). Scalars (w, c1*r1, c2*r2, chi) are drawn host-side for RNG
// parity with the reference's per-swarm scalar draws.
__global__ void smpso_velocity_kernel(
    const float* __restrict__ position,  // (n, d)
    const float* __restrict__ velocity,  // (n, d)
    const float* __restrict__ leader1,   // (d,)
    const float* __restrict__ leader2,   // (d,)
    const float* __restrict__ xlb, const float* __restrict__ xub,
    float* __restrict__ out, int n, int d, float w, float a1, float a2,
    float chi) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n * d) return;
  const int k = (int)(t % d);
  const float p = position[t];
  const float v = chi * (w * velocity[t] + a1 * (leader1[k] - p) +
                         a2 * (leader2[k] - p));
  const float delta = 0.5f * (xub[k] - xlb[k]);
  out[t] = fminf(fmaxf(v, -delta), delta);
}

extern "C" void launch_smpso_velocity(const float* position,
                                      const float* velocity,
                                      const float* leader1,
                                      const float* leader2, const float* xlb,
                                      const float* xub, float* out, int n,
                                      int d, float w, float a1, float a2,
                                      float chi, hipStream_t stream) {
  const long long total = (long long)n * d;
  hipLaunchKernelGGL(smpso_velocity_kernel,
                     dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     stream, position, velocity, leader1, leader2, xlb, xub,
                     out, n, d, w, a1, a2, chi);
}

// Row-wise concat of two blocks and a column sum: trivial kernels that
// replace at::cat / at::sum dispatches inside nsga2_select — each ATen
// call costs ~7-10 us of host time in the host-dispatch-bound generation
// loop; a raw launch costs ~2 us.
__global__ void cat_rows_kernel(const float* __restrict__ a,
                                const float* __restrict__ b,
                                float* __restrict__ out, long long na_elems,
                                long long total_elems) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total_elems) return;
  out[i] = (i < na_elems) ? a[i] : b[i - na_elems];
}

extern "C" void launch_cat_rows(const float* a, const float* b, float* out,
                                long long na_elems, long long total_elems,
                                hipStream_t stream) {
  hipLaunchKernelGGL(cat_rows_kernel,
                     dim3((int)((total_elems + 255) / 256)), dim3(256), 0,
                     stream, a, b, out, na_elems, total_elems);
}

// column sum of an (m, N) matrix -> (N,), fixed accumulation order over m
// (deterministic; m is the objective count, <= ~10)
__global__ void colsum_kernel(const float* __restrict__ per_dim,
                              float* __restrict__ out, int m, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float acc = 0.f;
  for (int j = 0; j < m; ++j) acc += per_dim[(long long)j * N + i];
  out[i] = acc;
}

extern "C" void launch_colsum(const float* per_dim, float* out, int m, int N,
                              hipStream_t stream) {
  hipLaunchKernelGGL(colsum_kernel, dim3((N + 255) / 256), dim3(256), 0,
                     stream, per_dim, out, m, N);
}
