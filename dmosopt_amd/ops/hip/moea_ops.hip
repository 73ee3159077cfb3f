// Small fused MOEA kernels for the per-generation loop.
//
// The generation loop is launch-count bound (~9-12 us of in-stream gap per
// kernel on this stack, measured from rocpd timelines), so these kernels
// exist to collapse chains of tiny torch ops into single launches:
//   tournament_kernel: stable rank sort + Gumbel top-k weighted sampling
//                      without replacement + pool gather  (~8 launches -> 1)
//   survivor_count_kernel: operator-success accounting against the
//                      survivor permutation                (~8 launches -> 1)
//   spawn_fused_kernel: tournament + event-decoded variation  (2 -> 1)
//   dom_bits_pair_kernel + nsga2_select_fused_kernel: the whole survivor
//                      selection of nsga2_select_acc          (11 -> 2)

#include "common.h"
#include "launchers.h"
#include "moea_device.h"
#include <math.h>
#include <algorithm>

#define TOUR_TPB 256
#define TOUR_NMAX 2048  // npow2 cap; LDS fits the 64 KB default

// Tournament order by a whole workgroup: afterwards idx[j], j < poolsize, is
// the population row of pool row j. rank (N,) int64; key / idx / gkey are LDS
// arrays of npow2 entries.
// Sampling: candidates sorted by (rank, index) ascending; candidate at
// sorted position i gets weight p*(1-p)^i (reference MOEA.py:385-395);
// weighted sampling WITHOUT replacement via Gumbel top-k on
// key_i = i*log(1-p) + Gumbel_i (constants cancel under top-k).
// COUNT: the descending order of the Gumbel keys is first COUNTED (place of a
// key = number of larger ones; no barriers) and only sorted by the network
// where two keys are equal, which is where the network's tie order shows.
// unsorted: two LDS ints. Returns the array that holds the order: idx, or
// with COUNT the front of key.
template <int TPB, bool COUNT>
__device__ __forceinline__ const int* tournament_order(
    const long long* __restrict__ rank, long long* key, int* idx, float* gkey,
    int* unsorted, int N, int npow2, float log1mp, unsigned long long seed) {
  const int tid = threadIdx.x;
  if (tid == 0) { unsorted[0] = 0; unsorted[1] = 0; }
  __syncthreads();
  // stage 1: stable sort by rank — composite integer key rank*N + index.
  // nsga2_select emits the population ALREADY rank-sorted, making this a
  // provable identity permutation (stable sort of a non-decreasing key):
  // detect and skip the whole bitonic pass in that (dominant) case.
  for (int i = tid; i < npow2; i += TPB) {
    key[i] = (i < N) ? (rank[i] * (long long)N + i) : 0x7FFFFFFFFFFFFFFFLL;
    idx[i] = i;
    if (i + 1 < N && rank[i] > rank[i + 1]) atomicOr(&unsorted[0], 1);
  }
  __syncthreads();
  if (unsorted[0])
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
  if (COUNT) {
    int* sel = (int*)key;  // the rank keys are dead
    bool tie = false;
    for (int i = tid; i < N; i += TPB) {
      const float gi = gkey[i];
      int pos = 0;
#pragma unroll 8
      for (int j = 0; j < N; ++j) {
        const float gj = gkey[j];
        pos += (gj > gi || (gj == gi && j < i)) ? 1 : 0;
        tie |= (gj == gi && j != i);
      }
      tie |= (gi != gi);
      sel[pos] = idx[i];  // pos < N whatever the keys
    }
    if (tie) atomicOr(&unsorted[1], 1);
    __syncthreads();
    if (!unsorted[1]) return sel;
  }
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
  return idx;
}

// population (N, d) f32; rank (N,) int64. Writes pool (poolsize, d) and
// pool_idx (poolsize,) int64.
template <int TPB>
__global__ __launch_bounds__(TPB) void tournament_kernel(
    const float* __restrict__ population, const long long* __restrict__ rank,
    float* __restrict__ pool, long long* __restrict__ pool_idx, int N, int d,
    int poolsize, int npow2, float log1mp, unsigned long long seed) {
  extern __shared__ char sh_raw[];
  long long* key = (long long*)sh_raw;        // npow2 (composite sort key)
  int* idx = (int*)(key + npow2);             // npow2
  float* gkey = (float*)(idx + npow2);        // npow2 (gumbel keys)
  __shared__ int unsorted[2];
  const int tid = threadIdx.x;
  tournament_order<TPB, false>(rank, key, idx, gkey, unsorted, N, npow2,
                               log1mp, seed);
  // stage 3: gather the pool rows
  for (int j = tid; j < poolsize; j += TPB) pool_idx[j] = idx[j];
  __syncthreads();
  for (long long t = tid; t < (long long)poolsize * d; t += TPB) {
    const int r = (int)(t / d), c = (int)(t % d);
    pool[t] = population[(long long)idx[r] * d + c];
  }
}

// Tournament and event-decoded variation in ONE launch: every workgroup works
// out the whole tournament order for itself (it is a few microseconds, and
// nothing has to pass between workgroups), keeps it in LDS, and its share of
// the events read their parents' rows from the population through it, so no
// pool is gathered. Same Philox counters and the same inlines as
// tournament_kernel + variation_events_kernel: the children are bitwise
// theirs.
template <int TPB>
__global__ __launch_bounds__(TPB) void spawn_fused_kernel(
    const float* __restrict__ population, const long long* __restrict__ rank,
    int N, int d, int npow2, float log1mp, unsigned long long seed_t,
    const long long* __restrict__ ci, const long long* __restrict__ mi,
    const long long* __restrict__ p1, const long long* __restrict__ p2,
    const long long* __restrict__ im, const float* __restrict__ di_c,
    const float* __restrict__ di_m, const float* __restrict__ lo,
    const float* __restrict__ hi, float* __restrict__ out, int C, int M,
    float mutation_rate, unsigned long long seed_sbx,
    unsigned long long seed_mut) {
  extern __shared__ char sh_raw[];
  long long* key = (long long*)sh_raw;
  int* idx = (int*)(key + npow2);
  float* gkey = (float*)(idx + npow2);
  __shared__ int unsorted[2];
  const int* pool_row = tournament_order<TPB, true>(
      rank, key, idx, gkey, unsorted, N, npow2, log1mp, seed_t);
  const int total = (C + M) * d;
  for (int t = blockIdx.x * TPB + threadIdx.x; t < total; t += gridDim.x * TPB)
    variation_event_gene<int>(population, pool_row, ci, mi, p1, p2, im, di_c, di_m,
                              lo, hi, out, t / d, t % d, C, d, mutation_rate,
                              seed_sbx, seed_mut);
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

// Same shape gate as launch_tournament (-1, launching nothing, beyond it).
extern "C" int launch_spawn_fused(
    const float* population, const long long* rank, int N, int d, int poolsize,
    float log1mp, unsigned long long seed_t, const long long* ci,
    const long long* mi, const long long* p1, const long long* p2,
    const long long* im, const float* di_c, const float* di_m, const float* lo,
    const float* hi, float* out, int C, int M, float mutation_rate,
    unsigned long long seed_sbx, unsigned long long seed_mut,
    hipStream_t stream) {
  int npow2 = 1;
  while (npow2 < N) npow2 <<= 1;
  if (npow2 > TOUR_NMAX || poolsize > N) return -1;
  const size_t lds = (size_t)npow2 * (8 + 4 + 4);
  // two genes a thread
  const long long total = (long long)(C + M) * d;
  const int tpb = npow2 > 512 ? 1024 : TOUR_TPB;
  const int blocks =
      (int)std::min<long long>(64, std::max<long long>(1, (total + 2 * tpb - 1) / (2 * tpb)));
  if (npow2 > 512)
    hipLaunchKernelGGL(spawn_fused_kernel<1024>, dim3(blocks), dim3(1024), lds,
                       stream, population, rank, N, d, npow2, log1mp, seed_t,
                       ci, mi, p1, p2, im, di_c, di_m, lo, hi, out, C, M,
                       mutation_rate, seed_sbx, seed_mut);
  else
    hipLaunchKernelGGL(spawn_fused_kernel<TOUR_TPB>, dim3(blocks), dim3(TOUR_TPB),
                       lds, stream, population, rank, N, d, npow2, log1mp,
                       seed_t, ci, mi, p1, p2, im, di_c, di_m, lo, hi, out, C,
                       M, mutation_rate, seed_sbx, seed_mut);
  return 0;
}

// ------------------------------------------------ fused survivor selection
// nsga2_select's whole chain (cat, dominator bits, peel, crowding, column
// sum, (rank, crowding, index) sort, gather, survivor count) in TWO launches:
// the dominator bits by the grid, everything else by one workgroup, every
// array its stages exchange in LDS. Row i < ng of
// the virtual concatenation is child i, the rest are the parents. Outputs
// are bitwise the chain's: dominance, ranks and the (key, idx) sort are exact
// and totally ordered, the crowding runs crowding_kernel's inline with the same
// npow2 and is summed over the objectives in the same fixed order. The peel
// stops at the front that straddles `keep` (rows beyond get a sentinel rank
// above every true one, as in coop_peel_bits_kernel): neither the kept rows
// nor their ranks and order depend on the ranks beyond.
#define SELF_TPB 512
#define SELF_CG 2  // objective columns sorted at once, 256 threads each

struct SelLds {  // byte offsets into the dynamic LDS block
  size_t keys, sidx, cvals, ys, db, fmask, ndom, rank, perdim, cross, ctrl, total;
};

static __host__ __device__ inline SelLds sel_lds(int N, int m, int ng,
                                                 int npow2) {
  const size_t W = (N + 31) / 32;
  SelLds L;
  size_t o = 0;
  L.keys = o;   o += (size_t)npow2 * 8;  // (key, row) of the final sort
  L.sidx = o;   o += (size_t)npow2 * 4;
  // (value, index) pairs of the crowding sorts, one set a thread group
  L.cvals = o;  o += (size_t)SELF_CG * npow2 * 8;
  L.ys = o;     o += (size_t)N * m * 4;
  L.db = o;     o += (size_t)N * W * 4;
  L.fmask = o;  o += W * 4;
  L.ndom = o;   o += (size_t)N * 4;
  L.rank = o;   o += (size_t)N * 4;
  L.perdim = o; o += (size_t)N * m * 4;
  L.cross = o;  o += (size_t)((ng + 31) / 32) * 4;
  L.ctrl = o;   o += 16;
  L.total = o;
  return L;
}

// Packed dominator bits of the virtual concatenation [y_gen; pop_obj], built
// GRID-wide (N^2 m compares are 25 us on the one CU of the selection kernel,
// a few us on the grid): dom_bits_kernel's predicate and layout, rows read
// where they are.
template <int M>
__global__ void dom_bits_pair_kernel(const float* __restrict__ y_gen,
                                     const float* __restrict__ pop_obj,
                                     unsigned int* __restrict__ Dbits, int ng,
                                     int N, int m, int W) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * W) return;
  const int j = idx / W, w = idx % W;
  const int mm = M > 0 ? M : m;
  const float* yj = (j < ng) ? y_gen + (size_t)j * mm
                             : pop_obj + (size_t)(j - ng) * mm;
  float cj[M > 0 ? M : 1];
  if (M > 0) {
#pragma unroll
    for (int t = 0; t < M; ++t) cj[t] = yj[t];
  }
  unsigned int bits = 0;
  const int i0 = w * 32;
  const int iend = min(32, N - i0);
  for (int b = 0; b < iend; ++b) {
    const int i = i0 + b;
    const float* yi = (i < ng) ? y_gen + (size_t)i * mm
                               : pop_obj + (size_t)(i - ng) * mm;
    bool le = true, lt = false;
    if (M > 0) {
#pragma unroll
      for (int t = 0; t < M; ++t) {
        const float a = yi[t];
        le &= (a <= cj[t]);
        lt |= (a < cj[t]);
      }
    } else {
      for (int t = 0; t < m; ++t) {
        const float a = yi[t], c = yj[t];
        le &= (a <= c);
        lt |= (a < c);
      }
    }
    if (le && lt && i != j) bits |= (1u << b);
  }
  Dbits[idx] = bits;
}

__global__ __launch_bounds__(SELF_TPB) void nsga2_select_fused_kernel(
    const float* __restrict__ x_gen, const float* __restrict__ y_gen,
    const float* __restrict__ pop_parm, const float* __restrict__ pop_obj,
    const unsigned int* __restrict__ Dbits, int ng, int np, int d, int m, int keep, int npow2,
    const long long* __restrict__ c_idx, int n_cross,
    float* __restrict__ parm_o, float* __restrict__ obj_o,
    long long* __restrict__ rank_o, long long* __restrict__ perm,
    long long* __restrict__ succ_cross, long long* __restrict__ succ_mut) {
  extern __shared__ char sh_raw[];
  const int N = ng + np, W = (N + 31) / 32;
  const SelLds L = sel_lds(N, m, ng, npow2);
  long long* keys = (long long*)(sh_raw + L.keys);
  int* sidx = (int*)(sh_raw + L.sidx);
  float* Ys = (float*)(sh_raw + L.ys);
  unsigned int* Db = (unsigned int*)(sh_raw + L.db);
  unsigned int* fmask = (unsigned int*)(sh_raw + L.fmask);
  int* n_dom = (int*)(sh_raw + L.ndom);
  int* rank = (int*)(sh_raw + L.rank);
  float* per_dim = (float*)(sh_raw + L.perdim);
  unsigned int* is_cross = (unsigned int*)(sh_raw + L.cross);
  int* ctrl = (int*)(sh_raw + L.ctrl);  // [front size, cross count, mut count]
  const int tid = threadIdx.x;

  for (int t = tid; t < N * m; t += SELF_TPB)
    Ys[t] = (t < ng * m) ? y_gen[t] : pop_obj[t - ng * m];
  for (int w = tid; w < (ng + 31) / 32; w += SELF_TPB) is_cross[w] = 0u;
  if (tid == 0) { ctrl[1] = 0; ctrl[2] = 0; }
  __syncthreads();

  // dominator bits of column j (dom_bits_pair_kernel) and their count
  for (int t = tid; t < N * W; t += SELF_TPB) Db[t] = Dbits[t];
  __syncthreads();
  for (int j = tid; j < N; j += SELF_TPB) {
    int cnt = 0;
    for (int w = 0; w < W; ++w) cnt += __popc(Db[j * W + w]);
    n_dom[j] = cnt;
    rank[j] = 0;
  }
  __syncthreads();

  // peel the fronts up to the one that straddles keep
  int ranked = 0;
  for (int k = 0; ranked < N && k <= N; ++k) {
    if (tid == 0) ctrl[0] = 0;
    for (int w = tid; w < W; w += SELF_TPB) fmask[w] = 0u;
    __syncthreads();
    for (int j = tid; j < N; j += SELF_TPB) {
      if (n_dom[j] == 0) {
        rank[j] = k;
        n_dom[j] = -1;
        atomicOr(&fmask[j >> 5], 1u << (j & 31));
        atomicAdd(&ctrl[0], 1);
      }
    }
    __syncthreads();
    const int fs = ctrl[0];
    if (fs == 0) break;
    ranked += fs;
    if (ranked >= keep) {  // fronts 0..k are complete
      for (int j = tid; j < N; j += SELF_TPB)
        if (n_dom[j] > 0) rank[j] = k + 1;  // sentinel > every true rank
      break;
    }
    for (int j = tid; j < N; j += SELF_TPB) {
      if (n_dom[j] <= 0) continue;
      int dec = 0;
#pragma unroll 4
      for (int w = 0; w < W; ++w) dec += __popc(Db[j * W + w] & fmask[w]);
      n_dom[j] -= dec;
    }
    __syncthreads();
  }
  __syncthreads();

  // crowding into per_dim (m, N): SELF_CG groups of threads, one objective
  // column each at a time
  {
    constexpr int GT = SELF_TPB / SELF_CG;
    const int grp = tid / GT, gtid = tid % GT;
    float* gv = (float*)(sh_raw + L.cvals) + (size_t)grp * 2 * npow2;
    int* gi = (int*)(gv + npow2);
    for (int o0 = 0; o0 < m; o0 += SELF_CG) {
      const int o = o0 + grp;
      const bool active = o < m;
      for (int i = gtid; active && i < npow2; i += GT) {
        gv[i] = (i < N) ? Ys[i * m + o] : INFINITY;
        gi[i] = i;
      }
      __syncthreads();
      crowding_sort_gaps(gv, gi, per_dim + (size_t)(active ? o : 0) * N, N,
                         npow2, gtid, GT, active);
      __syncthreads();
    }
  }

  // (rank, crowding, index) sort: rank_crowd_sort_kernel's key and order, the
  // column sum in colsum_kernel's order
  for (int i = tid; i < npow2; i += SELF_TPB) {
    if (i < N) {
      float acc = 0.f;
      for (int o = 0; o < m; ++o) acc += per_dim[(size_t)o * N + i];
      keys[i] = rank_crowd_key((long long)rank[i], acc);
      sidx[i] = i;
    } else {
      keys[i] = 0x7FFFFFFFFFFFFFFFLL;  // pads sort to the end
      sidx[i] = 0x7FFFFFFF;
    }
  }
  __syncthreads();
  key_idx_sort(keys, sidx, npow2, tid, SELF_TPB);

  // survivors: gather, and the operator-success counts of
  // survivor_count_kernel
  const int P = min(keep, N);
  for (int r = tid; r < P; r += SELF_TPB) {
    const int src = sidx[r];
    perm[r] = (long long)src;
    rank_o[r] = (long long)rank[src];
  }
  for (int t = tid; t < P * m; t += SELF_TPB)
    obj_o[t] = Ys[sidx[t / m] * m + t % m];
#pragma unroll 4
  for (int t = tid; t < P * d; t += SELF_TPB) {
    const int src = sidx[t / d], c = t % d;
    parm_o[t] = (src < ng) ? x_gen[(size_t)src * d + c]
                           : pop_parm[(size_t)(src - ng) * d + c];
  }
  if (succ_cross == nullptr) return;
  for (int i = tid; i < n_cross; i += SELF_TPB) {
    const int s = (int)c_idx[i];
    if (s >= 0 && s < ng) atomicOr(&is_cross[s >> 5], 1u << (s & 31));
  }
  __syncthreads();
  int lc = 0, lm = 0;
  for (int r = tid; r < P; r += SELF_TPB) {
    const int e = sidx[r];
    if (e < ng) {
      if (is_cross[e >> 5] & (1u << (e & 31))) ++lc;
      else ++lm;
    }
  }
  if (lc) atomicAdd(&ctrl[1], lc);
  if (lm) atomicAdd(&ctrl[2], lm);
  __syncthreads();
  if (tid == 0) {
    atomicAdd((unsigned long long*)succ_cross,
              (unsigned long long)(ctrl[1] / 2));
    atomicAdd((unsigned long long*)succ_mut, (unsigned long long)ctrl[2]);
  }
}

// Whether the fused selection takes ng children and np parents at m
// objectives: its LDS block within the 144 KB launch_peel_bits allows itself
// (N = 1003 at m = 2; the dominator bits are N^2 / 8 bytes of it).
extern "C" int nsga2_select_fused_fits(int ng, int np, int m) {
  const int N = ng + np;
  if (ng < 1 || np < 1 || m < 1 || N > 2048) return 0;
  int npow2 = 1;
  while (npow2 < N) npow2 <<= 1;
  return sel_lds(N, m, ng, npow2).total <= 144 * 1024 ? 1 : 0;
}

extern "C" int launch_nsga2_select_fused(
    const float* x_gen, const float* y_gen, const float* pop_parm,
    const float* pop_obj, int ng, int np, int d, int m, int keep,
    const long long* c_idx, int n_cross, unsigned int* dbits_scratch,
    float* parm_o, float* obj_o, long long* rank_o, long long* perm,
    long long* succ_cross, long long* succ_mut, hipStream_t stream) {
  if (!nsga2_select_fused_fits(ng, np, m)) return -1;
  const int N = ng + np;
  int npow2 = 1;
  while (npow2 < N) npow2 <<= 1;
  const size_t lds = sel_lds(N, m, ng, npow2).total;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)nsga2_select_fused_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              144 * 1024);
    attr_set = true;
  }
  const int W = (N + 31) / 32;
  const int blocks = (N * W + 255) / 256;
  if (m == 2)
    hipLaunchKernelGGL(dom_bits_pair_kernel<2>, dim3(blocks), dim3(256), 0,
                       stream, y_gen, pop_obj, dbits_scratch, ng, N, m, W);
  else if (m == 3)
    hipLaunchKernelGGL(dom_bits_pair_kernel<3>, dim3(blocks), dim3(256), 0,
                       stream, y_gen, pop_obj, dbits_scratch, ng, N, m, W);
  else
    hipLaunchKernelGGL(dom_bits_pair_kernel<0>, dim3(blocks), dim3(256), 0,
                       stream, y_gen, pop_obj, dbits_scratch, ng, N, m, W);
  hipLaunchKernelGGL(nsga2_select_fused_kernel, dim3(1), dim3(SELF_TPB), lds,
                     stream, x_gen, y_gen, pop_parm, pop_obj,
                     (const unsigned int*)dbits_scratch, ng, np, d, m, keep,
                     npow2, c_idx, n_cross, parm_o, obj_o, rank_o, perm,
                     succ_cross, succ_mut);
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
      keys[i] = rank_crowd_key((long long)rank[i], crowd[i]);
      idxs[i] = i;
    } else {
      keys[i] = 0x7FFFFFFFFFFFFFFFLL;  // pads sort to the end
      idxs[i] = 0x7FFFFFFF;
    }
  }
  __syncthreads();
  key_idx_sort(keys, idxs, M, tid, RCS_TPB);
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
