// Pareto ranking (Dominance Degree Matrix) and crowding distance.
//
// Replaces reference dda.py:25-120 and indicators.py:12-51.
//
// pareto_rank design (two size regimes, dispatched in bindings.cpp, which
// cover every N between them):
//   N <= 1024: bit-matrix path — dom_bits_kernel packs "i dominates j"
//     grid-wide into 32 bits/word, then peel_bits_kernel peels all fronts
//     in one small block with popcount(dom_mask & front_mask);
//   N > 1024: the same bit matrix kept in global memory and peeled by a
//     cooperative grid (coop_peel_bits_kernel), grid.sync() per front.
// dominance_matrix_kernel serves the dominance_degree_matrix op alone
// (reference dda.py:25-31); no ranking route reads the matrix.
//
// crowding design: one workgroup per objective dimension; (value, index)
// pairs bitonic-sorted in LDS (column min/max read off the sorted ends);
// per-dim gap rows are written WITHOUT atomics and summed in fixed order
// so results are bit-identical across replicated ranks.

#include "common.h"
#include "launchers.h"
#include "moea_device.h"
#include <math.h>

#define PTILE 32
#define PTPB 256

// D[i][j] = number of objectives with Y[i][k] <= Y[j][k], tile-wise with
// 32-row objective slabs in LDS. Identical rows keep their mutual m (and the
// diagonal its m), as in the reference: excluding them is a step of the
// ranking, not part of this matrix.
__global__ void dominance_matrix_kernel(const float* __restrict__ Y,  // (N, m)
                                        int* __restrict__ D,          // (N, N)
                                        int N, int m) {
  extern __shared__ float lds[];  // [2][PTILE][m]
  float* yi = lds;                // rows i (tile_y)
  float* yj = lds + PTILE * m;    // rows j (tile_x)
  const int ti = blockIdx.y * PTILE;
  const int tj = blockIdx.x * PTILE;
  for (int idx = threadIdx.x; idx < PTILE * m; idx += PTPB) {
    const int r = idx / m, c = idx % m;
    yi[idx] = (ti + r < N) ? Y[(ti + r) * m + c] : 0.f;
    yj[idx] = (tj + r < N) ? Y[(tj + r) * m + c] : 0.f;
  }
  __syncthreads();
  const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
#pragma unroll
  for (int sy = 0; sy < 2; ++sy)
#pragma unroll
    for (int sx = 0; sx < 2; ++sx) {
      const int li = ty * 2 + sy, lj = tx * 2 + sx;
      const int gi = ti + li, gj = tj + lj;
      if (gi >= N || gj >= N) continue;
      int cnt = 0;
      for (int k = 0; k < m; ++k)
        cnt += (yi[li * m + k] <= yj[lj * m + k]) ? 1 : 0;
      D[(long long)gi * N + gj] = cnt;
    }
}

extern "C" void launch_dominance_matrix(const float* Y, int* D, int N, int m,
                                        hipStream_t stream) {
  dim3 grid((N + PTILE - 1) / PTILE, (N + PTILE - 1) / PTILE);
  size_t lds_bytes = 2 * PTILE * m * sizeof(float);
  hipLaunchKernelGGL(dominance_matrix_kernel, grid, dim3(PTPB), lds_bytes,
                     stream, Y, D, N, m);
}

// ---------------------------------------------------------------------------
// Bit-matrix ranking: dominators of column j packed 32/word, built GRID-WIDE
// (the count pass was the single-CU bottleneck of the one-launch peel), then
// a single small block peels fronts with popcount(dom_mask & front_mask) —
// each round costs ~N/TPB * N/32 word-ops instead of N^2/TPB pair compares.
// M > 0: compile-time objective count (fully unrolled compare, row j
// cached in registers instead of re-read from L2 for every word); M == 0:
// generic runtime-m fallback.
template <int M>
__global__ void dom_bits_kernel(const float* __restrict__ Y,
                                unsigned int* __restrict__ Dbits,  // (N, W)
                                int N, int m, int W) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)N * W) return;
  const int j = (int)(idx / W), w = (int)(idx % W);
  unsigned int bits = 0;
  const int i0 = w * 32;
  const int iend = min(32, N - i0);
  if (M > 0) {
    float cj[M > 0 ? M : 1];
#pragma unroll
    for (int t = 0; t < M; ++t) cj[t] = Y[j * M + t];
    for (int b = 0; b < iend; ++b) {
      const int i = i0 + b;
      bool le = true, lt = false;
#pragma unroll
      for (int t = 0; t < M; ++t) {
        const float a = Y[i * M + t];
        le &= (a <= cj[t]);
        lt |= (a < cj[t]);
      }
      if (le && lt && i != j) bits |= (1u << b);
    }
  } else {
    for (int b = 0; b < iend; ++b) {
      const int i = i0 + b;
      if (i == j) continue;
      bool le = true, lt = false;
      for (int t = 0; t < m; ++t) {
        const float a = Y[i * m + t], c = Y[j * m + t];
        le &= (a <= c);
        lt |= (a < c);
      }
      if (le && lt) bits |= (1u << b);
    }
  }
  Dbits[idx] = bits;
}

#define PEELB_TPB 256

__global__ __launch_bounds__(PEELB_TPB) void peel_bits_kernel(
    const unsigned int* __restrict__ Dbits, int* __restrict__ rank, int N,
    int W) {
  extern __shared__ char sh_raw[];
  unsigned int* Db = (unsigned int*)sh_raw;      // N * W
  unsigned int* fmask = Db + (size_t)N * W;      // W
  int* n_dom = (int*)(fmask + W);                // N
  int* ctrl = n_dom + N;                         // [front_sz, remaining]
  const int tid = threadIdx.x;

  for (int i = tid; i < N * W; i += PEELB_TPB) Db[i] = Dbits[i];
  if (tid == 0) ctrl[1] = N;
  __syncthreads();
  for (int j = tid; j < N; j += PEELB_TPB) {
    int c = 0;
    for (int w = 0; w < W; ++w) c += __popc(Db[j * W + w]);
    n_dom[j] = c;
  }
  __syncthreads();

  for (int k = 0; ctrl[1] > 0 && k <= N; ++k) {
    if (tid == 0) ctrl[0] = 0;
    for (int w = tid; w < W; w += PEELB_TPB) fmask[w] = 0u;
    __syncthreads();
    for (int j = tid; j < N; j += PEELB_TPB) {
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
    for (int j = tid; j < N; j += PEELB_TPB) {
      if (n_dom[j] <= 0) continue;
      int dec = 0;
      for (int w = 0; w < W; ++w) dec += __popc(Db[j * W + w] & fmask[w]);
      n_dom[j] -= dec;
    }
    __syncthreads();
    if (tid == 0) ctrl[1] -= fs;
    __syncthreads();
  }
}

#define LAUNCH_DOM_BITS(blocks_, stream_, Y_, D_, N_, m_, W_)                  do {                                                                           if (m_ == 2)                                                                   hipLaunchKernelGGL(dom_bits_kernel<2>, dim3(blocks_), dim3(256), 0,                               stream_, Y_, D_, N_, m_, W_);                          else if (m_ == 3)                                                              hipLaunchKernelGGL(dom_bits_kernel<3>, dim3(blocks_), dim3(256), 0,                               stream_, Y_, D_, N_, m_, W_);                          else if (m_ == 5)                                                              hipLaunchKernelGGL(dom_bits_kernel<5>, dim3(blocks_), dim3(256), 0,                               stream_, Y_, D_, N_, m_, W_);                          else                                                                           hipLaunchKernelGGL(dom_bits_kernel<0>, dim3(blocks_), dim3(256), 0,                               stream_, Y_, D_, N_, m_, W_);                        } while (0)

extern "C" int launch_peel_bits(const float* Y, unsigned int* Dbits_scratch,
                                int* rank, int N, int m, hipStream_t stream) {
  const int W = (N + 31) / 32;
  const size_t lds = ((size_t)N * W + W) * sizeof(unsigned int) +
                     (N + 2) * sizeof(int);
  if (lds > 144 * 1024) return -1;
  static bool attr_set = false;
  if (!attr_set) {
    hipFuncSetAttribute((const void*)peel_bits_kernel,
                        hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
    attr_set = true;
  }
  const long long total = (long long)N * W;
  LAUNCH_DOM_BITS(((int)((total + 255) / 256)), stream, Y, Dbits_scratch, N,
                  m, W);
  hipLaunchKernelGGL(peel_bits_kernel, dim3(1), dim3(PEELB_TPB), lds, stream,
                     Dbits_scratch, rank, N, W);
  return 0;
}

// ---------------------------------------------------- cooperative peel
// Grid-wide SYNC-FREE-FROM-HOST ranking for N beyond the one-workgroup
// kernels' capacity (and their one-CU serialization): the packed dominator
// bit-matrix lives in GLOBAL memory (L2-resident: N=8192 -> 8 MB), every
// CU participates, and the front-peel loop synchronizes with grid.sync()
// instead of host readbacks (a readback per batch of fronts stalls
// pipelined generation loops — NOTES.md).
#include <hip/hip_cooperative_groups.h>

__global__ __launch_bounds__(256) void coop_peel_bits_kernel(
    const unsigned int* __restrict__ Dbits,  // (N, W) i-dominates-j bits
    unsigned int* __restrict__ fmask,        // (3*W,) triple-buffered scratch
    int* __restrict__ n_dom,                 // (N,) scratch
    int* __restrict__ ctrl,                  // (2,) scratch (only [0] used)
    int* __restrict__ rank,                  // (N,) out
    int N, int W, int stop) {
  // ONE grid.sync per front round (the peel is grid-barrier-latency bound):
  // the detect step is fused into the update step — when a point's
  // dominator count hits zero it immediately stamps its rank and flags
  // itself in the NEXT round's front mask. The mask is TRIPLE-buffered:
  // round k reads buf[k%3], writes buf[(k+1)%3], and clears buf[(k+2)%3]
  // (== the buffer round k-1 read, dead since the last barrier), so no
  // round ever waits on a separate clear phase.
  //
  // stop: peel until >= stop points are ranked, then stamp the remaining
  // alive points with a SENTINEL rank (last completed front + 1) and exit.
  // Exact for truncation selection (nsga2_select): the straddling front is
  // always completed before stopping, so every point that can enter the
  // kept top-`stop` carries its true rank; points beyond are discarded by
  // the caller and only need a rank larger than any kept one. stop >= N
  // peels everything (the public pareto_rank default).
  cooperative_groups::grid_group grid = cooperative_groups::this_grid();
  const int gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const int gsize = gridDim.x * blockDim.x;

  for (int j = gtid; j < N; j += gsize) {
    int c = 0;
    const unsigned int* row = Dbits + (size_t)j * W;
    for (int w = 0; w < W; ++w) c += __popc(row[w]);
    n_dom[j] = c;
    rank[j] = 0;
  }
  for (int w = gtid; w < 3 * W; w += gsize) fmask[w] = 0u;
  if (gtid == 0) ctrl[0] = 0;
  grid.sync();
  // front 0 into buffer 0
  for (int j = gtid; j < N; j += gsize) {
    if (n_dom[j] == 0) {
      n_dom[j] = -1;
      atomicOr(&fmask[j >> 5], 1u << (j & 31));
      atomicAdd(&ctrl[0], 1);
    }
  }
  grid.sync();

  int prev = -1;
  for (int k = 0; k < N; ++k) {
    const int total = ctrl[0];  // uniform: all writes pre-barrier
    if (total >= N || total == prev) break;
    if (total >= stop) {  // fronts 0..k are complete
      for (int j = gtid; j < N; j += gsize)
        if (n_dom[j] >= 0) rank[j] = k + 1;  // sentinel > every true rank
      break;
    }
    prev = total;
    const unsigned int* rd = fmask + (size_t)(k % 3) * W;
    unsigned int* wr = fmask + (size_t)((k + 1) % 3) * W;
    unsigned int* cl = fmask + (size_t)((k + 2) % 3) * W;
    for (int w = gtid; w < W; w += gsize) cl[w] = 0u;
    for (int j = gtid; j < N; j += gsize) {
      if (n_dom[j] <= 0) continue;
      int dec = 0;
      const unsigned int* row = Dbits + (size_t)j * W;
      for (int w = 0; w < W; ++w) dec += __popc(row[w] & rd[w]);
      if (dec) {
        const int nd = n_dom[j] - dec;
        if (nd == 0) {
          rank[j] = k + 1;
          n_dom[j] = -1;
          atomicOr(&wr[j >> 5], 1u << (j & 31));
          atomicAdd(&ctrl[0], 1);
        } else {
          n_dom[j] = nd;
        }
      }
    }
    grid.sync();
  }
}

extern "C" int launch_coop_peel(const float* Y, unsigned int* Dbits,
                                unsigned int* fmask, int* n_dom, int* ctrl,
                                int* rank, int N, int m, int stop,
                                hipStream_t stream) {
  const int W = (N + 31) / 32;
  if (stop <= 0 || stop > N) stop = N;
  static int coop_ok = -1;
  if (coop_ok < 0) {
    int dev = 0, attr = 0;
    hipGetDevice(&dev);
    hipDeviceGetAttribute(&attr, hipDeviceAttributeCooperativeLaunch, dev);
    coop_ok = attr ? 1 : 0;
  }
  if (!coop_ok) return -1;
  static int max_blocks = -1;
  if (max_blocks < 0) {
    int per_cu = 0;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, (const void*)coop_peel_bits_kernel, 256, 0);
    hipDeviceProp_t prop;
    int dev = 0;
    hipGetDevice(&dev);
    hipGetDeviceProperties(&prop, dev);
    max_blocks = per_cu * prop.multiProcessorCount;
    if (max_blocks < 1) max_blocks = 1;
  }
  const long long total = (long long)N * W;
  LAUNCH_DOM_BITS(((int)((total + 255) / 256)), stream, Y, Dbits, N, m, W);
  int blocks = (N + 255) / 256;
  if (blocks > max_blocks) blocks = max_blocks;
  void* args[] = {(void*)&Dbits, (void*)&fmask, (void*)&n_dom,
                  (void*)&ctrl, (void*)&rank, (void*)&N, (void*)&W,
                  (void*)&stop};
  const hipError_t err = hipLaunchCooperativeKernel(
      (const void*)coop_peel_bits_kernel, dim3(blocks), dim3(256),
      args, 0, stream);
  return err == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------- crowding
// One workgroup per objective dimension. Bitonic sort of (normalized value,
// index) in LDS; N padded to the next power of two with +inf sentinels.
#define CROWD_TPB 256

template <int TPB>
__global__ __launch_bounds__(TPB) void crowding_kernel(
    const float* __restrict__ Y,  // (N, m)
    float* __restrict__ out,      // (m, N)
    int N, int m, int npow2) {
  extern __shared__ float sh[];
  float* vals = sh;                       // npow2
  int* idxs = (int*)(sh + npow2);         // npow2
  const int j = blockIdx.x;               // objective dim

  // RAW column values: sorting is affine-invariant, and after the sort the
  // column min/max are vals[0]/vals[N-1] — the former host-side min/max/
  // span prep (~6 torch launches per call) is free here.
  for (int i = threadIdx.x; i < npow2; i += TPB) {
    vals[i] = (i < N) ? Y[i * m + j] : INFINITY;
    idxs[i] = i;
  }
  __syncthreads();

  // sort and gaps: the inline nsga2_select_fused_kernel runs too. Each dim
  // writes its own row of out (m, N) — NO atomics, so the sum order is
  // fixed and results are bit-identical across replicated ranks (float
  // atomicAdd order would not be).
  crowding_sort_gaps(vals, idxs, out + (long long)j * N, N, npow2,
                     threadIdx.x, TPB);
}

// out must be an (m, N) buffer; the host sums over dim 0 deterministically.
extern "C" void launch_crowding(const float* Y, float* out, int N, int m,
                                hipStream_t stream) {
  int npow2 = 1;
  while (npow2 < N) npow2 <<= 1;
  size_t lds_bytes = npow2 * (sizeof(float) + sizeof(int));
  // wide blocks for big sorts: at npow2=4096 a 256-thread block walks 16
  // elements per bitonic pass; 1024 threads walk 4 (measured 208 us ->
  // see profiles/README). Small sorts keep 256 (idle waves only add
  // barrier latency).
  if (npow2 > 512)
    hipLaunchKernelGGL(crowding_kernel<1024>, dim3(m), dim3(1024), lds_bytes,
                       stream, Y, out, N, m, npow2);
  else
    hipLaunchKernelGGL(crowding_kernel<CROWD_TPB>, dim3(m), dim3(CROWD_TPB),
                       lds_bytes, stream, Y, out, N, m, npow2);
}
