// NSGA-III reference-direction survival (Deb & Jain 2014), stateless per call,
// in three launches after the Pareto peel and without a host sync:
//
//   nsga3_normalize_kernel  one workgroup: rank histogram + scan -> last front
//                           l, |P|, |S|, R; ideal over S; ASF extremes over the
//                           first front; the m x m intercept solve in double
//   nsga3_associate_kernel  grid-wide: perpendicular distance of every row of
//                           S to every unit direction, (d, h) argmin, niche
//                           counts of P by integer atomics
//   nsga3_niche_kernel      one workgroup: the closed form of the niching loop
//                           (docs/optimizers.md) as two LDS bitonic sorts, then
//                           perm and the gather of parm / obj / rank
//
// Every reduction whose result could depend on arrival order compares an index
// as well, and no float is ever accumulated by an atomic, so the outputs are
// repeatable and a row's (niche, dist) depends on that row, ideal, scale and Z
// alone. Non-finite objectives are out of scope (they stay memory-safe).

#include "launchers.h"
#include "moea_device.h"

#include <limits.h>

#define NSGA3_MAX_N 4096
#define NSGA3_MAX_H 2048
#define NSGA3_MAX_M 16

// ctrl words written by the normalise kernel
#define NSGA3_L 0   // last front admitted
#define NSGA3_NP 1  // |P| = #{rank < l}
#define NSGA3_NS 2  // |S| = #{rank <= l}
#define NSGA3_R 3   // picks from the last front

// Dynamic LDS of the niche kernel: (key, row) pairs of the npow2(N)-entry sorts,
// and per direction the first-candidate word and the segment start.
#define NSGA3_NICHE_TPB 1024
#define NSGA3_NICHE_SLOTS (NSGA3_MAX_N / NSGA3_NICHE_TPB)
#define NSGA3_LDS_LIMIT (144 * 1024)

static size_t nsga3_niche_lds(int N, int H) {
  size_t M = 1;
  while (M < (size_t)N) M <<= 1;
  return 12 * M + 12 * (size_t)H;
}

// The largest block asked for, at the edge of the gate, is 72 KB: above the
// 64 KB a launch gets by default, so the launcher raises the kernel's limit
// to what this function admits.
extern "C" int nsga3_select_fits(int N, int H, int m) {
  return N >= 1 && N <= NSGA3_MAX_N && H >= 1 && H <= NSGA3_MAX_H && m >= 1 &&
         m <= NSGA3_MAX_M && nsga3_niche_lds(N, H) <= NSGA3_LDS_LIMIT;
}

// ------------------------------------------------------------------ normalise
__global__ __launch_bounds__(1024) void nsga3_normalize_kernel(
    const float* __restrict__ Y, const long long* __restrict__ rank, int N,
    int m, int K, int H, float* __restrict__ ideal, float* __restrict__ scale,
    int* __restrict__ ctrl, int* __restrict__ rho) {
  __shared__ int cum[2][NSGA3_MAX_N];
  __shared__ int s_ctrl[4];
  __shared__ float s_z[NSGA3_MAX_M], s_fmax[NSGA3_MAX_M];
  __shared__ int s_ext[NSGA3_MAX_M];
  __shared__ double s_E[NSGA3_MAX_M][NSGA3_MAX_M + 1];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6;

  for (int i = tid; i < N; i += nt) cum[0][i] = 0;
  for (int h = tid; h < H; h += nt) rho[h] = 0;
  __syncthreads();
  for (int i = tid; i < N; i += nt) {
    const long long r = rank[i];
    if (r >= 0 && r < N) atomicAdd(&cum[0][(int)r], 1);
  }
  __syncthreads();
  // inclusive scan of the histogram (Hillis-Steele, two buffers)
  int src = 0;
  for (int off = 1; off < N; off <<= 1) {
    for (int i = tid; i < N; i += nt)
      cum[src ^ 1][i] = cum[src][i] + (i >= off ? cum[src][i - off] : 0);
    __syncthreads();
    src ^= 1;
  }
  for (int i = tid; i < N; i += nt) {
    const int before = i ? cum[src][i - 1] : 0;
    if (cum[src][i] >= K && before < K) {  // exactly one i: cum[N-1] = N >= K
      s_ctrl[NSGA3_L] = i;
      s_ctrl[NSGA3_NP] = before;
      s_ctrl[NSGA3_NS] = cum[src][i];
      s_ctrl[NSGA3_R] = K - before;
    }
  }
  __syncthreads();
  const int l = s_ctrl[NSGA3_L];

  // column min over S and column max over the first front: wave j, column j
  if (wave < m) {
    float mn = INFINITY, mx = -INFINITY;
    for (int i = lane; i < N; i += WAVE_SIZE) {
      const long long r = rank[i];
      const float v = Y[(long long)i * m + wave];
      if (r <= l) mn = fminf(mn, v);
      if (r == 0) mx = fmaxf(mx, v);
    }
    for (int off = 32; off > 0; off >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, off, WAVE_SIZE));
      mx = fmaxf(mx, __shfl_xor(mx, off, WAVE_SIZE));
    }
    if (lane == 0) {
      s_z[wave] = mn;
      s_fmax[wave] = mx - mn;  // = max over F0 of (Y - z): x - z is monotone
    }
  }
  __syncthreads();

  // ASF extreme of axis j over the first front: wave j, ties to the lowest row
  if (wave < m) {
    float bv = INFINITY;
    int bi = INT_MAX;
    for (int i = lane; i < N; i += WAVE_SIZE) {
      if (rank[i] != 0) continue;
      float v = -INFINITY;
      for (int k = 0; k < m; ++k) {
        const float t = Y[(long long)i * m + k] - s_z[k];
        v = fmaxf(v, k == wave ? t : t / 1e-6f);
      }
      if (v < bv || bi == INT_MAX) { bv = v; bi = i; }  // i ascends per lane
    }
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, WAVE_SIZE);
      const int oi = __shfl_xor(bi, off, WAVE_SIZE);
      if (oi != INT_MAX && (bi == INT_MAX || ov < bv || (ov == bv && oi < bi))) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) s_ext[wave] = bi;
  }
  __syncthreads();

  if (tid == 0) {
    bool ok = true;
    for (int a = 0; a < m && ok; ++a) {
      if (s_ext[a] < 0 || s_ext[a] >= N) ok = false;
      for (int b = 0; b < a && ok; ++b) ok = s_ext[a] != s_ext[b];
    }
    if (ok) {
      // E a = 1, E_jk = T[e_j][k]: Gaussian elimination, partial pivoting
      for (int j = 0; j < m; ++j) {
        for (int k = 0; k < m; ++k)
          s_E[j][k] = (double)(Y[(long long)s_ext[j] * m + k] - s_z[k]);
        s_E[j][m] = 1.0;
      }
      for (int c = 0; c < m && ok; ++c) {
        int p = c;
        for (int r = c + 1; r < m; ++r)
          if (fabs(s_E[r][c]) > fabs(s_E[p][c])) p = r;
        if (s_E[p][c] == 0.0) { ok = false; break; }
        if (p != c)
          for (int k = c; k <= m; ++k) {
            const double t = s_E[c][k]; s_E[c][k] = s_E[p][k]; s_E[p][k] = t;
          }
        for (int r = c + 1; r < m; ++r) {
          const double f = s_E[r][c] / s_E[c][c];
          for (int k = c; k <= m; ++k) s_E[r][k] -= f * s_E[c][k];
        }
      }
      if (ok) {
        for (int c = m - 1; c >= 0; --c) {
          double acc = s_E[c][m];
          for (int k = c + 1; k < m; ++k) acc -= s_E[c][k] * s_E[k][m];
          s_E[c][m] = acc / s_E[c][c];
        }
        for (int j = 0; j < m; ++j) {
          const double a = s_E[j][m];
          if (!(isfinite(a) && a > 0.0)) ok = false;
        }
      }
    }
    for (int j = 0; j < m; ++j) {
      float s = ok ? (float)(1.0 / s_E[j][m]) : s_fmax[j];
      if (!(s >= 1e-6f)) s = 1.f;
      scale[j] = s;
      ideal[j] = s_z[j];
    }
    for (int q = 0; q < 4; ++q) ctrl[q] = s_ctrl[q];
  }
}

// ------------------------------------------------------------------ associate
#define NSGA3_TILE 256   // directions staged per pass
#define NSGA3_LPR 16     // lanes per row

__global__ __launch_bounds__(256) void nsga3_associate_kernel(
    const float* __restrict__ Y, const long long* __restrict__ rank,
    const float* __restrict__ ideal, const float* __restrict__ scale,
    const int* __restrict__ ctrl, const float* __restrict__ Z, int N, int H,
    int m, long long* __restrict__ niche, float* __restrict__ dist,
    int* __restrict__ rho) {
  // zt[k][h]: component k of unit direction h of the tile; lanes of a row read
  // consecutive h, so the reads are conflict-free
  __shared__ float zt[NSGA3_MAX_M][NSGA3_TILE];
  const int tid = threadIdx.x;
  const int sub = tid & (NSGA3_LPR - 1);
  const int row = blockIdx.x * (256 / NSGA3_LPR) + tid / NSGA3_LPR;
  const int l = ctrl[NSGA3_L];
  const long long r = row < N ? rank[row] : (long long)INT_MAX;
  const bool act = r <= l;

  float yp[NSGA3_MAX_M];
#pragma unroll
  for (int k = 0; k < NSGA3_MAX_M; ++k)
    yp[k] = (act && k < m) ? (Y[(long long)row * m + k] - ideal[k]) / scale[k]
                           : 0.f;

  float bd = INFINITY;
  int bh = INT_MAX;
  for (int h0 = 0; h0 < H; h0 += NSGA3_TILE) {
    __syncthreads();
    if (h0 + tid < H) {
      const float* z = Z + (long long)(h0 + tid) * m;
      float s = 0.f;
      for (int k = 0; k < m; ++k) s = fmaf(z[k], z[k], s);
      const float nrm = sqrtf(s);
      for (int k = 0; k < m; ++k) zt[k][tid] = z[k] / nrm;
    }
    __syncthreads();
    const int nh = min(NSGA3_TILE, H - h0);
    if (act) {
      for (int hh = sub; hh < nh; hh += NSGA3_LPR) {
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < NSGA3_MAX_M; ++k)
          if (k < m) dot = fmaf(yp[k], zt[k][hh], dot);
        float d2 = 0.f;
#pragma unroll
        for (int k = 0; k < NSGA3_MAX_M; ++k)
          if (k < m) {
            const float e = fmaf(-dot, zt[k][hh], yp[k]);  // the residual itself
            d2 = fmaf(e, e, d2);
          }
        const float d = sqrtf(d2);
        if (d < bd) { bd = d; bh = h0 + hh; }  // h ascends per lane
      }
    }
  }
  // (d, h) lexicographic min over the row's lanes
  for (int off = NSGA3_LPR / 2; off > 0; off >>= 1) {
    const float od = __shfl_xor(bd, off, WAVE_SIZE);
    const int oh = __shfl_xor(bh, off, WAVE_SIZE);
    if (od < bd || (od == bd && oh < bh)) { bd = od; bh = oh; }
  }
  if (sub == 0 && row < N) {
    if (act) {
      if (bh >= H) bh = 0;  // only with non-finite input: stay in bounds
      niche[row] = bh;
      dist[row] = bd;
      if (r < l) atomicAdd(&rho[bh], 1);
    } else {
      niche[row] = -1;
      dist[row] = INFINITY;
    }
  }
}

// ---------------------------------------------------------------------- niche
__global__ __launch_bounds__(NSGA3_NICHE_TPB) void nsga3_niche_kernel(
    const float* __restrict__ x_gen, const float* __restrict__ pop_parm,
    const float* __restrict__ Y, const long long* __restrict__ rank,
    const long long* __restrict__ niche, const float* __restrict__ dist,
    const int* __restrict__ ctrl, const int* __restrict__ rho,
    const long long* __restrict__ dir_prio,
    const long long* __restrict__ row_prio, int ng, int np, int d, int m, int H,
    int K, float* __restrict__ parm_o, float* __restrict__ obj_o,
    long long* __restrict__ rank_o, long long* __restrict__ perm) {
  extern __shared__ long long nsga3_lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int N = ng + np;
  int M = 1;
  while (M < N) M <<= 1;
  long long* keys = nsga3_lds;                                    // M
  unsigned long long* first = (unsigned long long*)(keys + M);    // H
  int* idxs = (int*)(first + H);                                  // M
  int* start = idxs + M;                                          // H
  const int l = ctrl[NSGA3_L];

  for (int h = tid; h < H; h += nt) {
    first[h] = ~0ull;
    start[h] = 0;
  }
  __syncthreads();
  // (d, i)-minimal candidate of every direction: d >= 0, so its bits ascend
  for (int i = tid; i < N; i += nt)
    if (rank[i] == l)
      atomicMin(&first[niche[i]],
                ((unsigned long long)__float_as_uint(dist[i]) << 32) |
                    (unsigned int)i);
  __syncthreads();
  // list order of the candidates: (direction, not-first, row_prio)
  for (int i = tid; i < M; i += nt) {
    long long key = LLONG_MAX;
    if (i < N && rank[i] == l) {
      const int h = (int)niche[i];
      const bool is_first = rho[h] == 0 && (unsigned int)first[h] == (unsigned int)i;
      key = ((long long)h << 32) | (is_first ? 0ll : 1ll << 31) | row_prio[i];
    }
    keys[i] = key;
    idxs[i] = i;
  }
  __syncthreads();
  key_idx_sort(keys, idxs, M, tid, nt);
  for (int p = tid; p < M; p += nt)
    if (keys[p] != LLONG_MAX) {
      const int h = (int)(keys[p] >> 32);
      if (p == 0 || (int)(keys[p - 1] >> 32) != h) start[h] = p;
    }
  __syncthreads();
  // selection keys: P in (rank, index) order, then candidate t of direction h
  // at (rho_h + t) H + dir_prio[h]; staged in registers, M / nt slots a thread
  long long nk[NSGA3_NICHE_SLOTS];
  int ni[NSGA3_NICHE_SLOTS];
#pragma unroll
  for (int q = 0; q < NSGA3_NICHE_SLOTS; ++q) {
    const int p = tid + q * nt;
    nk[q] = LLONG_MAX;
    ni[q] = p;
    if (p < M) {
      const int i = idxs[p];
      ni[q] = i;
      if (keys[p] != LLONG_MAX) {
        const int h = (int)(keys[p] >> 32);
        nk[q] = (1ll << 40) + (long long)(rho[h] + p - start[h]) * H + dir_prio[h];
      } else if (i < N && rank[i] < l) {
        nk[q] = rank[i] * N + i;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NSGA3_NICHE_SLOTS; ++q) {
    const int p = tid + q * nt;
    if (p < M) { keys[p] = nk[q]; idxs[p] = ni[q]; }
  }
  __syncthreads();
  key_idx_sort(keys, idxs, M, tid, nt);

  for (int p = tid; p < K; p += nt) {
    const int i = idxs[p];
    perm[p] = i;
    rank_o[p] = rank[i];
  }
  for (int e = tid; e < K * d; e += nt) {
    const int i = idxs[e / d], c = e % d;
    parm_o[e] = i < ng ? x_gen[(long long)i * d + c]
                       : pop_parm[(long long)(i - ng) * d + c];
  }
  for (int e = tid; e < K * m; e += nt)
    obj_o[e] = Y[(long long)idxs[e / m] * m + e % m];
}

extern "C" int launch_nsga3_select(
    const float* x_gen, const float* pop_parm, const float* Y,
    const long long* rank, const float* Z, const long long* dir_prio,
    const long long* row_prio, int ng, int np, int d, int m, int H, int K,
    int* ctrl, int* rho, float* ideal, float* scale, long long* niche,
    float* dist, float* parm_o, float* obj_o, long long* rank_o,
    long long* perm, hipStream_t stream) {
  const int N = ng + np;
  if (!nsga3_select_fits(N, H, m) || K < 1 || K > N || d < 1) return -1;
  hipLaunchKernelGGL(nsga3_normalize_kernel, dim3(1), dim3(1024), 0, stream, Y,
                     rank, N, m, K, H, ideal, scale, ctrl, rho);
  hipLaunchKernelGGL(nsga3_associate_kernel,
                     dim3((N + 256 / NSGA3_LPR - 1) / (256 / NSGA3_LPR)),
                     dim3(256), 0, stream, Y, rank, ideal, scale, ctrl, Z, N, H,
                     m, niche, dist, rho);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)nsga3_niche_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              NSGA3_LDS_LIMIT);
    attr_set = true;
  }
  hipLaunchKernelGGL(nsga3_niche_kernel, dim3(1), dim3(NSGA3_NICHE_TPB),
                     nsga3_niche_lds(N, H), stream, x_gen,
                     pop_parm, Y, rank, niche, dist, ctrl, rho, dir_prio,
                     row_prio, ng, np, d, m, H, K, parm_o, obj_o, rank_o, perm);
  return 0;
}
