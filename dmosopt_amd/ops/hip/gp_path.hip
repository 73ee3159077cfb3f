// Random-Fourier-feature term of a GP posterior sample path (decoupled
// pathwise sampling, Wilson et al. 2020):
//   f_b(u) = sum_{j<M} a_bj * cos(2 pi (tau_bj + sum_d Omega_bjd u_d)),
// u = (x - q_lb) * q_invrg the normalised query. The Matheron update
// k(u, X) alpha' is the posterior-mean launch with another weight vector; the
// finish kernel here adds y_std_b * f_b(u) into the block that launch wrote.
//
// The phase is counted in TURNS and summed in double: a heavy-tailed spectral
// draw (nu = 1/2, ell ~ 1e-3) gives 1e3..1e5 turns, of which only the
// fraction matters, and a float32 phase has no fraction left there. The
// fraction t - rint(t) lies in [-1/2, 1/2], is exact in double and goes to
// float for the cosine.
//
// Design (gfx950): one 256-thread block (4 waves) per 32 queries x PF_F = 64
// features and per batch row b; grid = (query tiles, feature chunks, B). The
// query slab [32][D|1] and the Omega chunk [64][D|1] are staged in LDS (odd
// row stride; 49.4 KiB at D = 128, inside the default 64 KiB). Thread t owns
// query q = t & 31 and the features (t >> 5) + 8r, r = 0..7: the lanes of a
// wave read 32 distinct query rows conflict-free and two Omega rows by
// broadcast.
//
// Determinism / batch invariance: no atomics, no memset. Every (query,
// feature) phase is ONE thread's index-ordered fma chain, tau first; a
// thread adds its 8 features in index order, then the 8 per-thread sums of a
// query are combined by one xor-32 shuffle and a 4-term LDS tree whose shape
// depends on PF_F alone. So a query's numbers do not depend on its position
// in the tile, on its neighbours or on P. Features past M are staged with
// Omega = tau = a = 0 and contribute exact zeros; rows past P are never
// written, and every partial the finish kernel reads has been written. The
// finish kernel adds the chunks in chunk order in double.

#include "common.h"
#include "launchers.h"
#include <math.h>

#define PF_TILE 32
#define PF_TPB 256
#define PF_F 64                      // features per block
#define PF_R (PF_F / (PF_TPB / 32))  // features per thread
#define PF_DMAX 128

__global__ __launch_bounds__(PF_TPB) void gp_path_partial_kernel(
    const float* __restrict__ Xq,     // (P, D) queries
    const float* __restrict__ Omega,  // (B, M, D) frequencies, turns per unit
    const float* __restrict__ tau,    // (B, M) phase offsets, turns
    const float* __restrict__ amp,    // (B, M)
    float* __restrict__ part,         // (B, S, P)
    int P, int M, int D,
    const float* __restrict__ q_lb,     // optional per-dim affine
    const float* __restrict__ q_invrg)  // applied to Xq at load
{
  extern __shared__ float lds[];
  const int DS = D | 1;
  float* q_tile = lds;                    // [32][DS] queries
  float* o_tile = q_tile + PF_TILE * DS;  // [PF_F][DS] frequencies
  float* t_j = o_tile + PF_F * DS;        // [PF_F]
  float* a_j = t_j + PF_F;                // [PF_F]
  float* red = a_j + PF_F;                // [4][32] per-wave sums

  const int b = blockIdx.z;
  const int s_idx = blockIdx.y;
  const int S = gridDim.y;
  const int p0 = blockIdx.x * PF_TILE, j0 = s_idx * PF_F;

  for (int idx = threadIdx.x; idx < PF_TILE * D; idx += PF_TPB) {
    const int row = idx / D;
    const int col = idx % D;
    const int gq = p0 + row;
    float qv = (gq < P) ? Xq[(long long)gq * D + col] : 0.f;
    if (q_lb != nullptr) qv = (qv - q_lb[col]) * q_invrg[col];
    q_tile[row * DS + col] = qv;
  }
  for (int idx = threadIdx.x; idx < PF_F * D; idx += PF_TPB) {
    const int row = idx / D;
    const int col = idx % D;
    const int gj = j0 + row;
    o_tile[row * DS + col] =
        (gj < M) ? Omega[((long long)b * M + gj) * D + col] : 0.f;
  }
  if (threadIdx.x < PF_F) {
    const int gj = j0 + threadIdx.x;
    const bool live = gj < M;
    t_j[threadIdx.x] = live ? tau[(long long)b * M + gj] : 0.f;
    a_j[threadIdx.x] = live ? amp[(long long)b * M + gj] : 0.f;
  }
  __syncthreads();

  const int ln = threadIdx.x & 31;
  const int lr = threadIdx.x >> 5;

  double t[PF_R];
#pragma unroll
  for (int r = 0; r < PF_R; ++r) t[r] = (double)t_j[lr + 8 * r];
  const float* qb = q_tile + ln * DS;
  for (int k = 0; k < D; ++k) {
    const double u = (double)qb[k];
#pragma unroll
    for (int r = 0; r < PF_R; ++r)
      t[r] = fma((double)o_tile[(lr + 8 * r) * DS + k], u, t[r]);
  }
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < PF_R; ++r) {
    const float fr = (float)(t[r] - rint(t[r]));
    acc = fmaf(a_j[lr + 8 * r], cosf(6.283185307179586f * fr), acc);
  }
  // lanes l and l ^ 32 hold the same query, feature groups 2w and 2w + 1
  acc += __shfl_xor(acc, 32, WAVE_SIZE);
  if ((threadIdx.x & 63) < 32) red[(threadIdx.x >> 6) * 32 + ln] = acc;
  __syncthreads();
  if (threadIdx.x < PF_TILE) {
    const int gq = p0 + threadIdx.x;
    if (gq < P)
      part[((long long)b * S + s_idx) * P + gq] =
          (red[threadIdx.x] + red[32 + threadIdx.x]) +
          (red[64 + threadIdx.x] + red[96 + threadIdx.x]);
  }
}

// out[p][b] += y_std_b * sum_s part[b][s][p], the chunks in index order,
// accumulated in double. out holds the posterior-mean launch's values.
__global__ void gp_path_finish_kernel(const float* __restrict__ part,
                                      const float* __restrict__ y_std,
                                      float* __restrict__ out, int B, int P,
                                      int S, int ldo) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)P * B) return;
  const int b = (int)(idx % B);
  const long long q = idx / B;
  const float* src = part + (long long)b * S * P + q;
  double s = 0.0;
  for (int t = 0; t < S; ++t) s += (double)src[(long long)t * P];
  out[q * ldo + b] += (float)s * y_std[b];
}

// PF_F-feature chunks of M: the number of partials per (b, query)
extern "C" int gp_path_splits(int M) { return (M + PF_F - 1) / PF_F; }

// part: (B, gp_path_splits(M), P) floats of scratch; out: P rows of stride
// ldo >= B whose first B columns are added into. D <= 128. Returns 0 or the
// hipError_t of the failed launch.
extern "C" int launch_gp_path(const float* Xq, const float* Omega,
                              const float* tau, const float* amp,
                              const float* y_std, float* part, float* out,
                              int B, int P, int M, int D, int ldo,
                              const float* q_lb, const float* q_invrg,
                              hipStream_t stream) {
  if (D > PF_DMAX || D < 1 || M < 1 || P < 1 || B < 1 || B > 65535)
    return (int)hipErrorInvalidValue;
  const int S = gp_path_splits(M);
  if (S > 65535) return (int)hipErrorInvalidValue;
  dim3 grid((P + PF_TILE - 1) / PF_TILE, S, B);
  const size_t lds_bytes =
      ((PF_TILE + PF_F) * (D | 1) + 2 * PF_F + 4 * 32) * sizeof(float);
  hipLaunchKernelGGL(gp_path_partial_kernel, grid, dim3(PF_TPB), lds_bytes,
                     stream, Xq, Omega, tau, amp, part, P, M, D, q_lb, q_invrg);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  const long long n = (long long)P * B;
  hipLaunchKernelGGL(gp_path_finish_kernel,
                     dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     part, y_std, out, B, P, S, ldo);
  return (int)hipGetLastError();
}
