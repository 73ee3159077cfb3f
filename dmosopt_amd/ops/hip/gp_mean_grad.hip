// Gradient of the GP posterior mean with respect to the QUERY point.
//
// With u = (x - q_lb) * q_invrg the normalised query, s_d = (u_d - X_id)/ell_d
// the scaled direct difference, r2 = sum_d s_d^2 and g = dk/d(r2):
//   d mu_b / d x_d = y_std_b * q_invrg_d * (2/ell_bd)
//                    * sum_i alpha_bi * sf2_b * g(r2_bi) * s_d,bi
// which is the (2/ell^2) * sum w (u_d - X_id) of docs/surrogates.md with one
// factor 1/ell kept inside the sum: the slabs are staged 1/ell-scaled for r2
// anyway, and the same LDS words serve both places. The difference is formed
// directly in BOTH places — never u_d * sum(w) - sum(w X_id), which cancels
// next to a training point.
//
// Design (gfx950): one 256-thread block (4 waves) per 32 queries x 32
// training points and per objective b; grid = (query tiles, N tiles, B). Both
// 32-row slabs are staged in LDS as in matern_assemble_kernel (odd row stride
// D|1). Phase 1: thread t owns point j = t & 31 and queries (t >> 5) + 8r,
// r = 0..3, sums r2 over k in index order and leaves
// w = sf2 * g(r2) * alpha_j in a 32 x 33 LDS tile (stride 33: phase 2 reads a
// column of it across the lanes). Phase 2: thread t owns query q = t & 31 and
// the dimensions (t >> 5) + 8j, j < 16 (D <= 128), and walks the 32 points in
// index order with fmaf(w, s_d, acc): the q slab is held in registers, the w
// tile is read conflict-free and the x slab by broadcast.
//
// Determinism / batch invariance: there are NO atomics and no cross-lane
// reduction. Every (query, point) r2 and every (query, d) partial is the
// work of ONE thread adding in index order, so a query's numbers do not
// depend on its position in the tile, on its neighbours or on P. The
// partials go to part[b][s][p][d], one s per 32-point tile (a function of N
// alone); every element the finish kernel reads has been written, so the
// workspace needs no zeroing. The finish kernel adds the tiles in tile order
// (in double) and applies the scale. Rows past P are never written, points
// past N enter with w = 0 and a zero slab row.

#include "common.h"
#include "launchers.h"
#include <math.h>

#define MG_TILE 32
#define MG_TPB 256
#define MG_WS 33       // w tile row stride
#define MG_DMAX 128    // 16 dimensions per phase-2 thread

// g(d2) = dk/d(d2); nu encoding as in matern.hip
template <int NU>
__device__ __forceinline__ float matern_dk(float d2) {
  if (NU == 0) return -0.5f * __expf(-0.5f * d2);
  const float r = sqrtf(fmaxf(d2, 0.f));
  if (NU == 1)  // kink at r = 0: a point the query sits on contributes 0
    return (r > 0.f) ? -__expf(-r) / (2.f * r) : 0.f;
  if (NU == 3) return -1.5f * __expf(-1.7320508075688772f * r);
  const float s = 2.23606797749979f * r;
  return -(5.f / 6.f) * (1.f + s) * __expf(-s);
}

template <int NU, bool ANISO>
__global__ __launch_bounds__(MG_TPB) void gp_mean_grad_partial_kernel(
    const float* __restrict__ Xq,     // (P, D) queries
    const float* __restrict__ X,      // (N, D)
    const float* __restrict__ theta,  // (B, p)
    const float* __restrict__ alpha,  // (B, N)
    float* __restrict__ part,         // (B, S, P, D)
    int P, int N, int D, int p,
    const float* __restrict__ q_lb,     // optional per-dim affine
    const float* __restrict__ q_invrg)  // applied to Xq at load
{
  extern __shared__ float lds[];
  const int DS = D | 1;
  float* q_tile = lds;                     // [32][DS] queries
  float* x_tile = q_tile + MG_TILE * DS;   // [32][DS] training points
  float* w_tile = x_tile + MG_TILE * DS;   // [32][33] (query, point)
  float* a_j = w_tile + MG_TILE * MG_WS;   // [32]

  const int b = blockIdx.z;
  const int s_idx = blockIdx.y;
  const int S = gridDim.y;
  const int p0 = blockIdx.x * MG_TILE, n0 = s_idx * MG_TILE;
  const float* th = theta + (long long)b * p;
  const float sf2 = __expf(th[0]);

  for (int idx = threadIdx.x; idx < MG_TILE * D; idx += MG_TPB) {
    const int row = idx / D;
    const int col = idx % D;
    const float inv_ell = ANISO ? __expf(-th[1 + col]) : __expf(-th[1]);
    const int gq = p0 + row, gx = n0 + row;
    float qv = (gq < P) ? Xq[(long long)gq * D + col] : 0.f;
    if (q_lb != nullptr) qv = (qv - q_lb[col]) * q_invrg[col];
    q_tile[row * DS + col] = qv * inv_ell;
    x_tile[row * DS + col] =
        (gx < N) ? X[(long long)gx * D + col] * inv_ell : 0.f;
  }
  if (threadIdx.x < MG_TILE) {
    const int gx = n0 + threadIdx.x;
    a_j[threadIdx.x] = (gx < N) ? alpha[(long long)b * N + gx] : 0.f;
  }
  __syncthreads();

  const int ln = threadIdx.x & 31;
  const int lr = threadIdx.x >> 5;

  // phase 1: w for (query lr + 8r, point ln)
  {
    float d2[4] = {0.f, 0.f, 0.f, 0.f};
    const float* xb = x_tile + ln * DS;
    for (int k = 0; k < D; ++k) {
      const float xv = xb[k];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float t = q_tile[(lr + 8 * r) * DS + k] - xv;
        d2[r] = fmaf(t, t, d2[r]);
      }
    }
    const bool live = (n0 + ln) < N;
    const float sa = sf2 * a_j[ln];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      w_tile[(lr + 8 * r) * MG_WS + ln] =
          live ? sa * matern_dk<NU>(d2[r]) : 0.f;
  }
  __syncthreads();

  // phase 2: (query ln, dimensions lr + 8j)
  float qv[MG_DMAX / 8], acc[MG_DMAX / 8];
#pragma unroll
  for (int j = 0; j < MG_DMAX / 8; ++j) {
    const int d = lr + 8 * j;
    qv[j] = (d < D) ? q_tile[ln * DS + d] : 0.f;
    acc[j] = 0.f;
  }
  const float* wq = w_tile + ln * MG_WS;
  for (int i = 0; i < MG_TILE; ++i) {
    const float w = wq[i];
    const float* xr = x_tile + i * DS + lr;
#pragma unroll
    for (int j = 0; j < MG_DMAX / 8; ++j)
      if (8 * j < D - lr) acc[j] = fmaf(w, qv[j] - xr[8 * j], acc[j]);
  }
  const int gq = p0 + ln;
  if (gq < P) {
    float* out = part + (((long long)b * S + s_idx) * P + gq) * D;
#pragma unroll
    for (int j = 0; j < MG_DMAX / 8; ++j) {
      const int d = lr + 8 * j;
      if (d < D) out[d] = acc[j];
    }
  }
}

// jac[p][b][d] = y_std_b * q_invrg_d * (2/ell_bd) * sum_s part[b][s][p][d],
// the N tiles in index order, accumulated in double.
template <bool ANISO>
__global__ void gp_mean_grad_finish_kernel(
    const float* __restrict__ part, const float* __restrict__ theta,
    const float* __restrict__ y_std, const float* __restrict__ q_invrg,
    float* __restrict__ jac, int B, int P, int D, int p, int S) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)P * B * D) return;
  const int d = (int)(idx % D);
  const int b = (int)((idx / D) % B);
  const long long q = idx / ((long long)D * B);
  const long long stride = (long long)P * D;
  const float* src = part + ((long long)b * S * P + q) * D + d;
  double s = 0.0;
  for (int t = 0; t < S; ++t) s += (double)src[t * stride];
  const float* th = theta + (long long)b * p;
  float scale = 2.f * (ANISO ? __expf(-th[1 + d]) : __expf(-th[1])) * y_std[b];
  if (q_invrg != nullptr) scale *= q_invrg[d];
  jac[idx] = (float)s * scale;
}

// 32-point tiles of N: the number of partials per (b, query, d)
extern "C" int gp_mean_grad_splits(int N) {
  return (N + MG_TILE - 1) / MG_TILE;
}

// part: (B, gp_mean_grad_splits(N), P, D) floats of scratch; jac: (P, B, D).
// D <= 128. Returns 0 or the hipError_t of the failed launch.
extern "C" int launch_gp_mean_grad(const float* Xq, const float* X,
                                   const float* theta, const float* alpha,
                                   const float* y_std, float* part, float* jac,
                                   int B, int P, int N, int D, int p,
                                   int nu_code, int aniso, const float* q_lb,
                                   const float* q_invrg, hipStream_t stream) {
  if (D > MG_DMAX) return (int)hipErrorInvalidValue;
  const int S = gp_mean_grad_splits(N);
  dim3 grid((P + MG_TILE - 1) / MG_TILE, S, B);
  const size_t lds_bytes =
      (2 * MG_TILE * (D | 1) + MG_TILE * MG_WS + MG_TILE) * sizeof(float);
  #define DISPATCH(NU, AN)                                                  \
    hipLaunchKernelGGL((gp_mean_grad_partial_kernel<NU, AN>), grid,         \
                       dim3(MG_TPB), lds_bytes, stream, Xq, X, theta,       \
                       alpha, part, P, N, D, p, q_lb, q_invrg)
  #define DISPATCH_AN(NU)                                                   \
    if (aniso) DISPATCH(NU, true); else DISPATCH(NU, false)
  switch (nu_code) {
    case 0: DISPATCH_AN(0); break;
    case 1: DISPATCH_AN(1); break;
    case 3: DISPATCH_AN(3); break;
    default: DISPATCH_AN(5); break;
  }
  #undef DISPATCH_AN
  #undef DISPATCH
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  const long long n = (long long)P * B * D;
  const dim3 fgrid((unsigned)((n + 255) / 256));
  if (aniso)
    hipLaunchKernelGGL(gp_mean_grad_finish_kernel<true>, fgrid, dim3(256), 0,
                       stream, part, theta, y_std, q_invrg, jac, B, P, D, p, S);
  else
    hipLaunchKernelGGL(gp_mean_grad_finish_kernel<false>, fgrid, dim3(256), 0,
                       stream, part, theta, y_std, q_invrg, jac, B, P, D, p, S);
  return (int)hipGetLastError();
}
