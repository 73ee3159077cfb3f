// Analytic gradient of the batched GP negative log marginal likelihood.
//
// theta = [log sf2, log ell (1 or D), log noise], K = sf2 C + (noise+jitter) I,
// alpha = K^-1 y, W = K^-1 - alpha alpha^T. With d2_ij the squared scaled
// distance, u_k,ij = ((x_ik - x_jk)/ell_k)^2 and g = -dc/d(d2):
//   d/d log sf2   = 1/2 sf2   sum_ij W_ij c_ij
//   d/d log noise = 1/2 noise sum_i  W_ii          (jitter is no parameter)
//   d/d log ell_k =     sf2   sum_ij W_ij g_ij u_k,ij   (isotropic: u -> d2)
// The caller supplies K^-1 (B,N,N) and alpha (B,N) from the Cholesky chain.
//
// Design (gfx950): one 256-thread block (4 waves) per 32x32 tile of the
// LOWER triangle of tile pairs (ti >= tj) and per candidate b; an
// off-diagonal tile stands for its mirror image too and counts twice (W, c,
// g and u are symmetric in i, j). Both 1/ell-scaled 32-row slabs are staged
// in LDS as in matern_assemble_kernel (odd row stride D|1), d2 is the
// direct-difference sum — never the norms+GEMM form, whose ~1e-7
// cancellation is all error next to the nu = 1/2 kink. Thread t owns column
// j = t & 31 and rows (t >> 5) + 8r, r = 0..3: a wave reads two 128-byte row
// segments of K^-1 per r, the x slab is read conflict-free (odd stride) and
// the q slab by broadcast.
//
// ARD keeps NO per-dimension accumulator in registers (D goes to 128): phase
// 1 leaves h_ij = weight * W_ij * g_ij for the whole tile in LDS, phase 2
// gives dimension k to wave k & 3, whose 64 lanes each add 16 pairs of
// h_ij (q_ik - x_jk)^2 from the slabs still resident in LDS and combine by
// xor shuffles.
//
// Determinism / batch invariance: there are NO atomics. Lanes add in
// register order, waves by fixed xor shuffles, the 4 waves in index order
// through LDS; every block writes all p entries of its row of
// part[b][tile][:], so the workspace needs no zeroing, and the finish kernel
// adds the tiles in tile order (in double). Nothing a candidate reads or
// writes depends on B.

#include "common.h"
#include "launchers.h"
#include <math.h>

#define GG_TILE 32
#define GG_TPB 256

// c(d2) and g(d2) = -dc/d(d2); nu encoding as in matern.hip
template <int NU>
__device__ __forceinline__ void matern_c_g(float d2, float* c, float* g) {
  if (NU == 0) {
    const float e = __expf(-0.5f * d2);
    *c = e;
    *g = 0.5f * e;
    return;
  }
  const float r = sqrtf(fmaxf(d2, 0.f));
  if (NU == 1) {
    const float e = __expf(-r);
    *c = e;
    *g = (r > 0.f) ? e / (2.f * r) : 0.f;  // u = 0 wherever r = 0
    return;
  }
  if (NU == 3) {
    const float s = 1.7320508075688772f * r;
    const float e = __expf(-s);
    *c = (1.f + s) * e;
    *g = 1.5f * e;
    return;
  }
  const float s = 2.23606797749979f * r;
  const float e = __expf(-s);
  *c = (1.f + s + (5.f / 3.f) * d2) * e;
  *g = (5.f / 6.f) * (1.f + s) * e;
}

template <int NU, bool ANISO>
__global__ __launch_bounds__(GG_TPB) void gp_nmll_grad_partial_kernel(
    const float* __restrict__ X,      // (N, D)
    const float* __restrict__ theta,  // (B, p)
    const float* __restrict__ Kinv,   // (B, N, N)
    const float* __restrict__ alpha,  // (B, N)
    float* __restrict__ part,         // (B, nT, p)
    int N, int D, int p, int nT) {
  extern __shared__ float lds[];
  const int DS = D | 1;
  float* q_tile = lds;                     // [32][DS] rows i
  float* x_tile = q_tile + GG_TILE * DS;   // [32][DS] rows j
  float* h_tile = x_tile + GG_TILE * DS;   // [32][32]
  float* a_i = h_tile + GG_TILE * GG_TILE;  // [32]
  float* a_j = a_i + GG_TILE;               // [32]
  float* red = a_j + GG_TILE;               // [4][3]

  const int b = blockIdx.y;
  const int tile = blockIdx.x;
  int ti, tj;
  tri_tile_decode(tile, &ti, &tj);
  const int i0 = ti * GG_TILE, j0 = tj * GG_TILE;
  const float* th = theta + (long long)b * p;
  const float* Kb = Kinv + (long long)b * N * N;
  const float* al = alpha + (long long)b * N;

  for (int idx = threadIdx.x; idx < GG_TILE * D; idx += GG_TPB) {
    const int row = idx / D;
    const int col = idx % D;
    const float inv_ell = ANISO ? __expf(-th[1 + col]) : __expf(-th[1]);
    const int gi = i0 + row, gj = j0 + row;
    q_tile[row * DS + col] =
        (gi < N) ? X[(long long)gi * D + col] * inv_ell : 0.f;
    x_tile[row * DS + col] =
        (gj < N) ? X[(long long)gj * D + col] * inv_ell : 0.f;
  }
  if (threadIdx.x < GG_TILE) {
    const int gi = i0 + threadIdx.x;
    a_i[threadIdx.x] = (gi < N) ? al[gi] : 0.f;
  } else if (threadIdx.x < 2 * GG_TILE) {
    const int gj = j0 + threadIdx.x - GG_TILE;
    a_j[threadIdx.x - GG_TILE] = (gj < N) ? al[gj] : 0.f;
  }
  __syncthreads();

  const int ln = threadIdx.x & 31;
  const int lr = threadIdx.x >> 5;
  const int gj = j0 + ln;
  const float wgt = (ti != tj) ? 2.f : 1.f;

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

  float s_sf2 = 0.f, s_noise = 0.f, s_ell = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int li = lr + 8 * r;
    const int gi = i0 + li;
    float h = 0.f;
    if (gi < N && gj < N) {
      float c, g;
      matern_c_g<NU>(d2[r], &c, &g);
      const float w =
          wgt * (Kb[(long long)gi * N + gj] - a_i[li] * a_j[ln]);
      s_sf2 = fmaf(w, c, s_sf2);
      if (gi == gj) s_noise += w;
      h = w * g;
      if (!ANISO) s_ell = fmaf(h, d2[r], s_ell);
    }
    if (ANISO) h_tile[li * GG_TILE + ln] = h;
  }

  s_sf2 = warp_reduce_sum(s_sf2);
  s_noise = warp_reduce_sum(s_noise);
  if (!ANISO) s_ell = warp_reduce_sum(s_ell);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    red[wave * 3 + 0] = s_sf2;
    red[wave * 3 + 1] = s_noise;
    red[wave * 3 + 2] = s_ell;
  }
  __syncthreads();  // also publishes h_tile

  float* out = part + ((long long)b * nT + tile) * p;
  if (threadIdx.x == 0) {
    out[0] = ((red[0] + red[3]) + red[6]) + red[9];
    out[p - 1] = ((red[1] + red[4]) + red[7]) + red[10];
    if (!ANISO) out[1] = ((red[2] + red[5]) + red[8]) + red[11];
  }
  if (ANISO) {
    const int lj = lane & 31;
    const int lih = lane >> 5;
    for (int k = wave; k < D; k += 4) {
      const float xv = x_tile[lj * DS + k];
      float acc = 0.f;
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const int li = 2 * m + lih;
        const float t = q_tile[li * DS + k] - xv;
        acc = fmaf(h_tile[li * GG_TILE + lj], t * t, acc);
      }
      acc = warp_reduce_sum(acc);
      if (lane == 0) out[1 + k] = acc;
    }
  }
}

// grad[b][e] = scale_e * sum_tile part[b][tile][e], tiles in index order,
// accumulated in double. A candidate without a finite NMLL (failed
// factorization) gets an all-zero row.
__global__ void gp_nmll_grad_finish_kernel(const float* __restrict__ part,
                                           const float* __restrict__ theta,
                                           const float* __restrict__ nmll,
                                           const int* __restrict__ info,
                                           float* __restrict__ grad, int B,
                                           int p, int nT) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * p) return;
  const int b = (int)(idx / p), e = (int)(idx % p);
  if (info[b] != 0 || !isfinite(nmll[b])) {
    grad[idx] = 0.f;
    return;
  }
  const float* src = part + (long long)b * nT * p + e;
  double s = 0.0;
  for (int t = 0; t < nT; ++t) s += (double)src[(long long)t * p];
  const double sf2 = exp((double)theta[(long long)b * p]);
  if (e == 0)
    s *= 0.5 * sf2;
  else if (e == p - 1)
    s *= 0.5 * exp((double)theta[(long long)b * p + p - 1]);
  else
    s *= sf2;
  grad[idx] = (float)s;
}

// Y (B, N, N) <- identity: the right-hand side of the K^-1 solves (a kernel,
// not a memset node: cholesky.hip, launch_zero_logdet).
__global__ void gp_fill_identity_kernel(float* __restrict__ Y, int N,
                                        long long total) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long long rc = idx % ((long long)N * N);
  Y[idx] = (rc / N == rc % N) ? 1.f : 0.f;
}

extern "C" int launch_gp_fill_identity(float* Y, int B, int N,
                                       hipStream_t stream) {
  const long long total = (long long)B * N * N;
  hipLaunchKernelGGL(gp_fill_identity_kernel,
                     dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     stream, Y, N, total);
  return (int)hipGetLastError();
}

// tiles of the lower triangle of the ceil(N/32)^2 tile grid
extern "C" int gp_nmll_grad_tiles(int N) {
  const int T = (N + GG_TILE - 1) / GG_TILE;
  return T * (T + 1) / 2;
}

// part: (B, gp_nmll_grad_tiles(N), p) floats of scratch; grad: (B, p).
// Returns the hipGetLastError() code of the launches.
extern "C" int launch_gp_nmll_grad(const float* X, const float* theta,
                                   const float* Kinv, const float* alpha,
                                   const float* nmll, const int* info,
                                   float* part, float* grad, int B, int N,
                                   int D, int p, int nu_code, int aniso,
                                   hipStream_t stream) {
  const int nT = gp_nmll_grad_tiles(N);
  dim3 grid(nT, B);
  const size_t lds_bytes =
      (2 * GG_TILE * (D | 1) + GG_TILE * GG_TILE + 2 * GG_TILE + 12) *
      sizeof(float);
  #define DISPATCH(NU, AN)                                                  \
    hipLaunchKernelGGL((gp_nmll_grad_partial_kernel<NU, AN>), grid,         \
                       dim3(GG_TPB), lds_bytes, stream, X, theta, Kinv,     \
                       alpha, part, N, D, p, nT)
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
  const long long n = (long long)B * p;
  hipLaunchKernelGGL(gp_nmll_grad_finish_kernel,
                     dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     part, theta, nmll, info, grad, B, p, nT);
  return (int)hipGetLastError();
}
