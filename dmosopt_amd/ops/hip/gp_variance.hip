// Posterior variance of the batched exact GP — the quadratic form
//   q[b,p] = sum_i ( sum_{j<=i} Linv[b,i,j] * Ks[b,p,j] )^2 = |L^-1 k*|^2
// and the epilogue var = y_std^2 * max(sf2 + noise - q, 0).
//
// Why this form: kss - k*^T K^-1 k* through an explicit fp32 K^-1 cancels
// through a matrix of condition ~1/(noise+jitter) ~ 1e6; the sum of squares
// with a precomputed L^-1 is non-negative term by term and only sees the
// square root of that conditioning (profiles/README.md has the numbers).
//
// Design (gfx950): the product V = Linv[b] * Ks[b]^T (N x P) is tiled
// 32 rows x 32 queries per 256-thread block (4 waves). Grid =
// (ceil(P/32), T = ceil(N/32), B): the rows of Linv are SPLIT over T
// workgroups per query tile, because B*ceil(P/32) alone is ~14 workgroups
// at the workload shape (B=2, P=200, N=300) and the machine has 256 CUs.
// Each block walks the column blocks j0 = 0, 32, .. up to and including
// its own diagonal block and stops there: Linv is lower triangular, the
// blocks strictly above the diagonal are never read. Per step the 32x32
// slab of Linv and the 32x32 slab of Ks are staged in LDS with coalesced
// 128-byte row reads (elements above the diagonal, rows >= N, queries >= P
// and columns >= N are staged as exact zeros; the loads of step s+1 are
// issued into registers before the MFMAs of step s), then the matrix units do
// the products: wave w owns the 16x16 subtile (rows (w>>1)*16, queries
// (w&1)*16) and issues v_mfma_f32_16x16x4_f32 over the 8 k-steps of the
// slab, fp32 accumulate. Lane layout as in matern.hip:
//   A: lane -> Linv[r16 + (lane&15)][k + (lane>>4)]
//   B: B[k][p] = Ks[p][k], lane -> Ks[c16 + (lane&15)][k + (lane>>4)]
//   C/D: query = lane&15, row = (lane>>4)*4 + reg.
// LDS row stride 34: a wave's operand read touches rows (lane&15) and
// columns k + (lane>>4); per 32-lane half that is bank 2*row + {0,1}
// (+const) — all 32 banks once, conflict-free; the staging writes are
// consecutive within a row.
//
// Determinism / batch invariance: there are NO atomics. A lane squares its
// 4 rows in register order, the 4 row groups of a wave are combined by two
// xor shuffles (16, then 32), the two row halves of the block are added
// through LDS in fixed order, and the block writes its partial sum to
// scratch[b][t][p]. The finish kernel adds the T partials in t order. The
// MFMA is a k-ordered fmaf chain per output element, and zero padding adds
// exact zeros, so q[b,p] depends only on Ks[b,p,:] and Linv[b] — not on P,
// not on where the query sits in its tile, not on its neighbours. Every
// partial with p < P is written, so the scratch buffer needs no zeroing
// (and no memset node that a captured graph could race with).

#include "common.h"
#include "launchers.h"
#include <math.h>

#define GV_TILE 32
#define GV_LD 34   // LDS row stride (floats), see the bank note above
#define GV_TPB 256

typedef __attribute__((ext_vector_type(4))) float gv_f32x4;

__global__ void gp_var_partial_kernel(
    const float* __restrict__ Linv,  // (B, N, N) lower triangular
    const float* __restrict__ Ks,    // (B, P, N)
    float* __restrict__ part,        // (B, T, P) per-row-tile partial sums
    int P, int N, int T) {
  __shared__ float l_tile[GV_TILE * GV_LD];
  __shared__ float k_tile[GV_TILE * GV_LD];
  __shared__ float red[2][GV_TILE];

  const int b = blockIdx.z;
  const int t = blockIdx.y;
  const int i0 = t * GV_TILE;           // first Linv row of this block
  const int p0 = blockIdx.x * GV_TILE;  // first query of this block
  const float* Lb = Linv + (long long)b * N * N;
  const float* Kb = Ks + (long long)b * P * N;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const int r16 = (wave >> 1) * 16, c16 = (wave & 1) * 16;
  const int scol = threadIdx.x & 31;  // staging column
  const int srow = threadIdx.x >> 5;  // staging row, +8 per pass

  // a thread's 4 + 4 elements of one slab pair, zeros where out of range
  float lreg[4], kreg[4];
  auto load_slab = [&](int j0) {
    const int gj = j0 + scol;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = i0 + srow + 8 * r;
      const int gp = p0 + srow + 8 * r;
      lreg[r] = (gi < N && gj <= gi) ? Lb[(long long)gi * N + gj] : 0.f;
      kreg[r] = (gp < P && gj < N) ? Kb[(long long)gp * N + gj] : 0.f;
    }
  };

  gv_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  load_slab(0);
  for (int j0 = 0; j0 <= i0; j0 += GV_TILE) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      l_tile[(srow + 8 * r) * GV_LD + scol] = lreg[r];
      k_tile[(srow + 8 * r) * GV_LD + scol] = kreg[r];
    }
    __syncthreads();
    // the next slab's loads fly under this slab's MFMAs: the block's walk
    // is a serial chain of up to T global-load latencies otherwise
    if (j0 + GV_TILE <= i0) load_slab(j0 + GV_TILE);
#pragma unroll
    for (int k = 0; k < GV_TILE; k += 4) {
      const float a = l_tile[(r16 + lr) * GV_LD + k + lk];
      const float bv = k_tile[(c16 + lr) * GV_LD + k + lk];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
    }
    __syncthreads();
  }

  // sum of squares over this wave's 16 rows, fixed order
  float s = acc[0] * acc[0];
  s = fmaf(acc[1], acc[1], s);
  s = fmaf(acc[2], acc[2], s);
  s = fmaf(acc[3], acc[3], s);
  s += __shfl_xor(s, 16, WAVE_SIZE);
  s += __shfl_xor(s, 32, WAVE_SIZE);
  if (lk == 0) red[wave >> 1][c16 + lr] = s;
  __syncthreads();
  if (threadIdx.x < GV_TILE) {
    const int gp = p0 + threadIdx.x;
    if (gp < P)
      part[((long long)b * T + t) * P + gp] =
          red[0][threadIdx.x] + red[1][threadIdx.x];
  }
}

// The one spelling of the decimal rounding (scale = 10^decimals): the engine
// hands these values to the MOEA as objectives.
__device__ __forceinline__ float round_decimals(float v, float scale) {
  return rintf(v * scale) / scale;
}

// Epilogue: q = sum_t part[b][t][p] in t order, then
// out[p][B + b] = y_std[b]^2 * max(sf2_b + noise_b - q, 0), optionally
// rounded. kss carries no jitter (it is the prior variance of a new point).
__global__ void gp_var_finish_kernel(const float* __restrict__ part,
                                     const float* __restrict__ theta,
                                     const float* __restrict__ y_std,
                                     float* __restrict__ out, int B, int P,
                                     int T, int theta_stride,
                                     float round_scale) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * P) return;
  const int b = (int)(idx / P), p = (int)(idx % P);
  const float* src = part + (long long)b * T * P + p;
  float q = 0.f;
  for (int t = 0; t < T; ++t) q += src[(long long)t * P];
  const float kss = __expf(theta[b * theta_stride]) +
                    __expf(theta[b * theta_stride + theta_stride - 1]);
  const float sd = y_std[b];
  float v = (sd * sd) * fmaxf(kss - q, 0.f);
  if (round_scale > 0.f) v = round_decimals(v, round_scale);
  out[(long long)p * (2 * B) + B + b] = v;
}

extern "C" int gp_var_tiles(int N) { return (N + GV_TILE - 1) / GV_TILE; }

// The partial sums alone, part: (B, gp_var_tiles(N), P) floats of scratch;
// the epilogue is the caller's (the variance finish below, or the
// probability-of-feasibility finish of gp_pof.hip).
extern "C" int launch_gp_var_partial(const float* Linv, const float* Ks,
                                     float* part, int B, int P, int N,
                                     hipStream_t stream) {
  const int T = gp_var_tiles(N);
  dim3 grid((P + GV_TILE - 1) / GV_TILE, T, B);
  hipLaunchKernelGGL(gp_var_partial_kernel, grid, dim3(GV_TPB), 0, stream,
                     Linv, Ks, part, P, N, T);
  return (int)hipGetLastError();
}

// part: (B, ceil(N/32), P) floats of scratch; out: (P, 2B), columns [B, 2B)
// are written here. Returns the hipGetLastError() code of the launches.
extern "C" int launch_gp_variance(const float* Linv, const float* Ks,
                                  const float* theta, const float* y_std,
                                  float* part, float* out, int B, int P,
                                  int N, int theta_stride, float round_scale,
                                  hipStream_t stream) {
  const int T = gp_var_tiles(N);
  const int rc = launch_gp_var_partial(Linv, Ks, part, B, P, N, stream);
  if (rc != 0) return rc;
  const long long n = (long long)B * P;
  hipLaunchKernelGGL(gp_var_finish_kernel, dim3((int)((n + 255) / 256)),
                     dim3(256), 0, stream, part, theta, y_std, out, B, P, T,
                     theta_stride, round_scale);
  return (int)hipGetLastError();
}
