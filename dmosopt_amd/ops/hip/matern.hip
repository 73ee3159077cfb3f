// Batched Matern / RBF kernel-matrix assembly — fused distance + transform.
//
// Replaces the reference's sklearn kernel evaluation (model.py:1227-1251).
// One launch assembles B hyperparameter candidates' kernel matrices:
//   K[b] = sf2[b] * matern_nu(||x_i/ell - x_j/ell||) (+ (noise+jitter) I)
//
// Design (gfx950): 32x32 output tile per 256-thread block (4 waves), both
// 32-row input slabs staged in LDS with the 1/ell scaling fused into the
// load. The pairwise cross terms run on the MATRIX UNITS:
// d2(i,j) = |q_i|^2 + |x_j|^2 - 2 q_i.x_j, with the q.x dot products
// computed by v_mfma_f32_16x16x4_f32 (exact fp32 at the f32 vector rate,
// one instruction per 16x16x4 tile — ~16x fewer issue slots than the
// per-pair FMA chain). d2 is clamped at 0 against cancellation before the
// Matern transform. Fusion (no separate cdist + transform passes) is the
// point; for the d <= 128 regime the kernel is bandwidth-trivial.

#include "common.h"
#include "launchers.h"
#include <math.h>

#define TILE 32
#define TPB 256  // 16x16 threads, each owns a 2x2 patch

// nu encoding: 0 -> RBF (exp(-0.5 r^2)), 1 -> 1/2, 3 -> 3/2, 5 -> 5/2
template <int NU>
__device__ __forceinline__ float matern_transform(float d2) {
  if (NU == 0) return __expf(-0.5f * d2);
  const float r = sqrtf(fmaxf(d2, 0.f));
  if (NU == 1) return __expf(-r);
  if (NU == 3) {
    const float s = 1.7320508075688772f * r;  // sqrt(3) r
    return (1.f + s) * __expf(-s);
  }
  // nu = 5/2
  const float s = 2.23606797749979f * r;  // sqrt(5) r
  return (1.f + s + (5.f / 3.f) * d2) * __expf(-s);
}

// theta layout per batch row: [log sf2, log ell (1 or D), log noise]
// DIRECT: exact (q-x)^2 accumulation instead of the norms+MFMA form. The
// train kernel (SYMMETRIC) always uses it; a CROSS kernel may ask for it
// (launch form 2) where the ~1e-7 cancellation in the norms-form d2 is too
// much — the posterior VARIANCE under nu = 1/2, whose kernel has an
// infinite slope in d2 at 0: a query on a training point gets r off by
// sqrt(1e-7) ~ 3e-4 and the variance off by twice that.
//
// PROLOGUE (train form only): the launch also initialises the side buffers
// of the factorization that follows it for its batch row — the first block
// of every tile row copies its 32-entry segment of the caller's y row into
// Z[b, :], and block (0, 0, b) sets logdet[b] = 0 and info[b] = 0. The
// kernel boundary before panel 0 orders this; K's arithmetic is untouched.
struct NmllPrologue {
  const float* y;  // (N,) shared or (B, N) rows
  int y_stride;    // 0 or N
  float* Z;        // (B, N)
  float* logdet;   // (B,)
  int* info;       // (B,)
};

template <int NU, bool ANISO, bool SYMMETRIC, bool DIRECT = SYMMETRIC,
          bool PROLOGUE = false>
__global__ void matern_assemble_kernel(
    const float* __restrict__ Xq,   // (P, D) query rows (== X when SYMMETRIC)
    const float* __restrict__ X,    // (N, D)
    const float* __restrict__ theta,  // (B, p)
    float* __restrict__ K,          // (B, P, N)
    int P, int N, int D, int theta_stride, float jitter,
    const float* __restrict__ q_lb = nullptr,   // optional per-dim affine
    const float* __restrict__ q_invrg = nullptr,  // applied to Xq at load
    NmllPrologue pro = NmllPrologue()) {
  extern __shared__ float lds[];  // [2][TILE][DS] scaled row slabs
  const int DS = D | 1;  // odd stride: row base spreads over all 32 banks
  float* q_tile = lds;
  float* x_tile = lds + TILE * DS;

  const int b = blockIdx.z;
  const int tile_p = blockIdx.y * TILE;
  const int tile_n = blockIdx.x * TILE;
  const float sf2 = __expf(theta[b * theta_stride + 0]);
  const float noise = __expf(theta[b * theta_stride + theta_stride - 1]);

  if (PROLOGUE && blockIdx.x == 0) {
    const int i = tile_p + (int)threadIdx.x;
    if (threadIdx.x < TILE && i < N)
      pro.Z[(long long)b * N + i] = pro.y[(long long)b * pro.y_stride + i];
    if (blockIdx.y == 0 && threadIdx.x == TILE) {
      pro.logdet[b] = 0.f;
      pro.info[b] = 0;
    }
  }

  // stage scaled rows: thread t covers elements strided over TILE*D
  for (int idx = threadIdx.x; idx < TILE * D; idx += TPB) {
    const int row = idx / D;
    const int col = idx % D;
    const float inv_ell =
        ANISO ? __expf(-theta[b * theta_stride + 1 + col])
              : __expf(-theta[b * theta_stride + 1]);
    const int gq = tile_p + row;
    float qv = (gq < P) ? Xq[gq * D + col] : 0.f;
    if (q_lb != nullptr) qv = (qv - q_lb[col]) * q_invrg[col];
    q_tile[row * DS + col] = qv * inv_ell;
    const int gx = tile_n + row;
    x_tile[row * DS + col] = (gx < N) ? X[gx * D + col] * inv_ell : 0.f;
  }
  __syncthreads();

  if (DIRECT) {
    // TRAIN kernel: exact (q-x)^2 accumulation. The norms+MFMA form
    // perturbs d2 by ~1e-6 (cancellation), which flips SCE-UA accept
    // decisions bit-wise and changes the fit's iteration count — the
    // train path stays bitwise-stable; the cross kernel (predictions,
    // tolerance-level effect) uses the matrix units below.
    const int ty = threadIdx.x / 16;
    const int tx = threadIdx.x % 16;
#pragma unroll
    for (int sy = 0; sy < 2; ++sy) {
#pragma unroll
      for (int sx = 0; sx < 2; ++sx) {
        const int lp = ty * 2 + sy;
        const int ln = tx * 2 + sx;
        const int gp = tile_p + lp;
        const int gn = tile_n + ln;
        if (gp >= P || gn >= N) continue;
        const float* qa = q_tile + lp * DS;
        const float* xb = x_tile + ln * DS;
        float d2 = 0.f;
        for (int k = 0; k < D; ++k) {
          const float t = qa[k] - xb[k];
          d2 = fmaf(t, t, d2);
        }
        float v = sf2 * matern_transform<NU>(d2);
        if (SYMMETRIC && gp == gn) v += noise + jitter;
        K[((long long)b * P + gp) * N + gn] = v;
      }
    }
    return;
  }

  // per-row squared norms of the scaled slabs
  float* qn = x_tile + TILE * DS;  // TILE floats
  float* xn = qn + TILE;          // TILE floats
  if (threadIdx.x < 2 * TILE) {
    const bool is_q = threadIdx.x < TILE;
    const int row = is_q ? threadIdx.x : threadIdx.x - TILE;
    const float* src = (is_q ? q_tile : x_tile) + row * DS;
    float acc = 0.f;
    for (int k = 0; k < D; ++k) acc = fmaf(src[k], src[k], acc);
    (is_q ? qn : xn)[row] = acc;
  }
  __syncthreads();

  // cross terms on the matrix units: wave w computes 16x16 subtile
  // (w>>1, w&1). A: lane -> q[(r16 + (lane&15))][k + (lane>>4)];
  // B[k][j] = x[j][k]; C/D: col = lane&15, row = (lane>>4)*4 + reg.
  typedef __attribute__((ext_vector_type(4))) float f32x4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const int r16 = (wave >> 1) * 16, c16 = (wave & 1) * 16;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < D; k += 4) {
    const bool ink = (k + lk) < D;
    const float a = ink ? q_tile[(r16 + lr) * DS + k + lk] : 0.f;
    const float bv = ink ? x_tile[(c16 + lr) * DS + k + lk] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int lp = r16 + lk * 4 + r;
    const int ln = c16 + lr;
    const int gp = tile_p + lp;
    const int gn = tile_n + ln;
    if (gp >= P || gn >= N) continue;
    const float d2 = fmaxf(qn[lp] + xn[ln] - 2.f * acc[r], 0.f);
    float v = sf2 * matern_transform<NU>(d2);
    if (SYMMETRIC && gp == gn) v += noise + jitter;
    K[((long long)b * P + gp) * N + gn] = v;
  }
}

extern "C" void launch_matern_assemble_affine(
    const float* Xq, const float* X, const float* theta, float* K, int B,
    int P, int N, int D, int theta_stride, float jitter, int nu_code,
    int aniso, int symmetric, const float* q_lb, const float* q_invrg,
    hipStream_t stream) {
  dim3 grid((N + TILE - 1) / TILE, (P + TILE - 1) / TILE, B);
  dim3 block(TPB);
  size_t lds_bytes = (2 * TILE * (D | 1) + 2 * TILE) * sizeof(float);
  #define DISPATCH(NU, AN, SY)                                              \
    hipLaunchKernelGGL((matern_assemble_kernel<NU, AN, SY>), grid, block,   \
                       lds_bytes, stream, Xq, X, theta, K, P, N, D,         \
                       theta_stride, jitter, q_lb, q_invrg, NmllPrologue())
  // symmetric: 0 = cross (norms+MFMA), 1 = train, 2 = cross, direct form
  #define DISPATCH_DIRECT(NU, AN)                                           \
    hipLaunchKernelGGL((matern_assemble_kernel<NU, AN, false, true>), grid, \
                       block, lds_bytes, stream, Xq, X, theta, K, P, N, D,  \
                       theta_stride, jitter, q_lb, q_invrg, NmllPrologue())
  #define DISPATCH_AN(NU)                                                   \
    if (symmetric == 2) {                                                   \
      if (aniso) DISPATCH_DIRECT(NU, true); else DISPATCH_DIRECT(NU, false); \
    } else if (aniso) {                                                     \
      if (symmetric) DISPATCH(NU, true, true); else DISPATCH(NU, true, false); \
    } else {                                                                \
      if (symmetric) DISPATCH(NU, false, true); else DISPATCH(NU, false, false); \
    }
  switch (nu_code) {
    case 0: DISPATCH_AN(0); break;
    case 1: DISPATCH_AN(1); break;
    case 3: DISPATCH_AN(3); break;
    default: DISPATCH_AN(5); break;
  }
  #undef DISPATCH_AN
  #undef DISPATCH_DIRECT
  #undef DISPATCH
}

// Train-form assembly (launch_matern_assemble_affine with symmetric = 1) whose
// launch also runs the NMLL prologue: Z = y rows, logdet = 0, info = 0.
extern "C" void launch_matern_train_prologue(
    const float* X, const float* theta, float* K, int B, int N, int D,
    int theta_stride, float jitter, int nu_code, int aniso, const float* y,
    int y_stride, float* Z, float* logdet, int* info, hipStream_t stream) {
  dim3 grid((N + TILE - 1) / TILE, (N + TILE - 1) / TILE, B);
  dim3 block(TPB);
  size_t lds_bytes = (2 * TILE * (D | 1) + 2 * TILE) * sizeof(float);
  const NmllPrologue pro = {y, y_stride, Z, logdet, info};
  #define DISPATCH(NU, AN)                                                   \
    hipLaunchKernelGGL((matern_assemble_kernel<NU, AN, true, true, true>),   \
                       grid, block, lds_bytes, stream, X, X, theta, K, N, N, \
                       D, theta_stride, jitter, (const float*)nullptr,       \
                       (const float*)nullptr, pro)
  #define DISPATCH_AN(NU) \
    if (aniso) DISPATCH(NU, true); else DISPATCH(NU, false)
  switch (nu_code) {
    case 0: DISPATCH_AN(0); break;
    case 1: DISPATCH_AN(1); break;
    case 3: DISPATCH_AN(3); break;
    default: DISPATCH_AN(5); break;
  }
  #undef DISPATCH_AN
  #undef DISPATCH
}

// Fused posterior-mean GEMV + de-standardization: out[p][b] =
// y_mean[b] + y_std[b] * dot(Ks[b,p,:], alpha[b,:]). One wave per (b,p)
// row (lane-strided coalesced loads, fixed-order shuffle reduce:
// deterministic), writing the CONTIGUOUS (P, B) result directly —
// replaces at::bmm + addcmul + transpose-contiguous (3 dispatches and
// ~30 us of host time per generation; the GEMM itself is overkill for a
// (B,P,N)x(B,N,1) matvec). ldo is the output row stride: B for the
// mean-only result, 2B when the means are the left half of the (P, 2B)
// mean|variance block — the SAME kernel serves both so the means are
// bitwise identical.
__global__ void gp_mean_gemv_kernel(const float* __restrict__ Ks,
                                    const float* __restrict__ alpha,
                                    const float* __restrict__ y_mean,
                                    const float* __restrict__ y_std,
                                    float* __restrict__ out, int B, int P,
                                    int N, int ldo) {
  const long long w =
      ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // wave id
  const int lane = threadIdx.x & 63;
  if (w >= (long long)B * P) return;
  const int b = (int)(w / P), p = (int)(w % P);
  const float* row = Ks + ((long long)b * P + p) * N;
  const float* al = alpha + (long long)b * N;
  float acc = 0.f;
  for (int n = lane; n < N; n += 64) acc = fmaf(row[n], al[n], acc);
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if (lane == 0) out[(long long)p * ldo + b] = fmaf(y_std[b], acc, y_mean[b]);
}

extern "C" void launch_gp_mean_gemv(const float* Ks, const float* alpha,
                                    const float* y_mean, const float* y_std,
                                    float* out, int B, int P, int N,
                                    int ldo, hipStream_t stream) {
  const long long waves = (long long)B * P;
  const long long threads = waves * 64;
  hipLaunchKernelGGL(gp_mean_gemv_kernel, dim3((int)((threads + 255) / 256)),
                     dim3(256), 0, stream, Ks, alpha, y_mean, y_std, out, B,
                     P, N, ldo);
}
