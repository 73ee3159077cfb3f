// Probability of feasibility of the batched exact GP: for constraint b and
// query p, with the standardised posterior mean mu_n and the noise-inclusive
// variance var_n = max(sf2 + noise - |L^-1 k*|^2, 0),
//   z   = (mu_n + y_mean_b / y_std_b) / sqrt(max(var_n, 1e-12))
//   PoF = P(c_b(x_p) > 0) = Phi(z) = 0.5 erfc(-z / sqrt 2)
// and rank_p = (1/B) sum_b PoF_b, the x-distance key of the optimizers.
//
// The pipeline is gp_predict_mean_var's up to its epilogue: the cross kernel,
// the mean gemv (into a (P, B) scratch block here) and the |L^-1 k*|^2
// partial sums of gp_variance.hip. Only the finish differs, and it is this
// file: one thread per query walks the B constraints in index order, adds
// the T partials of each in t order (the order of gp_var_finish_kernel, so
// var_n * y_std^2 is bitwise that kernel's unrounded variance), and writes
// the row [PoF_0 .. PoF_{B-1} | rank] of the (P, B + 1) block.
//
// The gemv writes de-standardised means y_mean + y_std mu_n; dividing by
// y_std recovers mu_n + y_mean / y_std, the numerator of z, in one rounding.
// erfcf keeps full relative accuracy in the lower tail, where 1 + erf(x)
// would cancel. No atomics: a row depends on the query's own Ks rows only,
// not on P and not on its place in the batch. A thread's reads of part are
// coalesced over p; B and T are a handful, so the loop is latency-, not
// bandwidth-bound, and 64-thread blocks spread it over the CUs.

#include "common.h"
#include "launchers.h"
#include <math.h>

#define GPOF_TPB 64

__global__ void gp_pof_finish_kernel(const float* __restrict__ part,   // (B,T,P)
                                     const float* __restrict__ mean,   // (P,B)
                                     const float* __restrict__ theta,
                                     const float* __restrict__ y_std,
                                     float* __restrict__ out,          // (P,B+1)
                                     int B, int P, int T, int theta_stride) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  float* row = out + p * (B + 1);
  float s = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* src = part + (long long)b * T * P + p;
    float q = 0.f;
    for (int t = 0; t < T; ++t) q += src[(long long)t * P];
    const float kss = __expf(theta[b * theta_stride]) +
                      __expf(theta[b * theta_stride + theta_stride - 1]);
    const float var_n = fmaxf(kss - q, 0.f);
    const float z = (mean[p * B + b] / y_std[b]) / sqrtf(fmaxf(var_n, 1e-12f));
    const float pof = 0.5f * erfcf(-z * 0.70710678118654752440f);
    row[b] = pof;
    s += pof;
  }
  row[B] = s / (float)B;
}

// part: (B, gp_var_tiles(N), P) floats of scratch; mean: the (P, B) block the
// mean gemv wrote; out: (P, B + 1). Returns 0 or the hipError_t of the failed
// launch.
extern "C" int launch_gp_pof(const float* Linv, const float* Ks,
                             const float* mean, const float* theta,
                             const float* y_std, float* part, float* out,
                             int B, int P, int N, int theta_stride,
                             hipStream_t stream) {
  const int rc = launch_gp_var_partial(Linv, Ks, part, B, P, N, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(gp_pof_finish_kernel,
                     dim3((P + GPOF_TPB - 1) / GPOF_TPB), dim3(GPOF_TPB), 0,
                     stream, part, mean, theta, y_std, out, B, P,
                     gp_var_tiles(N), theta_stride);
  return (int)hipGetLastError();
}
