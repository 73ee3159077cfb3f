// Micro-benchmark: what costs 2000 cycles per column in the panel factor?
// Variants of the 32-column diagonal factor, timed with wall clock around
// 2000 back-to-back iterations inside one launch (B=12 blocks, one wave
// active per block), three timed launches per variant, variants interleaved.
// Every variant also writes its factored block, logdet, info and (where it
// has one) solved rhs row of the LAST iteration; the host compares them bit
// for bit with the variant's parent and prints the mismatch counts.
//
// build+run (GPU box):
//   hipcc --offload-arch=gfx950 -O3 scripts_factor_micro.hip -o /tmp/fm && /tmp/fm
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#define BS 32

__device__ __forceinline__ float shfl_f(float v, int src) {
  return __shfl(v, src, 64);
}

// lane index must be a compile-time constant (v_readlane_b32 to an SGPR)
__device__ __forceinline__ float readlane_f(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// V0: full 2-col grouped factor (mirror of chol_panel_body's "lds" loop)
// V1: no __threadfence_block
// V2: no LDS broadcast at all (results wrong; rank-2 uses stale garbage)
// V3: no sqrt/div/log (linear ops only)
// V4: rounds without rank-2 update tail
// V5: register broadcast (v_readlane at constant lanes), log in the loop
// V6: V5 + one deferred logf per lane after the loop
// V7: V6 + the rhs riding as row 32 (lane 32), no separate solve
// V8 ("V0r"): V0 followed by today's 32-step shuffle solve of the rhs
enum { V0R = 8, NVAR = 9 };

template <int VARIANT>
__device__ __forceinline__ void factor_lds(float (&r)[BS], int lane,
                                           float (*colbuf)[BS], float& mylog,
                                           int& bad) {
#pragma unroll
  for (int g = 0; g < BS; g += 2) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int j = g + q;
      if (q == 1 && VARIANT != 2) {
        if (lane >= j) r[j] = fmaf(-r[g], colbuf[0][j], r[j]);
      }
      float d = shfl_f(r[j], j);
      if (VARIANT == 3) {
        d = d + 1.f;
        if (lane == j) r[j] = d;
        else if (lane > j) r[j] *= d;
      } else {
        if (d <= 0.0f || !isfinite(d)) {
          bad = bad ? bad : (j + 1);
          d = 1e-30f;
        }
        d = sqrtf(d);
        if (lane == j) { r[j] = d; mylog += logf(d); }
        else if (lane > j) r[j] /= d;
      }
      if (VARIANT != 2) {
        if (lane < BS) colbuf[q][lane] = r[j];
        if (VARIANT != 1) __threadfence_block();
      }
    }
    if (VARIANT != 4) {
#pragma unroll
      for (int t = 0; t < BS; ++t) {
        if (t < g + 2) continue;
        if (lane >= t) {
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const float c = (VARIANT == 2) ? shfl_f(r[g + q], t) : colbuf[q][t];
            r[t] = fmaf(-r[g + q], c, r[t]);
          }
        }
      }
    }
  }
}

// Right-looking, lane = row: column j's pivot and every multiplier come out
// of the owning lane's register through v_readlane_b32 at a constant lane.
// The division and the rank-1 update are unmasked: rows above the diagonal
// hold junk that no lane ever reads back, row 32 (if loaded) is the rhs.
template <bool DEFER_LOG>
__device__ __forceinline__ void factor_reg(float (&r)[BS], int lane,
                                           float& mylog, int& bad) {
  float dj = 1.0f;
#pragma unroll
  for (int j = 0; j < BS; ++j) {
    float d = readlane_f(r[j], j);
    if (d <= 0.0f || !isfinite(d)) {
      bad = bad ? bad : (j + 1);
      d = 1e-30f;
    }
    d = sqrtf(d);
    const float q = r[j] / d;
    r[j] = (lane == j) ? d : q;
    if (DEFER_LOG) dj = (lane == j) ? d : dj;
    else if (lane == j) mylog += logf(d);
#pragma unroll
    for (int t0 = j + 1; t0 < BS; t0 += 8) {
      float m[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (t0 + u < BS) m[u] = readlane_f(r[j], t0 + u);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (t0 + u < BS) r[t0 + u] = fmaf(-r[j], m[u], r[t0 + u]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  if (DEFER_LOG) mylog = (lane < BS) ? logf(dj) : 0.0f;
}

template <int VARIANT>
__global__ __launch_bounds__(384) void factor_kernel(
    const float* __restrict__ A, const float* __restrict__ y,
    float* __restrict__ outF,   // (B, 33, 32): factored block, row 32 = z
    float* __restrict__ outLd,  // (B,)
    int* __restrict__ outBad,   // (B,)
    int iters) {
  __shared__ float S[BS + 1][BS + 1];  // row 32: the rhs segment
  __shared__ float F[BS + 1][BS + 1];  // factored block (+ solved rhs row)
  __shared__ float colbuf[2][BS];
  constexpr bool REG = VARIANT >= 5 && VARIANT <= 7;
  constexpr bool RHS = VARIANT == 7 || VARIANT == V0R;
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  for (int idx = tid; idx < BS * BS; idx += blockDim.x)
    S[idx / BS][idx % BS] = A[b * BS * BS + idx];
  if (tid < BS) S[BS][tid] = y[b * BS + tid];
  __syncthreads();
  float acc = 0.f;
  for (int it = 0; it < iters; ++it) {
    if (tid < 64) {
      const int lane = tid;
      float r[BS];
      const int rows = (VARIANT == 7) ? BS + 1 : BS;
#pragma unroll
      for (int t = 0; t < BS; ++t)
        r[t] = (lane < rows) ? S[lane][t] + it * 1e-9f : 0.0f;
      float mylog = 0.0f;
      int bad = 0;
      if (REG) factor_reg<(VARIANT >= 6)>(r, lane, mylog, bad);
      else factor_lds<(VARIANT == V0R ? 0 : VARIANT)>(r, lane, colbuf, mylog, bad);
      if (lane < rows) {
#pragma unroll
        for (int t = 0; t < BS; ++t) F[lane][t] = r[t];
      }
      for (int off = 32; off > 0; off >>= 1) mylog += __shfl_down(mylog, off);
      if (lane == 0 && it == iters - 1) {
        outLd[b] = mylog;
        outBad[b] = bad;
      }
      acc += r[lane & (BS - 1)] + mylog;
    }
    if (RHS) __syncthreads();  // the kernel's post-factor barrier
    if (VARIANT == V0R && tid < 64) {
      const int j = tid;
      float v = (j < BS) ? S[BS][j] + it * 1e-9f : 0.0f;
      for (int t = 0; t < BS; ++t) {
        const float zt = shfl_f(v, t) / F[t][t];
        if (j == t) v = zt;
        else if (j > t && j < BS) v = fmaf(-F[j][t], zt, v);
      }
      if (j < BS) F[BS][j] = v;
      acc += v;
    }
    __syncthreads();
  }
  const int frows = RHS ? BS + 1 : BS;
  for (int idx = tid; idx < frows * BS; idx += blockDim.x)
    outF[b * (BS + 1) * BS + idx] = F[idx / BS][idx % BS];
  if (tid == 0 && acc == 123.456f) outBad[b] = -1;  // keeps acc live
}

typedef void (*kern_t)(const float*, const float*, float*, float*, int*, int);
static kern_t kerns[NVAR] = {
    factor_kernel<0>, factor_kernel<1>, factor_kernel<2>,
    factor_kernel<3>, factor_kernel<4>, factor_kernel<5>,
    factor_kernel<6>, factor_kernel<7>, factor_kernel<V0R>};
static const char* names[NVAR] = {
    "V0  full(2-col LDS+fence)", "V1  no fence", "V2  shfl only (no LDS)",
    "V3  no sqrt/div/log", "V4  no rank-2 tail", "V5  readlane broadcast",
    "V6  V5 + deferred log", "V7  V6 + rhs as row 32", "V0r V0 + shfl rhs solve"};

#define CK(x)                                                        \
  do {                                                               \
    hipError_t e_ = (x);                                             \
    if (e_ != hipSuccess) {                                          \
      printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
      return 2;                                                      \
    }                                                                \
  } while (0)

// bitwise mismatches of the lower triangle (and rows >= BS whole)
static int mism_block(const float* a, const float* b, int B, int rows) {
  int n = 0;
  for (int m = 0; m < B; ++m)
    for (int i = 0; i < rows; ++i)
      for (int t = 0; t < BS; ++t) {
        if (i < BS && t > i) continue;
        const int o = (m * (BS + 1) + i) * BS + t;
        n += memcmp(a + o, b + o, sizeof(float)) != 0;
      }
  return n;
}

int main() {
  const int B = 12, iters = 2000, REPS = 3;
  static float h[B * BS * BS], hy[B * BS];
  // SPD blocks (exponential kernel + nugget), one per matrix; matrix 3 has a
  // negative pivot at column 5 so the info / clamp path is compared too
  for (int m = 0; m < B; ++m)
    for (int i = 0; i < BS; ++i) {
      for (int j = 0; j < BS; ++j)
        h[(m * BS + i) * BS + j] =
            (1.0f + 0.05f * m) * expf(-0.15f * fabsf((float)(i - j))) +
            (i == j ? 0.01f * (m + 1) : 0.0f);
      hy[m * BS + i] = sinf(0.7f * i + m) + 0.25f;
    }
  h[(3 * BS + 5) * BS + 5] = -1.0f;
  float *A, *y, *outF, *outLd;
  int* outBad;
  const size_t fN = (size_t)B * (BS + 1) * BS;
  CK(hipMalloc(&A, sizeof(h)));
  CK(hipMalloc(&y, sizeof(hy)));
  CK(hipMalloc(&outF, fN * sizeof(float)));
  CK(hipMalloc(&outLd, B * sizeof(float)));
  CK(hipMalloc(&outBad, B * sizeof(int)));
  CK(hipMemcpy(A, h, sizeof(h), hipMemcpyHostToDevice));
  CK(hipMemcpy(y, hy, sizeof(hy), hipMemcpyHostToDevice));
  static float resF[NVAR][B * (BS + 1) * BS], resLd[NVAR][B];
  static int resBad[NVAR][B];
  float us[NVAR][REPS];
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int v = 0; v < NVAR; ++v) {  // warmup
    hipLaunchKernelGGL(kerns[v], dim3(B), dim3(384), 0, 0, A, y, outF, outLd,
                       outBad, 10);
    CK(hipDeviceSynchronize());
  }
  for (int rep = 0; rep < REPS; ++rep)
    for (int v = 0; v < NVAR; ++v) {
      CK(hipMemset(outF, 0, fN * sizeof(float)));
      CK(hipEventRecord(e0));
      hipLaunchKernelGGL(kerns[v], dim3(B), dim3(384), 0, 0, A, y, outF, outLd,
                         outBad, iters);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms = 0;
      CK(hipEventElapsedTime(&ms, e0, e1));
      us[v][rep] = ms * 1000.0f / iters;
      CK(hipMemcpy(resF[v], outF, fN * sizeof(float), hipMemcpyDeviceToHost));
      CK(hipMemcpy(resLd[v], outLd, B * sizeof(float), hipMemcpyDeviceToHost));
      CK(hipMemcpy(resBad[v], outBad, B * sizeof(int), hipMemcpyDeviceToHost));
    }
  for (int v = 0; v < NVAR; ++v) {
    float lo = us[v][0], hi = us[v][0];
    for (int rep = 1; rep < REPS; ++rep) {
      lo = fminf(lo, us[v][rep]);
      hi = fmaxf(hi, us[v][rep]);
    }
    float med = us[v][0] + us[v][1] + us[v][2] - lo - hi;
    printf("%-26s: %7.3f %7.3f %7.3f us  median %7.3f range %6.3f\n", names[v],
           us[v][0], us[v][1], us[v][2], med, hi - lo);
  }
  // bitwise comparison with the parent variant
  const int pairs[][2] = {{5, 0}, {6, 0}, {V0R, 0}, {7, V0R}};
  int total = 0;
  for (auto& p : pairs) {
    const int v = p[0], ref = p[1];
    const int rows = (v == 7) ? BS + 1 : BS;
    const int mb = mism_block(resF[v], resF[ref], B, rows);
    const int ml = memcmp(resLd[v], resLd[ref], sizeof(resLd[v])) != 0;
    int mi = 0;
    for (int m = 0; m < B; ++m) mi += resBad[v][m] != resBad[ref][m];
    printf("%-26s vs %-4.3s: block%s mismatches %d, logdet %s, info mismatches %d\n",
           names[v], names[ref], rows > BS ? "+z" : "", mb,
           ml ? "DIFFERS" : "equal", mi);
    total += mb + ml + mi;
  }
  printf("info of matrix 3 (expect 6): %d; logdet[0] = %.6f; z[0][31] = %.6f\n",
         resBad[0][3], resLd[0][0], resF[V0R][(BS)*BS + 31]);
  printf("TOTAL MISMATCHES %d\n", total);
  return total ? 1 : 0;
}
