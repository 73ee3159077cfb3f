// Fused SCE-UA CCE stage kernels.
//
// One CCE stage of the batched hyperparameter search (models/sceua.py,
// semantics of reference model.py:1419-1753) previously queued ~30 small
// torch elementwise/gather kernels around the batched NMLL evaluation.
// These two kernels replace that chain:
//   sceua_propose:  centroid + reflect(/oob random)/contract/random
//                   candidate assembly, Philox RNG in-kernel
//   sceua_accept:   sequential acceptance rule, worst-point replacement,
//                   per-complex re-sort, device-side icall accounting
// Every (stream, complex) pair is one small workgroup — the stage has
// S*G of them, so these kernels are latency-bound glue; the point is the
// ~28 fewer stream entries per stage, not their own throughput.
//
// Each comes in two forms that share ONE device body (same arithmetic, same
// Philox keying, same bits): the launch-argument form takes the stage's
// simplex positions and seed from the host per launch; the device-schedule
// form reads them from a per-shuffle schedule in device memory, so a captured
// stage (models/gp_core.py _StageGraph) replays with no per-stage argument.
// The shuffle-boundary kernels at the end replace the torch permute / gather
// / reduce glue between two shuffles.

#include "common.h"
#include "launchers.h"
#include <math.h>

#define SCEUA_TPB 64

// cx: (S, G, npg, nopt) f32, cf: (S, G, npg) f32, lcs: (nps,) int32
// cand out: (3, S*G, nopt) f32 in reflect/contract/random order.
__device__ __forceinline__ void sceua_propose_body(
    const float* __restrict__ cx, const int* __restrict__ lcs,
    const float* __restrict__ bl, const float* __restrict__ bu,
    float* __restrict__ cand, int S, int G, int npg, int nopt, int nps,
    unsigned long long seed) {
  const int sg = blockIdx.x;
  const float* base = cx + ((long long)sg) * npg * nopt;
  const int wi = lcs[nps - 1];  // worst simplex position
  __shared__ int oob_flag;
  if (threadIdx.x == 0) oob_flag = 0;
  __syncthreads();

  float* c_ref = cand + (long long)sg * nopt;
  float* c_con = cand + ((long long)(S * G) + sg) * nopt;
  float* c_rnd = cand + ((long long)(2 * S * G) + sg) * nopt;

  // pass 1: centroid/reflect/contract + oob detection
  for (int d = threadIdx.x; d < nopt; d += SCEUA_TPB) {
    float ce = 0.f;
    for (int i = 0; i < nps - 1; ++i)
      ce += base[(long long)lcs[i] * nopt + d];
    ce /= (float)(nps - 1);
    const float sw = base[(long long)wi * nopt + d];
    const float ref = ce + (ce - sw);
    if (ref < bl[d] || ref > bu[d]) atomicOr(&oob_flag, 1);
    c_ref[d] = ref;
    c_con[d] = sw + 0.5f * (ce - sw);
  }
  __syncthreads();
  // pass 2: randoms (Philox keyed by (seed, sg, d)) + oob replacement
  for (int d = threadIdx.x; d < nopt; d += SCEUA_TPB) {
    const float span = bu[d] - bl[d];
    Philox4 r = philox4x32(seed, ((unsigned long long)sg << 32) | (unsigned)d);
    c_rnd[d] = bl[d] + span * u01(r.c0);
    if (oob_flag) c_ref[d] = bl[d] + span * u01(r.c1);
  }
}

__global__ void sceua_propose_kernel(const float* __restrict__ cx,
                                     const int* __restrict__ lcs,
                                     const float* __restrict__ bl,
                                     const float* __restrict__ bu,
                                     float* __restrict__ cand, int S, int G,
                                     int npg, int nopt, int nps,
                                     unsigned long long seed) {
  sceua_propose_body(cx, lcs, bl, bu, cand, S, G, npg, nopt, nps, seed);
}

// fall: (3, S*G) f32 NMLL values for reflect/contract/random candidates.
// act: (S,) int32. icall: (S,) int32 accumulated on device.
// LDS (dynamic): keys npg f32, ord npg int, rowbuf npg * nopt f32.
__device__ __forceinline__ void sceua_accept_body(
    float* __restrict__ cx, float* __restrict__ cf,
    const float* __restrict__ cand, const float* __restrict__ fall,
    const int* __restrict__ lcs, const int* __restrict__ act,
    int* __restrict__ icall, int S, int G, int npg, int nopt, int nps) {
  extern __shared__ char sh_raw[];
  float* keys = (float*)sh_raw;      // npg
  int* ord = (int*)(keys + npg);     // npg
  float* rowbuf = (float*)(ord + npg);  // npg * nopt (sorted copy)

  const int sg = blockIdx.x;
  const int s = sg / G;
  const int wi = lcs[nps - 1];
  float* X = cx + (long long)sg * npg * nopt;
  float* F = cf + (long long)sg * npg;

  const float f_ref = fall[sg];
  const float f_con = fall[S * G + sg];
  const float f_rnd = fall[2 * S * G + sg];
  const float fw = F[wi];
  const bool use_con = f_ref > fw;
  const bool use_rnd = use_con && (f_con > fw);
  const float fnew = use_rnd ? f_rnd : (use_con ? f_con : f_ref);
  const float* snew = use_rnd ? (cand + ((long long)(2 * S * G) + sg) * nopt)
                      : use_con ? (cand + ((long long)(S * G) + sg) * nopt)
                                : (cand + (long long)sg * nopt);
  if (threadIdx.x == 0)
    atomicAdd(&icall[s], 1 + (use_con ? 1 : 0) + (use_rnd ? 1 : 0));
  if (!act[s]) return;

  // replace worst simplex point
  for (int d = threadIdx.x; d < nopt; d += blockDim.x) X[(long long)wi * nopt + d] = snew[d];
  if (threadIdx.x == 0) F[wi] = fnew;
  __syncthreads();

  // re-sort the complex ascending by objective (stable insertion order:
  // equal keys keep their index order, matching torch.argsort(stable))
  if (threadIdx.x == 0) {
    for (int i = 0; i < npg; ++i) {
      keys[i] = F[i];
      ord[i] = i;
    }
    for (int i = 1; i < npg; ++i) {
      const float kv = keys[i];
      const int ov = ord[i];
      int j = i - 1;
      while (j >= 0 && keys[j] > kv) {
        keys[j + 1] = keys[j];
        ord[j + 1] = ord[j];
        --j;
      }
      keys[j + 1] = kv;
      ord[j + 1] = ov;
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < npg * nopt; idx += blockDim.x)
    rowbuf[idx] = X[(long long)ord[idx / nopt] * nopt + idx % nopt];
  __syncthreads();
  for (int idx = threadIdx.x; idx < npg * nopt; idx += blockDim.x)
    X[idx] = rowbuf[idx];
  for (int i = threadIdx.x; i < npg; i += blockDim.x) F[i] = keys[i];
}

__global__ void sceua_accept_kernel(float* __restrict__ cx,
                                    float* __restrict__ cf,
                                    const float* __restrict__ cand,
                                    const float* __restrict__ fall,
                                    const int* __restrict__ lcs,
                                    const int* __restrict__ act,
                                    int* __restrict__ icall, int S, int G,
                                    int npg, int nopt, int nps) {
  sceua_accept_body(cx, cf, cand, fall, lcs, act, icall, S, G, npg, nopt, nps);
}

// ------------------------------------------------- device-schedule forms
// sched: (nspl, nps + 2) int32, row k = the nps simplex positions of stage k
// followed by the low and high words of its 64-bit Philox seed.
// step: 2 ints. step[0] is the stage counter the host resets to 0 with each
// shuffle's schedule; step[1] is the hand-over word. Both kernels run S*G
// blocks that all read the counter, so neither increments the word its own
// blocks read: propose reads step[0] and posts step[0] + 1 in step[1];
// accept reads step[1] and, as its last act, stores it to step[0]. Kernel
// boundaries order the two. A counter outside [0, nspl) (more replays than
// the schedule has rows) is clamped: it can cost a wrong stage, never an
// out-of-bounds read.
__global__ void sceua_propose_sched_kernel(
    const float* __restrict__ cx, const int* __restrict__ sched,
    int* __restrict__ step, const float* __restrict__ bl,
    const float* __restrict__ bu, float* __restrict__ cand, int S, int G,
    int npg, int nopt, int nps, int nspl) {
  const int k = step[0];
  const int* row = sched + (long long)min(max(k, 0), nspl - 1) * (nps + 2);
  const unsigned long long seed =
      (unsigned long long)(unsigned)row[nps] |
      ((unsigned long long)(unsigned)row[nps + 1] << 32);
  sceua_propose_body(cx, row, bl, bu, cand, S, G, npg, nopt, nps, seed);
  if (blockIdx.x == 0 && threadIdx.x == 0) step[1] = k + 1;
}

__global__ void sceua_accept_sched_kernel(
    float* __restrict__ cx, float* __restrict__ cf,
    const float* __restrict__ cand, const float* __restrict__ fall,
    const int* __restrict__ sched, int* __restrict__ step,
    const int* __restrict__ act, int* __restrict__ icall, int S, int G,
    int npg, int nopt, int nps, int nspl) {
  const int k1 = step[1];
  const int* row = sched + (long long)min(max(k1 - 1, 0), nspl - 1) * (nps + 2);
  sceua_accept_body(cx, cf, cand, fall, row, act, icall, S, G, npg, nopt, nps);
  if (blockIdx.x == 0 && threadIdx.x == 0) step[0] = k1;
}

// ------------------------------------------------------- shuffle boundary
// Un-partition the complexes into the population: x[s, p*G + g, :] =
// cx[s, g, p, :], xf[s, p*G + g] = cf[s, g, p] (the permute + reshape copies
// of models/sceua.py). One block per stream.
__global__ void sceua_unpartition_kernel(const float* __restrict__ cx,
                                         const float* __restrict__ cf,
                                         float* __restrict__ x,
                                         float* __restrict__ xf, int G,
                                         int npg, int nopt) {
  const int s = blockIdx.x;
  const int npt = G * npg;
  const float* cxs = cx + (long long)s * npt * nopt;
  const float* cfs = cf + (long long)s * npt;
  float* xs = x + (long long)s * npt * nopt;
  float* xfs = xf + (long long)s * npt;
  for (int idx = threadIdx.x; idx < npt * nopt; idx += blockDim.x) {
    const int r = idx / nopt, d = idx % nopt;
    const int p = r / G, g = r % G;
    xs[idx] = cxs[((long long)g * npg + p) * nopt + d];
  }
  for (int r = threadIdx.x; r < npt; r += blockDim.x)
    xfs[r] = cfs[(r % G) * npg + r / G];
}

// After the global sort: gather the population by the sort order into the
// sorted population (xs, xfs), partition it back into the complexes (cx, cf)
// and write the termination pack, per stream s a row of 2 + 2 nopt floats:
// [icall[s], best f, max over the population per dimension, min per
// dimension]. Max and min are exact and order-independent; the host finishes
// the geometric range from them. One block of SCEUA_PACK_TPB threads per
// stream; LDS: 2 * SCEUA_PACK_TPB floats.
#define SCEUA_PACK_TPB 256
__global__ void sceua_partition_pack_kernel(
    const float* __restrict__ x, const float* __restrict__ xf,
    const long long* __restrict__ order, const int* __restrict__ icall,
    float* __restrict__ xs, float* __restrict__ xfs, float* __restrict__ cx,
    float* __restrict__ cf, float* __restrict__ pack, int G, int npg,
    int nopt) {
  __shared__ float pmax[SCEUA_PACK_TPB];
  __shared__ float pmin[SCEUA_PACK_TPB];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int npt = G * npg;
  const float* x_s = x + (long long)s * npt * nopt;
  const float* xf_s = xf + (long long)s * npt;
  const long long* o = order + (long long)s * npt;
  float* xs_s = xs + (long long)s * npt * nopt;
  float* cx_s = cx + (long long)s * npt * nopt;
  float* row = pack + (long long)s * (2 + 2 * nopt);
  for (int idx = tid; idx < npt * nopt; idx += SCEUA_PACK_TPB) {
    const int r = idx / nopt, d = idx % nopt;
    const float v = x_s[o[r] * nopt + d];
    xs_s[idx] = v;
    cx_s[((long long)(r % G) * npg + r / G) * nopt + d] = v;
  }
  for (int r = tid; r < npt; r += SCEUA_PACK_TPB) {
    const float f = xf_s[o[r]];
    xfs[(long long)s * npt + r] = f;
    cf[(long long)s * npt + (r % G) * npg + r / G] = f;
    if (r == 0) {
      row[0] = (float)icall[s];
      row[1] = f;
    }
  }
  // per-dimension extrema of the (unsorted: same set) population. The
  // block's threads form `chunks` groups of nopt; group c walks rows c,
  // c + chunks, ..., thread (c, d) keeps dimension d.
  for (int d0 = 0; d0 < nopt; d0 += SCEUA_PACK_TPB) {
    const int width = min(nopt - d0, SCEUA_PACK_TPB);
    const int chunks = SCEUA_PACK_TPB / width;
    const int c = tid / width, d = d0 + tid % width;
    float mx = -INFINITY, mn = INFINITY;
    if (c < chunks)
      for (int r = c; r < npt; r += chunks) {
        const float v = x_s[(long long)r * nopt + d];
        mx = fmaxf(mx, v);
        mn = fminf(mn, v);
      }
    pmax[tid] = mx;
    pmin[tid] = mn;
    __syncthreads();
    if (c == 0) {
      for (int k = 1; k < chunks; ++k) {
        mx = fmaxf(mx, pmax[k * width + tid]);
        mn = fminf(mn, pmin[k * width + tid]);
      }
      row[2 + d] = mx;
      row[2 + nopt + d] = mn;
    }
    __syncthreads();
  }
}

extern "C" void launch_sceua_propose(const float* cx, const int* lcs,
                                     const float* bl, const float* bu,
                                     float* cand, int S, int G, int npg,
                                     int nopt, int nps,
                                     unsigned long long seed,
                                     hipStream_t stream) {
  hipLaunchKernelGGL(sceua_propose_kernel, dim3(S * G), dim3(SCEUA_TPB), 0,
                     stream, cx, lcs, bl, bu, cand, S, G, npg, nopt, nps,
                     seed);
}

// LDS of the accept kernels; above 60 KiB the caller uses the torch stage path
static inline size_t sceua_accept_lds(int npg, int nopt) {
  return (size_t)npg * sizeof(float) + npg * sizeof(int) +
         (size_t)npg * nopt * sizeof(float);
}

extern "C" int launch_sceua_accept(float* cx, float* cf, const float* cand,
                                   const float* fall, const int* lcs,
                                   const int* act, int* icall, int S, int G,
                                   int npg, int nopt, int nps,
                                   hipStream_t stream) {
  const size_t lds = sceua_accept_lds(npg, nopt);
  if (lds > 60 * 1024) return -1;
  hipLaunchKernelGGL(sceua_accept_kernel, dim3(S * G), dim3(SCEUA_TPB), lds,
                     stream, cx, cf, cand, fall, lcs, act, icall, S, G, npg,
                     nopt, nps);
  return 0;
}

extern "C" void launch_sceua_propose_sched(const float* cx, const int* sched,
                                           int* step, const float* bl,
                                           const float* bu, float* cand,
                                           int S, int G, int npg, int nopt,
                                           int nps, int nspl,
                                           hipStream_t stream) {
  hipLaunchKernelGGL(sceua_propose_sched_kernel, dim3(S * G), dim3(SCEUA_TPB),
                     0, stream, cx, sched, step, bl, bu, cand, S, G, npg, nopt,
                     nps, nspl);
}

extern "C" int launch_sceua_accept_sched(float* cx, float* cf,
                                         const float* cand, const float* fall,
                                         const int* sched, int* step,
                                         const int* act, int* icall, int S,
                                         int G, int npg, int nopt, int nps,
                                         int nspl, hipStream_t stream) {
  const size_t lds = sceua_accept_lds(npg, nopt);
  if (lds > 60 * 1024) return -1;
  hipLaunchKernelGGL(sceua_accept_sched_kernel, dim3(S * G), dim3(SCEUA_TPB),
                     lds, stream, cx, cf, cand, fall, sched, step, act, icall,
                     S, G, npg, nopt, nps, nspl);
  return 0;
}

extern "C" void launch_sceua_unpartition(const float* cx, const float* cf,
                                         float* x, float* xf, int S, int G,
                                         int npg, int nopt,
                                         hipStream_t stream) {
  hipLaunchKernelGGL(sceua_unpartition_kernel, dim3(S), dim3(SCEUA_PACK_TPB),
                     0, stream, cx, cf, x, xf, G, npg, nopt);
}

extern "C" void launch_sceua_partition_pack(
    const float* x, const float* xf, const long long* order, const int* icall,
    float* xs, float* xfs, float* cx, float* cf, float* pack, int S, int G,
    int npg, int nopt, hipStream_t stream) {
  hipLaunchKernelGGL(sceua_partition_pack_kernel, dim3(S),
                     dim3(SCEUA_PACK_TPB), 0, stream, x, xf, order, icall, xs,
                     xfs, cx, cf, pack, G, npg, nopt);
}
