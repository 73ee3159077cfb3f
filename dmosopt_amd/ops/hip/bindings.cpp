// PyTorch bindings for the dmosopt_amd gfx950 kernels.

#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <algorithm>
#include <vector>

#include "launchers.h"

#define CHECK_GPU(x) \
  TORCH_CHECK(x.is_cuda(), #x " must be a GPU tensor"); \
  TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

static hipStream_t cur_stream() {
  return (hipStream_t)c10::hip::getCurrentHIPStream().stream();
}

static int nu_code(double nu) {
  if (nu == 0.5) return 1;
  if (nu == 1.5) return 3;
  if (nu == 2.5) return 5;
  return 0;  // RBF / inf
}

// ------------------------------------------------------------------ GP ops
// The GP entry points share one argument check and one function per pipeline
// stage, so those that promise the same bits queue the same launches by
// construction. `fn` is the Python-visible name in the error messages. The
// checks are flag reads: gp_predict_mean runs once per generation.
struct GpArgs {
  const char* fn;
  const torch::Tensor &X, &theta;  // (N,D), (B,p)
  int nu;
  bool aniso;
  int64_t N, D, B, p;
  const float *q_lb, *q_invrg;  // per-dim affine of raw queries, or null
};

static void gp_check_f32(const char* fn, const char* name,
                         const torch::Tensor& t) {
  TORCH_CHECK(t.is_cuda(), fn, ": ", name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, fn, ": ", name,
              " must be float32");
}

static void gp_check_launch(const char* fn, const char* stage) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, fn, ": ", stage, " launch failed: ",
              hipGetErrorString(err));
}

static GpArgs gp_check_args(
    const char* fn, const torch::Tensor& X, const torch::Tensor& theta,
    double nu, bool aniso,
    const c10::optional<torch::Tensor>& q_lb = c10::nullopt,
    const c10::optional<torch::Tensor>& q_invrg = c10::nullopt) {
  gp_check_f32(fn, "X", X);
  gp_check_f32(fn, "theta", theta);
  TORCH_CHECK(X.dim() == 2 && theta.dim() == 2, fn,
              ": X (N,D) and theta (B,p) required");
  const int64_t N = X.size(0), D = X.size(1), B = theta.size(0),
                p = theta.size(1);
  TORCH_CHECK(N >= 1 && B >= 1 && D >= 1, fn, ": empty input");
  TORCH_CHECK(p == (aniso ? D + 2 : 3), fn,
              ": theta width does not match the kernel");
  TORCH_CHECK(q_lb.has_value() == q_invrg.has_value(), fn,
              ": q_lb and q_invrg come together");
  if (q_lb) {
    gp_check_f32(fn, "q_lb", *q_lb);
    gp_check_f32(fn, "q_invrg", *q_invrg);
    TORCH_CHECK(q_lb->numel() == D && q_invrg->numel() == D, fn,
                ": q_lb/q_invrg must be float32 (D,)");
  }
  return {fn, X, theta, nu_code(nu), aniso, N, D, B, p,
          q_lb ? q_lb->data_ptr<float>() : nullptr,
          q_lb ? q_invrg->data_ptr<float>() : nullptr};
}

// Targets of the NMLL calls: (N,) shared by all candidates or (B,N) rows.
static void gp_check_targets(const GpArgs& g, const torch::Tensor& y) {
  gp_check_f32(g.fn, "y", y);
  TORCH_CHECK((y.dim() == 1 && y.size(0) == g.N) ||
                  (y.dim() == 2 && y.size(0) == g.B && y.size(1) == g.N),
              g.fn, ": y must be (N,) or (B,N)");
}

// Query-side arguments of the predict calls.
static void gp_check_query(const GpArgs& g, const torch::Tensor& Xq,
                           const torch::Tensor& alpha,
                           const torch::Tensor& y_mean,
                           const torch::Tensor& y_std) {
  gp_check_f32(g.fn, "Xq", Xq);
  gp_check_f32(g.fn, "alpha", alpha);
  gp_check_f32(g.fn, "y_mean", y_mean);
  gp_check_f32(g.fn, "y_std", y_std);
  TORCH_CHECK(Xq.dim() == 2 && Xq.size(0) >= 1, g.fn,
              ": Xq (P,D) with P >= 1 required");
  TORCH_CHECK(Xq.size(1) == g.D, g.fn, ": Xq/X width mismatch");
  TORCH_CHECK(alpha.numel() == g.B * g.N && y_mean.numel() == g.B &&
                  y_std.numel() == g.B,
              g.fn, ": alpha/y_mean/y_std shape mismatch");
}

// Kernel matrix (B,P,N) of Xq (P,D) against X; `form` is the launcher's
// `symmetric` (0 cross, 1 train, 2 direct-difference cross). grid.z carries B
// and grid.y / grid.x the 32-wide tiles; the kernel indexes its inputs with
// ints and stages two 32 x (D|1) slabs in the default 64 KiB of LDS.
static void gp_check_assemble(const GpArgs& g, int64_t P) {
  TORCH_CHECK(g.B <= 65535 && (g.N + 31) / 32 <= 65535 &&
                  (P + 31) / 32 <= 65535 && P * g.D < (1LL << 31) &&
                  g.N * g.D < (1LL << 31) && g.D <= 254,
              g.fn, ": shape exceeds the launch bounds (B <= 65535, N and P "
              "<= 2097120, D <= 254)");
}

static void gp_assemble_into(const GpArgs& g, const torch::Tensor& Xq, int nu,
                             int form, float jitter, torch::Tensor& K) {
  const int64_t P = Xq.size(0);
  gp_check_assemble(g, P);
  launch_matern_assemble_affine(
      Xq.data_ptr<float>(), g.X.data_ptr<float>(), g.theta.data_ptr<float>(),
      K.data_ptr<float>(), g.B, P, g.N, g.D, g.p, jitter, nu, g.aniso ? 1 : 0,
      form, form == 1 ? nullptr : g.q_lb, form == 1 ? nullptr : g.q_invrg,
      cur_stream());
  gp_check_launch(g.fn, "kernel assembly");
}

static torch::Tensor gp_assemble(const GpArgs& g, const torch::Tensor& Xq,
                                 int nu, int form, float jitter) {
  auto K = torch::empty({g.B, Xq.size(0), g.N}, g.X.options());
  gp_assemble_into(g, Xq, nu, form, jitter, K);
  return K;
}

torch::Tensor matern_train(torch::Tensor X, torch::Tensor theta, double nu,
                           bool aniso, double jitter) {
  const GpArgs g = gp_check_args("matern_train", X, theta, nu, aniso);
  return gp_assemble(g, X, g.nu, 1, (float)jitter);
}

torch::Tensor matern_cross(torch::Tensor Xq, torch::Tensor X,
                           torch::Tensor theta, double nu, bool aniso) {
  const GpArgs g = gp_check_args("matern_cross", X, theta, nu, aniso);
  gp_check_f32(g.fn, "Xq", Xq);
  TORCH_CHECK(Xq.dim() == 2 && Xq.size(1) == g.D, g.fn, ": Xq/X width mismatch");
  return gp_assemble(g, Xq, g.nu, 0, 0.f);
}

static float gp_nmll_const(int N) {
  return 0.5f * (float)N * 1.8378770664093453f;  // N/2 log(2*pi)
}

// Back half of the NMLL value pipeline on initialised buffers (K assembled,
// Z = y rows, info = 0): factor with the fused forward solve, or factor and
// solve separately where the fused route does not apply, then the reduction.
static void gp_nmll_factor_reduce(const GpArgs& g, torch::Tensor& K,
                                  torch::Tensor& logdet, torch::Tensor& info,
                                  torch::Tensor& Z, torch::Tensor& out) {
  auto stream = cur_stream();
  const int B = g.B, N = g.N;
  // fused factor+solve: the rhs rides the multik launch chain (panel solves
  // its 32-entry segment, the SYRK's diagonal tiles apply the trailing
  // update) — no separate ~61 us serial TRSV kernel per NMLL
  if (launch_cholesky_fused_solve(K.data_ptr<float>(),
                                  logdet.data_ptr<float>(),
                                  info.data_ptr<int>(), Z.data_ptr<float>(),
                                  B, N, stream) != 0) {
    launch_cholesky_batched(K.data_ptr<float>(), logdet.data_ptr<float>(),
                            info.data_ptr<int>(), B, N, stream);
    launch_forward_solve_batched(K.data_ptr<float>(), Z.data_ptr<float>(), B,
                                 N, 1, stream);
  }
  launch_nmll_reduce(Z.data_ptr<float>(), logdet.data_ptr<float>(),
                     info.data_ptr<int>(), out.data_ptr<float>(), B, N,
                     gp_nmll_const(N), stream);
  gp_check_launch(g.fn, "NMLL pipeline");
}

// NMLL value pipeline: kernel assembly -> batched Cholesky with the forward
// solve of y -> reduction, all queued from ONE python call (the per-stage
// torch dispatch chain was ~40% of the SCE-UA fit's host time). K holds the
// factor L, Z = L^-1 y (B,N,1), info the factorization flags, out the NMLL
// (B,), +inf where the factorization failed.
struct NmllPipeline {
  torch::Tensor K, Z, info, out;
};

static NmllPipeline gp_nmll_pipeline(const GpArgs& g, const torch::Tensor& y,
                                     double jitter) {
  auto K = gp_assemble(g, g.X, g.nu, 1, (float)jitter);
  auto logdet = torch::empty({g.B}, g.X.options());
  auto info = torch::zeros({g.B}, g.X.options().dtype(torch::kInt32));
  // the solve runs in place on Z. With B = 1 the expanded view of a shared y
  // is already contiguous, contiguous() hands back y's own storage, and the
  // caller's y would come back as L^-1 y: that case needs its own copy.
  torch::Tensor Z = (y.dim() == 1)
                        ? (g.B == 1 ? y.unsqueeze(0).clone()
                                    : y.unsqueeze(0).expand({g.B, g.N}).contiguous())
                        : y.contiguous().clone();
  Z = Z.view({g.B, g.N, 1});
  auto out = torch::empty({g.B}, g.X.options());
  gp_nmll_factor_reduce(g, K, logdet, info, Z, out);
  return {K, Z, info, out};
}

// The same NMLL values (bit for bit) into CALLER-OWNED buffers K (B,N,N),
// Z (B,N), logdet (B,), info (B,) int32, out (B,): no allocation, so a
// captured graph of it owns nothing behind the caller's back. Where the
// look-ahead fused-solve route applies (N > 32, B <= 48, no switch against
// it) the prologue rides the assemble launch and the reduction the last step
// launch: ceil(N/32) + 1 launches, none of them a fill, a copy or a reduce.
// Elsewhere: today's launches on the caller's buffers. The buffers' previous
// contents are never read.
void gp_nmll_into(torch::Tensor X, torch::Tensor theta, torch::Tensor y,
                  torch::Tensor K, torch::Tensor Z, torch::Tensor logdet,
                  torch::Tensor info, torch::Tensor out, double nu, bool aniso,
                  double jitter) {
  const GpArgs g = gp_check_args("gp_nmll_into", X, theta, nu, aniso);
  gp_check_targets(g, y);
  gp_check_f32(g.fn, "K", K);
  gp_check_f32(g.fn, "Z", Z);
  gp_check_f32(g.fn, "logdet", logdet);
  gp_check_f32(g.fn, "out", out);
  TORCH_CHECK(info.is_cuda() && info.is_contiguous() &&
                  info.scalar_type() == torch::kInt32,
              g.fn, ": info must be a contiguous int32 GPU tensor");
  TORCH_CHECK(K.numel() == g.B * g.N * g.N && Z.numel() == g.B * g.N &&
                  logdet.numel() == g.B && info.numel() == g.B &&
                  out.numel() == g.B,
              g.fn, ": K (B,N,N), Z (B,N), logdet/info/out (B,) required");
  const int B = g.B, N = g.N;
  if (cholesky_nmll_chain_applies(B, N)) {
    gp_check_assemble(g, g.N);
    auto stream = cur_stream();
    launch_matern_train_prologue(
        X.data_ptr<float>(), theta.data_ptr<float>(), K.data_ptr<float>(), B,
        N, g.D, g.p, (float)jitter, g.nu, aniso ? 1 : 0, y.data_ptr<float>(),
        y.dim() == 1 ? 0 : N, Z.data_ptr<float>(), logdet.data_ptr<float>(),
        info.data_ptr<int>(), stream);
    launch_cholesky_nmll_chain(K.data_ptr<float>(), logdet.data_ptr<float>(),
                               info.data_ptr<int>(), Z.data_ptr<float>(),
                               out.data_ptr<float>(), B, N, gp_nmll_const(N),
                               stream);
    gp_check_launch(g.fn, "NMLL pipeline");
    return;
  }
  gp_assemble_into(g, g.X, g.nu, 1, (float)jitter, K);
  info.zero_();
  Z.view({g.B, g.N}).copy_(y.dim() == 1 ? y.unsqueeze(0).expand({g.B, g.N})
                                        : y);
  gp_nmll_factor_reduce(g, K, logdet, info, Z, out);
}

// Fused GP negative log marginal likelihood for a batch of theta.
// y: (N,) shared or (B, N) per-candidate.
torch::Tensor gp_nmll(torch::Tensor X, torch::Tensor theta, torch::Tensor y,
                      double nu, bool aniso, double jitter) {
  const GpArgs g = gp_check_args("gp_nmll", X, theta, nu, aniso);
  gp_check_targets(g, y);
  return gp_nmll_pipeline(g, y, jitter).out;
}

// Fused NMLL value AND analytic gradient for a batch of theta. The value is
// gp_nmll's pipeline; the gradient stages follow it on the same stream:
// backward solve for alpha, K^-1 by the forward and backward solves on an
// identity right-hand side, then the tile kernels of gp_nmll_grad.hip.
// Returns {nmll (B,), grad (B,p)}; a candidate whose factorization failed
// gets +inf and a zero gradient row.
std::vector<torch::Tensor> gp_nmll_grad(torch::Tensor X, torch::Tensor theta,
                                        torch::Tensor y, double nu,
                                        bool aniso, double jitter) {
  const GpArgs g = gp_check_args("gp_nmll_grad", X, theta, nu, aniso);
  gp_check_targets(g, y);
  // grid.y carries the N right-hand sides of the K^-1 solves; the gradient
  // kernel's slabs of a tile pair (2 x 32 x (D|1) floats) stay inside the
  // default 64 KiB of LDS
  TORCH_CHECK(g.N <= 65535 && g.D <= 128, g.fn,
              ": shape exceeds the launch bounds of the gradient stages "
              "(N <= 65535, D <= 128)");
  auto v = gp_nmll_pipeline(g, y, jitter);
  auto stream = cur_stream();
  const int B = g.B, N = g.N;
  // alpha = L^-T z, in place (the reduce has read z)
  launch_backward_solve_batched(v.K.data_ptr<float>(), v.Z.data_ptr<float>(),
                                B, N, 1, stream);
  auto Kinv = torch::empty({g.B, g.N, g.N}, X.options());
  int rc = launch_gp_fill_identity(Kinv.data_ptr<float>(), B, N, stream);
  TORCH_CHECK(rc == 0, g.fn, ": identity fill launch failed: ",
              hipGetErrorString((hipError_t)rc));
  launch_forward_solve_batched(v.K.data_ptr<float>(), Kinv.data_ptr<float>(),
                               B, N, N, stream);
  launch_backward_solve_batched(v.K.data_ptr<float>(), Kinv.data_ptr<float>(),
                                B, N, N, stream);
  gp_check_launch(g.fn, "solve");
  auto part =
      torch::empty({g.B, (int64_t)gp_nmll_grad_tiles(N), g.p}, X.options());
  auto grad = torch::empty({g.B, g.p}, X.options());
  rc = launch_gp_nmll_grad(
      X.data_ptr<float>(), theta.data_ptr<float>(), Kinv.data_ptr<float>(),
      v.Z.data_ptr<float>(), v.out.data_ptr<float>(), v.info.data_ptr<int>(),
      part.data_ptr<float>(), grad.data_ptr<float>(), B, N, g.D, g.p, g.nu,
      aniso ? 1 : 0, stream);
  TORCH_CHECK(rc == 0, g.fn, ": gradient kernel launch failed: ",
              hipGetErrorString((hipError_t)rc));
  return {v.out, grad};
}

// Predict front end: the affine cross kernel Ks (B,P,N), then the fused
// matvec + de-standardization into columns [0, B) of a fresh (P, cols) block,
// cols being the output row stride: one kernel instead of bmm + addcmul +
// transpose-contiguous. The gemv indexes its rows with ints.
struct PredictFront {
  torch::Tensor Ks, out;
};

static PredictFront gp_predict_front(const GpArgs& g, const torch::Tensor& Xq,
                                     const torch::Tensor& alpha,
                                     const torch::Tensor& y_mean,
                                     const torch::Tensor& y_std,
                                     int64_t cols) {
  gp_check_query(g, Xq, alpha, y_mean, y_std);
  const int64_t P = Xq.size(0);
  TORCH_CHECK(g.B * P < (1LL << 31), g.fn,
              ": shape exceeds the launch bounds (B * P < 2^31)");
  auto Ks = gp_assemble(g, Xq, g.nu, 0, 0.0f);
  auto out = torch::empty({P, cols}, g.X.options());
  launch_gp_mean_gemv(Ks.data_ptr<float>(), alpha.data_ptr<float>(),
                      y_mean.data_ptr<float>(), y_std.data_ptr<float>(),
                      out.data_ptr<float>(), g.B, P, g.N, cols, cur_stream());
  gp_check_launch(g.fn, "mean gemv");
  return {Ks, out};
}

// Fused posterior-mean predict for the inner-MOEA surrogate evaluate, (P, B),
// queued from one python call (the torch op chain costs ~0.1 ms of dispatch
// per generation). q_lb / q_invrg normalize RAW queries inside the kernel
// load; without them Xq must already be normalized to the unit box.
torch::Tensor gp_predict_mean(torch::Tensor Xq, torch::Tensor X,
                              torch::Tensor theta, torch::Tensor alpha,
                              torch::Tensor y_mean, torch::Tensor y_std,
                              double nu, bool aniso,
                              c10::optional<torch::Tensor> q_lb = c10::nullopt,
                              c10::optional<torch::Tensor> q_invrg = c10::nullopt) {
  const GpArgs g =
      gp_check_args("gp_predict_mean", X, theta, nu, aniso, q_lb, q_invrg);
  return gp_predict_front(g, Xq, alpha, y_mean, y_std, g.B).out;
}

// Posterior mean AND its gradient in the query point: {mean (P,B), jac
// (P,B,D)}, jac[p,b,d] = d mean[p,b] / d Xq[p,d] in the units the queries
// come in (raw with q_lb / q_invrg, unit box without). The mean is
// gp_predict_mean's front end; the gradient kernels (gp_mean_grad.hip) read
// only X, theta and alpha. Their (B, S, P, D) scratch is bounded by slicing P:
// a query's gradient does not depend on its slice.
std::vector<torch::Tensor> gp_predict_mean_grad(
    torch::Tensor Xq, torch::Tensor X, torch::Tensor theta,
    torch::Tensor alpha, torch::Tensor y_mean, torch::Tensor y_std, double nu,
    bool aniso, c10::optional<torch::Tensor> q_lb = c10::nullopt,
    c10::optional<torch::Tensor> q_invrg = c10::nullopt) {
  const GpArgs g =
      gp_check_args("gp_predict_mean_grad", X, theta, nu, aniso, q_lb, q_invrg);
  // the gradient kernel's phase 2 gives a thread 16 of the D dimensions
  TORCH_CHECK(g.D <= 128, g.fn,
              ": shape exceeds the launch bounds of the gradient stage "
              "(D <= 128)");
  auto f = gp_predict_front(g, Xq, alpha, y_mean, y_std, g.B);
  const int64_t P = Xq.size(0), S = gp_mean_grad_splits((int)g.N);
  auto jac = torch::empty({P, g.B, g.D}, X.options());
  // at most 64 MiB of partials per slice, whole 32-query tiles
  const int64_t per_query = g.B * S * g.D * (int64_t)sizeof(float);
  const int64_t slice =
      std::min(P, std::max<int64_t>(32, ((64LL << 20) / per_query) / 32 * 32));
  auto part = torch::empty({g.B, S, slice, g.D}, X.options());
  for (int64_t p0 = 0; p0 < P; p0 += slice) {
    const int64_t Pc = std::min(slice, P - p0);
    const int rc = launch_gp_mean_grad(
        Xq.data_ptr<float>() + p0 * g.D, X.data_ptr<float>(),
        theta.data_ptr<float>(), alpha.data_ptr<float>(),
        y_std.data_ptr<float>(), part.data_ptr<float>(),
        jac.data_ptr<float>() + p0 * g.B * g.D, g.B, Pc, g.N, g.D, g.p, g.nu,
        aniso ? 1 : 0, g.q_lb, g.q_invrg, cur_stream());
    TORCH_CHECK(rc == 0, g.fn, ": gradient kernel launch failed: ",
                hipGetErrorString((hipError_t)rc));
  }
  return {f.out, jac};
}

// One posterior sample path per batch row at the queries, (P, B):
//   y_mean_b + y_std_b * (k_b(u, X) alpha_path_b + sum_j amp_bj
//                         cos(2 pi (tau_bj + Omega_bj . u))).
// The Matheron-update term is gp_predict_mean's front end with alpha_path
// (the same launches, so amp = 0 gives gp_predict_mean's bits); the
// random-feature kernels (gp_path.hip) then add their term into that block.
// Omega (B,M,D) in turns per unit of the normalised query, tau (B,M) in
// turns, amp (B,M). The (B, S, P) scratch is bounded by slicing P: a
// query's value does not depend on its slice.
torch::Tensor gp_predict_path(
    torch::Tensor Xq, torch::Tensor X, torch::Tensor theta,
    torch::Tensor alpha_path, torch::Tensor y_mean, torch::Tensor y_std,
    double nu, bool aniso, torch::Tensor Omega, torch::Tensor tau,
    torch::Tensor amp, c10::optional<torch::Tensor> q_lb = c10::nullopt,
    c10::optional<torch::Tensor> q_invrg = c10::nullopt) {
  const GpArgs g =
      gp_check_args("gp_predict_path", X, theta, nu, aniso, q_lb, q_invrg);
  gp_check_f32(g.fn, "Omega", Omega);
  gp_check_f32(g.fn, "tau", tau);
  gp_check_f32(g.fn, "amp", amp);
  TORCH_CHECK(Omega.dim() == 3 && Omega.size(0) == g.B && Omega.size(2) == g.D,
              g.fn, ": Omega must be (B,M,D)");
  const int64_t M = Omega.size(1);
  TORCH_CHECK(tau.numel() == g.B * M && amp.numel() == g.B * M, g.fn,
              ": tau and amp must be (B,M)");
  // the feature kernel stages a 32-query and a 64-feature slab of D|1 floats
  // in the default 64 KiB of LDS; grid.y carries the feature chunks
  TORCH_CHECK(g.D <= 128 && g.B <= 65535 && M >= 1 && M <= 4194240, g.fn,
              ": shape exceeds the launch bounds of the feature stage "
              "(D <= 128, B <= 65535, 1 <= M <= 4194240)");
  const int64_t S = gp_path_splits((int)M);
  auto f = gp_predict_front(g, Xq, alpha_path, y_mean, y_std, g.B);
  const int64_t P = Xq.size(0);
  // at most 64 MiB of partials per slice, whole 32-query tiles
  const int64_t per_query = g.B * S * (int64_t)sizeof(float);
  const int64_t slice =
      std::min(P, std::max<int64_t>(32, ((64LL << 20) / per_query) / 32 * 32));
  auto part = torch::empty({g.B, S, slice}, X.options());
  for (int64_t p0 = 0; p0 < P; p0 += slice) {
    const int64_t Pc = std::min(slice, P - p0);
    const int rc = launch_gp_path(
        Xq.data_ptr<float>() + p0 * g.D, Omega.data_ptr<float>(),
        tau.data_ptr<float>(), amp.data_ptr<float>(), y_std.data_ptr<float>(),
        part.data_ptr<float>(), f.out.data_ptr<float>() + p0 * g.B, (int)g.B,
        (int)Pc, (int)M, (int)g.D, (int)g.B, g.q_lb, g.q_invrg, cur_stream());
    TORCH_CHECK(rc == 0, g.fn, ": feature kernel launch failed: ",
                hipGetErrorString((hipError_t)rc));
  }
  return f.out;
}

// Fused mean + variance predict (optimize_mean_variance mode): the front end
// of gp_predict_mean writes the left half of the (P, 2B) block, and the
// |Linv k*|^2 variance kernels (gp_variance.hip) read the same cross kernel
// and write the right half. var_decimals >= 0 rounds the variance columns to
// that many decimals in the epilogue.
torch::Tensor gp_predict_mean_var(
    torch::Tensor Xq, torch::Tensor X, torch::Tensor theta,
    torch::Tensor alpha, torch::Tensor Linv, torch::Tensor y_mean,
    torch::Tensor y_std, double nu, bool aniso,
    c10::optional<torch::Tensor> q_lb = c10::nullopt,
    c10::optional<torch::Tensor> q_invrg = c10::nullopt,
    int64_t var_decimals = -1) {
  const GpArgs g =
      gp_check_args("gp_predict_mean_var", X, theta, nu, aniso, q_lb, q_invrg);
  gp_check_f32(g.fn, "Linv", Linv);
  TORCH_CHECK(Linv.dim() == 3 && Linv.size(0) == g.B && Linv.size(1) == g.N &&
                  Linv.size(2) == g.N,
              g.fn, ": Linv must be (B,N,N)");
  TORCH_CHECK(var_decimals <= 9, g.fn, ": var_decimals <= 9");
  auto f = gp_predict_front(g, Xq, alpha, y_mean, y_std, 2 * g.B);
  // nu = 1/2 only: its kernel has an infinite slope in d2 at 0, so the
  // ~1e-7 cancellation of the norms-form d2 costs ~7e-4 of variance at a
  // query on a training point. The variance then reads a direct-difference
  // cross kernel; the mean keeps the norms form (gp_predict_mean's bits).
  torch::Tensor Kv = g.nu == 1 ? gp_assemble(g, Xq, 1, 2, 0.0f) : f.Ks;
  const int64_t P = Xq.size(0), T = (g.N + 31) / 32;  // one partial per row tile
  auto part = torch::empty({g.B, T, P}, X.options());
  float scale = 0.f;  // 0 = no rounding
  if (var_decimals >= 0) {
    scale = 1.f;
    for (int64_t i = 0; i < var_decimals; ++i) scale *= 10.f;
  }
  const int rc = launch_gp_variance(
      Linv.data_ptr<float>(), Kv.data_ptr<float>(), theta.data_ptr<float>(),
      y_std.data_ptr<float>(), part.data_ptr<float>(), f.out.data_ptr<float>(),
      g.B, P, g.N, g.p, scale, cur_stream());
  TORCH_CHECK(rc == 0, g.fn, ": variance kernel launch failed: ",
              hipGetErrorString((hipError_t)rc));
  return f.out;
}

// Probability of feasibility of a GP regressed on constraint values: the
// (P, B + 1) block [PoF_0 .. PoF_{B-1} | rank], PoF_b = Phi(z_b) with z_b the
// posterior mean over the noise-inclusive posterior deviation, rank their
// mean in column order. gp_predict_mean_var's launches up to the epilogue
// (the means go to a (P, B) scratch block), then the finish of gp_pof.hip.
torch::Tensor gp_predict_pof(
    torch::Tensor Xq, torch::Tensor X, torch::Tensor theta,
    torch::Tensor alpha, torch::Tensor Linv, torch::Tensor y_mean,
    torch::Tensor y_std, double nu, bool aniso,
    c10::optional<torch::Tensor> q_lb = c10::nullopt,
    c10::optional<torch::Tensor> q_invrg = c10::nullopt) {
  const GpArgs g =
      gp_check_args("gp_predict_pof", X, theta, nu, aniso, q_lb, q_invrg);
  gp_check_f32(g.fn, "Linv", Linv);
  TORCH_CHECK(Linv.dim() == 3 && Linv.size(0) == g.B && Linv.size(1) == g.N &&
                  Linv.size(2) == g.N,
              g.fn, ": Linv must be (B,N,N)");
  auto f = gp_predict_front(g, Xq, alpha, y_mean, y_std, g.B);
  // nu = 1/2: the variance reads the direct-difference cross kernel, as in
  // gp_predict_mean_var
  torch::Tensor Kv = g.nu == 1 ? gp_assemble(g, Xq, 1, 2, 0.0f) : f.Ks;
  const int64_t P = Xq.size(0);
  auto part = torch::empty({g.B, (int64_t)gp_var_tiles((int)g.N), P}, X.options());
  auto out = torch::empty({P, g.B + 1}, X.options());
  const int rc = launch_gp_pof(
      Linv.data_ptr<float>(), Kv.data_ptr<float>(), f.out.data_ptr<float>(),
      theta.data_ptr<float>(), y_std.data_ptr<float>(), part.data_ptr<float>(),
      out.data_ptr<float>(), g.B, P, g.N, g.p, cur_stream());
  TORCH_CHECK(rc == 0, g.fn, ": feasibility kernel launch failed: ",
              hipGetErrorString((hipError_t)rc));
  return out;
}

// Fused tournament selection: stable rank sort + Gumbel top-k weighted
// sampling without replacement + pool gather in ONE launch. Returns
// (pool, pool_idx); raises beyond launch_tournament's gate (N <= 2048).
std::vector<torch::Tensor> tournament_pool(torch::Tensor population,
                                           torch::Tensor rank,
                                           int64_t poolsize, double p_sel,
                                           int64_t seed) {
  CHECK_GPU(population);
  TORCH_CHECK(population.dtype() == torch::kFloat32 &&
                  rank.dtype() == torch::kLong,
              "tournament_pool: (float32 population, int64 rank) required");
  TORCH_CHECK(rank.size(0) == population.size(0) &&
                  poolsize <= population.size(0),
              "tournament_pool: shape mismatch");
  const int N = population.size(0), d = population.size(1);
  auto pool = torch::empty({poolsize, d}, population.options());
  auto pool_idx =
      torch::empty({poolsize}, population.options().dtype(torch::kLong));
  const float log1mp = logf(1.0f - (float)p_sel);
  const int rc = launch_tournament(
      population.data_ptr<float>(), (long long*)rank.data_ptr<int64_t>(),
      pool.data_ptr<float>(), (long long*)pool_idx.data_ptr<int64_t>(), N, d,
      (int)poolsize, log1mp, (unsigned long long)seed, cur_stream());
  TORCH_CHECK(rc == 0, "tournament_pool: N = ", N,
              " is beyond the one-workgroup tournament's gate (N <= 2048)");
  return {pool, pool_idx};
}

// Device-side operator-success accounting (no host sync, one launch).
bool survivor_count(torch::Tensor perm, torch::Tensor c_idx,
                    int64_t n_children, torch::Tensor succ_cross,
                    torch::Tensor succ_mut) {
  CHECK_GPU(perm);
  TORCH_CHECK(perm.dtype() == torch::kLong && c_idx.dtype() == torch::kLong &&
                  succ_cross.dtype() == torch::kLong &&
                  succ_mut.dtype() == torch::kLong,
              "survivor_count: int64 tensors required");
  return launch_survivor_count(
             (long long*)perm.data_ptr<int64_t>(), (long long*)c_idx.data_ptr<int64_t>(),
             perm.size(0), c_idx.size(0), (int)n_children,
             (long long*)succ_cross.data_ptr<int64_t>(), (long long*)succ_mut.data_ptr<int64_t>(),
             cur_stream()) == 0;
}

// Event-decoded whole-generation variation (variation_events_kernel):
// same child bits as sbx_batch + mutation_batch, addressed by the per-event
// slot lists so the host never materializes an inverse slot-to-child map.
torch::Tensor variation_events(torch::Tensor pool, torch::Tensor ci,
                               torch::Tensor mi, torch::Tensor p1,
                               torch::Tensor p2, torch::Tensor im,
                               torch::Tensor di_c, torch::Tensor di_m,
                               torch::Tensor lo, torch::Tensor hi,
                               double mutation_rate, int64_t seed_sbx,
                               int64_t seed_mut) {
  CHECK_GPU(pool);
  const int C = p1.size(0), M = im.size(0), d = pool.size(1);
  TORCH_CHECK(pool.dtype() == torch::kFloat32 && ci.dtype() == torch::kLong &&
                  mi.dtype() == torch::kLong && p2.size(0) == C &&
                  ci.size(0) == 2 * (int64_t)C && mi.size(0) == M,
              "variation_events: f32 pool, int64 slot/parent indices");
  auto out = torch::empty({(long)(2 * C + M), d}, pool.options());
  launch_variation_events(
      pool.data_ptr<float>(),
      C ? (long long*)ci.data_ptr<int64_t>() : nullptr,
      M ? (long long*)mi.data_ptr<int64_t>() : nullptr,
      C ? (long long*)p1.data_ptr<int64_t>() : nullptr,
      C ? (long long*)p2.data_ptr<int64_t>() : nullptr,
      M ? (long long*)im.data_ptr<int64_t>() : nullptr,
      di_c.data_ptr<float>(), di_m.data_ptr<float>(), lo.data_ptr<float>(),
      hi.data_ptr<float>(), out.data_ptr<float>(), C, M, d,
      (float)mutation_rate, (unsigned long long)seed_sbx,
      (unsigned long long)seed_mut, cur_stream());
  return out;
}

// Fused SCE-UA CCE stage: candidate proposal and acceptance+resort, one
// extension call each instead of ~30 torch kernels per stage.
torch::Tensor sceua_propose(torch::Tensor cx, torch::Tensor lcs,
                            torch::Tensor bl, torch::Tensor bu, int64_t nps,
                            int64_t seed) {
  CHECK_GPU(cx);
  TORCH_CHECK(cx.dtype() == torch::kFloat32 && cx.dim() == 4 &&
                  lcs.dtype() == torch::kInt32,
              "sceua_propose: cx (S,G,npg,nopt) f32 + int32 lcs required");
  const int S = cx.size(0), G = cx.size(1), npg = cx.size(2),
            nopt = cx.size(3);
  auto cand = torch::empty({3, (long)S * G, nopt}, cx.options());
  launch_sceua_propose(cx.data_ptr<float>(), lcs.data_ptr<int>(),
                       bl.data_ptr<float>(), bu.data_ptr<float>(),
                       cand.data_ptr<float>(), S, G, npg, nopt, (int)nps,
                       (unsigned long long)seed, cur_stream());
  return cand;
}

bool sceua_accept(torch::Tensor cx, torch::Tensor cf, torch::Tensor cand,
                  torch::Tensor fall, torch::Tensor lcs, torch::Tensor act,
                  torch::Tensor icall, int64_t nps) {
  CHECK_GPU(cx);
  const int S = cx.size(0), G = cx.size(1), npg = cx.size(2),
            nopt = cx.size(3);
  return launch_sceua_accept(cx.data_ptr<float>(), cf.data_ptr<float>(),
                             cand.data_ptr<float>(), fall.data_ptr<float>(),
                             lcs.data_ptr<int>(), act.data_ptr<int>(),
                             icall.data_ptr<int>(), S, G, npg, nopt, (int)nps,
                             cur_stream()) == 0;
}

// Device-schedule forms of the two stage kernels and the shuffle-boundary
// kernels (sceua_stage.hip). They write caller-owned buffers only, so a
// captured stage allocates nothing.
struct SceuaDims {
  int S, G, npg, nopt, nps, nspl;
};

static void sceua_check(const char* fn, const char* name,
                        const torch::Tensor& t, torch::ScalarType dt,
                        int64_t numel) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == dt &&
                  t.numel() == numel,
              fn, ": ", name, " has the wrong device, layout, dtype or size");
}

static SceuaDims sceua_check_stage(const char* fn, const torch::Tensor& cx,
                                   const torch::Tensor& sched,
                                   const torch::Tensor& step,
                                   const torch::Tensor& cand) {
  TORCH_CHECK(cx.dim() == 4 && sched.dim() == 2 && sched.size(1) >= 3, fn,
              ": cx (S,G,npg,nopt) and sched (nspl, nps + 2) required");
  const SceuaDims d = {(int)cx.size(0), (int)cx.size(1), (int)cx.size(2),
                       (int)cx.size(3), (int)sched.size(1) - 2,
                       (int)sched.size(0)};
  sceua_check(fn, "cx", cx, torch::kFloat32, cx.numel());
  sceua_check(fn, "sched", sched, torch::kInt32, sched.numel());
  sceua_check(fn, "step", step, torch::kInt32, 2);
  sceua_check(fn, "cand", cand, torch::kFloat32,
              3LL * d.S * d.G * d.nopt);
  TORCH_CHECK(d.nspl >= 1 && d.nps >= 2 && d.nps <= d.npg, fn,
              ": schedule shape does not match the complexes");
  return d;
}

void sceua_propose_sched(torch::Tensor cx, torch::Tensor sched,
                         torch::Tensor step, torch::Tensor bl,
                         torch::Tensor bu, torch::Tensor cand) {
  const char* fn = "sceua_propose_sched";
  const SceuaDims d = sceua_check_stage(fn, cx, sched, step, cand);
  sceua_check(fn, "bl", bl, torch::kFloat32, d.nopt);
  sceua_check(fn, "bu", bu, torch::kFloat32, d.nopt);
  launch_sceua_propose_sched(cx.data_ptr<float>(), sched.data_ptr<int>(),
                             step.data_ptr<int>(), bl.data_ptr<float>(),
                             bu.data_ptr<float>(), cand.data_ptr<float>(),
                             d.S, d.G, d.npg, d.nopt, d.nps, d.nspl,
                             cur_stream());
  gp_check_launch(fn, "propose");
}

void sceua_accept_sched(torch::Tensor cx, torch::Tensor cf,
                        torch::Tensor cand, torch::Tensor fall,
                        torch::Tensor sched, torch::Tensor step,
                        torch::Tensor act, torch::Tensor icall) {
  const char* fn = "sceua_accept_sched";
  const SceuaDims d = sceua_check_stage(fn, cx, sched, step, cand);
  sceua_check(fn, "cf", cf, torch::kFloat32, (int64_t)d.S * d.G * d.npg);
  sceua_check(fn, "fall", fall, torch::kFloat32, 3LL * d.S * d.G);
  sceua_check(fn, "act", act, torch::kInt32, d.S);
  sceua_check(fn, "icall", icall, torch::kInt32, d.S);
  const int rc = launch_sceua_accept_sched(
      cx.data_ptr<float>(), cf.data_ptr<float>(), cand.data_ptr<float>(),
      fall.data_ptr<float>(), sched.data_ptr<int>(), step.data_ptr<int>(),
      act.data_ptr<int>(), icall.data_ptr<int>(), d.S, d.G, d.npg, d.nopt,
      d.nps, d.nspl, cur_stream());
  TORCH_CHECK(rc == 0, fn, ": a complex does not fit the kernel's LDS");
  gp_check_launch(fn, "accept");
}

// (S,G,npg,.) complexes -> (S,npt,.) population, row p*G + g = position p of
// complex g.
void sceua_unpartition(torch::Tensor cx, torch::Tensor cf, torch::Tensor x,
                       torch::Tensor xf) {
  const char* fn = "sceua_unpartition";
  TORCH_CHECK(cx.dim() == 4, fn, ": cx (S,G,npg,nopt) required");
  const int S = cx.size(0), G = cx.size(1), npg = cx.size(2),
            nopt = cx.size(3);
  sceua_check(fn, "cx", cx, torch::kFloat32, cx.numel());
  sceua_check(fn, "cf", cf, torch::kFloat32, (int64_t)S * G * npg);
  sceua_check(fn, "x", x, torch::kFloat32, cx.numel());
  sceua_check(fn, "xf", xf, torch::kFloat32, (int64_t)S * G * npg);
  launch_sceua_unpartition(cx.data_ptr<float>(), cf.data_ptr<float>(),
                           x.data_ptr<float>(), xf.data_ptr<float>(), S, G,
                           npg, nopt, cur_stream());
  gp_check_launch(fn, "un-partition");
}

// Population gathered by `order` (S,npt) int64 -> sorted population (xs,
// xfs), its partition into complexes (cx, cf) and the termination pack
// (S, 2 + 2 nopt): icall, best f, per-dimension max, per-dimension min.
void sceua_partition_pack(torch::Tensor x, torch::Tensor xf,
                          torch::Tensor order, torch::Tensor icall,
                          torch::Tensor xs, torch::Tensor xfs,
                          torch::Tensor cx, torch::Tensor cf,
                          torch::Tensor pack) {
  const char* fn = "sceua_partition_pack";
  TORCH_CHECK(cx.dim() == 4, fn, ": cx (S,G,npg,nopt) required");
  const int S = cx.size(0), G = cx.size(1), npg = cx.size(2),
            nopt = cx.size(3);
  const int64_t rows = (int64_t)S * G * npg;
  sceua_check(fn, "x", x, torch::kFloat32, rows * nopt);
  sceua_check(fn, "xf", xf, torch::kFloat32, rows);
  sceua_check(fn, "order", order, torch::kInt64, rows);
  sceua_check(fn, "icall", icall, torch::kInt32, S);
  sceua_check(fn, "xs", xs, torch::kFloat32, rows * nopt);
  sceua_check(fn, "xfs", xfs, torch::kFloat32, rows);
  sceua_check(fn, "cx", cx, torch::kFloat32, rows * nopt);
  sceua_check(fn, "cf", cf, torch::kFloat32, rows);
  sceua_check(fn, "pack", pack, torch::kFloat32, (int64_t)S * (2 + 2 * nopt));
  launch_sceua_partition_pack(
      x.data_ptr<float>(), xf.data_ptr<float>(),
      (const long long*)order.data_ptr<int64_t>(), icall.data_ptr<int>(),
      xs.data_ptr<float>(), xfs.data_ptr<float>(), cx.data_ptr<float>(),
      cf.data_ptr<float>(), pack.data_ptr<float>(), S, G, npg, nopt,
      cur_stream());
  gp_check_launch(fn, "partition");
}

std::vector<torch::Tensor> cholesky_batched_(torch::Tensor A) {
  CHECK_GPU(A);
  const int B = A.size(0), N = A.size(1);
  auto logdet = torch::empty({B}, A.options());
  auto info = torch::zeros({B}, A.options().dtype(torch::kInt32));
  launch_cholesky_batched(A.data_ptr<float>(), logdet.data_ptr<float>(),
                          info.data_ptr<int>(), B, N, cur_stream());
  return {logdet, info};
}

// Multi-launch factorization with an EXPLICIT trailing-update schedule
// (0 = classic panel + SYRK launches, 1 = look-ahead step launches, 2 = the
// one-launch kernel where it fits, else look-ahead) and an optional rhs
// (B, N) carried through the fused forward solve.
// DMOSOPT_CHOL_LOOKAHEAD is latched per process, so this is the only way to
// compare the two schedules inside one process. In place: A -> L, rhs -> L^-1 rhs.
// factor picks the panel's diagonal factor the same way (0 = lds, 1 = reg,
// -1 = the process default latched from DMOSOPT_CHOL_FACTOR).
std::vector<torch::Tensor> cholesky_multik_sched_(
    torch::Tensor A, c10::optional<torch::Tensor> rhs, int64_t sched,
    int64_t factor) {
  CHECK_GPU(A);
  TORCH_CHECK(A.dim() == 3 && A.size(1) == A.size(2), "A must be (B, N, N)");
  TORCH_CHECK(A.scalar_type() == torch::kFloat32 && A.is_contiguous(),
              "A must be contiguous float32");
  TORCH_CHECK(sched >= 0 && sched <= 2, "sched must be 0, 1 or 2");
  TORCH_CHECK(factor >= -1 && factor <= 1, "factor must be -1, 0 or 1");
  const int B = A.size(0), N = A.size(1);
  float* rhs_ptr = nullptr;
  if (rhs.has_value()) {
    const torch::Tensor& r = rhs.value();
    CHECK_GPU(r);
    TORCH_CHECK(r.dim() == 2 && r.size(0) == B && r.size(1) == N,
                "rhs must be (B, N)");
    TORCH_CHECK(r.scalar_type() == torch::kFloat32, "rhs must be float32");
    rhs_ptr = r.data_ptr<float>();
  }
  auto logdet = torch::empty({B}, A.options());
  auto info = torch::zeros({B}, A.options().dtype(torch::kInt32));
  launch_cholesky_multik_sched(A.data_ptr<float>(), logdet.data_ptr<float>(),
                               info.data_ptr<int>(), rhs_ptr, B, N, (int)sched,
                               (int)factor, cur_stream());
  return {logdet, info};
}

void forward_solve_(torch::Tensor L, torch::Tensor Y) {
  CHECK_GPU(L);
  CHECK_GPU(Y);
  launch_forward_solve_batched(L.data_ptr<float>(), Y.data_ptr<float>(),
                               L.size(0), L.size(1), Y.size(2), cur_stream());
}

void backward_solve_(torch::Tensor L, torch::Tensor Y) {
  CHECK_GPU(L);
  CHECK_GPU(Y);
  launch_backward_solve_batched(L.data_ptr<float>(), Y.data_ptr<float>(),
                                L.size(0), L.size(1), Y.size(2), cur_stream());
}

torch::Tensor dominance_degree_matrix(torch::Tensor Y) {
  CHECK_GPU(Y);
  const int N = Y.size(0), m = Y.size(1);
  auto D = torch::empty({N, N}, Y.options().dtype(torch::kInt32));
  launch_dominance_matrix(Y.data_ptr<float>(), D.data_ptr<int>(), N, m,
                          cur_stream());
  return D;
}

// Route boundary of pareto_rank. N <= COOP_MIN_N takes the one-workgroup
// bit-matrix peel, whose LDS block is (N*W + W)*4 + (N + 2)*4 bytes with
// W = ceil(N/32): at N = 1024, W = 32, that is 135,304 bytes, inside the
// 144 KiB launch_peel_bits allows, and it only shrinks below. Every larger N
// takes the cooperative peel, which has no size limit. The two routes
// therefore cover every N >= 1.
constexpr int COOP_MIN_N = 1024;

torch::Tensor pareto_rank(torch::Tensor Y, int64_t stop = -1) {
  // stop > 0: truncation-selection mode — fronts are peeled only until
  // `stop` points are ranked (the straddling front always completes), the
  // rest receive a sentinel rank larger than every true one. Exact for
  // nsga2_select, which discards everything beyond the kept `pop`; the
  // public op default (-1) ranks everything. Only the cooperative path
  // exploits it — the one-workgroup peel is already ~us-scale.
  CHECK_GPU(Y);
  const int N = Y.size(0), m = Y.size(1);
  const int W = (N + 31) / 32;
  auto Yc = Y.contiguous().to(torch::kFloat32);
  auto opts_i = Y.options().dtype(torch::kInt32);
  auto Dbits = torch::empty({N, W}, opts_i);
  // empty, not zeros: both peels write every rank entry (the fill kernel
  // cost ~24 us/call at N=3200)
  auto rank = torch::empty({N}, opts_i);
  if (N <= COOP_MIN_N) {
    // grid-wide packed dominator build + popcount peel in one workgroup
    const int rc = launch_peel_bits(Yc.data_ptr<float>(),
                                    (unsigned int*)Dbits.data_ptr<int>(),
                                    rank.data_ptr<int>(), N, m, cur_stream());
    TORCH_CHECK(rc == 0, "pareto_rank: bit-matrix peel refused N = ", N,
                ", m = ", m, " (LDS block beyond 144 KiB)");
    return rank.to(torch::kLong);
  }
  // grid-wide COOPERATIVE peel — sync-free from the host and parallel across
  // all CUs (a one-workgroup peel serializes on one CU: 13.8 ms at N=8192
  // vs ~0.1-1 ms here)
  auto fmask = torch::empty({3 * W}, opts_i);  // triple-buffered front mask
  auto n_dom = torch::empty({N}, opts_i);
  auto ctrl = torch::empty({2}, opts_i);
  const int rc = launch_coop_peel(
      Yc.data_ptr<float>(), (unsigned int*)Dbits.data_ptr<int>(),
      (unsigned int*)fmask.data_ptr<int>(), n_dom.data_ptr<int>(),
      ctrl.data_ptr<int>(), rank.data_ptr<int>(), N, m, (int)stop,
      cur_stream());
  TORCH_CHECK(rc == 0, "pareto_rank: cooperative launch unavailable or ",
              "refused at N = ", N, ", m = ", m);
  return rank.to(torch::kLong);
}

torch::Tensor crowding_distance(torch::Tensor Y) {
  CHECK_GPU(Y);
  const int N = Y.size(0), m = Y.size(1);
  if (N == 1) return torch::ones({1}, Y.options());
  TORCH_CHECK(N <= 16384, "crowding_distance HIP kernel supports N <= 16384");
  auto per_dim = torch::empty({m, N}, Y.options());
  launch_crowding(Y.data_ptr<float>(), per_dim.data_ptr<float>(), N, m,
                  cur_stream());
  // fixed-order column sum (deterministic); a raw kernel instead of
  // at::sum saves ~8 us of host dispatch per generation
  auto out = torch::empty({N}, Y.options());
  launch_colsum(per_dim.data_ptr<float>(), out.data_ptr<float>(), m, N,
                cur_stream());
  return out;
}

// DMOSOPT_GEN_FUSED=0: the generation loop as before the fused select and
// spawn kernels and the native chunk driver. The bindings take `fused` = -1
// (this switch), 0 (the chains) or 1 (the fused kernels where they apply).
static int GEN_FUSED = []() {
  const char* e = getenv("DMOSOPT_GEN_FUSED");
  return e && e[0] == '0' ? 0 : 1;
}();

bool gen_fused_default() { return GEN_FUSED != 0; }

static bool gen_fused(int64_t fused) {
  return fused < 0 ? GEN_FUSED != 0 : fused != 0;
}

// Fused NSGA2 survivor selection: concatenate children+parents, pareto-rank,
// crowding, packed-key stable sort ((rank << 32) | ~float_bits(crowding)),
// truncate to pop and gather — one python call instead of ~15 dispatched
// ops per generation. Mirrors ops.remove_worst with the crowding metric.
// Where nsga2_select_fused_fits, all of it is TWO launches (grid-wide
// dominator bits, then nsga2_select_fused_kernel; bitwise the chain's
// outputs), the survivor accounting of nsga2_select_acc included; the chain
// of launches below stays for larger N and with the switch off.
static std::vector<torch::Tensor> nsga2_select_impl(
    const torch::Tensor& x_gen, const torch::Tensor& y_gen,
    const torch::Tensor& pop_parm, const torch::Tensor& pop_obj, int64_t pop,
    const torch::Tensor* c_idx, const torch::Tensor* succ_cross,
    const torch::Tensor* succ_mut, int64_t fused) {
  CHECK_GPU(x_gen);
  CHECK_GPU(y_gen);
  CHECK_GPU(pop_parm);
  CHECK_GPU(pop_obj);
  TORCH_CHECK(x_gen.dtype() == torch::kFloat32 &&
                  pop_parm.dtype() == torch::kFloat32 &&
                  y_gen.dtype() == torch::kFloat32 &&
                  pop_obj.dtype() == torch::kFloat32,
              "nsga2_select: float32 inputs required");
  TORCH_CHECK(x_gen.dim() == 2 && y_gen.dim() == 2 && pop_parm.dim() == 2 &&
                  pop_obj.dim() == 2 && x_gen.size(1) == pop_parm.size(1) &&
                  y_gen.size(1) == pop_obj.size(1) &&
                  x_gen.size(0) == y_gen.size(0) &&
                  pop_parm.size(0) == pop_obj.size(0) && pop >= 1,
              "nsga2_select: shape mismatch");
  if (c_idx) {
    CHECK_GPU((*c_idx));
    TORCH_CHECK(c_idx->dtype() == torch::kLong &&
                    succ_cross->dtype() == torch::kLong &&
                    succ_mut->dtype() == torch::kLong && succ_cross->is_cuda() &&
                    succ_mut->is_cuda(),
                "nsga2_select_acc: int64 GPU tensors required");
    // survivor_count_kernel's child bitmap holds 2048 slots; larger
    // generations go through nsga2_select and are counted by the caller
    TORCH_CHECK(x_gen.size(0) <= 2048, "nsga2_select_acc: ", x_gen.size(0),
                " children, the survivor count takes at most 2048");
  }
  const long long ng = x_gen.size(0), np_ = pop_parm.size(0);
  const long long dP = x_gen.size(1), dO = y_gen.size(1);
  if (gen_fused(fused) && ng + np_ <= 2048 && dP >= 1 &&
      nsga2_select_fused_fits((int)ng, (int)np_, (int)dO)) {
    const int64_t P = std::min<int64_t>(pop, ng + np_);
    auto lopt = x_gen.options().dtype(torch::kLong);
    auto parm_o = torch::empty({P, dP}, x_gen.options());
    auto obj_o = torch::empty({P, dO}, y_gen.options());
    auto rank_o = torch::empty({P}, lopt);
    auto perm = torch::empty({P}, lopt);
    const int64_t Nf = ng + np_;
    auto dbits = torch::empty({Nf * ((Nf + 31) / 32)},
                              x_gen.options().dtype(torch::kInt32));
    const int rc = launch_nsga2_select_fused(
        x_gen.data_ptr<float>(), y_gen.data_ptr<float>(),
        pop_parm.data_ptr<float>(), pop_obj.data_ptr<float>(), (int)ng,
        (int)np_, (int)dP, (int)dO, (int)P,
        c_idx ? (const long long*)c_idx->data_ptr<int64_t>() : nullptr,
        c_idx ? (int)c_idx->numel() : 0, (unsigned int*)dbits.data_ptr<int>(),
        parm_o.data_ptr<float>(),
        obj_o.data_ptr<float>(), (long long*)rank_o.data_ptr<int64_t>(),
        (long long*)perm.data_ptr<int64_t>(),
        c_idx ? (long long*)succ_cross->data_ptr<int64_t>() : nullptr,
        c_idx ? (long long*)succ_mut->data_ptr<int64_t>() : nullptr,
        cur_stream());
    TORCH_CHECK(rc == 0, "nsga2_select: fused selection refused its gate");
    gp_check_launch("nsga2_select", "fused selection");
    return {parm_o, obj_o, rank_o, perm};
  }
  auto parm = torch::empty({ng + np_, dP}, x_gen.options());
  auto obj = torch::empty({ng + np_, dO}, y_gen.options());
  launch_cat_rows(x_gen.data_ptr<float>(), pop_parm.data_ptr<float>(),
                  parm.data_ptr<float>(), ng * dP, (ng + np_) * dP,
                  cur_stream());
  launch_cat_rows(y_gen.data_ptr<float>(), pop_obj.data_ptr<float>(),
                  obj.data_ptr<float>(), ng * dO, (ng + np_) * dO,
                  cur_stream());
  const int64_t keep =
      std::min<int64_t>(pop, x_gen.size(0) + pop_parm.size(0));
  // truncation selection only consumes fronts up to the one straddling
  // `keep`; the early-stop peel skips the (typically ~half) deeper rounds
  auto rank = pareto_rank(obj, keep);              // (N,) long
  auto crowd = crowding_distance(obj).to(torch::kFloat32);  // (N,)
  const int N = obj.size(0), d = parm.size(1), m = obj.size(1);
  const int P0 = (int)std::min<int64_t>(pop, N);
  static int rcs_on = []() {
    const char* e = getenv("DMOSOPT_RCS");
    return e && e[0] == '0' ? 0 : 1;
  }();
  torch::Tensor perm;
  // single-block bitonic (key, idx) sort replaces pack + radix argsort
  // (3-4 launches -> 1); comparator (key asc, idx asc) == stable argsort.
  // Gated by N: the one-workgroup bitonic degrades ~N log^2 N on one CU
  // (122 us at N=3200) while the multi-block radix path stays ~40 us.
  static int rcs_max_n = []() {
    const char* e = getenv("DMOSOPT_RCS_MAX_N");
    return e ? atoi(e) : (1 << 30);
  }();
  auto perm_f = torch::empty({P0}, rank.options());
  if (rcs_on && N <= rcs_max_n &&
      launch_rank_crowd_sort((long long*)rank.data_ptr<int64_t>(),
                             crowd.data_ptr<float>(),
                             (long long*)perm_f.data_ptr<int64_t>(), N, P0,
                             cur_stream()) == 0) {
    perm = perm_f;
  } else {
    auto key = torch::empty({N}, rank.options());
    launch_pack_rank_crowd((long long*)rank.data_ptr<int64_t>(),
                           crowd.data_ptr<float>(),
                           (long long*)key.data_ptr<int64_t>(), N,
                           cur_stream());
    perm = torch::argsort(key, /*stable=*/true, /*dim=*/-1,
                          /*descending=*/false)
               .slice(0, 0, pop)
               .contiguous();
  }
  const int P = perm.size(0);
  auto parm_o = torch::empty({P, d}, parm.options());
  auto obj_o = torch::empty({P, m}, obj.options());
  auto rank_o = torch::empty({P}, rank.options());
  launch_gather3(parm.data_ptr<float>(), obj.data_ptr<float>(),
                 (long long*)rank.data_ptr<int64_t>(), (long long*)perm.data_ptr<int64_t>(),
                 parm_o.data_ptr<float>(), obj_o.data_ptr<float>(),
                 (long long*)rank_o.data_ptr<int64_t>(), P, d, m, cur_stream());
  if (c_idx) {
    const int rc = launch_survivor_count(
        (long long*)perm.data_ptr<int64_t>(),
        (long long*)c_idx->data_ptr<int64_t>(), perm.size(0), c_idx->size(0),
        (int)x_gen.size(0), (long long*)succ_cross->data_ptr<int64_t>(),
        (long long*)succ_mut->data_ptr<int64_t>(), cur_stream());
    TORCH_CHECK(rc == 0, "nsga2_select_acc: survivor count refused ",
                x_gen.size(0), " children");
  }
  return {parm_o, obj_o, rank_o, perm};
}

std::vector<torch::Tensor> nsga2_select(torch::Tensor x_gen,
                                        torch::Tensor y_gen,
                                        torch::Tensor pop_parm,
                                        torch::Tensor pop_obj, int64_t pop,
                                        int64_t fused) {
  return nsga2_select_impl(x_gen, y_gen, pop_parm, pop_obj, pop, nullptr,
                           nullptr, nullptr, fused);
}

// nsga2_select + device-side operator-success accounting in ONE python
// call (the generation loop is host-dispatch-bound; every binding round
// trip costs ~10 us of host time)
std::vector<torch::Tensor> nsga2_select_acc(
    torch::Tensor x_gen, torch::Tensor y_gen, torch::Tensor pop_parm,
    torch::Tensor pop_obj, int64_t pop, torch::Tensor c_idx,
    torch::Tensor succ_cross, torch::Tensor succ_mut, int64_t fused) {
  return nsga2_select_impl(x_gen, y_gen, pop_parm, pop_obj, pop, &c_idx,
                           &succ_cross, &succ_mut, fused);
}

// NSGA-III survivor selection (ops/hip/nsga3.hip): merged rows [x_gen;
// pop_parm], the existing peel for the rank, then normalise, associate and
// niche + gather: no host sync. Returns (parm, obj, rank, perm, ideal,
// scale, niche, dist); niche / dist cover all ng + np merged rows (-1 / +inf
// outside the fronts admitted).
bool nsga3_select_fits_py(int64_t N, int64_t H, int64_t m) {
  return N <= INT_MAX && H <= INT_MAX && m <= INT_MAX &&
         nsga3_select_fits((int)N, (int)H, (int)m) != 0;
}

std::vector<torch::Tensor> nsga3_select(
    torch::Tensor x_gen, torch::Tensor y_gen, torch::Tensor pop_parm,
    torch::Tensor pop_obj, int64_t keep, torch::Tensor Z,
    torch::Tensor dir_prio, torch::Tensor row_prio) {
  const char* fn = "nsga3_select";
  gp_check_f32(fn, "x_gen", x_gen);
  gp_check_f32(fn, "y_gen", y_gen);
  gp_check_f32(fn, "pop_parm", pop_parm);
  gp_check_f32(fn, "pop_obj", pop_obj);
  gp_check_f32(fn, "Z", Z);
  CHECK_GPU(dir_prio);
  CHECK_GPU(row_prio);
  TORCH_CHECK(x_gen.dim() == 2 && y_gen.dim() == 2 && pop_parm.dim() == 2 &&
                  pop_obj.dim() == 2 && Z.dim() == 2 &&
                  x_gen.size(1) == pop_parm.size(1) &&
                  y_gen.size(1) == pop_obj.size(1) &&
                  x_gen.size(0) == y_gen.size(0) &&
                  pop_parm.size(0) == pop_obj.size(0) &&
                  Z.size(1) == y_gen.size(1) && keep >= 1,
              "nsga3_select: shape mismatch");
  const int64_t ng = x_gen.size(0), np_ = pop_parm.size(0), N = ng + np_;
  const int64_t dP = x_gen.size(1), dO = y_gen.size(1), H = Z.size(0);
  TORCH_CHECK(dP >= 1 && nsga3_select_fits_py(N, H, dO), "nsga3_select: N = ",
              N, ", H = ", H, ", m = ", dO, " outside nsga3_select_fits");
  TORCH_CHECK(dir_prio.scalar_type() == torch::kLong && dir_prio.dim() == 1 &&
                  dir_prio.size(0) == H &&
                  row_prio.scalar_type() == torch::kLong &&
                  row_prio.dim() == 1 && row_prio.size(0) == N,
              "nsga3_select: dir_prio (H,) and row_prio (N,) must be int64");
  const int64_t K = std::min<int64_t>(keep, N);
  auto obj = torch::empty({N, dO}, y_gen.options());
  launch_cat_rows(y_gen.data_ptr<float>(), pop_obj.data_ptr<float>(),
                  obj.data_ptr<float>(), ng * dO, N * dO, cur_stream());
  auto rank = pareto_rank(obj, -1);  // (N,) long, every front
  auto lopt = x_gen.options().dtype(torch::kLong);
  auto iopt = x_gen.options().dtype(torch::kInt32);
  auto ctrl = torch::empty({4}, iopt);
  auto rho = torch::empty({H}, iopt);
  auto ideal = torch::empty({dO}, y_gen.options());
  auto scale = torch::empty({dO}, y_gen.options());
  auto niche = torch::empty({N}, lopt);
  auto dist = torch::empty({N}, y_gen.options());
  auto parm_o = torch::empty({K, dP}, x_gen.options());
  auto obj_o = torch::empty({K, dO}, y_gen.options());
  auto rank_o = torch::empty({K}, lopt);
  auto perm = torch::empty({K}, lopt);
  const int rc = launch_nsga3_select(
      x_gen.data_ptr<float>(), pop_parm.data_ptr<float>(),
      obj.data_ptr<float>(), (const long long*)rank.data_ptr<int64_t>(),
      Z.data_ptr<float>(), (const long long*)dir_prio.data_ptr<int64_t>(),
      (const long long*)row_prio.data_ptr<int64_t>(), (int)ng, (int)np_,
      (int)dP, (int)dO, (int)H, (int)K, ctrl.data_ptr<int>(),
      rho.data_ptr<int>(), ideal.data_ptr<float>(), scale.data_ptr<float>(),
      (long long*)niche.data_ptr<int64_t>(), dist.data_ptr<float>(),
      parm_o.data_ptr<float>(), obj_o.data_ptr<float>(),
      (long long*)rank_o.data_ptr<int64_t>(),
      (long long*)perm.data_ptr<int64_t>(), cur_stream());
  TORCH_CHECK(rc == 0, "nsga3_select: launcher refused its gate");
  gp_check_launch(fn, "selection");
  return {parm_o, obj_o, rank_o, perm, ideal, scale, niche, dist};
}

// Tournament pool + event-decoded variation inside one binding call: the
// pool tensor never surfaces to python. Two routes: the fused kernel (one
// launch), or tournament launch + variation_events. Beyond
// launch_tournament's gate (N <= 2048) both return an empty tensor and the
// caller falls back to the split path. rank_sorted stays in the signature
// for its callers; no route reads it any more (the tournament kernels detect
// a rank-sorted population themselves).
torch::Tensor generation_spawn(
    torch::Tensor population, torch::Tensor rank, int64_t poolsize,
    double p_sel, int64_t seed_t, torch::Tensor ci, torch::Tensor mi,
    torch::Tensor p1, torch::Tensor p2, torch::Tensor im, torch::Tensor di_c,
    torch::Tensor di_m, torch::Tensor lo, torch::Tensor hi,
    double mutation_rate, int64_t seed_sbx, int64_t seed_mut,
    bool /*rank_sorted*/, int64_t fused) {
  CHECK_GPU(population);
  TORCH_CHECK(population.dtype() == torch::kFloat32 &&
                  rank.dtype() == torch::kLong &&
                  poolsize <= population.size(0),
              "generation_spawn: f32 population, int64 rank");
  const int N = population.size(0), d = population.size(1);
  if (gen_fused(fused)) {
    // ONE launch (spawn_fused_kernel) under launch_tournament's shape gate
    CHECK_GPU(rank);
    const int C = p1.size(0), M = im.size(0);
    TORCH_CHECK(ci.dtype() == torch::kLong && mi.dtype() == torch::kLong &&
                    p1.dtype() == torch::kLong && p2.dtype() == torch::kLong &&
                    im.dtype() == torch::kLong && p2.size(0) == C &&
                    ci.size(0) == 2 * (int64_t)C && mi.size(0) == M &&
                    rank.size(0) == N && di_c.numel() == d &&
                    di_m.numel() == d && lo.numel() == d && hi.numel() == d,
                "generation_spawn: int64 slot/parent indices, (d,) bounds");
    auto out = torch::empty({(long)(2 * C + M), d}, population.options());
    if (C + M == 0) return out;
    const float l1p = logf(1.0f - (float)p_sel);
    if (launch_spawn_fused(
            population.data_ptr<float>(), (long long*)rank.data_ptr<int64_t>(),
            N, d, (int)poolsize, l1p, (unsigned long long)seed_t,
            C ? (long long*)ci.data_ptr<int64_t>() : nullptr,
            M ? (long long*)mi.data_ptr<int64_t>() : nullptr,
            C ? (long long*)p1.data_ptr<int64_t>() : nullptr,
            C ? (long long*)p2.data_ptr<int64_t>() : nullptr,
            M ? (long long*)im.data_ptr<int64_t>() : nullptr,
            di_c.data_ptr<float>(), di_m.data_ptr<float>(),
            lo.data_ptr<float>(), hi.data_ptr<float>(), out.data_ptr<float>(),
            C, M, (float)mutation_rate, (unsigned long long)seed_sbx,
            (unsigned long long)seed_mut, cur_stream()) != 0)
      return torch::Tensor();  // caller falls back to the split path
    gp_check_launch("generation_spawn", "fused spawn");
    return out;
  }
  auto pool = torch::empty({poolsize, d}, population.options());
  auto pool_idx =
      torch::empty({poolsize}, population.options().dtype(torch::kLong));
  const float log1mp = logf(1.0f - (float)p_sel);
  if (launch_tournament(population.data_ptr<float>(),
                        (long long*)rank.data_ptr<int64_t>(),
                        pool.data_ptr<float>(),
                        (long long*)pool_idx.data_ptr<int64_t>(), N, d,
                        (int)poolsize, log1mp, (unsigned long long)seed_t,
                        cur_stream()) != 0)
    return torch::Tensor();  // caller falls back to the split path
  return variation_events(pool, ci, mi, p1, p2, im, di_c, di_m, lo, hi,
                          mutation_rate, seed_sbx, seed_mut);
}

// Whether nsga2_run_generations takes a population of popsize rows with up to
// max_children children a generation at m objectives: the gates of the fused
// spawn and select kernels.
bool nsga2_generations_fit(int64_t popsize, int64_t max_children, int64_t m) {
  if (popsize < 1 || popsize > 2048 || max_children < 1 ||
      max_children > 2048 || m < 1 || m > 64)
    return false;
  return nsga2_select_fused_fits((int)max_children, (int)popsize, (int)m) != 0;
}

// Native chunk driver of the NSGA-II generation loop: queues `meta.size() / 10`
// generations — fused spawn, cross kernel, mean gemv, dominator bits and fused
// select each — with
// raw launches from one call: no Python and no allocation between them.
//   pop_parm (P,d), pop_obj (P,m), rank (P,) int64: the state, P = popsize
//   idx: the chunk's int64 index buffer (parents and child slots of every
//     generation, as _SpawnPrefetch uploads it)
//   meta: per generation seed_t, C, M, seed_sbx, seed_mut and the offsets of
//     its i1, i2, im, ci, mi lists in idx
// Returns {x_all (sum of children, d), y_all (., m), parm, obj, rank}: every
// generation's children and their predicted objectives in their own rows,
// and the state after the last generation. All five are views of the ONE
// workspace this call allocates (the population ping-pongs between two
// blocks of it), so no later call writes them.
std::vector<torch::Tensor> nsga2_run_generations(
    torch::Tensor pop_parm, torch::Tensor pop_obj, torch::Tensor rank,
    int64_t poolsize, double p_sel, torch::Tensor idx,
    std::vector<int64_t> meta, torch::Tensor di_c, torch::Tensor di_m,
    torch::Tensor lo, torch::Tensor hi, double mutation_rate, torch::Tensor X,
    torch::Tensor theta, torch::Tensor alpha, torch::Tensor y_mean,
    torch::Tensor y_std, double nu, bool aniso,
    c10::optional<torch::Tensor> q_lb, c10::optional<torch::Tensor> q_invrg,
    torch::Tensor succ_cross, torch::Tensor succ_mut) {
  const char* fn = "nsga2_run_generations";
  const GpArgs g = gp_check_args(fn, X, theta, nu, aniso, q_lb, q_invrg);
  gp_check_f32(fn, "pop_parm", pop_parm);
  gp_check_f32(fn, "pop_obj", pop_obj);
  gp_check_f32(fn, "alpha", alpha);
  gp_check_f32(fn, "y_mean", y_mean);
  gp_check_f32(fn, "y_std", y_std);
  gp_check_f32(fn, "di_c", di_c);
  gp_check_f32(fn, "di_m", di_m);
  gp_check_f32(fn, "lo", lo);
  gp_check_f32(fn, "hi", hi);
  CHECK_GPU(rank);
  CHECK_GPU(idx);
  CHECK_GPU(succ_cross);
  CHECK_GPU(succ_mut);
  TORCH_CHECK(pop_parm.dim() == 2 && pop_obj.dim() == 2 &&
                  pop_obj.size(0) == pop_parm.size(0) &&
                  rank.numel() == pop_parm.size(0),
              fn, ": pop_parm (P,d), pop_obj (P,m), rank (P,) required");
  const int64_t P = pop_parm.size(0), d = pop_parm.size(1),
                m = pop_obj.size(1);
  TORCH_CHECK(rank.dtype() == torch::kLong && idx.dtype() == torch::kLong &&
                  succ_cross.dtype() == torch::kLong &&
                  succ_mut.dtype() == torch::kLong,
              fn, ": rank, idx and the success counters must be int64");
  TORCH_CHECK(d == g.D && m == g.B, fn, ": the model has ", g.D,
              " inputs and ", g.B, " outputs, the population ", d, " and ", m);
  TORCH_CHECK(alpha.numel() == g.B * g.N && y_mean.numel() == g.B &&
                  y_std.numel() == g.B,
              fn, ": alpha/y_mean/y_std shape mismatch");
  TORCH_CHECK(di_c.numel() == d && di_m.numel() == d && lo.numel() == d &&
                  hi.numel() == d,
              fn, ": di_c, di_m, lo, hi must be (d,)");
  TORCH_CHECK(poolsize >= 1 && poolsize <= P, fn, ": 1 <= poolsize <= P");
  TORCH_CHECK(meta.size() % 10 == 0 && !meta.empty(), fn,
              ": meta holds 10 values a generation");
  const int64_t G = (int64_t)meta.size() / 10, n_idx = idx.numel();
  int64_t total = 0, max_ng = 0;
  for (int64_t k = 0; k < G; ++k) {
    const int64_t* q = &meta[10 * k];
    const int64_t C = q[1], M = q[2], ng = 2 * C + M;
    TORCH_CHECK(C >= 0 && M >= 0 && ng >= 1, fn, ": generation ", k,
                " has no children");
    TORCH_CHECK(q[5] >= 0 && q[5] + C <= n_idx && q[6] >= 0 &&
                    q[6] + C <= n_idx && q[7] >= 0 && q[7] + M <= n_idx &&
                    q[8] >= 0 && q[8] + 2 * C <= n_idx && q[9] >= 0 &&
                    q[9] + M <= n_idx,
                fn, ": index lists of generation ", k, " leave idx");
    total += ng;
    max_ng = std::max(max_ng, ng);
  }
  TORCH_CHECK(nsga2_generations_fit(P, max_ng, m), fn,
              ": shape outside the gate of the fused kernels");
  gp_check_assemble(g, max_ng);

  // one workspace: [rank A | rank B | perm] int64, then float32
  // [x_all | y_all | parm A | parm B | obj A | obj B | Ks | dominator bits]
  const int64_t n_long = 3 * P;
  const int64_t n_bits = (P + max_ng) * ((P + max_ng + 31) / 32);
  const int64_t n_f =
      total * (d + m) + 2 * P * (d + m) + g.B * max_ng * g.N + n_bits;
  auto ws = torch::empty({n_long * 8 + n_f * 4},
                         pop_parm.options().dtype(torch::kUInt8));
  auto wl = ws.slice(0, 0, n_long * 8).view(torch::kLong);
  auto wf = ws.slice(0, n_long * 8, n_long * 8 + n_f * 4).view(torch::kFloat32);
  int64_t o = 0;
  auto take = [&](int64_t n) { auto t = wf.slice(0, o, o + n); o += n; return t; };
  auto x_all = take(total * d).view({total, d});
  auto y_all = take(total * m).view({total, m});
  torch::Tensor parm_b[2] = {take(P * d).view({P, d}), take(P * d).view({P, d})};
  torch::Tensor obj_b[2] = {take(P * m).view({P, m}), take(P * m).view({P, m})};
  auto Ks = take(g.B * max_ng * g.N);
  unsigned int* dbits = (unsigned int*)take(n_bits).data_ptr<float>();
  torch::Tensor rank_b[2] = {wl.slice(0, 0, P), wl.slice(0, P, 2 * P)};
  long long* perm = (long long*)wl.data_ptr<int64_t>() + 2 * P;

  const long long* ix = (const long long*)idx.data_ptr<int64_t>();
  const float log1mp = logf(1.0f - (float)p_sel);
  hipStream_t stream = cur_stream();
  const float* cp = pop_parm.data_ptr<float>();
  const float* co = pop_obj.data_ptr<float>();
  const long long* cr = (const long long*)rank.data_ptr<int64_t>();
  int64_t row = 0;
  for (int64_t k = 0; k < G; ++k) {
    const int64_t* q = &meta[10 * k];
    const int C = (int)q[1], M = (int)q[2], ng = 2 * C + M;
    float* xg = x_all.data_ptr<float>() + row * d;
    float* yg = y_all.data_ptr<float>() + row * m;
    const int rc = launch_spawn_fused(
        cp, cr, (int)P, (int)d, (int)poolsize, log1mp,
        (unsigned long long)q[0], ix + q[8], ix + q[9], ix + q[5], ix + q[6],
        ix + q[7], di_c.data_ptr<float>(), di_m.data_ptr<float>(),
        lo.data_ptr<float>(), hi.data_ptr<float>(), xg, C, M,
        (float)mutation_rate, (unsigned long long)q[3],
        (unsigned long long)q[4], stream);
    TORCH_CHECK(rc == 0, fn, ": fused spawn refused its gate");
    launch_matern_assemble_affine(
        xg, g.X.data_ptr<float>(), g.theta.data_ptr<float>(),
        Ks.data_ptr<float>(), g.B, ng, g.N, g.D, g.p, 0.0f, g.nu,
        g.aniso ? 1 : 0, 0, g.q_lb, g.q_invrg, stream);
    launch_gp_mean_gemv(Ks.data_ptr<float>(), alpha.data_ptr<float>(),
                        y_mean.data_ptr<float>(), y_std.data_ptr<float>(), yg,
                        g.B, ng, g.N, g.B, stream);
    const int w = (int)(k & 1);
    const int rs = launch_nsga2_select_fused(
        xg, yg, cp, co, ng, (int)P, (int)d, (int)m, (int)P, ix + q[8], 2 * C,
        dbits, parm_b[w].data_ptr<float>(), obj_b[w].data_ptr<float>(),
        (long long*)rank_b[w].data_ptr<int64_t>(), perm,
        (long long*)succ_cross.data_ptr<int64_t>(),
        (long long*)succ_mut.data_ptr<int64_t>(), stream);
    TORCH_CHECK(rs == 0, fn, ": fused selection refused its gate");
    cp = parm_b[w].data_ptr<float>();
    co = obj_b[w].data_ptr<float>();
    cr = (const long long*)rank_b[w].data_ptr<int64_t>();
    row += ng;
  }
  gp_check_launch(fn, "generation chunk");
  const int w = (int)((G - 1) & 1);
  return {x_all, y_all, parm_b[w], obj_b[w], rank_b[w]};
}

std::vector<torch::Tensor> sbx_batch(torch::Tensor pool, torch::Tensor p1,
                                     torch::Tensor p2, torch::Tensor di,
                                     torch::Tensor lo, torch::Tensor hi,
                                     int64_t seed) {
  CHECK_GPU(pool);
  const int C = p1.size(0), d = pool.size(1);
  auto out = torch::empty({2 * C, d}, pool.options());
  launch_sbx_batch(pool.data_ptr<float>(), p1.data_ptr<int>(),
                   p2.data_ptr<int>(), di.data_ptr<float>(),
                   lo.data_ptr<float>(), hi.data_ptr<float>(),
                   out.data_ptr<float>(), C, d, (unsigned long long)seed,
                   cur_stream());
  return {out.narrow(0, 0, C), out.narrow(0, C, C)};
}

torch::Tensor mutation_batch(torch::Tensor pool, torch::Tensor parents,
                             torch::Tensor di, torch::Tensor lo,
                             torch::Tensor hi, double mutation_rate,
                             int64_t seed) {
  CHECK_GPU(pool);
  const int M = parents.size(0), d = pool.size(1);
  auto out = torch::empty({M, d}, pool.options());
  launch_mutation_batch(pool.data_ptr<float>(), parents.data_ptr<int>(),
                        di.data_ptr<float>(), lo.data_ptr<float>(),
                        hi.data_ptr<float>(), out.data_ptr<float>(), M, d,
                        (float)mutation_rate, (unsigned long long)seed,
                        cur_stream());
  return out;
}

int64_t hv_mc_uniform_hits(torch::Tensor P, torch::Tensor ideal,
                           torch::Tensor ref, int64_t n_samples,
                           int64_t seed) {
  CHECK_GPU(P);
  TORCH_CHECK(P.size(1) <= 16, "hv mc kernel supports d <= 16");
  auto hits = torch::zeros({1}, P.options().dtype(torch::kInt64));
  launch_hv_mc_uniform(P.data_ptr<float>(), ideal.data_ptr<float>(),
                       ref.data_ptr<float>(),
                       (unsigned long long*)hits.data_ptr<int64_t>(),
                       n_samples, P.size(0), P.size(1),
                       (unsigned long long)seed, cur_stream());
  return hits.item<int64_t>();
}

int64_t hv_fpras_hits(torch::Tensor P, torch::Tensor ref, torch::Tensor cdf,
                      int64_t n_samples, int64_t seed) {
  CHECK_GPU(P);
  TORCH_CHECK(P.size(1) <= 16, "hv fpras kernel supports d <= 16");
  auto hits = torch::zeros({1}, P.options().dtype(torch::kInt64));
  launch_hv_fpras(P.data_ptr<float>(), ref.data_ptr<float>(),
                  cdf.data_ptr<float>(),
                  (unsigned long long*)hits.data_ptr<int64_t>(), n_samples,
                  P.size(0), P.size(1), (unsigned long long)seed,
                  cur_stream());
  return hits.item<int64_t>();
}

torch::Tensor get_duplicates(torch::Tensor X, double eps) {
  CHECK_GPU(X);
  // distance-based duplicate mask on device via torch primitives;
  // semantics of MOEA.py:426-436. compute_mode 1 = direct differences:
  // the GEMM (x^2-2xy+y^2) formulation leaves exact duplicates at
  // norm-vs-dot rounding residuals that dwarf the eps=1e-16 threshold
  // in fp32 — the difference path is exact at zero distance.
  const int n = X.size(0);
  auto D = torch::cdist(X, X, 2.0, 1);
  auto iu = torch::triu_indices(n, n, 0, torch::TensorOptions()
                                              .dtype(torch::kLong)
                                              .device(X.device()));
  D.index_put_({iu[0], iu[1]},
               torch::full({iu.size(1)}, INFINITY, X.options()));
  D = torch::nan_to_num(D, INFINITY);
  return std::get<0>((D <= eps).max(1)).to(torch::kBool);
}

void cmaes_update_(torch::Tensor A, torch::Tensor Ainv, torch::Tensor pc,
                   torch::Tensor z, torch::Tensor psucc, double cc,
                   double ccov, double pthresh) {
  CHECK_GPU(A);
  CHECK_GPU(Ainv);
  CHECK_GPU(pc);
  const int K = A.size(0), d = A.size(1);
  TORCH_CHECK(d <= 256, "cmaes_update supports d <= 256");
  launch_cmaes_update(A.data_ptr<float>(), Ainv.data_ptr<float>(),
                      pc.data_ptr<float>(), z.data_ptr<float>(),
                      psucc.data_ptr<float>(), K, d, (float)cc, (float)ccov,
                      (float)pthresh, cur_stream());
}

// ------------------------------------------------------- exact hypervolume
double hv2d(torch::Tensor P, torch::Tensor ref) {
  CHECK_GPU(P);
  CHECK_GPU(ref);
  TORCH_CHECK(P.scalar_type() == torch::kFloat64, "hv2d expects float64");
  const int n = P.size(0);
  if (n == 0) return 0.0;
  TORCH_CHECK(n <= 8192, "hv2d kernel supports n <= 8192");
  auto out = torch::zeros({1}, P.options());
  launch_hv2d(P.data_ptr<double>(), ref.data_ptr<double>(),
              out.data_ptr<double>(), n, cur_stream());
  return out.item<double>();
}

torch::Tensor hv3d_slices(torch::Tensor Px, torch::Tensor z_thr,
                          torch::Tensor dz, torch::Tensor ref) {
  CHECK_GPU(Px);
  CHECK_GPU(z_thr);
  CHECK_GPU(dz);
  CHECK_GPU(ref);
  TORCH_CHECK(Px.scalar_type() == torch::kFloat64, "hv3d expects float64");
  const int n = Px.size(0);
  auto out = torch::zeros({std::max(n, 1)}, Px.options());
  if (n > 0)
    launch_hv3d_slices(Px.data_ptr<double>(), z_thr.data_ptr<double>(),
                       dz.data_ptr<double>(), ref.data_ptr<double>(),
                       out.data_ptr<double>(), n, cur_stream());
  return out;
}

torch::Tensor ehvi_batch(torch::Tensor L, torch::Tensor U, torch::Tensor mu,
                         torch::Tensor var) {
  CHECK_GPU(L);
  CHECK_GPU(U);
  CHECK_GPU(mu);
  CHECK_GPU(var);
  TORCH_CHECK(mu.scalar_type() == torch::kFloat64, "ehvi expects float64");
  const int B = mu.size(0), nb = L.size(0), d = mu.size(1);
  TORCH_CHECK(d <= 16, "ehvi kernel supports d <= 16");
  auto out = torch::zeros({B}, mu.options());
  if (B > 0 && nb > 0)
    launch_ehvi(L.data_ptr<double>(), U.data_ptr<double>(),
                mu.data_ptr<double>(), var.data_ptr<double>(),
                out.data_ptr<double>(), B, nb, d, cur_stream());
  return out;
}

std::vector<torch::Tensor> lacour_flags(torch::Tensor coords,
                                        torch::Tensor defs,
                                        torch::Tensor pts_aug,
                                        torch::Tensor z) {
  CHECK_GPU(coords);
  CHECK_GPU(defs);
  CHECK_GPU(pts_aug);
  CHECK_GPU(z);
  const int U = coords.size(0), d = coords.size(1);
  auto opts_u8 = coords.options().dtype(torch::kUInt8);
  auto dominated = torch::zeros({U}, opts_u8);
  auto okj = torch::zeros({U, d}, opts_u8);
  launch_lacour_flags(coords.data_ptr<double>(),
                      (const long long*)defs.data_ptr<int64_t>(),
                      pts_aug.data_ptr<double>(), z.data_ptr<double>(),
                      dominated.data_ptr<uint8_t>(), okj.data_ptr<uint8_t>(),
                      U, d, cur_stream());
  return {dominated, okj};
}

void lacour_scatter(torch::Tensor coords, torch::Tensor defs, torch::Tensor z,
                    torch::Tensor dominated, torch::Tensor okj,
                    torch::Tensor slotA, torch::Tensor slotBj,
                    torch::Tensor baseBj, int64_t baseK, int64_t point_idx,
                    torch::Tensor out_coords, torch::Tensor out_defs) {
  CHECK_GPU(coords);
  CHECK_GPU(out_coords);
  const int U = coords.size(0), d = coords.size(1);
  launch_lacour_scatter(
      coords.data_ptr<double>(), (const long long*)defs.data_ptr<int64_t>(),
      z.data_ptr<double>(), dominated.data_ptr<uint8_t>(),
      okj.data_ptr<uint8_t>(), (const long long*)slotA.data_ptr<int64_t>(),
      (const long long*)slotBj.data_ptr<int64_t>(),
      (const long long*)baseBj.data_ptr<int64_t>(), baseK, point_idx,
      out_coords.data_ptr<double>(), (long long*)out_defs.data_ptr<int64_t>(),
      U, d, cur_stream());
}

torch::Tensor lacour_volumes(torch::Tensor coords, torch::Tensor defs,
                             torch::Tensor pts_aug, torch::Tensor ref) {
  CHECK_GPU(coords);
  const int U = coords.size(0), d = coords.size(1);
  auto vol = torch::zeros({std::max(U, 1)}, coords.options());
  if (U > 0)
    launch_lacour_volumes(coords.data_ptr<double>(),
                          (const long long*)defs.data_ptr<int64_t>(),
                          pts_aug.data_ptr<double>(), ref.data_ptr<double>(),
                          vol.data_ptr<double>(), U, d, cur_stream());
  return vol.narrow(0, 0, U);
}

torch::Tensor smpso_velocity(torch::Tensor position, torch::Tensor velocity,
                             torch::Tensor leader1, torch::Tensor leader2,
                             torch::Tensor xlb, torch::Tensor xub, double w,
                             double a1, double a2, double chi) {
  CHECK_GPU(position);
  CHECK_GPU(velocity);
  const int n = position.size(0), d = position.size(1);
  auto out = torch::empty_like(position);
  launch_smpso_velocity(position.data_ptr<float>(), velocity.data_ptr<float>(),
                        leader1.data_ptr<float>(), leader2.data_ptr<float>(),
                        xlb.data_ptr<float>(), xub.data_ptr<float>(),
                        out.data_ptr<float>(), n, d, (float)w, (float)a1,
                        (float)a2, (float)chi, cur_stream());
  return out;
}

torch::Tensor minkowski_norm_matrix(torch::Tensor Y, double p) {
  CHECK_GPU(Y);
  const int m = Y.size(0), d = Y.size(1);
  TORCH_CHECK(d <= 16, "minkowski_norm_matrix supports d <= 16");
  auto D = torch::empty({m, m}, Y.options());
  launch_minkowski_norm_matrix(Y.data_ptr<float>(), D.data_ptr<float>(), m, d,
                               (float)p, cur_stream());
  return D;
}

torch::Tensor agemoea_survival(torch::Tensor D, torch::Tensor preselected) {
  CHECK_GPU(D);
  CHECK_GPU(preselected);
  const int m = D.size(0);
  TORCH_CHECK(m <= 8192, "agemoea_survival supports m <= 8192 (LDS)");
  TORCH_CHECK(D.scalar_type() == torch::kFloat32);
  auto crowd = torch::zeros({m}, D.options());
  launch_agemoea_survival(D.data_ptr<float>(),
                          preselected.data_ptr<uint8_t>(),
                          crowd.data_ptr<float>(), m, cur_stream());
  return crowd;
}

// --------------------------------------------------------------- bf16 path
torch::Tensor mfma_bf16_probe(torch::Tensor A, torch::Tensor B) {
  CHECK_GPU(A);
  CHECK_GPU(B);
  TORCH_CHECK(A.sizes() == torch::IntArrayRef({16, 32}) &&
              B.sizes() == torch::IntArrayRef({32, 16}));
  auto D = torch::zeros({16, 16}, A.options());
  launch_mfma_bf16_probe(A.data_ptr<float>(), B.data_ptr<float>(),
                         D.data_ptr<float>(), cur_stream());
  return D;
}

torch::Tensor matern_cross_bf16(torch::Tensor Xq, torch::Tensor X,
                                torch::Tensor theta, double nu, bool aniso,
                                c10::optional<torch::Tensor> q_lb = c10::nullopt,
                                c10::optional<torch::Tensor> q_invrg = c10::nullopt) {
  CHECK_GPU(Xq);
  CHECK_GPU(X);
  CHECK_GPU(theta);
  const int P = Xq.size(0), N = X.size(0), D = X.size(1), B = theta.size(0);
  auto K = torch::empty({B, P, N}, X.options());
  launch_matern_cross_bf16(
      Xq.data_ptr<float>(), X.data_ptr<float>(), theta.data_ptr<float>(),
      K.data_ptr<float>(), B, P, N, D, theta.size(1), nu_code(nu),
      aniso ? 1 : 0, q_lb ? q_lb->data_ptr<float>() : nullptr,
      q_invrg ? q_invrg->data_ptr<float>() : nullptr, cur_stream());
  return K;
}

std::vector<torch::Tensor> cholesky_batched_bf16_(torch::Tensor A) {
  CHECK_GPU(A);
  const int B = A.size(0), N = A.size(1);
  auto logdet = torch::empty({B}, A.options());
  auto info = torch::zeros({B}, A.options().dtype(torch::kInt32));
  launch_cholesky_multik_bf16(A.data_ptr<float>(), logdet.data_ptr<float>(),
                              info.data_ptr<int>(), B, N, cur_stream());
  return {logdet, info};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("matern_train", &matern_train, "Batched Matern train-kernel assembly");
  m.def("matern_cross", &matern_cross, "Batched Matern cross-kernel assembly");
  m.def("variation_events", &variation_events);
  m.def("tournament_pool", &tournament_pool);
  m.def("survivor_count", &survivor_count);
  m.def("sceua_propose", &sceua_propose);
  m.def("sceua_accept", &sceua_accept);
  m.def("sceua_propose_sched", &sceua_propose_sched,
        "sceua_propose reading its stage's simplex and seed from device memory");
  m.def("sceua_accept_sched", &sceua_accept_sched,
        "sceua_accept reading its stage's simplex from device memory");
  m.def("sceua_unpartition", &sceua_unpartition);
  m.def("sceua_partition_pack", &sceua_partition_pack);
  m.def("gp_nmll_into", &gp_nmll_into,
        "gp_nmll into caller-owned K, Z, logdet, info, out (no allocation)");
  m.def("nsga2_select", &nsga2_select, "Fused survivor selection (cat+rank+crowding+sort+gather)",
        py::arg("x_gen"), py::arg("y_gen"), py::arg("pop_parm"), py::arg("pop_obj"), py::arg("pop"),
        py::arg("fused") = -1);
  m.def("nsga2_select_acc", &nsga2_select_acc, py::arg("x_gen"), py::arg("y_gen"),
        py::arg("pop_parm"), py::arg("pop_obj"), py::arg("pop"), py::arg("c_idx"),
        py::arg("succ_cross"), py::arg("succ_mut"), py::arg("fused") = -1);
  m.def("nsga3_select", &nsga3_select,
        "NSGA-III survivor selection (cat+rank+normalise+associate+niche+gather)",
        py::arg("x_gen"), py::arg("y_gen"), py::arg("pop_parm"), py::arg("pop_obj"),
        py::arg("keep"), py::arg("Z"), py::arg("dir_prio"), py::arg("row_prio"));
  m.def("nsga3_select_fits", &nsga3_select_fits_py, py::arg("N"), py::arg("H"),
        py::arg("m"));
  m.def("gen_fused_default", &gen_fused_default,
        "False under DMOSOPT_GEN_FUSED=0: the generation loop's chains of launches");
  m.def("nsga2_generations_fit", &nsga2_generations_fit);
  m.def("nsga2_run_generations", &nsga2_run_generations,
        "Native chunk driver: spawn, predict and select of several generations in one call");
  m.def("generation_spawn", &generation_spawn, py::arg("population"), py::arg("rank"), py::arg("poolsize"), py::arg("p_sel"), py::arg("seed_t"), py::arg("ci"), py::arg("mi"), py::arg("p1"), py::arg("p2"), py::arg("im"), py::arg("di_c"), py::arg("di_m"), py::arg("lo"), py::arg("hi"), py::arg("mutation_rate"), py::arg("seed_sbx"), py::arg("seed_mut"), py::arg("rank_sorted") = false, py::arg("fused") = -1);
  m.def("gp_predict_mean", &gp_predict_mean, "Fused cross-kernel + posterior mean",
        py::arg("Xq"), py::arg("X"), py::arg("theta"), py::arg("alpha"),
        py::arg("y_mean"), py::arg("y_std"), py::arg("nu"), py::arg("aniso"),
        py::arg("q_lb") = py::none(), py::arg("q_invrg") = py::none());
  m.def("gp_predict_mean_var", &gp_predict_mean_var,
        "Fused cross-kernel + posterior mean + |Linv k*|^2 variance, (P, 2B)",
        py::arg("Xq"), py::arg("X"), py::arg("theta"), py::arg("alpha"),
        py::arg("Linv"), py::arg("y_mean"), py::arg("y_std"), py::arg("nu"),
        py::arg("aniso"), py::arg("q_lb") = py::none(),
        py::arg("q_invrg") = py::none(), py::arg("var_decimals") = -1);
  m.def("gp_predict_pof", &gp_predict_pof,
        "Fused GP probability of feasibility, (P, B + 1) = [Phi(mean / sd) | row mean]",
        py::arg("Xq"), py::arg("X"), py::arg("theta"), py::arg("alpha"),
        py::arg("Linv"), py::arg("y_mean"), py::arg("y_std"), py::arg("nu"),
        py::arg("aniso"), py::arg("q_lb") = py::none(),
        py::arg("q_invrg") = py::none());
  m.def("gp_predict_mean_grad", &gp_predict_mean_grad,
        "Fused posterior mean (P, B) and its query-point gradient (P, B, D)",
        py::arg("Xq"), py::arg("X"), py::arg("theta"), py::arg("alpha"),
        py::arg("y_mean"), py::arg("y_std"), py::arg("nu"), py::arg("aniso"),
        py::arg("q_lb") = py::none(), py::arg("q_invrg") = py::none());
  m.def("gp_predict_path", &gp_predict_path,
        "Posterior sample path (P, B): mean launches with alpha_path + random features",
        py::arg("Xq"), py::arg("X"), py::arg("theta"), py::arg("alpha_path"),
        py::arg("y_mean"), py::arg("y_std"), py::arg("nu"), py::arg("aniso"),
        py::arg("Omega"), py::arg("tau"), py::arg("amp"),
        py::arg("q_lb") = py::none(), py::arg("q_invrg") = py::none());
  m.def("gp_nmll", &gp_nmll, "Fused batched GP NMLL (assemble+chol+solve+reduce)");
  m.def("gp_nmll_grad", &gp_nmll_grad,
        "Fused batched GP NMLL value and analytic gradient");
  m.def("cholesky_batched_", &cholesky_batched_,
        "In-place batched Cholesky; returns (logdet, info)");
  m.def("cholesky_multik_sched_", &cholesky_multik_sched_,
        "In-place multi-launch Cholesky with an explicit schedule "
        "(0 classic, 1 look-ahead), an explicit diagonal factor (0 lds, "
        "1 reg, -1 process default) and optional fused rhs; returns "
        "(logdet, info)",
        py::arg("A"), py::arg("rhs") = py::none(), py::arg("sched") = 0,
        py::arg("factor") = -1);
  m.def("forward_solve_", &forward_solve_, "In-place batched L z = y solve");
  m.def("backward_solve_", &backward_solve_, "In-place batched L^T x = z solve");
  m.def("dominance_degree_matrix", &dominance_degree_matrix);
  m.def("pareto_rank", &pareto_rank, py::arg("Y"), py::arg("stop") = -1);
  m.def("crowding_distance", &crowding_distance);
  m.def("sbx_batch", &sbx_batch);
  m.def("mutation_batch", &mutation_batch);
  m.def("hv_mc_uniform_hits", &hv_mc_uniform_hits);
  m.def("hv_fpras_hits", &hv_fpras_hits);
  m.def("get_duplicates", &get_duplicates);
  m.def("smpso_velocity", &smpso_velocity,
        "Fused SMPSO constriction velocity + clamp");
  m.def("minkowski_norm_matrix", &minkowski_norm_matrix,
        "Row-normalized Minkowski-p distance matrix in one pass");
  m.def("agemoea_survival", &agemoea_survival,
        "Greedy 2-NN AGE-MOEA survival scores (single-workgroup loop)");
  m.def("mfma_bf16_probe", &mfma_bf16_probe,
        "Single-tile bf16 MFMA fragment-layout probe");
  m.def("matern_cross_bf16", &matern_cross_bf16,
        "bf16-MFMA Matern cross-kernel assembly", py::arg("Xq"), py::arg("X"),
        py::arg("theta"), py::arg("nu"), py::arg("aniso"),
        py::arg("q_lb") = c10::nullopt, py::arg("q_invrg") = c10::nullopt);
  m.def("cholesky_batched_bf16_", &cholesky_batched_bf16_,
        "Batched Cholesky with bf16-MFMA trailing updates");
  m.def("hv2d", &hv2d, "Exact 2D hypervolume (LDS bitonic staircase sweep)");
  m.def("hv3d_slices", &hv3d_slices,
        "Per-slice 2D sweep terms of the 3D hypervolume");
  m.def("ehvi_batch", &ehvi_batch,
        "Batched EHVI over the dominated-space box decomposition");
  m.def("lacour_flags", &lacour_flags);
  m.def("lacour_scatter", &lacour_scatter);
  m.def("lacour_volumes", &lacour_volumes);
  m.def("cmaes_update_", &cmaes_update_,
        "In-place batched MO-CMA-ES rank-1 Cholesky update");
}
