// The one declaration of every extern "C" launcher bindings.cpp calls, grouped by
// the .hip file that defines it. bindings.cpp and every .hip file include it, so
// a definition that drifts from its declaration fails to compile (C linkage has
// no mangling: without the header the mismatch would still link).
#pragma once

#include <hip/hip_runtime.h>

extern "C" {

// ---------------------------------------------------------------- matern.hip
// symmetric: 0 = cross kernel (norms form), 1 = train kernel (adds
// noise + jitter on the diagonal), 2 = cross kernel, direct-difference form.
// q_lb / q_invrg (both or neither): per-dim affine applied to Xq on load.
void launch_matern_assemble_affine(const float* Xq, const float* X, const float* theta, float* K,
    int B, int P, int N, int D, int theta_stride, float jitter, int nu_code, int aniso,
    int symmetric, const float* q_lb, const float* q_invrg, hipStream_t stream);
// train form whose launch also sets Z = y rows (y_stride 0 or N), logdet = 0, info = 0
void launch_matern_train_prologue(const float* X, const float* theta, float* K, int B, int N, int D,
    int theta_stride, float jitter, int nu_code, int aniso, const float* y, int y_stride, float* Z,
    float* logdet, int* info, hipStream_t stream);
void launch_gp_mean_gemv(const float* Ks, const float* alpha, const float* y_mean,
    const float* y_std, float* out, int B, int P, int N, int ldo, hipStream_t stream);

// -------------------------------------------------------------- cholesky.hip
void launch_nmll_reduce(const float* Z, const float* half_logdet, const int* info, float* out, int B,
    int N, float c, hipStream_t stream);
void launch_cholesky_multik_sched(float* A, float* logdet, int* info, float* rhs, int B, int N,
    int sched, int factor, hipStream_t stream);
void launch_cholesky_multik_bf16(float* A, float* logdet, int* info, int B, int N,
    hipStream_t stream);
// returns nonzero, launching nothing, when the fused path does not apply
int launch_cholesky_fused_solve(float* A, float* logdet, int* info, float* rhs, int B, int N,
    hipStream_t stream);
// factor + fused solve + NMLL after the prologue assemble: one launch where the one-launch schedule
// applies, else the look-ahead schedule's ceil(N/32); only where cholesky_nmll_chain_applies (the
// shapes and switches of the look-ahead fused-solve route)
int cholesky_nmll_chain_applies(int B, int N);
void launch_cholesky_nmll_chain(float* A, float* logdet, int* info, float* rhs, float* out, int B,
    int N, float c, hipStream_t stream);
void launch_cholesky_batched(float* A, float* logdet, int* info, int B, int N, hipStream_t stream);
void launch_forward_solve_batched(const float* L, float* Y, int B, int N, int R, hipStream_t stream);
void launch_backward_solve_batched(const float* L, float* Y, int B, int N, int R,
    hipStream_t stream);

// ----------------------------------------------------------- matern_bf16.hip
void launch_mfma_bf16_probe(const float* A, const float* B, float* D, hipStream_t s);
void launch_matern_cross_bf16(const float* Xq, const float* X, const float* theta, float* K, int B,
    int P, int N, int D, int theta_stride, int nu_code, int aniso, const float* q_lb,
    const float* q_invrg, hipStream_t stream);
// called by cholesky.hip's bf16 schedule, not by bindings.cpp
void launch_chol_syrk_bf16(float* A, int N, int k0, int n_pairs, int B, hipStream_t stream);

// ----------------------------------------------------------- gp_variance.hip
// launchers returning int give 0 or the hipError_t of the failed launch
int launch_gp_variance(const float* Linv, const float* Ks, const float* theta, const float* y_std,
    float* part, float* out, int B, int P, int N, int theta_stride, float round_scale,
    hipStream_t stream);
// row tiles of Linv = partial sums per query; the partial sums alone into part (B, tiles, P)
int gp_var_tiles(int N);
int launch_gp_var_partial(const float* Linv, const float* Ks, float* part, int B, int P, int N,
    hipStream_t stream);

// ---------------------------------------------------------------- gp_pof.hip
// mean: the (P, B) de-standardised means of launch_gp_mean_gemv; out (P, B + 1) = [PoF | rank]
int launch_gp_pof(const float* Linv, const float* Ks, const float* mean, const float* theta,
    const float* y_std, float* part, float* out, int B, int P, int N, int theta_stride,
    hipStream_t stream);

// ---------------------------------------------------------- gp_nmll_grad.hip
int launch_gp_fill_identity(float* Y, int B, int N, hipStream_t stream);
int gp_nmll_grad_tiles(int N);
int launch_gp_nmll_grad(const float* X, const float* theta, const float* Kinv, const float* alpha,
    const float* nmll, const int* info, float* part, float* grad, int B, int N, int D, int p,
    int nu_code, int aniso, hipStream_t stream);

// ---------------------------------------------------------- gp_mean_grad.hip
int gp_mean_grad_splits(int N);
int launch_gp_mean_grad(const float* Xq, const float* X, const float* theta, const float* alpha,
    const float* y_std, float* part, float* jac, int B, int P, int N, int D, int p, int nu_code,
    int aniso, const float* q_lb, const float* q_invrg, hipStream_t stream);

// --------------------------------------------------------------- gp_path.hip
int gp_path_splits(int M);
// adds y_std_b * sum_j amp_bj cos(2 pi (tau_bj + Omega_bj . u)) into out[p * ldo + b]
int launch_gp_path(const float* Xq, const float* Omega, const float* tau, const float* amp,
    const float* y_std, float* part, float* out, int B, int P, int M, int D, int ldo,
    const float* q_lb, const float* q_invrg, hipStream_t stream);

// ----------------------------------------------------------- sceua_stage.hip
void launch_sceua_propose(const float* cx, const int* lcs, const float* bl, const float* bu,
    float* cand, int S, int G, int npg, int nopt, int nps, unsigned long long seed,
    hipStream_t stream);
int launch_sceua_accept(float* cx, float* cf, const float* cand, const float* fall, const int* lcs,
    const int* act, int* icall, int S, int G, int npg, int nopt, int nps, hipStream_t stream);
// device-schedule forms: sched (nspl, nps + 2) int32 rows of simplex positions + seed words,
// step (2,) int32 stage counter and hand-over word
void launch_sceua_propose_sched(const float* cx, const int* sched, int* step, const float* bl,
    const float* bu, float* cand, int S, int G, int npg, int nopt, int nps, int nspl,
    hipStream_t stream);
int launch_sceua_accept_sched(float* cx, float* cf, const float* cand, const float* fall,
    const int* sched, int* step, const int* act, int* icall, int S, int G, int npg, int nopt,
    int nps, int nspl, hipStream_t stream);
// shuffle boundary: (S,G,npg,.) -> (S,npt,.), and back by a sort order with the termination pack
void launch_sceua_unpartition(const float* cx, const float* cf, float* x, float* xf, int S, int G,
    int npg, int nopt, hipStream_t stream);
void launch_sceua_partition_pack(const float* x, const float* xf, const long long* order,
    const int* icall, float* xs, float* xfs, float* cx, float* cf, float* pack, int S, int G,
    int npg, int nopt, hipStream_t stream);

// ---------------------------------------------------------------- pareto.hip
// both peels return nonzero, launching nothing or not the peel, when refused: launch_peel_bits
// beyond its 144 KiB LDS block, launch_coop_peel when the cooperative launch is not available
int launch_peel_bits(const float* Y, unsigned int* Dbits_scratch, int* rank, int N, int m,
    hipStream_t stream);
int launch_coop_peel(const float* Y, unsigned int* Dbits, unsigned int* fmask, int* n_dom, int* ctrl,
    int* rank, int N, int m, int stop, hipStream_t stream);
void launch_dominance_matrix(const float* Y, int* D, int N, int m, hipStream_t stream);
void launch_crowding(const float* Y, float* out, int N, int m, hipStream_t stream);

// ------------------------------------------------------------- variation.hip
void launch_sbx_batch(const float* pool, const int* p1, const int* p2, const float* di,
    const float* lo, const float* hi, float* out, int C, int d, unsigned long long seed,
    hipStream_t stream);
void launch_mutation_batch(const float* pool, const int* parents, const float* di, const float* lo,
    const float* hi, float* out, int M, int d, float mutation_rate, unsigned long long seed,
    hipStream_t stream);
void launch_variation_events(const float* pool, const long long* ci, const long long* mi,
    const long long* p1, const long long* p2, const long long* im, const float* di_c,
    const float* di_m, const float* lo, const float* hi, float* out, int C, int M, int d,
    float mutation_rate, unsigned long long seed_sbx, unsigned long long seed_mut,
    hipStream_t stream);

// -------------------------------------------------------------- moea_ops.hip
int launch_tournament(const float* population, const long long* rank, float* pool,
    long long* pool_idx, int N, int d, int poolsize, float log1mp, unsigned long long seed,
    hipStream_t stream);
// tournament + event-decoded variation in one launch; -1, launching nothing, outside
// launch_tournament's shape gate
int launch_spawn_fused(const float* population, const long long* rank, int N, int d, int poolsize,
    float log1mp, unsigned long long seed_t, const long long* ci, const long long* mi,
    const long long* p1, const long long* p2, const long long* im, const float* di_c,
    const float* di_m, const float* lo, const float* hi, float* out, int C, int M,
    float mutation_rate, unsigned long long seed_sbx, unsigned long long seed_mut,
    hipStream_t stream);
// whole survivor selection in two launches (grid-wide dominator bits into dbits_scratch,
// (ng + np) * ceil((ng + np) / 32) words; then one workgroup): 1 where its LDS block fits, and
// the launches (-1, launching nothing, where it does not). succ_cross null skips the counts.
int nsga2_select_fused_fits(int ng, int np, int m);
int launch_nsga2_select_fused(const float* x_gen, const float* y_gen, const float* pop_parm,
    const float* pop_obj, int ng, int np, int d, int m, int keep, const long long* c_idx,
    int n_cross, unsigned int* dbits_scratch, float* parm_o, float* obj_o, long long* rank_o,
    long long* perm, long long* succ_cross, long long* succ_mut, hipStream_t stream);
int launch_survivor_count(const long long* perm, const long long* c_idx, int n_perm, int n_cross,
    int n_children, long long* succ_cross, long long* succ_mut, hipStream_t stream);
void launch_pack_rank_crowd(const long long* rank, const float* crowd, long long* key, int N,
    hipStream_t stream);
void launch_gather3(const float* parm, const float* obj, const long long* rank,
    const long long* perm, float* parm_o, float* obj_o, long long* rank_o, int pop, int d, int m,
    hipStream_t stream);
int launch_rank_crowd_sort(const long long* rank, const float* crowd, long long* perm, int N,
    int pop, hipStream_t stream);
void launch_smpso_velocity(const float* position, const float* velocity, const float* leader1,
    const float* leader2, const float* xlb, const float* xub, float* out, int n, int d, float w,
    float a1, float a2, float chi, hipStream_t stream);
void launch_cat_rows(const float* a, const float* b, float* out, long long na_elems,
    long long total_elems, hipStream_t stream);
void launch_colsum(const float* per_dim, float* out, int m, int N, hipStream_t stream);

// ----------------------------------------------------------------- nsga3.hip
// NSGA-III survival after the peel: normalise (one workgroup), associate (grid-wide), niche +
// gather (one workgroup). Y (ng + np, m) is [y_gen; pop_obj], rank its Pareto rank, K <= ng + np
// the rows kept. ctrl (4,) int32 and rho (H,) int32 are scratch the first launch initialises.
// 1 where the shape is inside the kernels' LDS blocks (N <= 4096, H <= 2048, m <= 16, and the
// dynamic block the niche kernel asks for within the limit the launcher sets); the launcher
// returns -1, launching nothing, outside it.
int nsga3_select_fits(int N, int H, int m);
int launch_nsga3_select(const float* x_gen, const float* pop_parm, const float* Y,
    const long long* rank, const float* Z, const long long* dir_prio, const long long* row_prio,
    int ng, int np, int d, int m, int H, int K, int* ctrl, int* rho, float* ideal, float* scale,
    long long* niche, float* dist, float* parm_o, float* obj_o, long long* rank_o,
    long long* perm, hipStream_t stream);

// ------------------------------------------------------ agemoea_survival.hip
void launch_agemoea_survival(const float* D, const unsigned char* preselected, float* crowd, int m,
    hipStream_t s);
void launch_minkowski_norm_matrix(const float* Y, float* D, int m, int d, float p, hipStream_t s);

// ---------------------------------------------------------- cmaes_update.hip
void launch_cmaes_update(float* A, float* Ainv, float* pc, const float* z, const float* psucc, int K,
    int d, float cc, float ccov, float pthresh, hipStream_t stream);

// ----------------------------------------------------------------- hv_mc.hip
void launch_hv_mc_uniform(const float* P, const float* ideal, const float* ref,
    unsigned long long* hits, long long n_samples, int N, int d, unsigned long long seed,
    hipStream_t stream);
void launch_hv_fpras(const float* P, const float* ref, const float* cdf, unsigned long long* hits,
    long long n_samples, int N, int d, unsigned long long seed, hipStream_t stream);

// -------------------------------------------------------------- hv_exact.hip
void launch_hv2d(const double* P, const double* ref, double* out, int n, hipStream_t s);
void launch_hv3d_slices(const double* Px, const double* z_thr, const double* dz, const double* ref,
    double* out, int n, hipStream_t s);
void launch_ehvi(const double* L, const double* U, const double* mu, const double* var, double* out,
    int B, int nb, int d, hipStream_t s);
void launch_lacour_flags(const double* coords, const long long* defs, const double* pts_aug,
    const double* z, unsigned char* dominated, unsigned char* okj, int U, int d, hipStream_t s);
void launch_lacour_scatter(const double* coords, const long long* defs, const double* z,
    const unsigned char* dominated, const unsigned char* okj, const long long* slotA,
    const long long* slotBj, const long long* baseBj, long long baseK, long long point_idx,
    double* out_coords, long long* out_defs, int U, int d, hipStream_t s);
void launch_lacour_volumes(const double* coords, const long long* defs, const double* pts_aug,
    const double* ref, double* vol, int U, int d, hipStream_t s);

}  // extern "C"
