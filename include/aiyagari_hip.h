/* aiyagari_hip.h — C ABI of the MI355X (gfx950) solver for the hot path of
 * kostastril/Aiyagari-Replication (six MATLAB scripts).
 *
 * The reference has no plugin/operator/FFI interface: its hot path is inline script code.
 * Each entry point below replaces exactly one cited loop body, takes the same inputs and
 * returns the same outputs.  A MEX/mkoctfile gateway
 * (aiyagari-replication_amd/mex/) binds them one-to-one; INTEGRATION.md shows the binding.
 *
 * Two tiers:
 *   1. Host-pointer functions (aiy_*, ks_*): MATLAB column-major arrays exactly as the
 *      replaced variables are laid out, synchronous (return after the outputs are copied
 *      back).  Device buffers are library-owned and cached per shape across calls.
 *   2. Device-pointer functions (*_dev): arrays already resident in HBM, state-major layout
 *      ([N][Na] row-major == MATLAB Na x N column-major), asynchronous on `stream`
 *      (a hipStream_t; NULL = default stream).  Used by the python host mirror and bench.
 *
 * Conventions: all arrays fp64 unless typed otherwise; index outputs are 0-based in the
 * device tier and 1-based (MATLAB) in the host tier; every function returns an aiy_status
 * and leaves a message retrievable with aiy_last_error().
 */
#ifndef AIYAGARI_HIP_H
#define AIYAGARI_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    AIY_OK = 0,
    AIY_BAD_SHAPE = 1,   /* inconsistent or unsupported sizes */
    AIY_NON_FINITE = 2,  /* an input that must be finite is not */
    AIY_HIP_ERROR = 3,   /* HIP runtime failure (message has hipGetErrorString) */
    AIY_RCCL_ERROR = 4,  /* reserved: collective failure (multi-device entry points) */
    AIY_NO_DEVICE = 5,   /* no gfx950 device visible */
    AIY_BAD_ARG = 6,     /* invalid scalar / unsorted grid / NULL pointer */
    AIY_FIND_EMPTY = 7,  /* find(rand < cumsum(P(z,:)),1) empty: the reference would error */
    AIY_NO_MEMORY = 8
} aiy_status;

const char* aiy_last_error(void); /* thread-local message of the last failing call */
int aiy_version(void);            /* 100*major + minor */
int aiy_device_count(void);

/* ======================================================================================
 * Host tier (MATLAB layouts).  VFI arrays N x Na; EGM arrays Na x N; KS k x K x S.
 * ====================================================================================== */

/* Lifecycle.  The host tier keeps device buffers, workspaces and streams
 * per (device, shape) across calls.  aiy_release_all frees every one of them (the gateways
 * register it with mexAtExit, so `clear all` / `clear mex` — Krusell_Smith_VFI.m:2 — leaves
 * no device memory behind); the next call re-creates what it needs.  aiy_host_cache_bytes
 * reports the device bytes those caches hold (0 after a release). */
int aiy_release_all(void);
int64_t aiy_host_cache_bytes(void);

/* A1 — replaces Aiyagari_VFI.m:68-83 (one Bellman sweep).
 * in : v_old N x Na, a_grid Na (non-decreasing), s N, P N x N, r, w, beta, sigma
 * out: v_new, policy_k, policy_c (N x Na); policy_idx (N x Na, 1-based, may be NULL) */
int aiy_vfi_sweep(const double* v_old, const double* a_grid, const double* s, const double* P,
                  int64_t N, int64_t Na, double r, double w, double beta, double sigma,
                  double* v_new, double* policy_k, double* policy_c, int32_t* policy_idx);

/* A2 — replaces Aiyagari_VFI.m:65-90 (the sweep loop).  Break semantics of :85-88: on
 * return v_new is the converged iterate and v_old (in/out) the previous one; when max_iter
 * is exhausted v_old == v_new.  iters = the reference's `iter` at exit. */
int aiy_vfi_solve(double* v_old, const double* a_grid, const double* s, const double* P,
                  int64_t N, int64_t Na, double r, double w, double beta, double sigma,
                  double tol, int64_t max_iter, double* v_new, double* policy_k,
                  double* policy_c, int32_t* policy_idx, int64_t* iters);

/* A3 — replaces Aiyagari_Endogenous_Labor_VFI.m:69-112 / :64-122.  v_new and the policies
 * are in/out: states with no feasible (l, a') keep their incoming values (:85).
 * policy_lin (nullable) = 1-based column-major index into the Nl x Na choice matrix. */
int aiy_labor_vfi_sweep(const double* v_old, const double* a_grid, const double* s,
                        const double* P, const double* labor_choice, int64_t N, int64_t Na,
                        int64_t Nl, double r, double w, double beta, double sigma, double psi,
                        double eta, double* v_new, double* policy_k, double* policy_l,
                        double* policy_c, int32_t* policy_lin);
int aiy_labor_vfi_solve(double* v_old, const double* a_grid, const double* s, const double* P,
                        const double* labor_choice, int64_t N, int64_t Na, int64_t Nl, double r,
                        double w, double beta, double sigma, double psi, double eta, double tol,
                        int64_t max_iter, double* v_new, double* policy_k, double* policy_l,
                        double* policy_c, int32_t* policy_lin, int64_t* iters);

/* A4 — replaces Aiyagari_EGM.m:75-107 (one pass) and :71-110 (the while loop).
 * policy_c Na x N in; policy_c_next, policy_k Na x N out; dist = max|Δc|. */
int aiy_egm_step(const double* policy_c, const double* a_grid, const double* s,
                 const double* P, int64_t N, int64_t Na, double r, double w, double beta,
                 double sigma, double amin, double* policy_c_next, double* policy_k,
                 double* dist);
int aiy_egm_solve(double* policy_c, const double* a_grid, const double* s, const double* P,
                  int64_t N, int64_t Na, double r, double w, double beta, double sigma,
                  double amin, double tol, int64_t max_iter, double* policy_k, double* dist,
                  int64_t* iters);
/* A5 — replaces Aiyagari_Endogenous_Labor_EGM.m:68-104 / :67-107. */
int aiy_labor_egm_step(const double* policy_c, const double* a_grid, const double* s,
                       const double* P, int64_t N, int64_t Na, double r, double w, double beta,
                       double sigma, double phi, double theta, double amin,
                       double* policy_c_next, double* policy_k, double* policy_l,
                       double* dist);
int aiy_labor_egm_solve(double* policy_c, const double* a_grid, const double* s,
                        const double* P, int64_t N, int64_t Na, double r, double w,
                        double beta, double sigma, double phi, double theta, double amin,
                        double tol, int64_t max_iter, double* policy_k, double* policy_l,
                        double* dist, int64_t* iters);

/* A9 — replaces the simulation block Aiyagari_VFI.m:104-129 (:174-193 in the GE loop).
 * policy_k: N x Na (vfi_layout=1) or Na x N (vfi_layout=0, EGM scripts); z1 is 1-based
 * (sim_z(1)); k1 = sim_k(1); uniforms = the T-1 `rand` draws of :106.  Outputs mean(sim_k)
 * and, if non-NULL, the T-long sim_k path and 1-based sim_z path. */
int aiy_sim_capital(const double* policy_k, int vfi_layout, const double* a_grid,
                    const double* P, int64_t N, int64_t Na, int64_t z1, double k1, int64_t T,
                    const double* uniforms, double* k_supply, double* sim_k, int32_t* sim_z);

/* A10 (new; no reference code) — stationary distribution by histogram iteration.
 * On-grid policy (policy_idx, 1-based; pass policy_k = NULL) or off-grid lottery between
 * the bracketing nodes (policy_k; policy_idx = NULL).  All arrays in the script's layout:
 * N x Na if vfi_layout, else Na x N.  lambda in/out (in = initial guess).  Iterates until
 * max|Δλ| < tol or max_iter; returns K = Σ_ij λ(i,j)·a_j, iters, final max|Δλ|.
 * Any N >= 1: a monotone policy with N <= 16 pushes in one launch (a wave per state), larger
 * N in two (run gather + projection); a non-monotone policy takes the ordered-scan gather.
 * The additions are the same on every path (bit-identical λ). */
int aiy_dist_stationary(const int32_t* policy_idx, const double* policy_k, int vfi_layout,
                        const double* a_grid, const double* P, int64_t N, int64_t Na,
                        double tol, int64_t max_iter, double* lambda, double* k_supply,
                        int64_t* iters, double* dist);

/* A10 at C candidate policies (one GE round's supplies): candidate c's policy and lambda are
 * block c of policy_idx / policy_k and lambda (each block laid out as in aiy_dist_stationary);
 * lambda in (the candidate's start) / out, k_supply, iters, dist: host [C].  Every candidate's
 * results equal one aiy_dist_stationary call's bit for bit (aiy_dist_stationary_batch_dev). */
int aiy_dist_stationary_batch(int64_t C, const int32_t* policy_idx, const double* policy_k,
                              int vfi_layout, const double* a_grid, const double* P, int64_t N,
                              int64_t Na, double tol, int64_t max_iter, double* lambda,
                              double* k_supply, int64_t* iters, double* dist);

/* Config 4 / SURVEY B2 `ge_batch` — excess demand at C candidate rates: for each r(c) the
 * body of one GE step of Aiyagari_VFI.m:147-195: the VFI from v_start (N x Na, the common warm
 * start) to tol, the Monte-Carlo capital supply from (z1 1-based, k1) with the candidate's own
 * T-1 uniforms (column c of the (T-1) x C matrix `uniforms`), and K_d = labor·(α/(r+δ))^(1/(1-α)).
 * The candidates are split over n_devices GPUs of this process (batched solve + batched chains
 * per device, one host thread per device).  Out (C each): k_supply, k_demand, iters.  The
 * bracketing logic (:196-204) stays with the caller.  a_grid must be strictly increasing. */
int aiy_ge_batch(const double* r, int64_t C, const double* v_start, const double* a_grid,
                 const double* s, const double* P, int64_t N, int64_t Na, double alpha,
                 double delta, double beta, double sigma, double labor, double tol,
                 int64_t max_iter, int64_t z1, double k1, int64_t T, const double* uniforms,
                 int n_devices, double* k_supply, double* k_demand, int64_t* iters);

/* E2 — the same for the EGM scripts: for each candidate c the body of one GE step of
 * Aiyagari_EGM.m:177-242 (labor_flag: Aiyagari_Endogenous_Labor_EGM.m:174-240): the EGM solve
 * at (r[c], w[c]) from policy_c_start (Na x N, the common warm start; the scripts keep w at its
 * r0 value, so w is the caller's), the Monte-Carlo supply with column c of `uniforms`, and K_d
 * from `labor` (the aggregate).  One batched solve (aiy_egm_solve_batch_dev) and one batched
 * launch of the chains per device.  Out (C each): k_supply, k_demand, iters, status — 0 ok,
 * 1 = a non-increasing endogenous grid ended the candidate's solve, 2 = find() came up empty in
 * its chain; k_supply is NaN where status != 0 (the chain of a failed solve is skipped) and the
 * call still returns AIY_OK.  a_grid strictly increasing; N <= 16. */
int aiy_egm_ge_batch(const double* r, const double* w, int64_t C, const double* policy_c_start,
                     const double* a_grid, const double* s, const double* P, int64_t N,
                     int64_t Na, double alpha, double delta, double beta, double sigma,
                     double amin, int labor_flag, double phi, double theta, double labor,
                     double tol, int64_t max_iter, int64_t z1, double k1, int64_t T,
                     const double* uniforms, int n_devices, double* k_supply, double* k_demand,
                     int64_t* iters, int32_t* status);

/* E2 — the same for Aiyagari_Endogenous_Labor_VFI.m: for each candidate c the body of one GE
 * step (:166-245): the labour VFI at r[c] and its own w = (1-α)(α/(r+δ))^(α/(1-α)), every
 * candidate from the same v_start, incoming v_new and policies (N x Na column-major; the script
 * carries them across GE steps and a state with no feasible (l, a') keeps them, :85;
 * v_new_start, policy_*_start and policy_lin_start — 1-based — are nullable: zeros / index 1),
 * the Monte-Carlo supply on policy_k with column c of `uniforms`, and K_d from `labor`.  One
 * batched solve (aiy_labor_vfi_solve_batch_dev) and one batched launch of the chains per device.
 * Layouts, errors (AIY_FIND_EMPTY included) and the device split as aiy_ge_batch.  Out (C each):
 * k_supply, k_demand, iters. */
int aiy_labor_ge_batch(const double* r, int64_t C, const double* v_start,
                       const double* v_new_start, const double* policy_k_start,
                       const double* policy_l_start, const double* policy_c_start,
                       const int32_t* policy_lin_start, const double* a_grid, const double* s,
                       const double* P, const double* labor_choice, int64_t N, int64_t Na,
                       int64_t Nl, double alpha, double delta, double beta, double sigma,
                       double psi, double eta, double labor, double tol, int64_t max_iter,
                       int64_t z1, double k1, int64_t T, const double* uniforms, int n_devices,
                       double* k_supply, double* k_demand, int64_t* iters);

/* The histogram supply (A10) in place of the Monte-Carlo chains: aiy_ge_batch with K_s of
 * candidate c = Σ λ_c·a, λ_c the stationary distribution of the solve's index policy iterated
 * from lambda_start (N x Na column-major, the common start; NULL: uniform 1/(N·Na)) until
 * max|Δλ| < dist_tol or dist_max_iter pushes — one batched VFI solve and one batched histogram
 * solve (aiy_dist_stationary_batch_dev) per device.  Out (C each): k_supply, k_demand, iters
 * (VFI sweeps), dist_iters (pushes). */
int aiy_ge_hist_batch(const double* r, int64_t C, const double* v_start, const double* a_grid,
                      const double* s, const double* P, int64_t N, int64_t Na, double alpha,
                      double delta, double beta, double sigma, double labor, double tol,
                      int64_t max_iter, double dist_tol, int64_t dist_max_iter,
                      const double* lambda_start, int n_devices, double* k_supply,
                      double* k_demand, int64_t* iters, int64_t* dist_iters);
/* The same for the EGM scripts: aiy_egm_ge_batch with the lottery histogram on the solve's
 * policy_k (lambda_start Na x N, nullable).  A candidate with status 1 is skipped: k_supply NaN,
 * dist_iters 0. */
int aiy_egm_ge_hist_batch(const double* r, const double* w, int64_t C,
                          const double* policy_c_start, const double* a_grid, const double* s,
                          const double* P, int64_t N, int64_t Na, double alpha, double delta,
                          double beta, double sigma, double amin, int labor_flag, double phi,
                          double theta, double labor, double tol, int64_t max_iter,
                          double dist_tol, int64_t dist_max_iter, const double* lambda_start,
                          int n_devices, double* k_supply, double* k_demand, int64_t* iters,
                          int64_t* dist_iters, int32_t* status);

/* A6 — replaces Krusell_Smith_VFI.m:149-168 (policy improvement with fminbnd).
 * value, k_opt: k x K x S column-major (S = 4); B 4; P 4 x 4; params = 13 doubles {beta, alpha,
 * delta, k_min, k_max, ug, ub, l_bar, mu, z_grid(1), z_grid(2), eps_grid(1), eps_grid(2)}.  nfev (nullable,
 * k x K x S) = fminbnd function evaluations per node.
 * The A6/A7/A8 entry points need a strictly increasing k_grid (a repeated point:
 * AIY_BAD_ARG); the A6/A7 ones refuse ±inf in value (AIY_NON_FINITE; NaN is accepted). */
int ks_policy_improve(const double* value, const double* k_grid, const double* K_grid,
                      const double* B, const double* P, const double* params, int64_t nk,
                      int64_t nK, double* k_opt, int32_t* nfev);
/* A7 — replaces Krusell_Smith_VFI.m:172-192 (`steps` Jacobi Howard sweeps). value in/out. */
int ks_howard(double* value, const double* k_opt, const double* k_grid, const double* K_grid,
              const double* B, const double* P, const double* params, int64_t nk, int64_t nK,
              int64_t steps);
/* A6+A7 — replaces the VFI loop Krusell_Smith_VFI.m:143-204 for one ALM coefficient B:
 * improvement every 5th iteration, `howard_steps` sweeps, relative-diff stop (:195-203).
 * n_devices > 1 = ks_vfi_solve_sharded(..., n_devices, depth = 4).  k_opt is in/out (used
 * until the first improvement).  iters = VFI iterations run, rel_diff = last max relative
 * change. */
int ks_vfi_solve(double* value, double* k_opt, const double* k_grid, const double* K_grid,
                 const double* B, const double* P, const double* params, int64_t nk,
                 int64_t nK, int64_t howard_steps, double tol, int64_t max_vfi,
                 int n_devices, int64_t* iters, double* rel_diff);
/* The same loop over n_shards (K, Z) slices in one process: up to K_size
 * shards split the K range (all four s), up to 2·K_size split each K range by aggregate state
 * too (the reference K = 4 runs on 8 devices); shard d on device d % visible, peer access
 * enabled between the devices in use.  Howard sweeps run in blocks of `depth`: before a block
 * each shard receives the value columns of its ghost rectangle (every column its next `depth`
 * sweeps read, peer copies over xGMI) and sweeps the shrinking rectangles with the fused
 * Howard+slopes kernel — one exchange per block, event-synchronised on the streams.  depth = 0:
 * the direct schedule — no copies and no ghost sweeps: every sweep reads each forecast column
 * where its owner keeps it (peer pointers; needs peer access between the devices in use) and
 * waits only for its neighbours' previous sweep (stream-event waits).  Results equal the
 * single-device solve bit for bit for every n_shards and depth. */
int ks_vfi_solve_sharded(double* value, double* k_opt, const double* k_grid,
                         const double* K_grid, const double* B, const double* P,
                         const double* params, int64_t nk, int64_t nK, int64_t howard_steps,
                         double tol, int64_t max_vfi, int n_shards, int depth, int64_t* iters,
                         double* rel_diff);

/* A6+A7 at C candidate economies in one launch: workgroup c runs ks_vfi_solve's one-workgroup
 * loop (improvement on iterations 1, 6, 11, ..., `howard_steps` Jacobi sweeps with the slopes
 * rebuilt before each, the NaN-ignoring relative-difference stop) on candidate c's own value and
 * k_opt with its own K_grid row, B, P and params; k_grid, the sizes, howard_steps, tol and
 * max_vfi are shared.  Layouts as ks_vfi_solve, candidate-major: value and k_opt [C] of
 * k x K x 4 column-major (in/out), K_grid [C][nK], B [C][4], P [C] of MATLAB 4 x 4, params
 * [C][13]; iters, rel_diff [C].  Candidate c's value, k_opt, iters and rel_diff equal one
 * ks_vfi_solve call's bit for bit; a candidate cannot affect another (a NaN value block runs to
 * max_vfi on its own).  Refused before any device work: NULL arguments, C outside [1, 65,535],
 * k_size < 3, max_vfi outside [1, 2^31), a k_grid that is not strictly increasing, ±inf in a
 * candidate's value (AIY_NON_FINITE naming the candidate; NaN is accepted), and a size past the
 * one-workgroup rule (k_size * K_size * 4 <= 4,096 nodes) -> AIY_BAD_SHAPE: the batch has NO
 * tiled fallback (ks_vfi_solve runs such sizes tiled, one economy per call).  Scratch: the
 * library's cached host-tier buffers. */
int ks_vfi_solve_batch(int64_t C, double* value, double* k_opt, const double* k_grid,
                       const double* K_grid, const double* B, const double* P,
                       const double* params, int64_t nk, int64_t nK, int64_t howard_steps,
                       double tol, int64_t max_vfi, int64_t* iters, double* rel_diff);

/* A8: the EGM policy iteration of Krusell_Smith_EGM.m:129-209 for the current B (replaces the
 * `for egm_iter = 1:max_egm` loop, :130-209).  k_opt: k_size x K_size x 4, in/out (:96 start).
 * Gauss-Seidel over (s_i outer, K_i inner) exactly as the script: each (s, K) column is
 * overwritten as soon as it is computed (:199).  Stops when max|k_opt - k_opt_old| < tol
 * (:204-207) or after max_iter sweeps; iters = sweeps run, diff = the last max change.
 * AIY_NON_FINITE if some (s, K) pair has fewer than 2 EGM points inside [k_min, k_max]
 * (MATLAB's griddedInterpolant would raise there). */
int ks_egm_solve(double* k_opt, const double* k_grid, const double* K_grid, const double* B,
                 const double* P, const double* params, int64_t nk, int64_t nK, double tol,
                 int64_t max_iter, int64_t* iters, double* diff);

/* F1 — the Jacobi variant of A8, flagged NON-PARITY: every (s, K) pair of a
 * sweep reads the previous sweep's k_opt (the script is Gauss-Seidel, Krusell_Smith_EGM.m:199,
 * so this converges to the same fixed point within tol but along a different path and in a
 * different number of sweeps).  All pairs of a sweep run in parallel, one workgroup each.
 * Same arguments, layout, stop rule and errors as ks_egm_solve; bit-exact against the C/numpy
 * Jacobi restatements (oracle/). */
int ks_egm_solve_jacobi(double* k_opt, const double* k_grid, const double* K_grid,
                        const double* B, const double* P, const double* params, int64_t nk,
                        int64_t nK, double tol, int64_t max_iter, int64_t* iters, double* diff);

/* A8 at C candidate economies in one launch: workgroup c runs ks_egm_solve's loop on candidate
 * c's own k_opt with its own K_grid row, B, P and params; k_grid, the sizes, tol and max_iter are
 * shared.  Layouts as ks_egm_solve, candidate-major: k_opt [C] of k x K x 4 column-major
 * (in/out), K_grid [C][nK], B [C][4], P [C] of MATLAB 4 x 4, params [C][13]; iters, diff, status
 * [C].  Every candidate's k_opt, iters and diff equal one ks_egm_solve call's bit for bit.
 * The return code is about the call: status[c] = 1 marks a candidate that met fewer than 2 valid
 * EGM points (ks_egm_solve's AIY_NON_FINITE; its k_opt slice is unspecified), the others are
 * unaffected and the call returns AIY_OK.  Refused before any device work: NULL arguments, C
 * outside [1, 65,535], k_size < 3, max_iter outside [1, 2^31), a size past the one-workgroup LDS
 * rule of ks_egm_solve, a k_grid that is not strictly increasing, a K_grid row that is not
 * positive and finite.  Scratch: the library's cached host-tier buffers. */
int ks_egm_solve_batch(int64_t C, double* k_opt, const double* k_grid, const double* K_grid,
                       const double* B, const double* P, const double* params, int64_t nk,
                       int64_t nK, double tol, int64_t max_iter, int64_t* iters, double* diff,
                       int32_t* status);

/* F3 — replaces the shock simulation Krusell_Smith_VFI.m:57-94 (also Krusell_Smith_EGM.m).
 * uniforms: the script's `rand` stream, ks_shock_draws(T, population) values in its draw order
 * (T-1 aggregate draws :63/:65, `population` draws :71, then (T-1)*population draws with t
 * outer and i inner :89/:91).  params: the 13 KS doubles (ug = params[5], ub = params[6]).
 * out: zi_shock T (0 good / 1 bad: the value after `zi_shock - 1`, :68) and epsi_shock
 * T x population column-major (1 employed / 2 unemployed). */
int64_t ks_shock_draws(int64_t T, int64_t population);
int ks_shocks(int64_t T, int64_t population, const double* uniforms, const double* params,
              double* zi_shock, double* epsi_shock);

/* F2 — replaces the capital path simulation Krusell_Smith_VFI.m:206-248 (Krusell_Smith_EGM.m
 * :211-253).  k_opt k x K x 4; zi_shock T; epsi_shock T x population (as ks_shocks returns);
 * k_population in/out (it persists across ALM iterations in the script, :101); K_ts out (T).
 * Every agent moves to griddedInterpolant({k_grid, K_grid}, k_opt(:,:,s))(k, K_ts(t)) (2-D
 * linear, linear extrapolation), s from (z_t, eps_t,i) in s_grid order; K_ts(t+1) =
 * mean(k_population) summed in the fixed order documented in DESIGN.md (MATLAB's is unpinned). */
int ks_simulate_capital(const double* k_opt, const double* k_grid, const double* K_grid,
                        int64_t nk, int64_t nK, const double* zi_shock,
                        const double* epsi_shock, int64_t T, int64_t population,
                        double* k_population, double* K_ts);

/* F2 histogram — the non-stochastic simulation (Young 2010) of the capital path beside the
 * agent panel of ks_simulate_capital (new; no reference counterpart).  A distribution lam over
 * (employment, node of x_grid) is pushed through M aggregate shock paths with the period's
 * policy; K_ts(t, m) = sum(lam .* x) is its first moment (not normalised).  k_opt k x K x 4;
 * x_grid nx (strictly increasing, nx >= 2); params: the 13 KS doubles; zi_shock T x M
 * column-major (0 good / 1 bad); lam nx x 2 x M column-major, in/out (column 1 employed,
 * 2 unemployed; out: the distribution of period T); K_ts out T x M; slow_periods (nullable,
 * M): periods whose lottery keys were not monotone and were summed by the ordered scan.
 * The recursion and both summation orders are stated in csrc/ks_hist_kernels.hip and DESIGN.md
 * §5.  One launch: path m is one workgroup, so a path's state must fit one CU's LDS
 * (8*(8*nx + K_size + 8) + 4*(5*nx + 4) <= 160 KiB, else AIY_BAD_SHAPE); 1 <= M <= 65,535,
 * T >= 2. */
int ks_simulate_hist(const double* k_opt, const double* k_grid, const double* K_grid, int64_t nk,
                     int64_t nK, const double* x_grid, int64_t nx, const double* params,
                     const double* zi_shock, int64_t T, int64_t M, double* lam, double* K_ts,
                     int64_t* slow_periods);
/* The same with one policy per path: path m is simulated with candidate c = policy_of_path[m]
 * (int32, 0-based, each in [0, C)): k_opt block c of [C] k x K x 4, row c of K_grid [C][K_size],
 * and the employment transitions of params row c of [C][13].  k_grid, x_grid, T and the layouts
 * of zi_shock, lam, K_ts and slow_periods are ks_simulate_hist's; path m's results equal one
 * ks_simulate_hist call with candidate c alone bit for bit.  All of ks_simulate_hist's checks
 * (per candidate where the input is), 1 <= C <= 65,535 and the range of policy_of_path are made
 * before the device is touched. */
int ks_simulate_hist_multi(int64_t C, const double* k_opt, const double* k_grid,
                           const double* K_grid, int64_t nk, int64_t nK, const double* x_grid,
                           int64_t nx, const double* params, const int32_t* policy_of_path,
                           const double* zi_shock, int64_t T, int64_t M, double* lam,
                           double* K_ts, int64_t* slow_periods);

/* ======================================================================================
 * Device tier: [N][Na] (z-major) arrays in HBM, async on `stream` (hipStream_t).
 * A workspace holds the per-shape scratch (EV/D tables, init/partial buffers, events).
 * ====================================================================================== */
typedef struct aiy_ws aiy_ws;
int aiy_ws_create(int64_t N, int64_t Na, int64_t Nl, aiy_ws** ws);
int aiy_ws_destroy(aiy_ws* ws);
/* instrumentation.  enable bit 0: HIP events bracket the dominant kernel of every call on its
 * stream (aiy_ws_timing reads the accumulated milliseconds and launch count); bit 1: the
 * screened sweep counts its work (aiy_ws_counters; atomics, so never together with timing
 * when the time matters). */
int aiy_ws_set_timing(aiy_ws* ws, int enable);
int aiy_ws_timing(aiy_ws* ws, double* total_ms, int64_t* launches, int64_t* hits);
/* work counters of the screened Bellman sweep since aiy_ws_set_timing(ws, 2): out[0] exact
 * candidate evaluations, out[1] superblock (512-candidate) tests, out[2] block (64) tests,
 * out[3] candidates screened individually — each counted per state.  Instrumentation only. */
int aiy_ws_counters(aiy_ws* ws, int64_t out[4]);
/* 8-candidate blocks the tree sweep's candidate screen ran since aiy_ws_set_timing(ws, 2), by
 * body: out[0] with the clamp max(c, 0), out[1] without it (the block lies below every feasible
 * prefix of its wave, where the clamp is the identity).  Instrumentation only. */
int aiy_ws_screen_paths(aiy_ws* ws, int64_t out[2]);
/* per-work-item trace of the last tree sweep (aiy_ws_set_timing bit 2): 16 int64 per item
 * {start clock, end clock (100 MHz wall clock), XCD id, superblock tests, block tests,
 * candidates, exact evaluations, hardware block id, wave-0 shader cycles in: startup and
 * superblock tests, superblock bound tests, fine screens, exact paths; 4 reserved}.
 * Instrumentation only. */
int aiy_ws_trace(aiy_ws* ws, int64_t* out, int64_t cap, int64_t* n);
/* The workspace caches the feasible prefixes #{k : a_k < cash(j, l)}, which depend on
 * (r, w, a_grid, s, labor_choice) only, keyed by r, w and the pointers.  Call this after
 * overwriting a_grid / s / labor_choice in place. */
int aiy_ws_invalidate(aiy_ws* ws);
/* search knobs (defaults tuned for gfx950): coarse stride for cold starts, k-chunk (a multiple
 * of 64: candidates a' per screen work item). */
int aiy_ws_set_search(aiy_ws* ws, int coarse_stride, int k_chunk);
/* VFI solves (A2, all tiers) enqueue up to max_batch sweeps between reads of max|v_new-v_old|
 * (default 16; 0 or 1 = one synchronisation per sweep).  Sweeps past the stopping sweep are
 * discarded, so iteration count, v_new, v_old and policies do not depend on it; memory: two
 * batches in flight — 2·max_batch + 1 value buffers and 2·max_batch policy sets per workspace. */
int aiy_ws_set_speculation(aiy_ws* ws, int max_batch);
/* The small-grid sweep (A1 / A3 at integer sigma in [2, 9], mode 0/1, Nz below the MFMA
 * expectation's threshold): ONE launch per sweep — expectation, screen, merge and outputs —
 * with a workgroup of `waves` waves (4, 8 or 16) per tile of `states` states (8, 16, 32 or 64;
 * each wave splits the candidates into 64 / states slices) and `splits` workgroups per tile
 * splitting the candidate range further.  Used when Na <= max_na and the variant is the default
 * (-1) or has bit 25 set.  max_na = -1: the default bound; 0: never.  splits / waves / states =
 * 0: chosen by size.  Results are identical to the tree sweep's for every setting. */
int aiy_ws_set_wide(aiy_ws* ws, int max_na, int splits, int waves, int states);
/* on = 1: every small-grid sweep launch of this workspace (aiy_ws_set_wide) reserves whole CUs
 * (each workgroup asks for >= 88 KiB of LDS, so no second workgroup that uses LDS can share its
 * CU).  For solves run concurrently on several streams (the speculative GE driver): a workgroup
 * sharing its CU with another solve's becomes the straggler of its sweep.  Default 0.  Results do
 * not depend on it. */
int aiy_ws_set_cu_exclusive(aiy_ws* ws, int on);
/* The A9 chain (aiy_sim_capital_dev) on this workspace: mode -1 (default) runs the speculative-
 * segment chain (16 waves each run a segment of the k recurrence from a guess, then repair it
 * from its predecessor's true end until the stored path matches bit for bit; the state path by a
 * parallel scan of composed transition maps) for 2,048 <= T <= 16,384, N <= 7, 64 <= Na <= 960,
 * the serial kernels otherwise — spread over 16 workgroups (four launches: the state path; the
 * segments; the first repair pass; further passes if any and the in-order sum); 0: always the
 * serial kernels; 1: the speculative chain in one workgroup per chain wherever it applies; 2: the
 * spread variant wherever it applies.  Results (K_s, the paths, find() errors) are identical for
 * every mode. */
int aiy_ws_set_sim(aiy_ws* ws, int mode);
/* kernel shapes and A/B knobs (tuning only; results are identical for every value in
 * [-1, 2^30)).  VFI, bit 3 clear (default): the bound tree screen, bit 0 = 2 states per lane
 * (else 1), bits 1-2 = 1, 2, 4 or 8 cooperating waves per tile, bit 4 = XCD-aware tile order,
 * bit 6 / bit 11 = one-wave tiles dispatched from a per-workspace permutation that keeps each
 * XCD's tile range and deals it heaviest first / row-major with its cheapest tiles last, bit 13 =
 * one-wave tiles narrowed to ceil(N·Na / 3072) states (>= 16), bits 16-17 = (with bit 6 or
 * 11, A1 at sigma = 5) 1, 2, 4 or 8 one-wave tiles per workgroup, bit 21 = the start-up
 * extrapolates the argmax drift from the last two sweeps' shifts (else the last shift), bit 22 =
 * every screen keeps its clamp (no identity fast path: A/B and tests), bit 23 =
 * the hint's own window is the hint alone when the extrapolated window is evaluated, bit 24
 * (with 23) = not even the hint then;
 * bit 3 set: the chunked screen + merge, with bit 0 = 4 states per lane (else 2), bit 1 =
 * registers capped for 8 waves per SIMD, bit 2 = fp64-only screen (else the packed fp32
 * pre-screen with directed-rounding bounds first).  Tree screen extras: bit 5 = no hill-climb
 * from the hint, bits 7-8 = hint window half-width 1, 2, 4 or 8, bit 9 = no extrapolated
 * (hint + last shift) start, bit 10 = the plain exhaustive scan, bit 12 = cooperating waves
 * deal the first superblock's passing 8-blocks round-robin (else by 64-block), bits 14 / 15 =
 * force the VALU / MFMA expectation.  EGM steps on this workspace (their own bits, so a VFI
 * variant never changes the EGM path): bit 18 = two launches per step even when Na <= 1024
 * (default there: one fused launch); bit 19 = no chaining in the solve loops (two launches per
 * step); bit 20 = no interp1 segment windows.  Bit 25: the small-grid one-launch sweep
 * (aiy_ws_set_wide) even with an explicit variant.  Bit 26 (with bit 6 or 11, A1 at sigma = 5):
 * the hybrid tree launch — two-wave workgroups that run two one-wave tiles, or one of each XCD
 * range's heaviest tiles on both waves; bits 27-29: those cooperative tiles per XCD range,
 * 8 << value.  -1 (default): chosen by size — Na <= 4096:
 * 2 cooperating waves per tile (A1), 4 with bit 12 (labour); else 16 | 2048 | 1 << 16 |
 * 1 << 21 | 1 << 23 | 1 << 24 (A1), 16 | 1 << 21 (labour) and 16 | 1 << 21 (the batched
 * multi-rate solve). */
int aiy_ws_set_variant(aiy_ws* ws, int variant);

/* A1 on device.  hint (nullable, [N][Na] int32 0-based) = previous sweep's argmax; the result
 * does not depend on it, only the run time.  diff (nullable, device double[2]) receives
 * {max|v_new-v_old| ignoring NaN, 1 if any non-NaN}.  mode: 0 = auto, 1 = screened
 * exhaustive (integer sigma>=2), 2 = plain exhaustive (any sigma). */
int aiy_vfi_sweep_dev(aiy_ws* ws, const double* v_old, const double* a_grid, const double* s,
                      const double* P, double r, double w, double beta, double sigma,
                      const int32_t* hint, int mode, double* v_new, int32_t* idx,
                      double* policy_k, double* policy_c, double* diff, void* stream);
/* nsweeps sweeps of A1 on device (Aiyagari_VFI.m:70-83 repeated, as the A2 loop runs them
 * without the stop test): sweep 1 reads v_a and writes v_b, sweep g reads the buffer sweep g-1
 * wrote (ping-pong), so after the call v_new is in v_b when nsweeps is odd, else in v_a.  hint
 * (nullable) is sweep 1's hint, every later sweep's hint is idx (the previous argmax).  idx,
 * policy_k, policy_c hold the last sweep's policies; diff (nullable, device double[2]) its
 * {max|v_new-v_old|, any}.  Results equal nsweeps aiy_vfi_sweep_dev calls bit for bit. */
int aiy_vfi_sweeps_dev(aiy_ws* ws, double* v_a, double* v_b, const double* a_grid,
                       const double* s, const double* P, double r, double w, double beta,
                       double sigma, const int32_t* hint, int64_t nsweeps, int mode, int32_t* idx,
                       double* policy_k, double* policy_c, double* diff, void* stream);
/* A2 on device: v_a (in: v_old) and v_b are ping-pong buffers; on return *out_new points
 * (0 = v_a, 1 = v_b) to the buffer holding v_new, the other holds v_old (break semantics).
 * idx doubles as the hint between sweeps. */
int aiy_vfi_solve_dev(aiy_ws* ws, double* v_a, double* v_b, const double* a_grid,
                      const double* s, const double* P, double r, double w, double beta,
                      double sigma, double tol, int64_t max_iter, int mode, int32_t* idx,
                      double* policy_k, double* policy_c, int64_t* iters, int* out_new,
                      void* stream);
/* Config 4 (BASELINE configs[3]) on device: C candidate rates solved together, each the A2
 * loop of Aiyagari_VFI.m:147-171 (its own stop at :85, break semantics :85-88).  r, w: host
 * [C]; v_a (in: each candidate's starting v_old), v_b, idx, policy_k, policy_c: device
 * [C][N][Na].  use_hint != 0: idx holds a hint (e.g. the r0 solution's argmax) on entry.
 * Out (host [C]): iters = sweeps of each candidate, which = 1 if its v_new is in v_b (its
 * v_old in v_a), else 0.  Every sweep is one launch pair over all running candidates; results
 * equal C separate aiy_vfi_solve_dev calls bit for bit. */
int aiy_vfi_solve_batch_dev(aiy_ws* ws, int64_t C, const double* r, const double* w,
                            double* v_a, double* v_b, const double* a_grid, const double* s,
                            const double* P, double beta, double sigma, double tol,
                            int64_t max_iter, int use_hint, int32_t* idx, double* policy_k,
                            double* policy_c, int64_t* iters, int32_t* which, void* stream);
int aiy_labor_vfi_sweep_dev(aiy_ws* ws, const double* v_old, const double* a_grid,
                            const double* s, const double* P, const double* labor_choice,
                            double r, double w, double beta, double sigma, double psi,
                            double eta, const int32_t* hint, double* v_new, int32_t* lin,
                            double* policy_k, double* policy_l, double* policy_c, double* diff,
                            void* stream);
/* nsweeps A3 sweeps on device (Aiyagari_Endogenous_Labor_VFI.m:69-112 repeated, as the loop
 * :64-122 runs them without the stop test), ping-pong from v_a as aiy_vfi_sweeps_dev: sweep 1
 * reads v_a and writes v_b (a state with no feasible (l, a') keeps v_b's incoming value), later
 * sweeps keep v_old there (:120); sweep 1's hint is `hint` (nullable), later ones lin.  lin and
 * the policies hold the last sweep's; diff (nullable, device double[2]) its {max|dv|, any}. */
int aiy_labor_vfi_sweeps_dev(aiy_ws* ws, double* v_a, double* v_b, const double* a_grid,
                             const double* s, const double* P, const double* labor_choice,
                             double r, double w, double beta, double sigma, double psi,
                             double eta, const int32_t* hint, int64_t nsweeps, int32_t* lin,
                             double* policy_k, double* policy_l, double* policy_c, double* diff,
                             void* stream);
/* A3 at C candidate rates on device: candidate c's whole loop
 * Aiyagari_Endogenous_Labor_VFI.m:64-122 at (r[c], w[c]) (host [C]; GE copy :166-219), its own
 * stop at :115-118.  v_a (in: each candidate's starting v_old), v_b (in: each candidate's
 * incoming v_new, which a state with no feasible (l, a') keeps, :85), lin (0-based l + Nl·k, as
 * the sweep entry points; in: the incoming index, and sweep 1's hint when use_hint != 0),
 * policy_k, policy_l, policy_c (in/out, nullable): device [C][N][Na]; labor_choice: device [Nl],
 * Nl the workspace's.  Out (host [C]): iters, which = 1 if the candidate's v_new is in v_b (its
 * v_old in v_a), else 0.  Where the shape takes the small-grid one-launch sweep (integer sigma in
 * [2, 9], Na within aiy_ws_set_wide's bound, Nl <= 16, N < 32) and C is at least the workspace's
 * threshold (aiy_ws_set_labor_batch), every sweep is ONE launch over all candidates still
 * running, each candidate tested and frozen on the device, and the host reads the stop flags
 * once per aiy_ws_set_speculation sweeps; otherwise the candidates run one after another through
 * the single-rate solve.  Either way the outputs equal C separate solves (aiy_labor_vfi_solve)
 * bit for bit.  The call synchronises the stream.  Errors before any device work: NULL
 * arguments, C outside [1, 2^20], max_iter < 1 (AIY_BAD_ARG / AIY_BAD_SHAPE), non-finite r or w
 * (AIY_NON_FINITE), C·Nl·N·Na past int32 (AIY_BAD_SHAPE). */
int aiy_labor_vfi_solve_batch_dev(aiy_ws* ws, int64_t C, const double* r, const double* w,
                                  double* v_a, double* v_b, const double* a_grid,
                                  const double* s, const double* P, const double* labor_choice,
                                  double beta, double sigma, double psi, double eta, double tol,
                                  int64_t max_iter, int use_hint, int32_t* lin, double* policy_k,
                                  double* policy_l, double* policy_c, int64_t* iters,
                                  int32_t* which, void* stream);
/* the batched labour solve's dispatch on this workspace: the one-launch-per-sweep path from
 * min_candidates on (0, the default: the measured threshold, DESIGN.md §5 — never a single
 * candidate; 1: whenever the shape fits).  Results do not depend on it. */
int aiy_ws_set_labor_batch(aiy_ws* ws, int min_candidates);
/* how often aiy_labor_vfi_solve_batch_dev took each path on this workspace since it was created:
 * batched solves (calls), and per-candidate solves of the other path (both nullable). */
int aiy_ws_labor_batch_counts(aiy_ws* ws, int64_t* batched_solves, int64_t* fallback_solves);
int aiy_egm_step_dev(aiy_ws* ws, const double* policy_c, const double* a_grid,
                     const double* s, const double* P, double r, double w, double beta,
                     double sigma, double amin, int labor, double phi, double theta,
                     double* policy_c_next, double* policy_k, double* policy_l, double* diff,
                     void* stream);
/* A4/A5 solve loop on device (Aiyagari_EGM.m:71-110, labour :64-107): policy_c (in: the guess,
 * out: the last policy_c_next) [N][Na]; policy_k, policy_l (labour, nullable otherwise)
 * [N][Na].  Speculative batches of steps between dist reads, as aiy_egm_solve; for Na > 1024
 * each step is ONE launch (interp1 of step t with the Euler RHS of step t+1 on the same tiles;
 * variant bit 13: two launches).  iters, dist: host. */
int aiy_egm_solve_dev(aiy_ws* ws, double* policy_c, const double* a_grid, const double* s,
                      const double* P, double r, double w, double beta, double sigma,
                      double amin, int labor, double phi, double theta, double tol,
                      int64_t max_iter, double* policy_k, double* policy_l, int64_t* iters,
                      double* dist, void* stream);
/* A4/A5 at C candidate rates on device: candidate c's whole solve loop at (r[c], w[c]) (host
 * [C]) from policy_c[c] (device [C][N][Na], in: the start, out: the last policy_c_next);
 * policy_k, policy_l (nullable unless labor): device [C][N][Na]; iters, dist, status: host [C].
 * Where a candidate's arrays fit one CU's LDS (Na <= 1024 and (2N+1)·Na doubles, labour 3N·Na,
 * within 160 KiB) and C is at least the workspace's threshold (aiy_ws_set_egm_batch), ONE launch
 * runs one workgroup per candidate with no host read between steps and the call synchronises
 * once; otherwise the candidates run one after another through aiy_egm_solve_dev.  For every
 * candidate with status 0 the outputs equal one aiy_egm_solve_dev call bit for bit (max_iter = 0
 * and tol >= 1 included).  status 1: a non-increasing endogenous grid ended that candidate's
 * loop (its outputs are undefined); the others are unaffected and the call returns AIY_OK. */
int aiy_egm_solve_batch_dev(aiy_ws* ws, int64_t C, const double* r, const double* w,
                            double* policy_c, const double* a_grid, const double* s,
                            const double* P, double beta, double sigma, double amin, int labor,
                            double phi, double theta, double tol, int64_t max_iter,
                            double* policy_k, double* policy_l, int64_t* iters, double* dist,
                            int32_t* status, void* stream);
/* the batched EGM solve's dispatch on this workspace: the one-launch path from min_candidates
 * on (-1, the default: the measured threshold; 1: whenever the shape fits; 0:
 * never).  Results do not depend on it. */
int aiy_ws_set_egm_batch(aiy_ws* ws, int min_candidates);
/* how often aiy_egm_solve_batch_dev took each path on this workspace since it was created:
 * one-launch batches, and per-candidate solves of the other path (both nullable). */
int aiy_ws_egm_batch_counts(aiy_ws* ws, int64_t* launches, int64_t* fallback_solves);
/* A9 on device: policy_rows [N][Na]; z1 0-based; k_supply (device double), sim_k/sim_z
 * nullable (device), status (device int32: 0 ok, 1 = find() empty). */
int aiy_sim_capital_dev(aiy_ws* ws, const double* policy_rows, const double* a_grid,
                        const double* P, int64_t z1, double k1, int64_t T,
                        const double* uniforms, double* k_supply, double* sim_k,
                        int32_t* sim_z, int32_t* status, void* stream);
/* A10 on device: one push λ → λ' ([N][Na]); policy_idx (0-based) or policy_k (lottery);
 * diff (nullable, device [2]) = {max|λ'−λ| bits, any}.  Synchronises once to read the
 * monotonicity flag (non-monotone policies take an exact ordered-scan fallback). */
int aiy_dist_update_dev(aiy_ws* ws, const double* lambda, const int32_t* policy_idx,
                        const double* policy_k, const double* a_grid, const double* P,
                        double* lambda_out, double* diff, void* stream);
/* A10 on device: the fixed-point loop of aiy_dist_stationary with everything in HBM.  The
 * policy's plan (run offsets) is built once; pushes run in speculative batches of up to 32
 * between reads of max|Δλ| (one synchronisation per batch).  lambda [N][Na] in (initial
 * guess, not modified); lambda_out [N][Na] = the last push; k_supply (nullable, device
 * double) = Σ λ·a; iters, dist host out. */
int aiy_dist_stationary_dev(aiy_ws* ws, const double* lambda, const int32_t* policy_idx,
                            const double* policy_k, const double* a_grid, const double* P,
                            double tol, int64_t max_iter, double* lambda_out,
                            double* k_supply, int64_t* iters, double* dist, void* stream);
/* A10 at C candidate policies on device: candidate c's fixed point from lambda[c] on
 * policy_idx[c] (0-based) or policy_k[c] (lottery) — all device [C][N][Na] — into lambda_out[c];
 * k_supply (nullable): device [C]; iters, dist: host [C].  For every candidate λ, K, iters and
 * dist equal one aiy_dist_stationary_dev call's bit for bit.  Where a candidate's arrays fit one
 * CU's LDS (N <= 16 and 8·N·Na·(2 + lottery) + 4·N·(Na+1) + 2.2 KB within 160 KiB) and C is at
 * least the workspace's threshold (aiy_ws_set_dist_batch), one prepare launch pair builds all
 * plans, their flags are read once, and ONE launch runs one workgroup per monotone candidate
 * with the whole loop in LDS, followed by one synchronisation.  A non-monotone candidate — and
 * every candidate otherwise — runs through the per-candidate solve.  An index outside [1, Na]
 * in any candidate: AIY_BAD_ARG naming the candidate (1-based), before any solve. */
int aiy_dist_stationary_batch_dev(aiy_ws* ws, int64_t C, const double* lambda,
                                  const int32_t* policy_idx, const double* policy_k,
                                  const double* a_grid, const double* P, double tol,
                                  int64_t max_iter, double* lambda_out, double* k_supply,
                                  int64_t* iters, double* dist, void* stream);
/* the batched histogram solve's dispatch on this workspace: the one-launch path from
 * min_candidates on (-1, the default: the measured threshold; 1: whenever the
 * shape fits; 0: never).  Results do not depend on it. */
int aiy_ws_set_dist_batch(aiy_ws* ws, int min_candidates);
/* how often aiy_dist_stationary_batch_dev took the one-launch path on this workspace, and how
 * many candidates it solved one by one (both nullable) */
int aiy_ws_dist_batch_counts(aiy_ws* ws, int64_t* launches, int64_t* fallback_solves);

/* ---- Transition paths (perfect foresight, MIT shocks; new — the scripts are stationary).
 * C price paths of T periods per call, ONE workgroup per path and pass, no launch between
 * periods.  Arrays are [N][Na] rows per (path, period).  A shape whose arrays do not fit one CU's
 * LDS is refused with AIY_BAD_ARG (no per-step fallback):
 *   backward: N <= 16, Na <= 1024, (2N+1)·Na doubles + 2.4 KB within 160 KiB;
 *   forward:  N <= 16, 8·N·Na·3 + 4·N·(Na+1) + 8·Na + 2.2 KB within 160 KiB.
 * The two-rate EGM step of period t (pc_next = the consumption policy of period t+1):
 *   RHS(j,a) = sum_m ((beta(1+r[t+1])) P(j,m)) u'(pc_next(m,a)),  c~ = RHS^(-1/sigma),
 *   a^(j,a) = ((c~ + a_grid(a)) - w[t] s_j) / (1 + r[t]),
 *   g = interp1(a^_j, a_grid, a_grid(a), linear, extrap), g < amin -> amin,
 *   pk_t = g,  pc_t = ((1 + r[t]) a_grid(a) + w[t] s_j) - g
 * — aiy_egm_step's operations with r split in two: on r[t+1] == r[t] it equals that step bit for
 * bit.  The labour step, A5, has the same entries under aiy_labor_* (below).
 *
 * Backward pass on device: r host [C][T+1] (r[c][T]: the terminal rate of period T-1's Euler
 * equation), w host [C][T]; pc_T device [C][N][Na], or one [N][Na] for all paths (pc_T_shared);
 * policy_k, policy_c (nullable): device [C][T][N][Na]; status, fail_t: host [C].  Exactly T steps
 * from t = T-1 down.  status 1: the endogenous grid of period fail_t was not increasing (NaN
 * included) — that path stops there (periods above fail_t are complete, the others undefined);
 * the other paths are unaffected and the call returns AIY_OK.  Refused on the host before any
 * launch: C < 1, T < 1, a non-finite r or w, 1 + r <= 0.  Synchronises once. */
int aiy_egm_backward_batch_dev(aiy_ws* ws, int64_t C, int64_t T, const double* r, const double* w,
                               const double* pc_T, int pc_T_shared, const double* a_grid,
                               const double* s, const double* P, double beta, double sigma,
                               double amin, double* policy_k, double* policy_c, int32_t* status,
                               int32_t* fail_t, void* stream);
/* Forward pass on device: from lambda0 (device [C][N][Na], or one [N][Na]: lambda0_shared), period
 * t = 0 .. T-1: the lottery plan of policy_k[c][t] (aiy_dist_update_dev's), K[c][t] = sum
 * lambda_t a (aiy_dist_stationary_dev's k_supply sum), one push.  K: device [C][T+1] (K[c][T] of
 * the last lambda); lambda_T (nullable): device [C][N][Na]; status, fail_t: host [C].  status 2:
 * the keys of policy_k[c][fail_t] are not monotone — that path stops there (K up to fail_t is
 * written, the rest NaN, lambda_T = lambda at fail_t).  Synchronises once. */
int aiy_dist_forward_batch_dev(aiy_ws* ws, int64_t C, int64_t T, const double* policy_k,
                               const double* lambda0, int lambda0_shared, const double* a_grid,
                               const double* P, double* K, double* lambda_T, int32_t* status,
                               int32_t* fail_t, void* stream);
/* The same two passes on host arrays (P column-major N x N, as aiy_egm_step).  Also refused
 * before any launch: an a_grid that is not strictly increasing. */
int aiy_egm_backward_batch(int64_t C, int64_t T, const double* r, const double* w,
                           const double* pc_T, int pc_T_shared, const double* a_grid,
                           const double* s, const double* P, int64_t N, int64_t Na, double beta,
                           double sigma, double amin, double* policy_k, double* policy_c,
                           int32_t* status, int32_t* fail_t);
int aiy_dist_forward_batch(int64_t C, int64_t T, const double* policy_k, const double* lambda0,
                           int lambda0_shared, const double* a_grid, const double* P, int64_t N,
                           int64_t Na, double* K, double* lambda_T, int32_t* status,
                           int32_t* fail_t);
/* Both passes on one stream: the period policies stay on the device and the host reads K
 * [C][T+1], status and fail_t [C] only.  A path the backward pass stopped (status 1) has K all
 * NaN; status 2 as aiy_dist_forward_batch_dev. */
int aiy_transition_batch(int64_t C, int64_t T, const double* r, const double* w,
                         const double* pc_T, int pc_T_shared, const double* lambda0,
                         int lambda0_shared, const double* a_grid, const double* s,
                         const double* P, int64_t N, int64_t Na, double beta, double sigma,
                         double amin, double* K, int32_t* status, int32_t* fail_t);
/* Sequence-space Jacobian of the capital path (fake-news algorithm; n = N·Na).
 *
 * Expectation vectors of C policies: with dist_update's lottery plan of policy_k[c] (x = the
 * policy clamped to the grid, lo its bracket, wr = (x - a(lo)) / (a(lo+1) - a(lo)), wl = 1 - wr),
 * E_0 = y0 and, t = 0 .. T-2,
 *   G_t(i,k') = sum_m P(i,m) E_t(m,k')  (m ascending),
 *   E_{t+1}(i,k) = wl(i,k) G_t(i,lo(i,k)) + (1 - wl(i,k)) G_t(i,lo(i,k)+1)
 * — the transpose of the forward pass's push: E_t·lambda_0 = y0·lambda_t under the constant
 * policy.  No fused multiply-adds.  policy_k: [C][N][Na]; y0: [C][N][Na], or one [N][Na] for all
 * (y0_shared); E: [C][T][N][Na].  ONE workgroup per c, exactly T-1 steps.  Fit rule (else
 * AIY_BAD_ARG, no per-step fallback): N <= 16, 28·N·Na + 2 KB within 160 KiB.  A NaN in
 * policy_k[c] stays inside E[c].  The device entry only enqueues on `stream`. */
int aiy_dist_expect_batch_dev(aiy_ws* ws, int64_t C, int64_t T, const double* policy_k,
                              const double* y0, int y0_shared, const double* a_grid,
                              const double* P, double* E, void* stream);
/* host arrays; P column-major N x N; also refused: an a_grid that is not strictly increasing */
int aiy_dist_expect_batch(int64_t C, int64_t T, const double* policy_k, const double* y0,
                          int y0_shared, const double* a_grid, const double* P, int64_t N,
                          int64_t Na, double* E);
/* Fake-news matrices and Jacobians of n_in inputs.  E: [T][n]; lambda1: [n_in + 1][T][n], block 0
 * the base path's one-step distributions, block x + 1 those of input x, period T-1-s holding the
 * response to news s periods ahead.  With D_x[s] = (lambda1[x+1][T-1-s] - lambda1[0][T-1-s]) / h
 * (elementwise; never stored),
 *   F[x][t][s] = sum_k E[t][k] D_x[s][k]   (fp64 matrix cores, k ascending in steps of 4),
 *   J[x][t][s] = F[x][t][s] + J[x][t-1][s-1] for t, s >= 1, = F[x][t][s] otherwise.
 * F, J: [n_in][T][T].  An entry's bits depend on its own row of E and of D only — not on n_in,
 * the other entries or the run (no atomics).  Refused: T outside [1, 32768], n_in outside
 * [1, 65535], n < 1, h <= 0 or not finite.  The device entry only enqueues on `stream`. */
int aiy_ssj_fake_news_dev(int64_t T, int64_t n_in, int64_t n, const double* E,
                          const double* lambda1, double h, double* F, double* J, void* stream);
int aiy_ssj_fake_news(int64_t T, int64_t n_in, int64_t n, const double* E, const double* lambda1,
                      double h, double* F, double* J);
/* The Jacobians of K_{t+1} in r_s and w_s around a steady state (host arrays; policy_c, lambda:
 * [N][Na]; P column-major), everything between the inputs and J staying on the device:
 *   1. aiy_egm_backward_batch's pass of 3 paths from policy_c: r = r_ss, w = w_ss; r[T-1] + h;
 *      w[T-1] + h;
 *   2. aiy_dist_forward_batch's pass of the 3T period policies, one push each from lambda;
 *   3. the expectation vectors of the base path's period-0 policy, y0 = a_grid in every row;
 *   4. the fake-news matrices, and 5. the Jacobians, of the two inputs.
 * J_r, J_w: [T][T], J[t][s] = dK_{t+1}/dx_s; F_r, F_w [T][T] and E [T][N][Na] are nullable.
 * *backward_status / *forward_status: the OR of the passes' per-path status words; if either is
 * not 0 the Jacobians are NaN (the call still returns AIY_OK).  stage_ms (nullable): the device
 * time of stages 1, 2, 3 and 4-5 in ms, from events recorded as they are dispatched. */
int aiy_ssj_jacobian(const double* policy_c, const double* lambda, double r_ss, double w_ss,
                     const double* a_grid, const double* s, const double* P, int64_t N,
                     int64_t Na, double beta, double sigma, double amin, int64_t T, double h,
                     double* J_r, double* J_w, double* F_r, double* F_w, double* E,
                     int32_t* backward_status, int32_t* forward_status, double* stage_ms);
/* aiy_ssj_jacobian of C steady states in one call: the same four stages, each ONE launch over the
 * economies of a chunk (3 backward paths, 3T one-step pushes, 1 expectation pass and 2 T x T
 * tiles' worth of workgroups per economy).  Economy e has its own policy_c[e], lambda[e]
 * ([N][Na]), r_ss[e], w_ss[e], beta[e], sigma[e], amin[e], a_grid[e] [Na], s[e] [N] and P[e]
 * (N x N column-major); N, Na, T and h are shared.  J_r, J_w: [C][T][T]; F_r, F_w [C][T][T] and
 * E [C][T][N][Na] are nullable; backward_status, forward_status: [C]; stage_ms (nullable): [4],
 * summed over the chunks.
 * Economy e's outputs equal aiy_ssj_jacobian's on e alone bit for bit and do not depend on C, on
 * e's place in the batch or on the chunking.  An economy with a pass that stopped gets its status
 * words (the OR over its paths) and NaN J_r, J_w; the others are not touched by it.
 * Memory: the period policies and Lambda1 are 3 T N Na doubles each per economy, so the entry
 * works through the economies `chunk` at a time; chunk = 0: as many as fit 4 GiB of device
 * memory (8 (7 T N Na + 4 T^2) bytes an economy), at least one.
 * Refused before any device is asked for, in this order: NULL arguments (the nullable ones
 * apart); C outside [1, 2^24]; N, Na, the fit rules, T and h as aiy_ssj_jacobian; chunk outside
 * [0, 32767]; then per economy e = 0 .. C-1, the message starting "economy e: ": a grid that is
 * not finite and strictly increasing, r_ss not finite or 1 + r_ss <= 0, w_ss not finite, beta
 * or sigma not finite or <= 0, amin not finite. */
int aiy_ssj_jacobian_batch(int64_t C, const double* policy_c, const double* lambda,
                           const double* r_ss, const double* w_ss, const double* a_grid,
                           const double* s, const double* P, int64_t N, int64_t Na,
                           const double* beta, const double* sigma, const double* amin, int64_t T,
                           double h, double* J_r, double* J_w, double* F_r, double* F_w, double* E,
                           int32_t* backward_status, int32_t* forward_status, double* stage_ms,
                           int64_t chunk);

/* ---- Transition paths of the endogenous-labour economy (A5; new).  The same five entries and the
 * same conventions as above.  Fit rules (else AIY_BAD_ARG, no per-step fallback):
 *   backward: N <= 16, Na <= 1024, 3·N·Na doubles + 2.4 KB within 160 KiB;
 *   forward:  N <= 16, 8·N·Na·3 + 4·N·(Na+1) + 8·Na + 2.3 KB within 160 KiB.
 * The two-rate labour step of period t (pc_next = the consumption policy of period t+1;
 * labor(c, x) = ((x u'(c)) / phi)^(1/theta), the power skipped when 1/theta == 1):
 *   RHS(j,a) = sum_m ((beta(1+r[t+1])) P(j,m)) u'(pc_next(m,a)),  c~ = RHS^(-1/sigma),
 *   l~ = labor(c~, w[t] s_j),  a^(j,a) = ((c~ + a_grid(a)) - (w[t] s_j) l~) / (1 + r[t]),
 *   g = interp1(a^_j, c~_j, a_grid(a), linear, extrap),  a_grid(a) < amin -> g = amin,  pc_t = g,
 *   pl_t = labor(g, w[t] s_j),  k = ((1 + r[t]) a_grid(a) + (w[t] s_j) pl_t) - g,
 *   pk_t = k < 0 ? 0 : k
 * — aiy_labor_egm_step's operations with r split in two: on r[t+1] == r[t] it equals that step
 * bit for bit.  policy_k, policy_l, policy_c (nullable): [C][T][N][Na].  status 1 as
 * aiy_egm_backward_batch_dev.  Also refused before any launch: phi <= 0 or not finite, theta = 0
 * or not finite. */
int aiy_labor_egm_backward_batch_dev(aiy_ws* ws, int64_t C, int64_t T, const double* r,
                                     const double* w, const double* pc_T, int pc_T_shared,
                                     const double* a_grid, const double* s, const double* P,
                                     double beta, double sigma, double phi, double theta,
                                     double amin, double* policy_k, double* policy_l,
                                     double* policy_c, int32_t* status, int32_t* fail_t,
                                     void* stream);
/* aiy_dist_forward_batch_dev and the hours in efficiency units, H[c][t] = sum lambda_t(j,a)
 * (s_j policy_l[c][t](j,a)), t = 0 .. T-1 (device [C][T]): the inner product rounded first, the
 * summation order K[t]'s.  K[t] and H[t] are formed before period t's monotonicity check: on
 * status 2 both are written up to fail_t and NaN beyond.  K, lambda_T, status and fail_t equal
 * aiy_dist_forward_batch_dev's on the same policy_k bit for bit. */
int aiy_labor_dist_forward_batch_dev(aiy_ws* ws, int64_t C, int64_t T, const double* policy_k,
                                     const double* policy_l, const double* lambda0,
                                     int lambda0_shared, const double* a_grid, const double* s,
                                     const double* P, double* K, double* H, double* lambda_T,
                                     int32_t* status, int32_t* fail_t, void* stream);
/* The same two passes on host arrays (P column-major N x N).  Also refused before any launch: an
 * a_grid that is not strictly increasing. */
int aiy_labor_egm_backward_batch(int64_t C, int64_t T, const double* r, const double* w,
                                 const double* pc_T, int pc_T_shared, const double* a_grid,
                                 const double* s, const double* P, int64_t N, int64_t Na,
                                 double beta, double sigma, double phi, double theta, double amin,
                                 double* policy_k, double* policy_l, double* policy_c,
                                 int32_t* status, int32_t* fail_t);
int aiy_labor_dist_forward_batch(int64_t C, int64_t T, const double* policy_k,
                                 const double* policy_l, const double* lambda0,
                                 int lambda0_shared, const double* a_grid, const double* s,
                                 const double* P, int64_t N, int64_t Na, double* K, double* H,
                                 double* lambda_T, int32_t* status, int32_t* fail_t);
/* Both passes on one stream, the period policies staying on the device: K [C][T+1], H [C][T],
 * status and fail_t [C].  A path the backward pass stopped (status 1) has K and H all NaN. */
int aiy_labor_transition_batch(int64_t C, int64_t T, const double* r, const double* w,
                               const double* pc_T, int pc_T_shared, const double* lambda0,
                               int lambda0_shared, const double* a_grid, const double* s,
                               const double* P, int64_t N, int64_t Na, double beta, double sigma,
                               double phi, double theta, double amin, double* K, double* H,
                               int32_t* status, int32_t* fail_t);
/* The Jacobians of K_{t+1} and of H_t in r_s and w_s around a steady state of the labour economy
 * (host arrays; policy_c, lambda: [N][Na]; P column-major), everything between the inputs and the
 * J matrices staying on the device:
 *   1. aiy_labor_egm_backward_batch's pass of 3 paths from policy_c (as aiy_ssj_jacobian);
 *   2. aiy_labor_dist_forward_batch's pass of the 3T period policies, one push each from lambda:
 *      Lambda1 [3][T][N][Na] and H1 [3][T], the hours of each period policy under lambda;
 *   3. the expectation vectors under the base path's period-0 policy_k of y0 = a_grid (E_a) and
 *      of y0 = s_j policy_l_base,0 (E_h);
 *   4. with D_x[s] = (Lambda1[x+1][T-1-s] - Lambda1[0][T-1-s]) / h:
 *        F_K[x][t][s] = E_a[t]·D_x[s];
 *        F_H[x][0][s] = (H1[x+1][T-1-s] - H1[0][T-1-s]) / h  (hours jump on impact),
 *        F_H[x][t][s] = E_h[t-1]·D_x[s] for t >= 1  (aiy_ssj_fake_news's contraction);
 *   5. J[t][s] = F[t][s] + J[t-1][s-1] down each diagonal, for all four.
 * J_Kr, J_Kw: [T][T], J[t][s] = dK_{t+1}/dx_s; J_Hr, J_Hw: [T][T], J[t][s] = dH_t/dx_s.  The four
 * F [T][T], E_a and E_h [T][N][Na] are nullable.  Status words and stage_ms as aiy_ssj_jacobian. */
int aiy_ssj_jacobian_labor(const double* policy_c, const double* lambda, double r_ss,
                           double w_ss, const double* a_grid, const double* s, const double* P,
                           int64_t N, int64_t Na, double beta, double sigma, double phi,
                           double theta, double amin, int64_t T, double h, double* J_Kr,
                           double* J_Kw, double* J_Hr, double* J_Hw, double* F_Kr, double* F_Kw,
                           double* F_Hr, double* F_Hw, double* E_a, double* E_h,
                           int32_t* backward_status, int32_t* forward_status, double* stage_ms);

/* ---- Second moments and the Gaussian likelihood from the sequence-space Jacobian (new).
 * G: [n_o][T][T], G[o][t][s] = dX_{o,t}/dZ_s, the general-equilibrium Jacobians of n_o observables
 * in the shock (estimation.ge_jacobians); dZ: [C][T], the MA coefficients of C shock processes.
 *   m[c][o][t] = sum_s G[o][t][s] dZ[c][s]   (fp64 matrix cores, s ascending in steps of 4)
 * m: [C][n_o][T].  An entry's bits depend on row (o, t) of G and row c of dZ only — not on C, n_o
 * or the run (no atomics).  Refused: n_o outside [1, 64], T outside [1, 32768], C outside
 * [1, 2^24].  The device entry only enqueues on `stream`. */
int aiy_ssj_ma_batch_dev(int64_t n_o, int64_t T, int64_t C, const double* G, const double* dZ,
                         double* m, void* stream);
int aiy_ssj_ma_batch(int64_t n_o, int64_t T, int64_t C, const double* G, const double* dZ,
                     double* m);
/* Autocovariances and log-likelihood of C candidates, ONE workgroup per candidate, everything in
 * LDS.  m: [C][n_o][T]; y: [L][n_o], the observed deviations from the steady state, shared by all
 * candidates; me_var: the measurement-error variances, [n_o] (me_var_shared) or [C][n_o].  With
 * n = L n_o and row i = t n_o + o, no fused multiply-adds:
 *   1. Gamma[l][o][p] = sum_{u=0}^{T-1-l} m[o][u+l] m[p][u], u ascending from +0; l >= T: +0;
 *   2. V[(t,o)][(t',p)] = Gamma[t-t'][o][p] for t >= t' (lower triangle), me_var[o] added to the
 *      diagonal's Gamma[0][o][o]; z = y;
 *   3. j = 0 .. n-1: d_j = V[j][j]; unless d_j > 0: status 1, fail j, loglik NaN, stop; else
 *      w_i = V[i][j], l_i = w_i / d_j (i = j+1 .. n-1, and z's w = z_j, l = z_j / d_j),
 *      V[i][k] = V[i][k] - (l_i w_k) for j < k <= i, z_k = z_k - (l w_k) for k > j;
 *   4. logdet = sum_j aiy_log(d_j), quad = sum_j (z_j z_j) / d_j, j ascending from +0;
 *      loglik = -0.5 ((n 1.8378770664093453 + logdet) + quad); status 0, fail -1.
 * loglik: [C]; status, fail: [C]; Gamma (nullable): [C][L][n_o][n_o], step 1's sums without
 * me_var; d (nullable): [C][n], the pivots (on status 1: up to d[fail], NaN beyond).  y NULL:
 * step 1 only — Gamma is the result and me_var, loglik, status and fail are not touched.
 * A candidate's bits do not depend on C, on the other candidates or on the run; a NaN in m[c]
 * gives candidate c status 1 and stays there.  Fit rule (else AIY_BAD_ARG, no fallback):
 * max(n(n+1)/2, n_o T) + n n_o + 3n + 2 doubles within 160 KiB (n_o = 1: L <= 197).  The host
 * entry also refuses a me_var that is negative or not finite.  The device entry only enqueues. */
int aiy_ssj_loglik_batch_dev(int64_t C, int64_t n_o, int64_t T, int64_t L, const double* m,
                             const double* y, const double* me_var, int me_var_shared,
                             double* loglik, int32_t* status, int32_t* fail, double* Gamma,
                             double* d, void* stream);
int aiy_ssj_loglik_batch(int64_t C, int64_t n_o, int64_t T, int64_t L, const double* m,
                         const double* y, const double* me_var, int me_var_shared, double* loglik,
                         int32_t* status, int32_t* fail, double* Gamma, double* d);

/* ---- Dense solve, many systems per launch (new).  C systems A_c X_c = B_c by Gaussian
 * elimination with partial pivoting, ONE workgroup per system.  All arrays row-major: A [C][n][n],
 * B [C][n][R], X [C][n][R] (out), status and fail [C].  A and B are not modified: the kernel
 * works on a copy (A_c | B_c) in `work`, device [C][n][n+R].  No fused multiply-adds:
 *   1. j = 0 .. n-1: p = j, best = |A[j][j]|; i = j+1 .. n-1 ascending: |A[i][j]| > best takes it
 *      (ties: the lowest index; a NaN is never taken over a number).  Unless best > 0 and finite:
 *      status 1, fail j, the whole X block NaN, stop.  Swap rows j and p of A and of B.  i > j:
 *      l_i = A[i][j] / A[j][j], A[i][k] = A[i][k] - (l_i A[j][k]) for k > j, B[i][q] = B[i][q] -
 *      (l_i B[j][q]);
 *   2. j = n-1 .. 0: X[j][q] = B[j][q] / A[j][j]; B[i][q] = B[i][q] - (A[i][j] X[j][q]), i < j;
 *   3. status 0, fail -1.
 * A system's bits do not depend on C, on its place in the batch, on the other systems or on the
 * run.  Refused before any device is asked for: NULL arguments, C < 1, n outside [1, 4096],
 * R < 1, n (n + R) >= 2^31, chunk < 0.  The device entry only enqueues on `stream`.  The host
 * entry stages `chunk` systems at a time; chunk = 0: as many as fit 4 GiB of device memory
 * (16 (n^2 + n R) bytes a system), at least one. */
int aiy_dense_solve_batch_dev(int64_t C, int64_t n, int64_t R, const double* A, const double* B,
                              double* X, double* work, int32_t* status, int32_t* fail,
                              void* stream);
int aiy_dense_solve_batch(int64_t C, int64_t n, int64_t R, const double* A, const double* B,
                          double* X, int32_t* status, int32_t* fail, int64_t chunk);

/* ---- A6/A7 device tier for one process per GPU.  A handle owns the shard
 * K in [K0, K1) of all four s; V / Vold / Vout / kopt are full k x K x S column-major device
 * arrays (the layout of Krusell_Smith_VFI.m's `value`).  Each call writes only the shard's
 * nodes; the caller exchanges the owned value slices between ranks (an RCCL all-gather,
 * aiyagari-replication_amd/ks_dist.py) after every Howard sweep.  Same kernels as
 * ks_vfi_solve, so any sharding gives the single-device result bit for bit.
 * k_grid must be strictly increasing (a repeated point: AIY_BAD_ARG, as MATLAB's interpolants
 * refuse it).  Precondition on the device arrays, which no call reads back to check: every
 * entry of V is finite or NaN.  An infinite entry makes the slopes next to it NaN where the
 * script keeps ±inf (the host-tier entry points return AIY_NON_FINITE for such a value). */
typedef struct ks_dev ks_dev;
int ks_dev_create(const double* k_grid, const double* K_grid, const double* B, const double* P,
                  const double* params, int64_t nk, int64_t nK, int64_t K0, int64_t K1,
                  ks_dev** out);
/* (K, Z) slices: the shard K in [K0, K1) of the s blocks [s0, s1) only —
 * s = 0, 1 share the first aggregate state z and s = 2, 3 the second, so [0, 2) / [2, 4) are
 * the two Z slices of a K range.  ks_dev_create(...) == ks_dev_create_slice(..., 0, 4, ...). */
int ks_dev_create_slice(const double* k_grid, const double* K_grid, const double* B,
                        const double* P, const double* params, int64_t nk, int64_t nK,
                        int64_t K0, int64_t K1, int64_t s0, int64_t s1, ks_dev** out);
int ks_dev_destroy(ks_dev* h);
/* :148-168 policy improvement (pchip slopes + fminbnd) on the shard */
int ks_dev_improve(ks_dev* h, const double* V, double* kopt, void* stream);
/* :173-191 one Jacobi Howard sweep on the shard: Vout (!= V) gets the shard's new values */
int ks_dev_howard(ks_dev* h, const double* V, const double* kopt, double* Vout, void* stream);
/* :195 max relative change over the shard, NaN ignored; out = device uint64[2]
 * {IEEE bits of the max, nonzero if any node was not NaN} */
/* The fused schedule (one launch per Howard sweep): ks_dev_slopes writes the pchip slopes
 * of every column h reads into dV (caller-owned k x K x S); ks_dev_howard_fused then sweeps h's
 * nodes reading (V, dV) and writes the new values AND their slopes (Vout, dVout) on h's nodes,
 * so consecutive sweeps over nested ghost rectangles need no slope launch in between.
 * Bit-identical to ks_dev_howard. */
int ks_dev_slopes(ks_dev* h, const double* V, double* dV, void* stream);
int ks_dev_howard_fused(ks_dev* h, const double* V, const double* dV, const double* kopt,
                        double* Vout, double* dVout, void* stream);
int ks_dev_reldiff(ks_dev* h, const double* V, const double* Vold, void* out, void* stream);
/* The direct (peer-read) schedule of ks_vfi_solve_sharded(depth = 0): each shard keeps only its
 * own columns current and reads every forecast column where its owner keeps it — table = a
 * device array of 4·K_size value-column pointers then 4·K_size slope-column pointers (into the
 * owners' buffers on this device or a peer; NULL restores the caller's full arrays), used by
 * ks_dev_howard_fused (its V / dV arguments are then not read) and ks_dev_improve_direct.
 * ks_dev_slopes_own writes the slopes of the shard's own columns (the schedule's start). */
int ks_dev_set_columns(ks_dev* h, const void* const* table);
int ks_dev_slopes_own(ks_dev* h, const double* V, double* dV, void* stream);
int ks_dev_improve_direct(ks_dev* h, double* kopt, void* stream);
/* The direct schedule under one process per GPU (ks_dist.DirectPeers; no reference
 * counterpart — the reference is one MATLAB process): the column buffers are shared through
 * IPC handles and the sweep hand-off through counters in a host page every rank maps.
 * aiy_ipc_get_handle: the IPC handle (AIY_IPC_HANDLE_BYTES) of the allocation holding dptr and
 * dptr's offset in it; aiy_ipc_open maps it in this process (peer access enabled on demand;
 * *dptr = base + offset) and aiy_ipc_close unmaps.  aiy_host_register pins and maps a host
 * range for the device (*dptr: its device address).  Counter slot q is the uint64 at
 * flags + 128·q (q < 64).  aiy_flags_wait enqueues one wave that holds the stream until every
 * slot q in `mask` is >= value; after timeout_s seconds without that it stores 1 + q in *err
 * (host-mapped) and lets the stream go (the caller checks err; results are then invalid; once
 * err is set, later waits return at once).
 * aiy_flag_set enqueues a system-scope release store value -> slot. */
#define AIY_IPC_HANDLE_BYTES 64
int aiy_ipc_get_handle(const void* dptr, void* handle, int64_t* offset);
int aiy_ipc_open(const void* handle, int64_t offset, void** dptr);
int aiy_ipc_close(void* dptr, int64_t offset);
int aiy_host_register(void* p, int64_t bytes, void** dptr);
int aiy_host_unregister(void* p);
int aiy_flags_wait(const void* flags, uint64_t mask, uint64_t value, double timeout_s, void* err,
                   void* stream);
int aiy_flag_set(void* flags, int32_t slot, uint64_t value, void* stream);
/* The staged direct schedule.  ks_dev_set_split: the shard's own columns
 * c = s·K_size + K in two host lists — `interior` columns read only forecast columns the shard
 * owns, `boundary` columns read at least one a peer owns; ks_dev_howard_fused_part sweeps one
 * list (part 0 / 1) like ks_dev_howard_fused.
 * ks_dev_staged_sweep: one whole sweep in ONE launch — first publish pub_v in slot `slot` of
 * `flags` (the previous launch on the stream produced that version; system-scope release), then
 * copy src[q] -> dst[q] (DEVICE arrays of column pointers, q < n_halo: the owners' value and
 * slope columns, system-scope loads) once every slot in `mask` holds >= wait_v (timeout: *err =
 * 1 + q, as aiy_flags_wait), sweep the interior columns without waiting and the boundary columns
 * once every copy is in (an in-kernel agent-scope counter hand-off); own columns are stored
 * write-through (system scope).  flags = NULL: no publish and no wait.
 * ks_dev_direct_sweeps: nsweeps such sweeps on three buffers — version v in buffer (v - 1) mod 3:
 * sweep i reads buffer b = (cur + i) mod 3 (V[b], dV[b], column table tabs[b], copies from
 * srcs[b]) and writes buffer (b + 1) mod 3, waiting for / publishing n0 + i; then one launch
 * publishes n0 + nsweeps.  tabs, V, dV, srcs: HOST arrays of three device pointers.
 * ks_dev_halo_copy: the same copies once, stream-ordered (before an improvement). */
int ks_dev_set_split(ks_dev* h, const int32_t* interior, int32_t n_int, const int32_t* boundary,
                     int32_t n_bnd);
int ks_dev_howard_fused_part(ks_dev* h, int part, const double* V, const double* dV,
                             const double* kopt, double* Vout, double* dVout, void* stream);
int ks_dev_staged_sweep(ks_dev* h, const double* V, const double* dV, const double* kopt,
                        double* Vout, double* dVout, const void* const* src, void* const* dst,
                        int32_t n_halo, void* flags, uint64_t mask, uint64_t wait_v, int32_t slot,
                        uint64_t pub_v, double timeout_s, void* err, void* stream);
int ks_dev_direct_sweeps(ks_dev* h, void* const* tabs, double* const* V, double* const* dV,
                         double* kopt, int32_t cur, int64_t nsweeps, void* const* srcs,
                         void* const* dst, int32_t ncopy, int64_t col_bytes, void* flags,
                         int32_t slot, uint64_t mask, uint64_t n0, double timeout_s, void* err,
                         void* stream);
int ks_dev_halo_copy(const void* const* src, void* const* dst, int32_t ncopy, int64_t col_bytes,
                     void* stream);
/* Ghost shards (ks_dist.py exchanges halos every m Howard sweeps and sweeps a widening
 * rectangle of other ranks' columns redundantly in between — same kernels, so still bit-exact):
 * h uses owner's segment-hint array (same grid and device; destroying owner while a handle
 * still shares it fails with AIY_BAD_ARG), and
 * ks_dev_hints recomputes the hints of h's nodes from kopt (for k_opt received from other
 * ranks).  Hints only short-cut Howard's segment search: results never depend on them. */
int ks_dev_share_hints(ks_dev* h, ks_dev* owner);
int ks_dev_hints(ks_dev* h, const double* kopt, void* stream);
/* Host-only (no device): the forecast column K'_idx(s, K) that bellman_value reads for every
 * node of slice (K, s) (Krusell_Smith_VFI.m:335-343, clamp + nearest index), 0-based,
 * out[s * nK + K].  The sharded driver builds its halo exchange from it: a rank needs, besides
 * its own slices, exactly the columns K'_idx of its nodes, for all four s'. */
int ks_forecast_index(const double* K_grid, const double* B, const double* params, int64_t nK,
                      int32_t* out);

/* ---- F3 / F2 device tier.  uniforms, zi (int8 [T], 0 good / 1 bad) and eps (int8
 * [T][population] row-major, 0 employed / 1 unemployed: t-major so each period is one
 * contiguous row) in HBM; k_opt k x K x 4 column-major; k_population in/out; K_ts out [T];
 * scratch: ks_panel_scratch_bytes(population) bytes of device memory. */
int ks_shocks_dev(int64_t T, int64_t population, const double* uniforms, const double* params,
                  int8_t* zi, int8_t* eps, void* stream);
int64_t ks_panel_scratch_bytes(int64_t population);
int ks_simulate_capital_dev(int64_t nk, int64_t nK, const double* k_grid, const double* K_grid,
                            const double* k_opt, int64_t T, int64_t population,
                            const int8_t* zi, const int8_t* eps, double* k_population,
                            double* K_ts, void* scratch, void* stream);

/* ---- F2 histogram device tier.  Grids, k_opt (k x K x 4 column-major), zi (int8 [M][T]), lam
 * ([M][2][nx], in/out) and K_ts ([M][T], out) and slow_periods (int64 [M], nullable) in HBM;
 * params on the host.  Shapes and params are validated before the launch; the contents of
 * device arrays are the caller's (a zi code other than 0 counts as 1). */
int ks_simulate_hist_dev(int64_t nk, int64_t nK, const double* k_grid, const double* K_grid,
                         const double* k_opt, const double* x_grid, int64_t nx,
                         const double* params, const int8_t* zi, int64_t T, int64_t M,
                         double* lam, double* K_ts, int64_t* slow_periods, void* stream);
/* One policy per path on device (ks_simulate_hist_multi): k_opt [C][4][K_size][k_size] and
 * K_grid [C][K_size] in HBM, the other device arrays as ks_simulate_hist_dev; params [C][13] and
 * policy_of_path [M] are HOST arrays, validated (with the shapes) before the device is touched.
 * scratch: ks_hist_multi_scratch_bytes(C, M) bytes of device memory owned by the caller, which
 * receive the candidates' employment tables and policy_of_path; the call waits for that upload
 * (one synchronisation of `stream`, so the host tables may die at return and a scratch still
 * read by an earlier launch on the same stream is not overwritten early), then enqueues the one
 * launch and returns. */
int64_t ks_hist_multi_scratch_bytes(int64_t C, int64_t M);
int ks_simulate_hist_multi_dev(int64_t C, int64_t nk, int64_t nK, const double* k_grid,
                               const double* K_grid, const double* k_opt, const double* x_grid,
                               int64_t nx, const double* params, const int32_t* policy_of_path,
                               const int8_t* zi, int64_t T, int64_t M, double* lam, double* K_ts,
                               int64_t* slow_periods, void* scratch, void* stream);

/* ---- A8 batch device tier (ks_egm_solve_batch): k_opt [C][4][K_size][k_size] (in/out), k_grid,
 * iters (int64), diff and status (int32) [C] in HBM; K_grid [C][K_size], B [C][4], P [C] of
 * MATLAB 4 x 4 and params [C][13] are HOST arrays (the per-pair scalars are libm on the host, as
 * in ks_egm_solve).  Host arguments and shapes are validated before any device work; the
 * contents of k_grid (strictly increasing) are the caller's.
 * Scratch ownership: the host tier stages everything in the library's cached buffers; this tier
 * owns none — scratch is ks_egm_batch_scratch_bytes(C, K_size) bytes of device memory owned by
 * the caller and receives the host-built candidate tables.  The call waits for that upload (one
 * synchronisation of `stream`: the host tables die at return, and a scratch still read by an
 * earlier solve on the same stream is not overwritten early), then enqueues the one launch and
 * returns; the outputs are valid once `stream` has run it. */
int64_t ks_egm_batch_scratch_bytes(int64_t C, int64_t nK);
int ks_egm_solve_batch_dev(int64_t C, double* k_opt, const double* k_grid, const double* K_grid,
                           const double* B, const double* P, const double* params, int64_t nk,
                           int64_t nK, double tol, int64_t max_iter, int64_t* iters, double* diff,
                           int32_t* status, void* scratch, void* stream);

/* ---- A6/A7 batch device tier (ks_vfi_solve_batch): value and k_opt [C][4][K_size][k_size]
 * (in/out; k_opt in the layout ks_simulate_hist_multi_dev reads, so the two launches of an ALM
 * round need no repacking), k_grid, iters (int64) and rel_diff [C] in HBM; K_grid [C][K_size],
 * B [C][4], P [C] of MATLAB 4 x 4 and params [C][13] are HOST arrays (the slice tables are libm
 * on the host, as in ks_vfi_solve).  Host arguments and shapes are validated before any device
 * work; preconditions on device contents are the caller's: k_grid strictly increasing, value
 * finite or NaN (no ±inf).  No tiled fallback: a size past the one-workgroup rule is
 * AIY_BAD_SHAPE.  Scratch is ks_vfi_batch_scratch_bytes(C, K_size) bytes of device memory owned
 * by the caller and receives the host-built candidate tables.  The call waits for that upload
 * (one synchronisation of `stream`), then enqueues the one launch and returns; the outputs are
 * valid once `stream` has run it. */
int64_t ks_vfi_batch_scratch_bytes(int64_t C, int64_t nK);
int ks_vfi_solve_batch_dev(int64_t C, double* value, double* k_opt, const double* k_grid,
                           const double* K_grid, const double* B, const double* P,
                           const double* params, int64_t nk, int64_t nK, int64_t howard_steps,
                           double tol, int64_t max_vfi, int64_t* iters, double* rel_diff,
                           void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
