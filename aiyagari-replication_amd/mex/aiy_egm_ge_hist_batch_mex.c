/* [k_supply, k_demand, iters, status, dist_iters] = aiy_egm_ge_hist_batch_mex(r, policy_c, a_grid,
 *                                    s, P, w, alpha, delta, beta, sigma, amin, labor, tol, max_iter,
 *                                    dist_tol, dist_max_iter, n_devices, lambda_start[, phi, theta])
 * aiy_egm_ge_batch_mex with the stationary histogram (A10) as the supply estimator: at every
 * candidate rate r(c) the EGM solve from policy_c (Na x N, the common warm start) at wage w (a
 * scalar, as the scripts keep it, or one per rate), then K_s = sum of lambda .* a at the
 * stationary distribution of policy_k — each state's mass split between the bracketing grid
 * nodes — iterated from lambda_start (Na x N; []: uniform) until max|dlambda| < dist_tol or
 * dist_max_iter pushes, and K_d.  With phi and theta: Aiyagari_Endogenous_Labor_EGM.m.
 * status(c): 0 ok, 1 = the endogenous grid stopped increasing (k_supply(c) NaN, dist_iters(c) 0).
 * The script keeps its bracket logic (:245-251). */
#include "mexcommon.h"
void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    aiy_nargs(nrhs, 18, 20, nlhs, 5, "[k_supply,k_demand,iters,status,dist_iters] = aiy_egm_ge_hist_batch_mex(r,policy_c,a_grid,s,P,w,alpha,delta,beta,sigma,amin,labor,tol,max_iter,dist_tol,dist_max_iter,n_devices,lambda_start[,phi,theta])");
    if (nrhs == 19) aiy_err("aiy:usage", "phi and theta are given together");
    mwSize C = 0, nw = 0;
    const double* r = aiy_vec(prhs[0], "r", 0, &C);
    mwSize Na = mxGetM(prhs[1]), N = mxGetN(prhs[1]);
    const double* pc = aiy_in(prhs[1], "policy_c", 0, 0);
    const double* a = aiy_vec(prhs[2], "a_grid", Na, NULL);
    const double* s = aiy_vec(prhs[3], "s", N, NULL);
    const double* P = aiy_in(prhs[4], "P", N, N);
    const double* w = aiy_vec(prhs[5], "w", 0, &nw);
    if (nw != 1 && nw != C) aiy_err("aiy:shape", "w must be a scalar or have one element per rate");
    double alpha = aiy_scalar(prhs[6], "alpha"), delta = aiy_scalar(prhs[7], "delta");
    double beta = aiy_scalar(prhs[8], "beta"), sigma = aiy_scalar(prhs[9], "sigma");
    double amin = aiy_scalar(prhs[10], "amin"), labor = aiy_scalar(prhs[11], "labor");
    double tol = aiy_scalar(prhs[12], "tol"), mi = aiy_scalar(prhs[13], "max_iter");
    double dtol = aiy_scalar(prhs[14], "dist_tol"), dmi = aiy_scalar(prhs[15], "dist_max_iter");
    double nd = aiy_scalar(prhs[16], "n_devices");
    const double* lam = NULL;
    if (mxGetNumberOfElements(prhs[17]) != 0) lam = aiy_in(prhs[17], "lambda_start", Na, N);
    int lab = nrhs == 20;
    double phi = lab ? aiy_scalar(prhs[18], "phi") : 1.0;
    double theta = lab ? aiy_scalar(prhs[19], "theta") : 1.0;
    if (mi != (double)(int64_t)mi || dmi != (double)(int64_t)dmi || nd != (double)(int)nd)
        aiy_err("aiy:type", "max_iter, dist_max_iter and n_devices must be integers");
    mxArray* ks = aiy_out(C, 1);
    mxArray* kd = aiy_out(C, 1);
    mwSize Cn = C ? C : 1;
    double* wv = (double*)malloc(sizeof(double) * Cn);
    int64_t* it = (int64_t*)malloc(sizeof(int64_t) * Cn);
    int64_t* dit = (int64_t*)malloc(sizeof(int64_t) * Cn);
    int32_t* st = (int32_t*)malloc(sizeof(int32_t) * Cn);
    for (mwSize q = 0; q < C; ++q) wv[q] = nw == 1 ? w[0] : w[q];
    aiy_begin();
    int rc = aiy_egm_ge_hist_batch(r, wv, (int64_t)C, pc, a, s, P, (int64_t)N, (int64_t)Na, alpha,
                                   delta, beta, sigma, amin, lab, phi, theta, labor, tol,
                                   (int64_t)mi, dtol, (int64_t)dmi, lam, (int)nd, mxGetPr(ks),
                                   mxGetPr(kd), it, dit, st);
    free(wv);
    if (rc != AIY_OK) {
        free(it);
        free(dit);
        free(st);
        mxDestroyArray(ks);
        mxDestroyArray(kd);
    }
    aiy_check(rc);
    plhs[0] = ks;
    if (nlhs > 1) plhs[1] = kd;
    else mxDestroyArray(kd);
    if (nlhs > 2) {
        plhs[2] = aiy_out(C, 1);
        for (mwSize q = 0; q < C; ++q) mxGetPr(plhs[2])[q] = (double)it[q];
    }
    if (nlhs > 3) {
        plhs[3] = aiy_out(C, 1);
        for (mwSize q = 0; q < C; ++q) mxGetPr(plhs[3])[q] = (double)st[q];
    }
    if (nlhs > 4) {
        plhs[4] = aiy_out(C, 1);
        for (mwSize q = 0; q < C; ++q) mxGetPr(plhs[4])[q] = (double)dit[q];
    }
    free(it);
    free(dit);
    free(st);
}
