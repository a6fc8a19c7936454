/* [k_supply, k_demand, iters, dist_iters] = aiy_ge_hist_batch_mex(r, v_old, a_grid, s, P, alpha,
 *                                              delta, beta, sigma, labor, tol, max_iter, dist_tol,
 *                                              dist_max_iter, n_devices[, lambda_start])
 * aiy_ge_batch_mex with the stationary histogram (A10) as the supply estimator: at every
 * candidate rate r(c) the VFI from v_old (N x Na, the common warm start), then K_s = sum of
 * lambda .* a at the stationary distribution of the solve's index policy, iterated from
 * lambda_start (N x Na; omitted or []: uniform) until max|dlambda| < dist_tol or dist_max_iter
 * pushes, and K_d = labor*(alpha/(r+delta))^(1/(1-alpha)).  No random draws: a candidate's
 * result depends on its rate alone.  The script keeps its bracket logic (:196-204). */
#include "mexcommon.h"
void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    aiy_nargs(nrhs, 15, 16, nlhs, 4, "[k_supply,k_demand,iters,dist_iters] = aiy_ge_hist_batch_mex(r,v_old,a_grid,s,P,alpha,delta,beta,sigma,labor,tol,max_iter,dist_tol,dist_max_iter,n_devices[,lambda_start])");
    mwSize C = 0;
    const double* r = aiy_vec(prhs[0], "r", 0, &C);
    mwSize N = mxGetM(prhs[1]), Na = mxGetN(prhs[1]);
    const double* v = aiy_in(prhs[1], "v_old", 0, 0);
    const double* a = aiy_vec(prhs[2], "a_grid", Na, NULL);
    const double* s = aiy_vec(prhs[3], "s", N, NULL);
    const double* P = aiy_in(prhs[4], "P", N, N);
    double alpha = aiy_scalar(prhs[5], "alpha"), delta = aiy_scalar(prhs[6], "delta");
    double beta = aiy_scalar(prhs[7], "beta"), sigma = aiy_scalar(prhs[8], "sigma");
    double labor = aiy_scalar(prhs[9], "labor"), tol = aiy_scalar(prhs[10], "tol");
    double mi = aiy_scalar(prhs[11], "max_iter"), dtol = aiy_scalar(prhs[12], "dist_tol");
    double dmi = aiy_scalar(prhs[13], "dist_max_iter"), nd = aiy_scalar(prhs[14], "n_devices");
    const double* lam = NULL;
    if (nrhs == 16 && mxGetNumberOfElements(prhs[15]) != 0)
        lam = aiy_in(prhs[15], "lambda_start", N, Na);
    if (mi != (double)(int64_t)mi || dmi != (double)(int64_t)dmi || nd != (double)(int)nd)
        aiy_err("aiy:type", "max_iter, dist_max_iter and n_devices must be integers");
    mxArray* ks = aiy_out(C, 1);
    mxArray* kd = aiy_out(C, 1);
    int64_t* it = (int64_t*)malloc(sizeof(int64_t) * (C ? C : 1));
    int64_t* dit = (int64_t*)malloc(sizeof(int64_t) * (C ? C : 1));
    aiy_begin();
    int rc = aiy_ge_hist_batch(r, (int64_t)C, v, a, s, P, (int64_t)N, (int64_t)Na, alpha, delta,
                               beta, sigma, labor, tol, (int64_t)mi, dtol, (int64_t)dmi, lam,
                               (int)nd, mxGetPr(ks), mxGetPr(kd), it, dit);
    if (rc != AIY_OK) {
        free(it);
        free(dit);
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
        for (mwSize q = 0; q < C; ++q) mxGetPr(plhs[3])[q] = (double)dit[q];
    }
    free(it);
    free(dit);
}
