/* [K_ts, lam, slow_periods] = ks_simulate_hist_mex(k_opt, k_grid, K_grid, x_grid, params,
 *                                                 zi_shock, lam)
 * The histogram (non-stochastic) simulation of the capital path, beside the agent panel of
 * ks_simulate_capital_mex (Krusell_Smith_VFI.m:206-248).  k_opt: k_size x K_size x 4; x_grid: nx
 * histogram nodes; params: the 13 KS doubles; zi_shock: T x M (0/1), one aggregate shock path
 * per column; lam: nx x 2 x M (column 1 employed, 2 unemployed), the start distributions.
 * K_ts: T x M; lam: the distributions of period T; slow_periods: M x 1. */
#include "mexcommon.h"
void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    aiy_nargs(nrhs, 7, 7, nlhs, 3, "[K_ts,lam,slow_periods] = ks_simulate_hist_mex(k_opt,k_grid,K_grid,x_grid,params,zi_shock,lam)");
    mwSize nk = 0, nK = 0, nx = 0;
    const double* kg = aiy_vec(prhs[1], "k_grid", 0, &nk);
    const double* Kg = aiy_vec(prhs[2], "K_grid", 0, &nK);
    const double* xg = aiy_vec(prhs[3], "x_grid", 0, &nx);
    const double* prm = aiy_vec(prhs[4], "params", 13, NULL);
    if (mxGetNumberOfElements(prhs[0]) != nk * nK * 4)
        aiy_err("aiy:shape", "k_opt must be k_size x K_size x 4");
    const double* ko = aiy_in(prhs[0], "k_opt", 0, 0);
    const double* zi = aiy_in(prhs[5], "zi_shock", 0, 0);
    const mwSize T = mxGetM(prhs[5]), M = mxGetN(prhs[5]);
    const double* l0 = aiy_in(prhs[6], "lam", nx, 0);
    if (mxGetNumberOfElements(prhs[6]) != nx * 2 * M)
        aiy_err("aiy:shape", "lam must be numel(x_grid) x 2 x size(zi_shock, 2)");
    const mwSize dims[3] = {nx, 2, M};
    mxArray* K_ts = aiy_out(T, M);
    mxArray* lam = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    mxArray* slow = aiy_out(M, 1);
    memcpy(mxGetPr(lam), l0, sizeof(double) * nx * 2 * M);
    int64_t* sp = (int64_t*)malloc(sizeof(int64_t) * (M ? M : 1));
    if (!sp) {
        mxDestroyArray(K_ts);
        mxDestroyArray(lam);
        mxDestroyArray(slow);
        aiy_err("aiy:NO_MEMORY", "out of host memory");
    }
    aiy_begin();
    int rc = ks_simulate_hist(ko, kg, Kg, (int64_t)nk, (int64_t)nK, xg, (int64_t)nx, prm, zi,
                              (int64_t)T, (int64_t)M, mxGetPr(lam), mxGetPr(K_ts), sp);
    if (rc == AIY_OK)
        for (mwSize m = 0; m < M; ++m) mxGetPr(slow)[m] = (double)sp[m];
    free(sp);
    if (rc != AIY_OK) {
        mxDestroyArray(K_ts);
        mxDestroyArray(lam);
        mxDestroyArray(slow);
    }
    aiy_check(rc);
    plhs[0] = K_ts;
    if (nlhs > 1) plhs[1] = lam;
    else mxDestroyArray(lam);
    if (nlhs > 2) plhs[2] = slow;
    else mxDestroyArray(slow);
}
