/* [k_supply, k_demand, iters] = aiy_labor_ge_batch_mex(r, v_old, v_new, policy_k, policy_l,
 *     policy_c, policy_lin, a_grid, s, P, labor_choice, alpha, delta, beta, sigma, psi, eta,
 *     labor, tol, max_iter, z1, k1, uniforms, n_devices)
 * The body of one GE step of Aiyagari_Endogenous_Labor_VFI.m:166-245 at every candidate rate r(c)
 * at once — the labour VFI at r(c) and its own wage from v_old, the incoming v_new and the
 * policies (N x Na, the common start the script carries across GE steps; policy_lin = the 1-based
 * index into the Nl x Na choice matrix; v_new, the policies and policy_lin may be [] = zeros /
 * index 1), the Monte-Carlo capital supply from (z1, k1) with the c-th column of `uniforms`
 * ((T-1) x C) and K_d = labor*(alpha/(r+delta))^(1/(1-alpha)).  The candidates are spread over
 * n_devices GPUs.  The script keeps its bracket logic (:240-245). */
#include "mexcommon.h"
/* an N x Na start array, or [] (NULL: zeros) */
static const double* start_in(const mxArray* a, const char* name, mwSize N, mwSize Na) {
    if (mxIsDouble(a) && mxGetNumberOfElements(a) == 0) return NULL;
    return aiy_in(a, name, N, Na);
}
void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    aiy_nargs(nrhs, 24, 24, nlhs, 3, "[k_supply,k_demand,iters] = aiy_labor_ge_batch_mex(r,v_old,v_new,policy_k,policy_l,policy_c,policy_lin,a_grid,s,P,labor_choice,alpha,delta,beta,sigma,psi,eta,labor,tol,max_iter,z1,k1,uniforms,n_devices)");
    mwSize C = 0, Nl = 0;
    const double* r = aiy_vec(prhs[0], "r", 0, &C);
    mwSize N = mxGetM(prhs[1]), Na = mxGetN(prhs[1]);
    const double* v = aiy_in(prhs[1], "v_old", 0, 0);
    const double* vn = start_in(prhs[2], "v_new", N, Na);
    const double* pk = start_in(prhs[3], "policy_k", N, Na);
    const double* pl = start_in(prhs[4], "policy_l", N, Na);
    const double* pc = start_in(prhs[5], "policy_c", N, Na);
    const double* plin = start_in(prhs[6], "policy_lin", N, Na);
    const double* a = aiy_vec(prhs[7], "a_grid", Na, NULL);
    const double* s = aiy_vec(prhs[8], "s", N, NULL);
    const double* P = aiy_in(prhs[9], "P", N, N);
    const double* L = aiy_vec(prhs[10], "labor_choice", 0, &Nl);
    double alpha = aiy_scalar(prhs[11], "alpha"), delta = aiy_scalar(prhs[12], "delta");
    double beta = aiy_scalar(prhs[13], "beta"), sigma = aiy_scalar(prhs[14], "sigma");
    double psi = aiy_scalar(prhs[15], "psi"), eta = aiy_scalar(prhs[16], "eta");
    double labor = aiy_scalar(prhs[17], "labor"), tol = aiy_scalar(prhs[18], "tol");
    double mi = aiy_scalar(prhs[19], "max_iter"), z1 = aiy_scalar(prhs[20], "z1");
    double k1 = aiy_scalar(prhs[21], "k1");
    const double* U = aiy_in(prhs[22], "uniforms", 0, C);
    int64_t T = (int64_t)mxGetM(prhs[22]) + 1;
    double nd = aiy_scalar(prhs[23], "n_devices");
    if (mi != (double)(int64_t)mi || z1 != (double)(int64_t)z1 || nd != (double)(int)nd)
        aiy_err("aiy:type", "max_iter, z1 and n_devices must be integers");
    size_t n = (size_t)N * Na;
    if (plin)
        for (size_t q = 0; q < n; ++q)
            if (plin[q] != (double)(int32_t)plin[q])
                aiy_err("aiy:type", "policy_lin must hold integers");
    int32_t* lin = plin ? (int32_t*)malloc(sizeof(int32_t) * (n ? n : 1)) : NULL;
    for (size_t q = 0; lin && q < n; ++q) lin[q] = (int32_t)plin[q];
    mxArray* ks = aiy_out(C, 1);
    mxArray* kd = aiy_out(C, 1);
    int64_t* it = (int64_t*)malloc(sizeof(int64_t) * (C ? C : 1));
    aiy_begin();
    int rc = aiy_labor_ge_batch(r, (int64_t)C, v, vn, pk, pl, pc, lin, a, s, P, L, (int64_t)N,
                                (int64_t)Na, (int64_t)Nl, alpha, delta, beta, sigma, psi, eta,
                                labor, tol, (int64_t)mi, (int64_t)z1, k1, T, U, (int)nd,
                                mxGetPr(ks), mxGetPr(kd), it);
    free(lin);
    if (rc != AIY_OK) {
        free(it);
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
    free(it);
}
