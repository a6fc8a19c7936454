% aiyagari_egm_ge_hist_multisection_gpu.m -- the GE search of the two EGM scripts with the
% stationary histogram (DESIGN.md §1 row A10) as the supply estimator, evaluated breadth-first
% on the MI355X solver, from MATLAB/Octave.
%
% labor_model = false: Aiyagari_EGM.m:157-253; true: Aiyagari_Endogenous_Labor_EGM.m:154-251.
% Every midpoint the bisection could visit in its next `levels` steps (2^levels - 1 rates, each
% computed from its own bracket exactly as the sequential loop computes it) goes to the GPUs in
% ONE call, aiy_egm_ge_hist_batch_mex: the EGM solve of every rate from the common warm start
% (the r0 = 0.04 policy) in one launch, K_s = sum(lambda .* a) at the stationary distribution of
% every candidate's policy_k (mass split between the bracketing nodes) in another, and K_d.  No
% random draws: K_s has no sampling noise.  The script then walks the sequential loop's path through
% the evaluated tree, so r, r_history and the early stop are the bisection's.  Like the scripts,
% it keeps the wage of r = 0.04 inside the loop (w_stale).  A candidate off the path may fail
% (status ~= 0) without consequence; one on the path is an error.
%
% Requires the gateways (see aiyagari_egm_gpu.m).  n_devices = GPUs of this process.

clear; clc;
labor_model = false;
beta = 0.96; sigma = 5; alpha = 0.36; delta = 0.08; phi = 1; theta = 1; b = 0;
if labor_model
    rho = 0.6; sigma_e = 0.2;
else
    rho = 0.75; sigma_e = 0.75;
end
N = 7; Na = 400; tol = 1e-5; max_iter = 1000; dist_tol = 1e-13; dist_max_iter = 100000;
n_steps = 10; levels = 6; n_devices = 1;

l_grid = ((1:N) - 4) * sigma_e;
edges = [-Inf, ((1:N-1) - 3.5) * sigma_e, Inf];
sd = sigma_e * sqrt(1 - rho^2);
P = zeros(N, N);
for i = 1:N
    for j = 1:N
        P(i, j) = integral(@(x) normpdf(x, rho * l_grid(i), sd), edges(j), edges(j + 1));
    end
end
s = exp(l_grid);
pi_stat = [P' - eye(N); ones(1, N)] \ [zeros(N, 1); 1];
labor = s * pi_stat;
wmin = (1 - alpha) * (alpha / ((1 / beta - 1) + delta))^(alpha / (1 - alpha));
amin = min(b, wmin * s(1));
kmax = delta^(1 / (alpha - 1));
amax = kmax^alpha + (1 - delta) * kmax;
a_grid = amin + (amax - amin) * (linspace(0, 1, Na).^2)';

% common warm start: the r0 = 0.04 solution from the scripts' starting policy
r0 = 0.04;
w_stale = (1 - alpha) * (alpha / (r0 + delta))^(alpha / (1 - alpha));
guess = repmat((1 + r0) * a_grid + w_stale * mean(s), 1, N);
if labor_model
    [pc0, ~, ~, ~, it0] = aiy_labor_egm_solve_mex(guess, a_grid, s, P, r0, w_stale, beta, sigma, ...
                                                  phi, theta, amin, tol, max_iter);
else
    [pc0, ~, ~, it0] = aiy_egm_solve_mex(guess, a_grid, s, P, r0, w_stale, beta, sigma, amin, ...
                                         tol, max_iter);
end

lo = -0.05; hi = 1 / beta - 1;
step = 0; done = false; n_rates = 0;
r_history = []; k_supply = []; k_demand = [];
tic;
while ~done && step < n_steps
    L = min(levels, n_steps - step);
    % breadth-first midpoints of the subtree below (lo, hi): node q has bracket br(q, :)
    br = [lo, hi]; nodes = zeros(0, 4);           % [r, lo, hi, depth]
    for lev = 1:L
        nb = zeros(0, 2);
        for q = 1:size(br, 1)
            m = (br(q, 1) + br(q, 2)) / 2;
            nodes(end + 1, :) = [m, br(q, 1), br(q, 2), step + lev]; %#ok<AGROW>
            nb = [nb; br(q, 1), m; m, br(q, 2)]; %#ok<AGROW>
        end
        br = nb;
    end
    % lambda_start = []: every candidate's histogram starts from the uniform distribution
    if labor_model
        [Ks, Kd, it, st, dit] = aiy_egm_ge_hist_batch_mex(nodes(:, 1), pc0, a_grid, s, P, w_stale, ...
            alpha, delta, beta, sigma, amin, labor, tol, max_iter, dist_tol, dist_max_iter, ...
            n_devices, [], phi, theta);
    else
        [Ks, Kd, it, st, dit] = aiy_egm_ge_hist_batch_mex(nodes(:, 1), pc0, a_grid, s, P, w_stale, ...
            alpha, delta, beta, sigma, amin, labor, tol, max_iter, dist_tol, dist_max_iter, ...
            n_devices, []);
    end
    n_rates = n_rates + size(nodes, 1);
    % walk the sequential loop's path through the evaluated tree
    for lev = 1:L
        q = find(nodes(:, 2) == lo & nodes(:, 3) == hi, 1);
        r = nodes(q, 1);
        if st(q) ~= 0
            error('aiy:candidate', 'step %d at r = %.10f: candidate status %d', step + lev, r, st(q));
        end
        r_history(end + 1) = r; k_supply(end + 1) = Ks(q); k_demand(end + 1) = Kd(q); %#ok<AGROW>
        if abs(Ks(q) - Kd(q)) < 1e-5
            done = true;
            break;
        elseif Ks(q) > Kd(q)
            hi = r;
        else
            lo = r;
        end
    end
    step = step + L;
end
fprintf('equilibrium r = %.10f (%d steps, %d candidate rates) in %.3f s\n', ...
        r_history(end), numel(r_history), n_rates, toc);
