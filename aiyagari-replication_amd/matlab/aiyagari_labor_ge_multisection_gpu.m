% aiyagari_labor_ge_multisection_gpu.m -- the GE search of Aiyagari_Endogenous_Labor_VFI.m
% (:155-250) evaluated breadth-first on the MI355X solver (DESIGN.md §1 row E2), from
% MATLAB/Octave.
%
% Every midpoint the bisection could visit in its next `levels` steps (2^levels - 1 rates, each
% computed from its own bracket exactly as the sequential loop computes it) goes to the GPUs in
% ONE call, aiy_labor_ge_batch_mex: the labour VFI of every rate at its own wage from the common
% warm start (the r0 = 0.04 solution: v_old, v_new and the policies), one launch per sweep over
% all rates still running, then the Monte-Carlo supplies with the uniforms block of each node's
% depth, and K_d.  The script then walks the sequential loop's path through the evaluated tree,
% so r, r_history and the early stop are the bisection's.
%
% Requires the gateways (see aiyagari_labor_vfi_gpu.m).  n_devices = GPUs of this process.

clear; clc;
beta = 0.96; sigma = 5; alpha = 0.36; delta = 0.08; psi = 1; eta = 2; b = 0;
rho = 0.6; sigma_e = 0.2;
N = 7; Na = 400; tol = 1e-5; max_iter = 1000; T = 10000;
n_steps = 10; levels = 2; n_devices = 1;
labor_choice = linspace(0.01, 1.5, 10);

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

% the script's stream: randi(N), randi(Na), then T-1 draws per simulation (initial + steps)
rng(5489, 'twister');
z1 = randi(N);
k1 = a_grid(randi(Na));
U = rand(T - 1, n_steps + 1);          % column d+1 = the draws of bisection step d

% common warm start: the r0 = 0.04 solution from v = 0 (the script's first solve)
r0 = 0.04;
w0 = (1 - alpha) * (alpha / (r0 + delta))^(alpha / (1 - alpha));
[v_new0, v_old0, pk0, pl0, pc0, it0] = aiy_labor_vfi_solve_mex(zeros(N, Na), a_grid, s, P, ...
    labor_choice, r0, w0, beta, sigma, psi, eta, tol, max_iter);

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
    [Ks, Kd, it] = aiy_labor_ge_batch_mex(nodes(:, 1), v_old0, v_new0, pk0, pl0, pc0, [], ...
        a_grid, s, P, labor_choice, alpha, delta, beta, sigma, psi, eta, labor, tol, max_iter, ...
        z1, k1, U(:, nodes(:, 4) + 1), n_devices);
    n_rates = n_rates + size(nodes, 1);
    % walk the sequential loop's path through the evaluated tree
    for lev = 1:L
        q = find(nodes(:, 2) == lo & nodes(:, 3) == hi, 1);
        r = nodes(q, 1);
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
