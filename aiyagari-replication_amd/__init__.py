"""MI355X-native (gfx950, fp64) solver for the hot path of kostastril/Aiyagari-Replication.

The MATLAB scripts' inner loops (Bellman sweeps, EGM steps, the Monte-Carlo capital supply,
the Krusell-Smith improvement/Howard steps) run as hand-written HIP kernels behind the C ABI
in include/aiyagari_hip.h.  This package is the Python host mirror of that boundary.
There is no CPU fallback: importing works without a GPU, calling a solver without the HIP
library or a device raises.
"""
from . import calibration
from .dist import (dist_stationary, dist_stationary_batch, dist_stationary_batch_dev,
                   dist_stationary_dev, dist_update_dev)
from .egm import (egm_solve, egm_solve_batch_dev, egm_solve_dev, egm_step, egm_step_dev,
                  labor_egm_solve, labor_egm_step)
from ._capi import AiyError, LIB_PATH, declared_symbols, lib
from . import ge
from . import ge_batch
from . import ks_dist
from . import ks_panel
from . import stats
from .ks import (ks_egm_solve, ks_egm_solve_batch, ks_egm_solve_batch_dev, ks_howard, ks_params,
                 ks_policy_improve, ks_vfi_solve, ks_vfi_solve_batch, ks_vfi_solve_batch_dev)
from .ks_panel import (HistSimMulti, krusell_smith_egm, krusell_smith_egm_batch,
                       krusell_smith_vfi, krusell_smith_vfi_batch, ks_simulate_hist_multi)
from .sim import sim_capital, sim_capital_dev
from . import transition
from .transition import (aiyagari_transition, aiyagari_transition_newton, dist_forward_batch,
                         egm_backward_batch, expectation_batch, fake_news, impulse_response,
                         jacobian, prices_from_K, steady_state, transition_batch)
from .transition import (aiyagari_labor_transition, aiyagari_labor_transition_newton,
                         impulse_response_labor, jacobian_labor, labor_dist_forward_batch,
                         labor_dist_forward_batch_dev, labor_egm_backward_batch,
                         labor_egm_backward_batch_dev, labor_transition_batch, prices_from_ratio,
                         steady_state_labor)
from . import estimation
from .estimation import (ar1_loglik, ar1_ma, ar1_mle, autocovariance_batch, ge_jacobians,
                         ge_jacobians_labor, loglik_batch, loglik_batch_dev, ma_batch,
                         ma_batch_dev, moments)
from .estimation import (dense_solve_batch, dense_solve_batch_dev, ge_ma_batch,
                         structural_loglik)
from .transition import jacobian_batch
from . import vfi
from .vfi import (Workspace, labor_solve_batch_dev, labor_vfi_solve, labor_vfi_sweep,
                  solve_batch_dev, vfi_solve, vfi_sweep)

__all__ = ["estimation", "ar1_loglik", "ar1_ma", "ar1_mle", "autocovariance_batch", "ge_jacobians",
           "ge_jacobians_labor", "loglik_batch", "loglik_batch_dev", "ma_batch", "ma_batch_dev",
           "moments", "dense_solve_batch", "dense_solve_batch_dev", "ge_ma_batch",
           "structural_loglik", "jacobian_batch",
           "aiyagari_labor_transition", "aiyagari_labor_transition_newton",
           "impulse_response_labor", "jacobian_labor", "labor_dist_forward_batch",
           "labor_dist_forward_batch_dev", "labor_egm_backward_batch",
           "labor_egm_backward_batch_dev", "labor_transition_batch", "prices_from_ratio",
           "steady_state_labor",
           "transition", "aiyagari_transition", "aiyagari_transition_newton", "expectation_batch", "fake_news", "impulse_response", "jacobian", "dist_forward_batch", "egm_backward_batch", "prices_from_K", "steady_state", "transition_batch", "ge", "ge_batch", "ks_dist", "ks_panel", "stats", "ks_egm_solve", "ks_egm_solve_batch", "ks_egm_solve_batch_dev", "HistSimMulti", "krusell_smith_egm", "krusell_smith_egm_batch", "ks_simulate_hist_multi", "ks_howard", "ks_params", "ks_policy_improve", "ks_vfi_solve", "ks_vfi_solve_batch", "ks_vfi_solve_batch_dev", "krusell_smith_vfi", "krusell_smith_vfi_batch", "dist_stationary", "dist_stationary_batch", "dist_stationary_batch_dev", "dist_stationary_dev", "dist_update_dev", "egm_solve", "egm_solve_batch_dev", "egm_solve_dev", "egm_step", "egm_step_dev", "labor_egm_solve", "labor_egm_step",
           "AiyError", "LIB_PATH", "Workspace", "calibration", "declared_symbols", "lib",
           "labor_solve_batch_dev", "labor_vfi_solve", "sim_capital", "sim_capital_dev", "labor_vfi_sweep", "vfi_solve", "vfi_sweep"]
