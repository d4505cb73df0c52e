// Host-side handle of a batch of ObstacleAvoidanceMPC objects (AM/include/HighLvlMpc.h:4-33) and the
// device workspace of the fused control step.  Shared by mpc_solve.hip and step.hip.
#pragma once
#include <type_traits>
#include <utility>
#include <vector>
#include "mpc_device.h"

struct amk_mpc {
    double T = 0, dt = 0;
    int N = 0, K = 0, S = 0, nx = 0, nref = 0;
    int run_scenes = 0;       // internal (amk_pipeline, a gang that is not full): launches cover scenes [0, run_scenes); 0 = all S
    int launch_scenes() const { return run_scenes > 0 && run_scenes < S ? run_scenes : S; }
    amk::NlpDims dims() const { return {N, K}; }   // nx and nref above are dims().nx() and SceneRecord{N, K}.len()
    double h_prm[amk::PRM_LEN];
    double drag[3] = {0.0, 0.0, 0.0};   // amk_mpc_set_drag_coefficient: v' = a - drag .* v (host-side: only A, B, c see it)
    amk::SolveOpts opt;
    size_t lds_bytes = 0;     // fp64 scratchpad; the fp32 kernels take half
    int precision = 64;       // arithmetic of the solve: 64 (default) or 32 (amk_mpc_set_precision)
    amk::DevBuf<double> prm;  // [PRM_LEN]
    amk::DevBuf<double> w0;   // [S][nx]  mNlpW0
    amk::DevBuf<double> ybuf; // [S][N][K][4]  per collision term: its two multipliers + the geometry cache of the derivative pass (scratch of one solve)
    amk::DevBuf<double> gains; // [S][N][GAIN_STAGE = 32] Riccati feedback gains, structural zeros left out (scratch of one interior-point iteration)
    amk::DevBuf<double> plan_coef;  // item coefficients + lane-role constants of the Riccati plan (mpc_device.h)
    amk::DevBuf<int> plan_meta;     // [PLAN_ITEMS] PlanItemMeta + [64] LaneRole
    // amk_mpc_eval_gamma: d(A, B, c)/d tau (mpc_model.h DtauBlock, recomputed when tau changes)
    amk::DevBuf<double> ev_dtau;
    double ev_dtau_tau[4] = {0, 0, 0, 0};
    bool ev_dtau_valid = false;
    // control-step workspace (allocated by the first amk_step_batch)
    amk::DevBuf<float> knn_pts;     // [S][N][K][3] neighbours of every reference point
    amk::DevBuf<double> knn_d2;     // [S][N][K]
    amk::DevBuf<float> edge_pt;     // [S][3]       nearest edge point of reference point 0
    amk::DevBuf<double> edge_d2;    // [S]
    amk::DevBuf<double> ref_states; // [S][nref]    vecRefStates handed to Solve
    amk::DevBuf<int> done;          // [S]          1: scene left the re-plan loop (:333-335); 2: its solve is paused (iteration budget)
    amk::DevBuf<double> resume_rec; // [S][8 N + 8] what a paused solve needs beside w0 and ybuf (mpc_device.h: SolveSched)
    int solve_budget = 0;           // amk_mpc_set_solve_budget: iterations per launch in the first budget_rounds rounds of a step (0: off)
    int budget_rounds = 0;
    // per-frame raw query results of amk_step_batch_frames (allocated by its first call)
    int mf_frames = 0;
    amk::DevBuf<float> mf_knn_pts, mf_edge_pt;    // [F][S][N][K][3], [F][S][3]
    amk::DevBuf<double> mf_knn_d2, mf_edge_d2;    // [F][S][N][K],    [F][S]
    amk::DevBuf<char> mf_exact;                   // step_frames.hip: FrameExact, when a frame is in AMK_TIES_NANOFLANN mode
    std::vector<char> mf_exact_host;
    amk::HostStage stage;   // staging of the *_host entries: the two evals, the solve, amk_step_batch_host
};

// Internal (not in include/avoid_mpc_amd.h; tests/test_mpc_model.py), host only, needs no device: the model's A [10][10], B [10][4],
// c [10] at tau[4], drag[3], dt, and with dtau (mpc_model.h DtauBlock, [3][150]; null: not wanted) their derivatives in tau_0..2.
// With dtau, A, B, c are the value part of the dual-number run.  The handle's dynamics and amk_mpc_eval_gamma both come from here.
extern "C" int amk__mpc_dynamics(const double *tau, const double *drag, double dt, double *A, double *B, double *c, double *dtau);

namespace amk {
// The horizons with a kernel instantiation of their own (N baked in: LDS offsets become immediates, as the reference bakes N into its
// plugin) -- the BASELINE configs'.  Every other horizon runs the generic instantiation, NT = 0.  This list is the only place they are named.
using BakedHorizons = std::integer_sequence<int, 10, 20, 30>;
template <class F, int... NT>
void with_horizon(int N, F &&f, std::integer_sequence<int, NT...>) {
    if (!((N == NT && (f(std::integral_constant<int, NT>{}), true)) || ...)) f(std::integral_constant<int, 0>{});
}
// calls f(std::integral_constant<int, NT>) with the instantiation that serves horizon N
template <class F>
void with_horizon(int N, F &&f) { with_horizon(N, f, BakedHorizons{}); }

// amk_mpc::run_scenes for the length of a scope (amk_pipeline's control step): whichever way the scope is left, it is 0 again
struct RunScenes {
    amk_mpc *m;
    RunScenes(amk_mpc *mpc, int n) : m(mpc) { m->run_scenes = n; }
    ~RunScenes() { m->run_scenes = 0; }
    RunScenes(const RunScenes &) = delete;
};
// Launches the solve for every scene of `m` (skipping scenes with d_done[s] != 0 when given).
// d_ref_path / d_step_flags: control-step mode (refill mRefPath, count solves / iterations).
// budget / max_passes (control step only, amk_step_batch): see mpc_device.h SolveSched; both 0 = the plain solve.
int launch_solve(amk_mpc *m, const double *d_ref_states, double *d_u, double *d_x0array, int *d_info, const int *d_done,
                 double *d_ref_path, int *d_step_flags, hipStream_t stream, int budget = 0, int max_passes = 0);
}  // namespace amk
