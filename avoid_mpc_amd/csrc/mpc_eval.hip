// The NLP functions of the reference's generated solver plugin, evaluated on the device at caller-supplied points.
//
// The reference's plugin (AM/tools/mpc_obstacle_casadi.py:290-300 -> so/mpc_obstacle_v2.so, loaded at
// AM/src/HighLvlMpc.cpp:50,52) exports nlp_f, nlp_g, nlp_grad_f, nlp_jac_g, nlp_hess_l of the multiple-shooting NLP
//   x = [X_0, U_0, X_1, ..., U_{N-1}, X_N]                                  mpc_obstacle_casadi.py:158,164,217,224
//   f = objective                                                            :153-214
//   g = [X_0 - P[0:10] ; F(X_k, U_k) - X_{k+1}]                              :156-160,219
// amk_mpc_eval computes all of them for a batch of scenes; casadi_plugin.hip wraps
// it in the plugin's own C ABI.  One wavefront per scene: the decision vector is loaded into LDS and the objective
// pass of the solver (mpc_device_impl.h evaluate<true, EXACT>) runs on it in the plugin's form -- |s| itself, its
// derivative sign(s), no curvature from the abs() (CasADi's SX rule for fabs).  The constraints are linear in x
// (F = A x + B u + c with the drag term off, mpc_parameters.yaml:4), so jac_g is constant and hess_l = lam_f hess f.
#include "mpc_handle.h"

#include <cstring>
#include <vector>

using namespace amk;

namespace {

// What both kernels open with: the scene's record and decision vector w = [X_0, U_0, ..., X_N] into LDS -- the solver's own carve-up
// with A and B behind the parameters, LdsMap(N, PRM_LEN) -- and the solver's objective pass on it.  Returns f; q, r, H6 (and X, U,
// cy, sy, the parameters) are in LDS behind the barrier it ends with.  io: the scene's reference states and obstacle points.
__device__ __forceinline__ double load_and_evaluate(double *sm, const LdsMap &L, const SceneRecord &R, const double *__restrict__ prm,
                                                    const double *__restrict__ P, const double *__restrict__ w, SceneIO &io) {
    const int lane = threadIdx.x, N = R.N;
    io.ref = R.ref(P);
    io.obs = R.obs(P);
    load_scene(sm, L, N, prm, PRM_LEN, P + R.x_init(), R.target(P), io);   // the solve's own opening, with A and B
    for (int e = lane; e < (N + 1) * SD; e += 64) sm[L.X + e] = w[NlpDims::kStage * (e / SD) + e % SD];
    for (int e = lane; e < N * UD; e += 64) sm[L.U + e] = w[NlpDims::kStage * (e / UD) + SD + e % UD];
    __syncthreads();
    const double f = evaluate<true, true>(sm, L, io, N, R.K, sm + L.X, sm + L.U, 0.0, 0.0, 0.0, nullptr, nullptr);
    __syncthreads();
    return f;
}

template <int NT>
__global__ __launch_bounds__(64) void mpc_eval_kernel(int Nrt, int K, int nref, int nx, const double *__restrict__ prm,
                                                      const double *__restrict__ w_all, const double *__restrict__ ref_states,
                                                      const double *__restrict__ lam_f, double *__restrict__ f_out,
                                                      double *__restrict__ grad_out, double *__restrict__ g_out,
                                                      double *__restrict__ jac_out, double *__restrict__ hess_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_raw[];
    double *sm = reinterpret_cast<double *>(sm_raw);
    const int s = blockIdx.x, lane = threadIdx.x;
    const int N = NT > 0 ? NT : Nrt;
    const LdsMap L(N, PRM_LEN);
    const NlpDims D{N, K};
    SceneIO io;
    const double f = load_and_evaluate(sm, L, SceneRecord{N, K}, prm, ref_states + (size_t)s * nref, w_all + (size_t)s * nx, io);
    const double *pr = sm + L.prm;
    if (f_out && lane == 0) f_out[s] = f;
    if (grad_out) {  // zero on X_0 (no cost is attached to it), q on X_1..X_N, r on U_k
        double *go = grad_out + (size_t)s * nx;
        for (int e = lane; e < (N + 1) * SD; e += 64) go[NlpDims::kStage * (e / SD) + e % SD] = e < SD ? 0.0 : sm[L.q + e];
        for (int e = lane; e < N * UD; e += 64) go[NlpDims::kStage * (e / UD) + SD + e % UD] = sm[L.r + e];
    }
    if (g_out) {
        double *go = g_out + (size_t)s * D.ng();
        const double *A = pr + PRM_A, *B = pr + PRM_B, *c = pr + PRM_C;
        if (lane < SD) go[lane] = sm[L.X + lane] - sm[L.xinit + lane];  // :160
        for (int e = lane; e < N * SD; e += 64) {                      // F(X_k, U_k) - X_{k+1}, :219
            const int k = e / SD, i = e % SD;
            double a = 0.0;
#pragma unroll
            for (int j = 0; j < SD; ++j) a += A[i * SD + j] * sm[L.X + k * SD + j];
#pragma unroll
            for (int j = 0; j < UD; ++j) a += B[i * UD + j] * sm[L.U + k * UD + j];
            go[SD + e] = (a + c[i]) - sm[L.X + (k + 1) * SD + i];
        }
    }
    if (jac_out) {  // constant; column-major, rows ascending (see amk_mpc_jac_sparsity)
        double *jo = jac_out + (size_t)s * D.nnz_jac();
        const double *A = pr + PRM_A, *B = pr + PRM_B;
        for (int e = lane; e < (N + 1) * SD + N * UD; e += 64) {  // one decision variable = one column per lane-step
            const bool is_u = e >= (N + 1) * SD;
            const int k = is_u ? (e - (N + 1) * SD) / UD : e / SD, i = is_u ? (e - (N + 1) * SD) % UD : e % SD;
            int r[3];
            if (is_u) {
                int pos = D.jac_u(k);  // after X_k's column block
                for (int a = 0; a < i; ++a) pos += rows_of_B(a, r);
                const int nr = rows_of_B(i, r);
                for (int t = 0; t < nr; ++t) jo[pos + t] = B[r[t] * UD + i];
            } else {
                int pos = D.jac_x(k);
                for (int j = 0; j < i; ++j) pos += 1 + (k < N ? rows_of_A(j, r) : 0);
                jo[pos] = k == 0 ? 1.0 : -1.0;  // d(X_0 - x_init)/dX_0 or d(-X_k)/dX_k of the previous defect
                if (k < N) {
                    const int nr = rows_of_A(i, r);
                    for (int t = 0; t < nr; ++t) jo[pos + 1 + t] = A[r[t] * SD + i];
                }
            }
        }
    }
    if (hess_out) {  // lam_f * upper triangle, column-major (see amk_mpc_hess_sparsity)
        double *ho = hess_out + (size_t)s * D.nnz_hess();
        const double sig = lam_f ? lam_f[s] : 1.0;
        for (int e = lane; e < NlpDims::kHessX * (N - 1); e += 64) {  // X_1 .. X_{N-1}
            const int k = e / NlpDims::kHessX, t = e % NlpDims::kHessX;  // Hessian block of X_{k+1}, cost stage k
            const int i = hess_entry(t).row, j = hess_entry(t).col;
            double h = 0.0;
            const RotEntry rot = rot_entry(i, j);
            if (rot.block >= 0) {  // rotated 2x2 blocks of 2 R'Q_pen R, :174-185,206-208
                const double cy = sm[L.cy + k], sy = sm[L.sy + k];
                const double w0q = 2.0 * pr[PRM_W + 10 + 4 * rot.block], w1q = 2.0 * pr[PRM_W + 11 + 4 * rot.block];
                const int which = rot.which;
                h = which == 0 ? cy * cy * w0q + sy * sy * w1q : which == 1 ? -cy * sy * w0q + sy * cy * w1q : sy * sy * w0q + cy * cy * w1q;
            } else if (i == j) {
                h = 2.0 * pr[PRM_W + 10 + i];
            }
            const int pi = pv_inv(i), pj = pv_inv(j);
            if (pi >= 0 && pj >= 0) h += sm[L.H6 + k * 21 + pj * (pj + 1) / 2 + pi];  // i <= j: lower-triangle index (pj, pi)
            ho[D.hess_x(k + 1) + t] = sig * h;
        }
        for (int e = lane; e < SD; e += 64) ho[D.hess_x(N) + e] = sig * 2.0 * pr[PRM_W + e];  // X_N: 2 Q_goal
        for (int e = lane; e < N * UD; e += 64) {                                                      // U_k: 2 Q_u
            const int k = e / UD, a = e % UD;
            ho[D.hess_u(k) + a] = sig * 2.0 * pr[PRM_W + 20 + a];
        }
    }
}

// ---- nlp_grad (mpc_obstacle_casadi.py:294-303 emits it with the other dependencies; CasADi's nlpsol evaluates it after a solve
// for lam_p): gamma = lam_f f + lam_g' g;  outputs grad_x gamma = lam_f grad f + J' lam_g and grad_p gamma over the WHOLE
// parameter vector p = [x_init | ref | obstacles | target | gain(4) | tau(4) | weights(25) | radius].  dtau: d(A, B, c)/d tau_a
// for a = 0, 1, 2 (mpc_model.h DtauBlock), from the model's affine probe on dual numbers (amk__mpc_dynamics).
template <int NT>
__global__ __launch_bounds__(64) void mpc_eval_gamma_kernel(int Nrt, int K, int nref, int nx, const double *__restrict__ prm,
                                                            const double *__restrict__ dtau, const double *__restrict__ w_all,
                                                            const double *__restrict__ ref_states,
                                                            const double *__restrict__ lam_f_all,
                                                            const double *__restrict__ lam_g_all, double *__restrict__ gx_out,
                                                            double *__restrict__ gp_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_raw[];
    double *sm = reinterpret_cast<double *>(sm_raw);
    const int s = blockIdx.x, lane = threadIdx.x;
    const int N = NT > 0 ? NT : Nrt;
    const LdsMap L(N, PRM_LEN);
    const NlpDims D{N, K};
    const SceneRecord R{N, K};
    const double *lg = lam_g_all ? lam_g_all + (size_t)s * D.ng() : nullptr;
    const double sig = lam_f_all ? lam_f_all[s] : 1.0;
    SceneIO io;
    load_and_evaluate(sm, L, R, prm, ref_states + (size_t)s * nref, w_all + (size_t)s * nx, io);
    const double *pr = sm + L.prm;
    auto lam = [&](int row) { return lg ? lg[row] : 0.0; };   // multiplier of row `row` of g
    auto lam_F = [&](int k, int i) { return lam(SD + SD * k + i); };   // ... of row i of the defect F(X_k, U_k) - X_{k+1}
    if (gx_out) {
        double *go = gx_out + (size_t)s * nx;
        const double *A = pr + PRM_A, *B = pr + PRM_B;
        int r[3];
        for (int e = lane; e < (N + 1) * SD; e += 64) {
            const int k = e / SD, i = e % SD;
            double a = sig * (k == 0 ? 0.0 : sm[L.q + e]);
            a += k == 0 ? lam(i) : -lam_F(k - 1, i);
            if (k < N) {
                const int nr = rows_of_A(i, r);
                for (int t = 0; t < nr; ++t) a += A[r[t] * SD + i] * lam_F(k, r[t]);
            }
            go[NlpDims::kStage * k + i] = a;
        }
        for (int e = lane; e < N * UD; e += 64) {
            const int k = e / UD, c = e % UD;
            double a = sig * sm[L.r + e];
            const int nr = rows_of_B(c, r);
            for (int t = 0; t < nr; ++t) a += B[r[t] * UD + c] * lam_F(k, r[t]);
            go[NlpDims::kStage * k + SD + c] = a;
        }
    }
    if (!gp_out) return;
    double *gp = gp_out + (size_t)s * D.np();
    const double lamw = pr[PRM_W + 24], radius = pr[PRM_RADIUS];
    if (lane < SD) gp[R.x_init() + lane] = -lam(lane);                                   // x_init: g[0:10] = X_0 - x_init
    // ---- reference states and the Q_pen part of the weights: lane = path stage
    double wq[SD];
#pragma unroll
    for (int i = 0; i < SD; ++i) wq[i] = 0.0;
    for (int k = lane; k < N; k += 64) {
        double *o = gp + R.ref() + k * SD;
        if (k >= N - 1) {  // the last reference state is not used by the objective (:168-171)
            for (int i = 0; i < SD; ++i) o[i] = 0.0;
            continue;
        }
        const double *xk = sm + L.X + (k + 1) * SD, *rf = io.ref + k * SD;
        const double cy = sm[L.cy + k], sy = sm[L.sy + k];
        double d[SD], y[SD];
        for (int i = 0; i < SD; ++i) { d[i] = xk[i] - rf[i]; y[i] = d[i]; }
        y[0] = cy * d[0] - sy * d[1]; y[1] = sy * d[0] + cy * d[1];
        y[4] = cy * d[4] - sy * d[5]; y[5] = sy * d[4] + cy * d[5];
        double wy[SD];
        for (int i = 0; i < SD; ++i) { wy[i] = 2.0 * pr[PRM_W + 10 + i] * y[i]; wq[i] += y[i] * y[i]; }
        double qq[SD];
        for (int i = 0; i < SD; ++i) qq[i] = wy[i];
        qq[0] = cy * wy[0] + sy * wy[1]; qq[1] = -sy * wy[0] + cy * wy[1];
        qq[4] = cy * wy[4] + sy * wy[5]; qq[5] = -sy * wy[4] + cy * wy[5];
        for (int i = 0; i < SD; ++i) o[i] = -sig * qq[i];
        // yaw_ref also turns the rotation: dy0 = y1, dy1 = -y0 (and 4, 5 alike) per unit of yaw_ref
        o[3] = sig * (-wy[3] + (wy[0] * y[1] - wy[1] * y[0]) + (wy[4] * y[5] - wy[5] * y[4]));
    }
    // ---- obstacle points, d/d lambda, d/d radius: lane = collision term
    double dl = 0.0, dr = 0.0;
    for (int e = lane; e < N * K; e += 64) {
        const int k = e / K;
        double *o = gp + R.obs() + 3 * e;
        if (k >= N - 1) { o[0] = o[1] = o[2] = 0.0; continue; }
        const double *xk = sm + L.X + (k + 1) * SD;
        const double *op = io.obs + 3 * (size_t)e;
        const double d0 = op[0] - xk[0], d1 = op[1] - xk[1], d2 = op[2] - xk[2];
        const double rho = sqrt(d0 * d0 + d1 * d1 + d2 * d2), ir = 1.0 / rho;
        const double x = -32.0 * (rho - radius), ex = exp(x), g = log(1.0 + ex), sg = ex / (1.0 + ex), gpr = -32.0 * sg;
        const double n[3] = {d0 * ir, d1 * ir, d2 * ir};
        const double sv = xk[4] * n[0] + xk[5] * n[1] + xk[6] * n[2];
        const double sgn = sv > 0.0 ? 1.0 : (sv < 0.0 ? -1.0 : 0.0);
        const double t[3] = {xk[4] - sv * n[0], xk[5] - sv * n[1], xk[6] - sv * n[2]};
        for (int i = 0; i < 3; ++i) o[i] = sig * lamw * sgn * (gpr * n[i] * sv + g * t[i] * ir);  // = -d/dp of the term
        dl += g * fabs(sv);
        dr += lamw * 32.0 * sg * fabs(sv);
    }
    dl = wave_sum(dl); dr = wave_sum(dr);
    double wsum[SD];
#pragma unroll
    for (int i = 0; i < SD; ++i) wsum[i] = wave_sum(wq[i]);
    // ---- control weights, d/d tau
    double wu[UD] = {0.0, 0.0, 0.0, 0.0}, dt3[3] = {0.0, 0.0, 0.0};
    for (int k = lane; k < N; k += 64) {
        const double *uk = sm + L.U + k * UD, *xk = sm + L.X + k * SD;
        const double uref[4] = {0.0, 0.0, kGz, 0.0};
        for (int i = 0; i < UD; ++i) wu[i] += (uk[i] - uref[i]) * (uk[i] - uref[i]);
        for (int a = 0; a < DtauBlock::kAxes; ++a) {
            const double *dA = dtau + a * DtauBlock::kLen + DtauBlock::kA, *dB = dtau + a * DtauBlock::kLen + DtauBlock::kB,
                         *dc = dtau + a * DtauBlock::kLen + DtauBlock::kC;
            double acc = 0.0;
            for (int i = 0; i < SD; ++i) {
                double fi = dc[i];
                for (int j = 0; j < SD; ++j) fi += dA[i * SD + j] * xk[j];
                for (int j = 0; j < UD; ++j) fi += dB[i * UD + j] * uk[j];
                acc += lam_F(k, i) * fi;
            }
            dt3[a] += acc;
        }
    }
    for (int i = 0; i < UD; ++i) wu[i] = wave_sum(wu[i]);
    for (int a = 0; a < 3; ++a) dt3[a] = wave_sum(dt3[a]);
    double *tg = gp + R.target();
    if (lane < SD) {
        const double dgl = sm[L.X + N * SD + lane] - sm[L.target + lane];
        tg[lane] = -sig * 2.0 * pr[PRM_W + lane] * dgl;                        // target
        tg[SD + NlpDims::kTailW + lane] = sig * dgl * dgl;                     // Q_goal
    }
    if (lane == 0) {
        double *tail = tg + SD;   // gain(4) tau(4) weights(25) radius
        double *tw = tail + NlpDims::kTailW;   // weights: Q_goal[10] (above) Q_pen[10] Q_u[4] lambda, as PRM_W
        for (int i = 0; i < 4; ++i) tail[NlpDims::kTailGain + i] = 0.0;       // gain: unused by the model (:114-121)
        for (int a = 0; a < 3; ++a) tail[NlpDims::kTailTau + a] = dt3[a];
        tail[NlpDims::kTailTau + 3] = 0.0;                                    // tau_yaw: unused
        for (int i = 0; i < SD; ++i) tw[10 + i] = sig * wsum[i];              // Q_pen
        for (int i = 0; i < UD; ++i) tw[20 + i] = sig * wu[i];                // Q_u
        tw[24] = sig * dl;                                                    // lambda
        tail[NlpDims::kTailRadius] = sig * dr;                                // radius
    }
}

hipError_t wait_null_stream() { return hipStreamSynchronize(nullptr); }

}  // namespace

extern "C" {

int amk_mpc_ng(const amk_mpc *m) { return m ? m->dims().ng() : -1; }
int amk_mpc_np(const amk_mpc *m) { return m ? m->dims().np() : -1; }
int amk_mpc_jac_nnz(const amk_mpc *m) { return m ? m->dims().nnz_jac() : -1; }
int amk_mpc_hess_nnz(const amk_mpc *m) { return m ? m->dims().nnz_hess() : -1; }

int amk_mpc_jac_sparsity(const amk_mpc *m, int *colind, int *row) {
    if (!m || !colind || !row) return AMK_ERR_INVALID_ARG;
    const int N = m->N;
    auto defect = [](int k, int i) { return SD + SD * k + i; };   // row i of F(X_k, U_k) - X_{k+1}
    int pos = 0, col = 0, r[3];
    for (int k = 0; k <= N; ++k) {
        for (int i = 0; i < SD; ++i) {  // column of X_k[i]
            colind[col++] = pos;
            row[pos++] = k == 0 ? i : defect(k - 1, i);
            if (k < N)
                for (int t = 0, nr = rows_of_A(i, r); t < nr; ++t) row[pos++] = defect(k, r[t]);
        }
        if (k < N)
            for (int a = 0; a < UD; ++a) {  // column of U_k[a]
                colind[col++] = pos;
                for (int t = 0, nr = rows_of_B(a, r); t < nr; ++t) row[pos++] = defect(k, r[t]);
            }
    }
    colind[col] = pos;
    return pos == m->dims().nnz_jac() && col == m->nx ? AMK_OK : AMK_ERR_UNSUPPORTED;
}

int amk_mpc_hess_sparsity(const amk_mpc *m, int *colind, int *row) {
    if (!m || !colind || !row) return AMK_ERR_INVALID_ARG;
    const int N = m->N;
    int pos = 0, col = 0;
    for (int k = 0; k <= N; ++k) {
        for (int j = 0; j < SD; ++j) {  // column of X_k[j]
            colind[col++] = pos;
            if (k == 0) continue;       // no cost on X_0
            if (k == N) { row[pos++] = NlpDims::kStage * k + j; continue; }
            for (int t = 0; t < NlpDims::kHessX; ++t)
                if (hess_entry(t).col == j) row[pos++] = NlpDims::kStage * k + hess_entry(t).row;
        }
        if (k < N)
            for (int a = 0; a < UD; ++a) {
                colind[col++] = pos;
                row[pos++] = NlpDims::kStage * k + SD + a;
            }
    }
    colind[col] = pos;
    return pos == m->dims().nnz_hess() && col == m->nx ? AMK_OK : AMK_ERR_UNSUPPORTED;
}

int amk_mpc_eval(amk_mpc *m, const double *d_w, const double *d_ref_states, const double *d_lam_f, double *d_f,
                 double *d_grad_f, double *d_g, double *d_jac_g, double *d_hess_l, void *stream) {
    if (!m || !d_w || !d_ref_states) return AMK_ERR_INVALID_ARG;
    // the kernel lays its scratchpad out with LdsMap(N, PRM_LEN) -- A and B in LDS, 140 doubles more than the solver's map
    const size_t lds = sizeof(double) * (size_t)LdsMap(m->N, PRM_LEN).total;
    with_horizon(m->N, [&](auto nt) {
        hipLaunchKernelGGL(mpc_eval_kernel<decltype(nt)::value>, dim3(m->S), dim3(64), lds, (hipStream_t)stream, m->N, m->K, m->nref,
                           m->nx, m->prm.p, d_w, d_ref_states, d_lam_f, d_f, d_grad_f, d_g, d_jac_g, d_hess_l);
    });
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_mpc_eval_gamma(amk_mpc *m, const double *d_w, const double *d_ref_states, const double *d_lam_f, const double *d_lam_g,
                       double *d_grad_x, double *d_grad_p, void *stream) {
    if (!m || !d_w || !d_ref_states) return AMK_ERR_INVALID_ARG;
    constexpr int kDtau = DtauBlock::kAxes * DtauBlock::kLen;
    if (!m->ev_dtau.p) AMK_HIP(m->ev_dtau.alloc(kDtau));
    if (!m->ev_dtau_valid || std::memcmp(m->ev_dtau_tau, m->h_prm + PRM_TAU, sizeof m->ev_dtau_tau) != 0) {
        double h[kDtau], A[SD * SD], B[SD * UD], c[SD];   // A, B, c: the value part, which the handle holds already
        amk__mpc_dynamics(m->h_prm + PRM_TAU, m->drag, m->dt, A, B, c, h);
        AMK_HIP(hipMemcpy(m->ev_dtau.p, h, sizeof h, hipMemcpyHostToDevice));
        std::memcpy(m->ev_dtau_tau, m->h_prm + PRM_TAU, sizeof m->ev_dtau_tau);
        m->ev_dtau_valid = true;
    }
    const size_t lds = sizeof(double) * (size_t)LdsMap(m->N, PRM_LEN).total;
    with_horizon(m->N, [&](auto nt) {
        hipLaunchKernelGGL(mpc_eval_gamma_kernel<decltype(nt)::value>, dim3(m->S), dim3(64), lds, (hipStream_t)stream, m->N, m->K,
                           m->nref, m->nx, m->prm.p, m->ev_dtau.p, d_w, d_ref_states, d_lam_f, d_lam_g, d_grad_x, d_grad_p);
    });
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_mpc_eval_gamma_host(amk_mpc *m, const double *h_w, const double *h_ref_states, const double *h_lam_f,
                            const double *h_lam_g, double *h_grad_x, double *h_grad_p) {
    if (!m || !h_w || !h_ref_states) return AMK_ERR_INVALID_ARG;
    const NlpDims D = m->dims();
    const size_t B = sizeof(double) * m->S;   // bytes of one double per scene
    enum { W, REF, LAM_F, LAM_G, GRAD_X, GRAD_P };
    return m->stage.call({to_device(h_w, B * D.nx()), to_device(h_ref_states, B * m->nref), if_given(to_device(h_lam_f, B)),
                          if_given(to_device(h_lam_g, B * D.ng())), if_given(to_host(h_grad_x, B * D.nx())),
                          if_given(to_host(h_grad_p, B * D.np()))},
                         [&](const HostStage::Dev *d) {
                             return amk_mpc_eval_gamma(m, d[W], d[REF], d[LAM_F], d[LAM_G], d[GRAD_X], d[GRAD_P], nullptr);
                         },
                         wait_null_stream);
}

int amk_mpc_eval_host(amk_mpc *m, const double *h_w, const double *h_ref_states, const double *h_lam_f, double *h_f,
                      double *h_grad_f, double *h_g, double *h_jac_g, double *h_hess_l) {
    if (!m || !h_w || !h_ref_states) return AMK_ERR_INVALID_ARG;
    const NlpDims D = m->dims();
    const size_t B = sizeof(double) * m->S;   // bytes of one double per scene
    enum { W, REF, LAM_F, F, GRAD_F, G, JAC_G, HESS_L };
    return m->stage.call({to_device(h_w, B * D.nx()), to_device(h_ref_states, B * m->nref), if_given(to_device(h_lam_f, B)),
                          if_given(to_host(h_f, B)), if_given(to_host(h_grad_f, B * D.nx())), if_given(to_host(h_g, B * D.ng())),
                          if_given(to_host(h_jac_g, B * D.nnz_jac())), if_given(to_host(h_hess_l, B * D.nnz_hess()))},
                         [&](const HostStage::Dev *d) {
                             return amk_mpc_eval(m, d[W], d[REF], d[LAM_F], d[F], d[GRAD_F], d[G], d[JAC_G], d[HESS_L], nullptr);
                         },
                         wait_null_stream);
}

}  // extern "C"
