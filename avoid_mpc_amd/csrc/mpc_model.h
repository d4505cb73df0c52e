// The MPC's model, stated once for the host and the device: the quadrotor ODE with its RK4 x 4 step and affine probe (generic in
// the scalar), the structure that follows from it (non-zeros of A and B, the Hessian pattern, the rotated 2x2 blocks), and the packed
// layouts both sides index (the scene record P, the NLP's sizes, the parameter tail, the d/d tau block).
// Specification: AM/tools/mpc_obstacle_casadi.py:36-122,153-224,338-357; packing: AM/src/HighLvlMpc.cpp:74-107.
// Plain C++17: a host compiler reads it without HIP (the model has a CPU test and a stand-alone sanitizer program).
#pragma once
#include "../../include/avoid_mpc_amd.h"

#if defined(__HIPCC__)
#define AMK_HD __host__ __device__ __forceinline__
#else
#define AMK_HD inline
#endif

namespace amk {

constexpr int SD = AMK_S_DIM;  // 10
constexpr int UD = AMK_U_DIM;  // 4
constexpr double kGz = 9.81;   // mpc_obstacle_casadi.py:39

// ---- structure ----------------------------------------------------------------------------------------------------------------
// nonzero rows of column j of A / column a of B (fixed by the model: p <- v <- a chains per axis,
// yaw <- yaw_dot; mpc_obstacle_casadi.py:106-122).  Returns count, rows in r[3].
AMK_HD int rows_of_A(int j, int r[3]) {
    if (j < 4) { r[0] = j; return 1; }                     // p_x,p_y,p_z,yaw: identity column
    if (j < 7) { r[0] = j - 4; r[1] = j; return 2; }       // v_a: rows p_a, v_a
    r[0] = j - 7; r[1] = j - 3; r[2] = j; return 3;        // a_a: rows p_a, v_a, a_a
}
AMK_HD int rows_of_B(int a, int r[3]) {
    if (a == 3) { r[0] = 3; return 1; }                    // yaw_dot -> yaw
    r[0] = a; r[1] = 4 + a; r[2] = 7 + a; return 3;        // a_cmd -> p_a, v_a, a_a
}

// position/velocity slots of the 10-state, and the inverse map (-1 = not in the 6-block)
AMK_HD int pv_of(int i) { return i < 3 ? i : i + 1; }   // 0..5 -> {0,1,2,4,5,6}
AMK_HD int pv_inv(int s) { return s < 3 ? s : (s >= 4 && s <= 6 ? s - 1 : -1); }

// Entry (i, j) of a stage's state Hessian inside the rotated 2x2 blocks of 2 R'Q_pen R (:174-185,206-208): block 0 is (px, py),
// block 1 (vx, vy), -1 none; which = 0: [0][0], 1: the off-diagonal, 2: [1][1] (the order of LdsMap::rotQ's three per block)
struct RotEntry { int block, which; };
AMK_HD RotEntry rot_entry(int i, int j) {
    const int bi = (i == 0 || i == 1) ? 0 : ((i == 4 || i == 5) ? 1 : -1);
    const int bj = (j == 0 || j == 1) ? 0 : ((j == 4 || j == 5) ? 1 : -1);
    return {bi == bj ? bi : -1, ((i == 1 || i == 5) ? 1 : 0) + ((j == 1 || j == 5) ? 1 : 0)};
}

// ---- layouts ------------------------------------------------------------------------------------------------------------------
// the scene record P = [x_init 10 | ref 10 N | obs 3 K N | target 10] (HighLvlMpc.cpp:74-96): offsets in doubles
struct SceneRecord {
    int N, K;
    AMK_HD int x_init() const { return 0; }
    AMK_HD int ref() const { return SD; }
    AMK_HD int obs() const { return SD + SD * N; }
    AMK_HD int target() const { return SD + SD * N + 3 * K * N; }
    AMK_HD int len() const { return target() + SD; }
    // the same slices of the record at P, each from the one before it (the form the solve kernels' address arithmetic was written in)
    template <class T> AMK_HD T *ref(T *P) const { return P + SD; }
    template <class T> AMK_HD T *obs(T *P) const { return ref(P) + SD * N; }
    template <class T> AMK_HD T *target(T *P) const { return obs(P) + 3 * K * N; }
};

// the multiple-shooting NLP: x = [X_0, U_0, ..., U_{N-1}, X_N], g = [X_0 - x_init ; F(X_k, U_k) - X_{k+1}], p = [P | tail]
struct NlpDims {
    static constexpr int kStage = SD + UD;   // 14: one [X_k, U_k] row of x (and of x0array)
    static constexpr int kJacX = 29;         // Jacobian entries of the 10 columns of X_k, k < N: 10 x (-+1) + the 19 of A
    static constexpr int kJacU = 10;         // ... of the 4 columns of U_k: the 10 of B
    static constexpr int kHessX = 25;        // upper-triangle entries of the Hessian block of X_k, 1 <= k <= N - 1
    static constexpr int kHessU = 4;         // ... of U_k: 2 Q_u
    // tail of p: gain(4) tau(4) weights(25) radius (HighLvlMpc.cpp:97-107)
    static constexpr int kTailGain = 0, kTailTau = 4, kTailW = 8, kTailRadius = 33, kTail = 34;
    int N, K;
    AMK_HD int nx() const { return SD + kStage * N; }
    AMK_HD int ng() const { return SD + SD * N; }
    AMK_HD int np() const { return SceneRecord{N, K}.len() + kTail; }
    AMK_HD int nnz_jac() const { return SD + (kJacX + kJacU) * N; }
    AMK_HD int nnz_hess() const { return kHessX * (N - 1) + SD + kHessU * N; }
    // where a stage's entries start in the two value arrays (columns in the order of x)
    AMK_HD int jac_x(int k) const { return (kJacX + kJacU) * k; }
    AMK_HD int jac_u(int k) const { return jac_x(k) + kJacX; }
    AMK_HD int hess_u(int k) const { return k == 0 ? 0 : kHessU * k + kHessX * k; }       // X_0 has no entries
    AMK_HD int hess_x(int k) const { return kHessU * k + kHessX * (k - 1); }               // 1 <= k <= N
};

// order of the 25 structural non-zeros of the upper triangle of the Hessian block of X_k (1 <= k <= N-1), column-major,
// rows ascending inside a column (CCS): the 6x6 (p,v) block is dense, yaw and the accelerations only have a diagonal
struct HessEntry { int row, col; };
AMK_HD HessEntry hess_entry(int t) {
    constexpr signed char row[NlpDims::kHessX] = {0, 0, 1, 0, 1, 2, 3, 0, 1, 2, 4, 0, 1, 2, 4, 5, 0, 1, 2, 4, 5, 6, 7, 8, 9};
    constexpr signed char col[NlpDims::kHessX] = {0, 1, 1, 2, 2, 2, 3, 4, 4, 4, 4, 5, 5, 5, 5, 5, 6, 6, 6, 6, 6, 6, 7, 8, 9};
    return {row[t], col[t]};
}

// d(A, B, c)/d tau_a for a = 0, 1, 2 (tau_yaw is not used by the model): [kAxes][kLen] doubles
struct DtauBlock {
    static constexpr int kAxes = 3, kA = 0, kB = SD * SD, kC = kB + SD * UD, kLen = kC + SD;   // A 100 | B 40 | c 10 = 150
};

// ---- the model ----------------------------------------------------------------------------------------------------------------
// value and derivative along one direction: the second scalar the model is run on
struct Dual { double v, d; };
AMK_HD Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
AMK_HD Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
AMK_HD Dual operator-(Dual a, double b) { return {a.v - b, a.d}; }
AMK_HD Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
AMK_HD Dual operator*(Dual a, double b) { return {a.v * b, a.d * b}; }
AMK_HD Dual operator*(double a, Dual b) { return {a * b.v, a * b.d}; }
AMK_HD Dual operator/(Dual a, double b) { return {a.v / b, a.d / b}; }

// The quadrotor ODE (mpc_obstacle_casadi.py:95-122).  Drag (:95-105, yaml use_drag_coefficient): `rotmat * diag(k, k, k) *
// rotmat.T * v` read as matrix products is k v whatever the attitude (R (k I) R' = k I) -- linear in the state, so the step stays
// affine with the same sparsity (amk_mpc_set_drag_coefficient): v' = a - drag .* v.
template <class T>
AMK_HD void ode(const T *x, const T *u, const T *tau, const double *drag, T *xd) {
    xd[0] = x[4]; xd[1] = x[5]; xd[2] = x[6];
    xd[3] = u[3];
    xd[4] = x[7] - drag[0] * x[4]; xd[5] = x[8] - drag[1] * x[5]; xd[6] = x[9] - drag[2] * x[6];
    xd[7] = (u[0] - x[7]) * tau[0];
    xd[8] = (u[1] - x[8]) * tau[1];
    xd[9] = (u[2] - kGz - x[9]) * tau[2];
}

// F(x, u): RK4 x 4 over dt (:338-357)
template <class T>
AMK_HD void rk4(const T *x, const T *u, const T *tau, const double *drag, double dt, T *xn) {
    const int M = 4;
    const double DT = dt / M;
    T X[SD], k1[SD], k2[SD], k3[SD], k4[SD], t[SD];
    for (int i = 0; i < SD; ++i) X[i] = x[i];
    for (int m = 0; m < M; ++m) {
        ode(X, u, tau, drag, k1);
        for (int i = 0; i < SD; ++i) { k1[i] = k1[i] * DT; t[i] = X[i] + 0.5 * k1[i]; }
        ode(t, u, tau, drag, k2);
        for (int i = 0; i < SD; ++i) { k2[i] = k2[i] * DT; t[i] = X[i] + 0.5 * k2[i]; }
        ode(t, u, tau, drag, k3);
        for (int i = 0; i < SD; ++i) { k3[i] = k3[i] * DT; t[i] = X[i] + k3[i]; }
        ode(t, u, tau, drag, k4);
        for (int i = 0; i < SD; ++i) { k4[i] = k4[i] * DT; X[i] = X[i] + (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) / 6.0; }
    }
    for (int i = 0; i < SD; ++i) xn[i] = X[i];
}

// F probed for its affine form F(x, u) = A x + B u + c (exactly affine: the ODE is linear in x and u) at zero, the unit states and
// the unit controls.  A [SD][SD], B [SD][UD] row-major, c [SD].
template <class T>
AMK_HD void affine_probe(const T *tau, const double *drag, double dt, T *A, T *B, T *c) {
    T z10[SD], z4[UD], e10[SD], e4[UD], f[SD];
    for (int i = 0; i < SD; ++i) z10[i] = T{};
    for (int i = 0; i < UD; ++i) z4[i] = T{};
    rk4(z10, z4, tau, drag, dt, c);
    for (int j = 0; j < SD; ++j) {
        for (int i = 0; i < SD; ++i) e10[i] = T{i == j ? 1.0 : 0.0};
        rk4(e10, z4, tau, drag, dt, f);
        for (int i = 0; i < SD; ++i) A[i * SD + j] = f[i] - c[i];
    }
    for (int j = 0; j < UD; ++j) {
        for (int i = 0; i < UD; ++i) e4[i] = T{i == j ? 1.0 : 0.0};
        rk4(z10, e4, tau, drag, dt, f);
        for (int i = 0; i < SD; ++i) B[i * UD + j] = f[i] - c[i];
    }
}

// A, B, c at tau (plain run), or, with dtau ([DtauBlock::kAxes][kLen]), their derivatives in tau_0..2 from three dual runs -- A, B, c
// are then the value part of the first of them, which is the plain run's operations in the plain run's order.
inline void mpc_dynamics(const double *tau, const double *drag, double dt, double *A, double *B, double *c, double *dtau) {
    if (!dtau) {
        affine_probe<double>(tau, drag, dt, A, B, c);
        return;
    }
    for (int a = 0; a < DtauBlock::kAxes; ++a) {
        Dual t[4], dA[SD * SD], dB[SD * UD], dc[SD];
        for (int i = 0; i < 4; ++i) t[i] = {tau[i], i == a ? 1.0 : 0.0};
        affine_probe<Dual>(t, drag, dt, dA, dB, dc);
        double *o = dtau + a * DtauBlock::kLen;
        for (int e = 0; e < SD * SD; ++e) { o[DtauBlock::kA + e] = dA[e].d; if (a == 0) A[e] = dA[e].v; }
        for (int e = 0; e < SD * UD; ++e) { o[DtauBlock::kB + e] = dB[e].d; if (a == 0) B[e] = dB[e].v; }
        for (int e = 0; e < SD; ++e) { o[DtauBlock::kC + e] = dc[e].d; if (a == 0) c[e] = dc[e].v; }
    }
}

}  // namespace amk
